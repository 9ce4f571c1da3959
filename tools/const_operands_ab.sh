#!/bin/bash
# tools/const_operands_ab.sh -- which of a, a^2 and 2M should k_kerr_direct<float, Rk4<float>> read from VGPRs (pinned)
# and which from SGPRs?  (pin_consts, lt_device.hpp; DirectPin / LT_K2_F32_PIN, lt_kernels.hpp)
# A mask has one bit per PINNED constant: 1 = a, 2 = a^2, 4 = 2M; 7 is what every other kernel does, 0 what this kernel is committed with.
#
#   build MASK...                  (no GPU) ab_builds/libltrace_pinMASK.so: this checkout with -DLT_K2_F32_PIN=MASK
#   ab PARENT_DIR OUT N MASK...    (GPU) PARENT_DIR (a built checkout of the parent commit) and libltrace_pinMASK.so of
#                                  every mask in turn, N rounds: python3 bench.py --gpus 1 --steps 20 --warmup 5,
#                                  every run a process of its own; the parent runs in its own checkout with its own library
#   trace PARENT_DIR OUT MASK      (GPU) rocprofv3 --kernel-trace --stats of the same command, parent then MASK
#   table OUT                      condense OUT/*.json into OUT/summary.txt
# Every GPU step has its own time limit and the script stops at the first failure.
# The build id hashes the sources and the project's flags, not -DLT_K2_F32_PIN: every variant library reports the committed
# build id, so bench.py takes the committed profiles/valu_counts.json record as fresh for it and computes each variant's
# roofline and frac_at_held_clock with the committed kernel's SQ_INSTS_VALU (the variants' counts differ by 0.005 %).
set -u -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
ARGS="--gpus 1 --steps 20 --warmup 5"
mode=${1:-}; shift || true

bench() { # name, directory, library ("" = the directory's own), extra bench arguments...
  local name=$1 dir=$2 lib=$3; shift 3
  (cd "$dir" && env ${lib:+LTRACE_LIB="$lib"} timeout -k 10 240 python3 bench.py $ARGS "$@" > "$OUT/$name.json" 2> "$OUT/$name.err"); rc=$?
  [ $rc = 0 ] || { echo "$name rc=$rc"; tail -5 "$OUT/$name.err"; exit $rc; }
  echo "$name $(grep -o '"ms_per_step": [0-9.]*' "$OUT/$name.json" | head -1)"
}
lib() { echo "$ROOT/ab_builds/libltrace_pin$1.so"; }
outdir() { mkdir -p "$1"; OUT=$(cd "$1" && pwd); }

case "$mode" in
build)
  cd "$ROOT"
  for m in "$@"; do
    python3 -c "import os, __graft_entry__ as g; g._compile(os.path.join(g.ROOT, 'ab_builds', 'libltrace_pin$m.so'), ['-DLT_K2_F32_PIN=${m}u'])" > /dev/null || exit 1
    echo "built $(lib $m)"
  done ;;
ab)
  PARENT=$(cd "$1" && pwd); outdir "$2"; N=$3; shift 3
  for i in $(seq 1 "$N"); do
    bench "ab_parent_$i" "$PARENT" ""
    for m in "$@"; do bench "ab_pin${m}_$i" "$ROOT" "$(lib $m)"; done
  done ;;
trace)
  PARENT=$(cd "$1" && pwd); outdir "$2"; M=$3
  for side in parent pin$M; do
    P=$OUT/prof_$side; mkdir -p "$P"; echo "$ARGS ($side)" > "$P/args.txt"
    dir=$ROOT; l=$(lib $M); [ $side = parent ] && { dir=$PARENT; l=; }
    (cd "$dir" && env ${l:+LTRACE_LIB="$l"} timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$P/trace" -- python3 bench.py $ARGS > "$P/bench_trace.log" 2>&1); rc=$?
    [ $rc = 0 ] || { echo "trace $side rc=$rc"; tail -8 "$P/bench_trace.log"; exit $rc; }
    { echo "######## rocprofv3 --kernel-trace --stats, $side"; python3 "$ROOT/tools/prof_summary.py" "$P" 5; } > "$OUT/trace_$side.txt" 2>&1
    find "$P/trace" -type f ! -name '*kernel_stats.csv' -delete
  done ;;
table)
  outdir "$1"
  python3 - "$OUT" <<'EOF' | tee "$OUT/summary.txt"
import glob, json, os, re, sys
out = sys.argv[1]
rows = {}
for f in sorted(glob.glob(os.path.join(out, "*.json")), key=lambda p: [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", p)]):
    lines = [ln for ln in open(f).read().splitlines() if ln.startswith("{")]
    if not lines:
        continue
    d = json.loads(lines[-1])
    key = re.sub(r"_\d+$", "", os.path.basename(f)[:-5])
    ex = d["roofline"].get("executed", {})
    rows.setdefault(key, []).append((d["ms_per_step"], d["ranks"]["integrate_ms"][0], ex.get("clock_mhz_held"),
                                     d["roofline"].get("frac_at_held_clock") or ex.get("frac_at_held_clock")))
stat = {}
for key, r in rows.items():
    ms = [x[0] for x in r]
    stat[key] = (sum(ms) / len(ms), min(ms), max(ms))
    print(f"{key:16s} " + " ".join(f"{x[0]:.4f}" for x in r) + " | " + " ".join(f"{x[1]:.3f}" for x in r))
    print(f"{'':16s} mean {stat[key][0]:.4f}  range {stat[key][1]:.4f} ... {stat[key][2]:.4f}   held clock MHz " +
          " ".join(str(x[2]) for x in r) + "   frac_at_held_clock " + " ".join(str(x[3]) for x in r))
# the rule: the variant's range wholly below the parent's AND the gap of the means at least the wider range
if "ab_parent" in stat:
    pm, plo, phi = stat["ab_parent"]
    for key, (m, lo, hi) in stat.items():
        if key.startswith("ab_pin"):
            wider = max(phi - plo, hi - lo)
            apart = hi < plo
            print(f"== {key} against the parent: ranges {'apart' if apart else 'OVERLAP or above'}; means {pm:.4f} -> {m:.4f} "
                  f"({100 * (m / pm - 1):+.2f} %), gap {pm - m:+.4f} ms, wider range {wider:.4f} ms: "
                  f"{'PASSES' if apart and pm - m >= wider else 'does not pass'} on this lease")
EOF
  ;;
*) sed -n '2,12p' "$0"; exit 2 ;;
esac
