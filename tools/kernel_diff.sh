#!/bin/bash
# tools/kernel_diff.sh PARENT_DIR [OUT_DIR] -- is the device code of this checkout the device code of PARENT_DIR (a checkout
# of the commit a host-only change is based on)?  No GPU needed.  Both translation units are compiled device-only at both
# checkouts with the project's flags and a fixed -DLT_BUILD_ID (the HIP compilation-unit id is hashed from the command line),
# for the product build and for the -DLT_PROBES build; the gfx950 code objects are compared:
#   same   .text and .rodata byte-identical and the same kernel symbols;
#   moved  kernels changed places inside .text, but every kernel's bytes (symbol address + size out of .text), its
#          descriptor and its metadata record (registers, private segment, LDS, kernarg size and arguments) are
#          identical one by one -- the moved kernels are listed;
#   DIFF   anything else -- the differing kernels are listed.  Exit status 1.
set -u -o pipefail
[ $# -ge 1 ] || { echo "usage: $0 PARENT_DIR [OUT_DIR]"; exit 2; }
ROOT=$(cd "$(dirname "$0")/.." && pwd); PARENT=$(cd "$1" && pwd)
OUT=${2:-$ROOT/bench_outputs/kernel_diff}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=fast -fno-slp-vectorize -DLT_BUILD_ID=\"x\" --offload-device-only"

unit() { # side directory, build name, source, extra flags...: leaves $OUT/<side>_<build>_<source>.{elf,text,rodata,syms,notes}
  local side=$1 dir=$2 build=$3 src=$4; shift 4
  local b=$OUT/${side}_${build}_${src%.hip}
  (cd "$dir/light-path-tracer_amd/csrc" && ${HIPCC:-hipcc} $FLAGS "$@" -c -o "$b.co" "$src") &&
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hip-amdgcn-amd-amdhsa--gfx950 --input="$b.co" --output="$b.elf" &&
  "$LLVM/llvm-objcopy" --dump-section .text="$b.text" --dump-section .rodata="$b.rodata" "$b.elf" /dev/null &&
  "$LLVM/llvm-readelf" --sections --symbols --wide "$b.elf" > "$b.syms" && "$LLVM/llvm-readelf" --notes "$b.elf" > "$b.notes"
}

pids=()
for build in product probes; do
  extra=(); [ $build = probes ] && extra=(-DLT_PROBES)
  for side in parent branch; do
    dir=$ROOT; [ $side = parent ] && dir=$PARENT
    unit $side "$dir" $build lt_api.hip "${extra[@]}" & pids+=($!)
    unit $side "$dir" $build lt_k2_lone.hip "${extra[@]}" -mllvm -amdgpu-sched-strategy=max-ilp & pids+=($!)
  done
done
for p in "${pids[@]}"; do wait "$p" || { echo "a compile or dump step failed"; exit 2; }; done

echo "# parent $(git -C "$PARENT" rev-parse --short HEAD 2>/dev/null || echo "$PARENT"), $(${HIPCC:-hipcc} --version | grep -m1 -i 'hip version')"
python3 - "$OUT" <<'EOF'
import re, sys
out = sys.argv[1]

def kernels(base):
    """{symbol: (bytes, metadata record)} of one code object: every function out of .text, every object out of .rodata
    (the kernel descriptors, with the one field that holds the distance to the kernel's code left out)."""
    data = {sec: bytearray(open(base + "." + sec, "rb").read()) for sec in ("text", "rodata")}
    secs, syms, covered = {}, {}, []
    for ln in open(base + ".syms"):
        m = re.match(r"\s*\[\s*(\d+)\] \.(text|rodata)\s+PROGBITS\s+([0-9a-f]+)", ln)
        if m:
            secs[m.group(1)] = (m.group(2), int(m.group(3), 16))   # symbol values are addresses: the section's comes off
        f = ln.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6] in secs:
            sec, s0 = secs[f[6]]
            a, n = int(f[1], 16) - s0, int(f[2])
            b = bytes(data[sec][a:a + n])
            syms[f[7]] = b[:16] + b[24:] if f[7].endswith(".kd") else b   # kernel_code_entry_byte_offset
            covered.append((sec, a, n))
    notes = open(base + ".notes").read()
    recs = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        m = re.search(r"\.name:\s+(\S+)", blk)
        recs[m.group(1)] = re.sub(r"\.symbol:\s+\S+", "", blk.split("amdhsa.target")[0])
    n_kd = sum(n.endswith(".kd") for n in syms)
    if len(recs) != n_kd or any(n[:-3] not in recs for n in syms if n.endswith(".kd")):
        sys.exit(f"{base}: {len(recs)} metadata records parsed for {n_kd} kernel descriptors")
    for sec, a, n in covered:   # what no symbol covers (constants without a name) is compared as one more item
        data[sec][a:a + n] = bytes(n)
    syms["(.rodata outside symbols)"] = bytes(data["rodata"])
    return {n: (b, recs.get(n)) for n, b in syms.items()}

bad = 0
for build in ("product", "probes"):
    for src in ("lt_api", "lt_k2_lone"):
        p, b = (f"{out}/{side}_{build}_{src}" for side in ("parent", "branch"))
        kp, kb = kernels(p), kernels(b)
        same_sec = all(open(p + e, "rb").read() == open(b + e, "rb").read() for e in (".text", ".rodata"))
        diff = sorted(set(kp) ^ set(kb)) + sorted(n for n in set(kp) & set(kb) if kp[n] != kb[n])
        n_text = len(open(b + ".text", "rb").read())
        if same_sec and not diff:
            verdict = "same"
        elif not diff:
            verdict = "moved"
        else:
            verdict, bad = "DIFF", 1
        n_k = sum(n.endswith(".kd") for n in kb)
        order = lambda base: [ln.split()[7] for ln in sorted((ln for ln in open(base + ".syms") if " FUNC " in ln), key=lambda ln: ln.split()[1])]
        moved = list(dict.fromkeys(y for x, y in zip(order(p), order(b)) if x != y)) if verdict == "moved" else []
        print(f"{build:8s} {src + '.hip':15s} {verdict:5s} {n_k:3d} kernels compared, {len(moved)} moved, {len(diff)} differ; .text {n_text} bytes")
        for n in diff:
            print("    differs:", n)
        for n in moved:
            print("    moved:", n)
sys.exit(bad)
EOF
