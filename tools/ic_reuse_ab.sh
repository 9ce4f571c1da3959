#!/bin/bash
# tools/ic_reuse_ab.sh [PARENT_DIR [OUT_DIR]] -- what reusing the camera prologue's ray records buys on the
# benchmark frame, on the GPU box, one lease:
#   1. (with PARENT_DIR, a built checkout of the commit before the change) its bench line against this build with
#      LT_IC_REUSE=0, alternating, three times: the switch must be the old behaviour within the run-to-run spread;
#   2. LT_IC_REUSE=0 / 1 alternating, five times each: python bench.py --steps 20 --warmup 5;
#   3. the first frame of a view (new stream, one call, synchronize), switch off / on, three processes each;
#   4. rocprofv3 --kernel-trace --stats of the same command, switch off and on (kernel trace only).
# Every GPU step has its own time limit and the script stops at the first failure.
# Result: OUT_DIR/summary.txt (default bench_outputs/ic_reuse_ab; kept as profiles/ic_reuse_ab.txt).
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd); PARENT=${1:-}
OUT=${2:-$ROOT/bench_outputs/ic_reuse_ab}; rm -rf "$OUT"; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd)
ARGS="--steps 20 --warmup 5"
bench() { # name, directory, environment assignment
  (cd "$2" && env "$3" timeout -k 10 240 python3 bench.py $ARGS > "$OUT/$1.json" 2> "$OUT/$1.err"); rc=$?
  [ $rc = 0 ] || { echo "$1 rc=$rc"; tail -5 "$OUT/$1.err"; exit $rc; }
}
cd "$ROOT"
if [ -n "$PARENT" ]; then
  for i in 1 2 3; do bench ab_parent_$i "$PARENT" LT_IC_REUSE=1; bench ab_offp_$i "$ROOT" LT_IC_REUSE=0; done
fi
for i in 1 2 3 4 5; do bench ab_off_$i "$ROOT" LT_IC_REUSE=0; bench ab_on_$i "$ROOT" LT_IC_REUSE=1; done
S=$OUT/summary.txt
{ echo "# python bench.py $ARGS, build $(cat "$ROOT/light-path-tracer_amd/lib/libltrace_hip.so.buildid")"; python3 tools/ic_reuse_ab.py table "$OUT"; } > "$S"
echo "== first frame of a view: new stream, one lt_render_dev call (4096^2), synchronize; wall ms, eight streams per process" >> "$S"
for i in 1 2 3; do
  for sw in 0 1; do
    LT_IC_REUSE=$sw timeout -k 10 240 python3 tools/ic_reuse_ab.py cold >> "$S" 2>> "$OUT/cold_frame.err"; rc=$?
    [ $rc = 0 ] || { echo "cold frame rc=$rc"; tail -5 "$OUT/cold_frame.err"; exit $rc; }
  done
done
for sw in 0 1; do
  name=$([ $sw = 0 ] && echo off || echo on)
  P=$OUT/prof_$name; mkdir -p "$P"; echo "$ARGS   (LT_IC_REUSE=$sw)" > "$P/args.txt"
  cp "$OUT/ab_${name}_4.json" "$P/bench_plain_a.json"; cp "$OUT/ab_${name}_5.json" "$P/bench_plain_b.json"
  LT_IC_REUSE=$sw timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$P/trace" -- python3 bench.py $ARGS > "$P/bench_trace.log" 2>&1; rc=$?
  [ $rc = 0 ] || { echo "trace $name rc=$rc"; tail -8 "$P/bench_trace.log"; exit $rc; }
  { echo; echo "######## rocprofv3 --kernel-trace --stats, LT_IC_REUSE=$sw (the two runs 'without profiler' are runs 4 and 5 of the table above)"
    python3 tools/prof_summary.py "$P" 5; } >> "$S" 2>&1
  find "$P/trace" -type f ! -name '*kernel_stats.csv' -delete
done
cat "$S"
