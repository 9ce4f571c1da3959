#!/usr/bin/env python3
"""Helpers of tools/ic_reuse_ab.sh.
  ic_reuse_ab.py table DIR   condense the bench lines DIR/ab_{parent,offp,off,on}_*.json into the A/B table
  ic_reuse_ab.py cold        first frame of a view: eight times a new stream, ONE lt_render_dev call of the 4096^2
                             benchmark frame, synchronize -- wall time per call (LT_IC_REUSE from the environment)"""
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(out):
    def rows(pat):
        r = []
        for f in sorted(glob.glob(os.path.join(out, pat))):
            with open(f) as fh:
                lines = [ln for ln in fh.read().splitlines() if ln.startswith("{")]
            d = json.loads(lines[-1])
            other = d["roofline"]["other_kernels_ms"]
            r.append((os.path.basename(f), d["ms_per_step"], d["value"], d["ranks"]["integrate_ms"][0], other["prologue"],
                      other["epilogue"]))
        return r

    means = {}
    for key, label, pat in (("parent", "parent build", "ab_parent_*.json"),
                            ("offp", "this build, LT_IC_REUSE=0, alternating with the parent build", "ab_offp_*.json"),
                            ("off", "LT_IC_REUSE=0, alternating with LT_IC_REUSE=1", "ab_off_*.json"),
                            ("on", "LT_IC_REUSE=1 (default)", "ab_on_*.json")):
        r = rows(pat)
        if not r:
            continue
        print("==", label)
        print("%-20s %12s %10s %13s %12s %12s" % ("run", "ms_per_step", "Mrays/s", "integrate_ms", "prologue_ms", "epilogue_ms"))
        for x in r:
            print("%-20s %12.4f %10.1f %13.4f %12.4f %12.4f" % x)
        for i, name in ((1, "ms_per_step"), (2, "Mrays/s"), (3, "integrate_ms"), (4, "prologue_ms")):
            v = [x[i] for x in r]
            means[key, name] = (sum(v) / len(v), min(v), max(v))
            print("   %-12s mean %.4f  min %.4f  max %.4f" % ((name,) + means[key, name]))
    if ("off", "ms_per_step") in means and ("on", "ms_per_step") in means:
        off, on = means["off", "ms_per_step"], means["on", "ms_per_step"]
        need = means["off", "prologue_ms"][0] - 0.03
        print("== verdict: ranges %s; difference of the means %.4f ms, required >= prologue (off) - 0.03 = %.4f ms; %+.2f %% Mrays/s"
              % ("do not overlap" if on[2] < off[1] else "OVERLAP", off[0] - on[0], need,
                 100 * (means["on", "Mrays/s"][0] / means["off", "Mrays/s"][0] - 1)))


def cold():
    sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import ltrace
    import hipmini
    n = 4096
    fov = float(np.radians(40.0))
    cam = ltrace.Camera(n, n, fov, fov, 0.0, 0.0, 50.0, np.pi / 2)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    rgba = hipmini.DeviceArray((n, n, 4), np.uint8)

    def one(reps):
        s = hipmini.Stream()
        o = ltrace.default_opts(precision=32)
        o.stream = s.ptr
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            ltrace.render_dev(cam, met, o, d_rgba=rgba.ptr)
            s.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ltrace.release_stream(s.ptr)
        return ts

    one(6)                      # code objects loaded, clocks settled
    t = [one(1)[0] for _ in range(8)]
    print("cold_frame_ms LT_IC_REUSE=%s" % os.environ.get("LT_IC_REUSE", "default"), " ".join("%.3f" % x for x in t),
          "| median %.3f min %.3f" % (float(np.median(t)), min(t)), "| (hits, misses)", ltrace.ic_reuse_counts(), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "cold":
        cold()
    else:
        sys.exit(__doc__)
