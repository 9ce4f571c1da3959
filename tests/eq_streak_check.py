"""Renders a set of Kerr frames twice in one process, with the float32 streak's fixed-quadrant loop enabled and disabled
(ltrace.set_eq_streak), and prints one JSON line: per frame, the names of the outputs and counters that differ between the
two (none may), and the fixed-quadrant iterations counted with the loop enabled / disabled.  tests/test_gpu_eq_streak.py
runs it under the switches that are read once per process (LT_D_PERSIST, LT_D_LONG, LT_Q_LONG)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))

import numpy as np   # noqa: E402
import ltrace        # noqa: E402

OUTPUTS = ("fa", "winding", "steps", "status", "rgba")
# what a frame's rays determine; the direct schedule's wavefronts are tiles, so their iteration counts are determined too
# (the queue schedule deals rays to wavefronts in the order the queue head is reached, which varies from run to run)
COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "bg_tiles_lds", "bg_tiles_global")
DIRECT_COUNTERS = ("wave_iters", "waves")


def frames():
    """(name, render function of (opts), precision, schedules)"""
    fov = np.radians(40.0)

    def plain(n, theta_deg, a):
        cam = ltrace.Camera(n, n, fov, fov, 0.0, 0.0, 50.0, np.radians(theta_deg))
        met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, a)
        return lambda o: ltrace.render(cam, met, o, want=OUTPUTS)

    out = [(f"plain{n}_th{th}_a{a}", plain(n, th, a), 32, ("direct", "queue"))
           for n, th, a in ((192, 90.0, 0.9), (192, 60.0, 0.9), (192, 25.0, 0.9), (192, 135.0, -0.9))]
    # more tiles than the chip has wavefront slots (5 120): the launch that hands tiles out from a queue head (LT_D_PERSIST)
    out.append(("plain768_th90_a0.9", plain(768, 90.0, 0.9), 32, ("direct",)))
    out.append(("plain96_th90_a0.9_f64", plain(96, 90.0, 0.9), 64, ("direct", "queue")))
    cam = ltrace.Camera(96, 96, fov, fov, 0.0, 0.0, 50.0, np.radians(80.0))
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk()
    out.append(("disk96", lambda o: ltrace.render_disk(cam, met, o, disk, want=OUTPUTS + ("disk",)), 32, ("direct",)))
    out.append(("disk_images96", lambda o: ltrace.render_disk_images(cam, met, o, disk, want=OUTPUTS + ("images", "n_hits")), 32,
                ("direct",)))
    return out


def main():
    report = {}
    for name, render, prec, schedules in frames():
        for sched in schedules:
            o = ltrace.default_opts(integrator="rk4", precision=prec, schedule=sched)
            got = {}
            for on in (True, False):
                ltrace.set_eq_streak(on)
                got[on] = render(o)
            ltrace.set_eq_streak(True)
            a, b = got[True], got[False]
            differ = [k for k in a if k != "stats" and a[k].tobytes() != b[k].tobytes()]
            names = COUNTERS + (DIRECT_COUNTERS if sched == "direct" else ()) + tuple(k for k in ("disk", "disk_hits") if k in a["stats"])
            differ += ["stats." + k for k in names if a["stats"][k] != b["stats"][k]]
            report[f"{name}|{sched}"] = dict(differ=differ, outputs=sorted(k for k in a if k != "stats"),
                                             eq_iters_on=a["stats"]["eq_iters"], eq_iters_off=b["stats"]["eq_iters"],
                                             wave_iters=a["stats"]["wave_iters"])
    print("report", json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
