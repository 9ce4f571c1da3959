"""Traces frames and ray sets with the unit-step form of the float32 streak's fixed-quadrant loop switched on and off
(ltrace.set_unit_streak) in one process, the ray sets also by the general iteration alone
(ltrace.trace_batch_kerr_general_probe), and prints one JSON line: per frame the outputs and counters that differ between
the two settings, per ray set how many rays differ from the yardstick under either setting (none may, anywhere), and what
shows that a case reached the code it is there for.  tests/test_gpu_unit_streak.py runs it under the switches that are
read once per process (LT_D_LONG)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))

import numpy as np   # noqa: E402
import ltrace        # noqa: E402
from streak_test_check import rays, trace   # noqa: E402  (the ray fan and the batch call of the streak's own test)

COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid")
# the direct schedule's alone: the queue schedule deals rays to wavefronts in the order the queue head is reached, which
# varies from run to run, and with it what a wavefront iterates over
DIRECT_COUNTERS = ("wave_iters", "waves", "eq_iters")


def cameras():
    """name -> (a, r_obs, theta_obs): 128 x 128 frames, 40 degrees wide; the axis-refine columns (60 to 68) cut through the
    8 x 8 tiles of columns 56 to 71, so those wavefronts mix base steps of 1 and of 0.5 and the others step by 1 throughout"""
    return {"equator": (0.9, 50.0, np.pi / 2), "th1.0": (0.9, 50.0, 1.0), "th0.3": (0.9, 50.0, 0.3), "r12": (0.9, 12.0, np.pi / 2),
            "axis_a0.99": (0.99, 50.0, 0.005)}


def sets():
    """name -> (a, r_obs, theta_obs, lambda_max, refine flags or None for the rule's)"""
    return {"equator": (0.9, 50.0, np.pi / 2, 5000.0, None),
            "th1.0": (0.9, 50.0, 1.0, 5000.0, None),
            "th0.3": (0.9, 50.0, 0.3, 5000.0, None),
            "r12": (0.9, 12.0, np.pi / 2, 5000.0, None),
            "axis_a0.99": (0.99, 50.0, 0.005, 5000.0, None),
            "axis_a0.99_refine": (0.99, 50.0, 0.005, 5000.0, 1),
            "no_refine": (0.9, 50.0, np.pi / 2, 5000.0, 0),
            # the hoisted range test fails from the first call on: lam + 65 <= lambda_max - 1 never holds, and every ray runs
            # into the range limit inside a streak
            "lam37.25": (0.9, 50.0, np.pi / 2, 37.25, None),
            "lam60.5": (0.9, 50.0, np.pi / 2, 60.5, None),
            # it holds for the first call (0 + 65 <= 99.5) and fails for the second (65 + 65): the unit-step form hands
            # over to the tested form, in which the rays that are still under way reach the limit
            "lam100.5": (0.9, 50.0, np.pi / 2, 100.5, None)}


def main():
    report = {}
    n, fov = 128, np.radians(40.0)
    for name, (a, r_obs, tho) in cameras().items():
        cam, met = ltrace.Camera(n, n, fov, fov, 0.0, 0.0, r_obs, tho), ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, a)
        refine_cols = ltrace.pixel_angles(cam, want_theta=False)[2]
        for sched in ("direct", "queue"):
            out = {}
            for on in (True, False):
                ltrace.set_unit_streak(on)
                out[on] = ltrace.render(cam, met, ltrace.default_opts(integrator="rk4", precision=32, schedule=sched),
                                        want=("fa", "winding", "status", "steps"))
            ltrace.set_unit_streak(True)
            differ = [k for k in ("fa", "winding", "status", "steps") if out[True][k].tobytes() != out[False][k].tobytes()]
            differ += [k for k in COUNTERS + (DIRECT_COUNTERS if sched == "direct" else ()) if out[True]["stats"][k] != out[False]["stats"][k]]
            st = out[True]["stats"]
            tiles = refine_cols.reshape(-1, 8)
            report[f"frame|{name}|{sched}"] = dict(
                differ=differ, rays=st["rays"], steps=st["steps"], wave_iters=st["wave_iters"], eq_iters=st["eq_iters"],
                escaped=st["escaped"], captured=st["captured"],
                tile_columns_mixed=int((tiles.any(axis=1) & ~tiles.all(axis=1)).sum()),
                tile_columns_unit=int((~tiles.any(axis=1)).sum()))
    al, th, rule = rays()
    for name, (a, r_obs, tho, lam, flags) in sets().items():
        ar = rule if flags is None else np.full(al.size, flags, dtype=np.uint8)
        ref = trace(ltrace.trace_batch_kerr_general_probe, a, r_obs, tho, lam, al, th, ar, 32)
        for sched in ("direct", "queue"):
            differ = {}
            for on in (True, False):
                ltrace.set_unit_streak(on)
                got = trace(ltrace.trace_batch_kerr, a, r_obs, tho, lam, al, th, ar, 32, integrator="rk4", schedule=sched)
                differ["on" if on else "off"] = {
                    k: int((got[k].view(np.uint64) != ref[k].view(np.uint64)).sum()) if k == "fa" else int((got[k] != ref[k]).sum())
                    for k in ref}
            ltrace.set_unit_streak(True)
            st, ev = ref["status"], ref["evals"].astype(np.int64)
            report[f"batch|{name}|{sched}"] = dict(
                differ=differ, rays=int(al.size), escaped=int((st == 1).sum()), captured=int((st == -1).sum()),
                evals_total=int(ev.sum()),
                # steps of a ray that is never refined and ends at the range limit after base steps of 1 alone
                full_range_unit=int((ev[ar == 0] == 4 * int(np.ceil(lam))).sum()))
    print("report", json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
