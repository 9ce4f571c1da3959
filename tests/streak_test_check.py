"""Traces sets of Kerr rays twice in one process -- by the production batch path (far-field streak and general iteration)
and by the general iteration alone (ltrace.trace_batch_kerr_general_probe) -- and prints one JSON line: per set, how many
rays differ in final_alpha (bit patterns), winding, status and right-hand-side evaluations, and what shows that the set
reached the code it is there for.  tests/test_gpu_streak_test.py runs it under the switches that are read once per process
(LT_D_LONG, LT_EQ_STREAK)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))

import numpy as np   # noqa: E402
import ltrace        # noqa: E402

ALPHA_MAX = 0.36


def rays():
    """64 alphas from 0 to 0.36 rad x 64 screen angles round the circle = 4096 rays (64 wavefronts); the axis-refine flag
    by the frames' rule: within 7 % of the half width of the image's vertical axis."""
    al, ang = np.linspace(0.0, ALPHA_MAX, 64), np.arange(64) * (2 * np.pi / 64)
    al, th = np.tile(al, 64), np.repeat(ang, 64)
    return al, th, (np.abs(al * np.cos(th)) < 0.07 * ALPHA_MAX).astype(np.uint8)


def sets():
    """name -> (a, r_obs, theta_obs, lambda_max, refine flags or None for the rule's)"""
    out = {"A": (0.9, 50.0, np.pi / 2, 5000.0, None),
           "B_th1.0": (0.9, 50.0, 1.0, 5000.0, None),       # angles leave the band of the fixed-quadrant loop in mid-streak
           "B_th0.3": (0.9, 50.0, 0.3, 5000.0, None),
           "C": (0.9, 12.0, np.pi / 2, 5000.0, None),       # starts near 4 r_capture: the streak leaves on r < rc4 often
           "D_lam37.25": (0.9, 50.0, np.pi / 2, 37.25, None),  # every ray runs into lam <= lam_limit inside a streak
           "D_lam60.5": (0.9, 50.0, np.pi / 2, 60.5, None),
           "E": (0.99, 50.0, 0.005, 5000.0, 1)}             # the camera 0.005 rad from the spin axis, every ray axis-refine
    return out


def trace(fn, a, r_obs, tho, lam, al, th, ar, prec, **kw):
    n = al.size
    fa, w = np.empty(n), np.empty(n, dtype=np.int64)
    st, ev = np.empty(n, dtype=np.int8), np.empty(n, dtype=np.uint32)
    fn(1.0, a, r_obs, al, th, tho, lam, ar, fa, w, precision=prec, out_status=st, out_rhs_evals=ev, **kw)
    return dict(fa=fa, winding=w, status=st, evals=ev)


def main():
    al, th, rule = rays()
    report = {}
    for name, (a, r_obs, tho, lam, flags) in sets().items():
        ar = rule if flags is None else np.full(al.size, flags, dtype=np.uint8)
        for prec in (32, 64):
            ref = trace(ltrace.trace_batch_kerr_general_probe, a, r_obs, tho, lam, al, th, ar, prec)
            for sched in ("direct", "queue"):
                got = trace(ltrace.trace_batch_kerr, a, r_obs, tho, lam, al, th, ar, prec, integrator="rk4", schedule=sched)
                differ = {k: int((got[k].view(np.uint64) != ref[k].view(np.uint64)).sum()) if k == "fa" else int((got[k] != ref[k]).sum())
                          for k in ref}
                st, ev = ref["status"], ref["evals"]
                report[f"{name}|f{prec}|{sched}"] = dict(
                    differ=differ, rays=int(al.size), escaped=int((st == 1).sum()), captured=int((st == -1).sum()),
                    invalid=int((st == 0).sum()), invalid_in_flight=int(((st == 0) & (ev > 0)).sum()),
                    fa_nan_where_not_escaped=bool(np.isnan(ref["fa"][st != 1]).all() and np.isnan(got["fa"][got["status"] != 1]).all()),
                    evals_hist={str(int(k)): int((ev[ar == 0] == k).sum()) for k in (152, 244)},
                    evals_hist_refine={str(int(k)): int((ev[ar == 1] == k).sum()) for k in (300,)},
                    evals_total=int(ev.astype(np.int64).sum()))
    # the fixed-quadrant loop's counter exists per frame: the frame of set A's camera over set A's alphas
    fov = 2 * ALPHA_MAX
    cam = ltrace.Camera(64, 64, fov, fov, 0.0, 0.0, 50.0, np.pi / 2)
    out = ltrace.render(cam, ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_opts(integrator="rk4", precision=32),
                        want=("status",))
    report["frame_A"] = dict(eq_iters=int(out["stats"]["eq_iters"]), wave_iters=int(out["stats"]["wave_iters"]))
    print("report", json.dumps(report), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
