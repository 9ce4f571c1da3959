"""Where k_kerr_direct<float, Rk4<float>> reads a, a^2 and 2M from (pin_consts / DirectPin) changes no bit.

That kernel leaves the three constants in scalar registers; the queue schedule's kernel (and every other one) copies them
into vector registers.  The operations are the same, so a direct-schedule frame against the queue-schedule frame of the
same scene is a comparison of the two operand forms of the same arithmetic, and every comparison here is an equality:
final_alpha, winding, status, step counts and RGBA8 byte for byte, and every counter of the call: rays, steps,
right-hand-side evaluations, the three endings, and the epilogue's background tiles of either path.  (wave_iters and waves
describe how a schedule groups rays into wavefronts and differ between the schedules by construction; they are compared
among the direct-schedule runs.  eq_iters counts the iterations of a loop the switches below turn off.)

Cases, float32 RK4, 64 x 64 and 96 x 64 pixels: a = 0 through the Kerr kernel (the constant is a zero), a = 0.9, a = -0.7,
a = 0.998 seen from 0.005 rad off the spin axis (axis-refine lanes, retried steps), and M = 2 (2M = 4, r - M changes).
Each case also runs with the fixed-quadrant loop off (set_eq_streak(0)) and with its unit-step form off
(set_unit_streak(0)), so that all four forms of the streak loop and the general iteration run with scalar operands.
Phases: as is, and with every wavefront in its ghost-lane phase from the first iteration (LT_D_LONG=1, LT_Q_LONG=0, read
once per process, as tests/test_gpu_ghost_lanes.py sets them): one process per phase runs this file as a script."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (M, a, r_obs, theta_obs)
CASES = {"a0_kerr": (1.0, 0.0, 50.0, 1.5707963267948966), "a0.9": (1.0, 0.9, 50.0, 1.5707963267948966),
         "a-0.7": (1.0, -0.7, 50.0, 1.2), "a0.998_axis": (1.0, 0.998, 50.0, 0.005), "M2": (2.0, 1.4, 50.0, 1.5707963267948966)}
SIZES = ((64, 64), (96, 64))
PHASES = {"as_is": {}, "ghost_lanes_from_the_start": {"LT_D_LONG": "1", "LT_Q_LONG": "0"}}
ARRAYS = ("fa", "winding", "status", "steps", "rgba")
COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "bg_tiles_lds", "bg_tiles_global")
DIRECT_COUNTERS = ("wave_iters", "waves")
_reports = {}


def main():
    sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))
    import numpy as np
    import ltrace

    def frame(cam, met, bg, sched, eq=True, unit=True):
        ltrace.set_eq_streak(eq)
        ltrace.set_unit_streak(unit)
        try:
            out = ltrace.render(cam, met, ltrace.default_opts(integrator="rk4", precision=32, schedule=sched), background=bg,
                                want=ARRAYS)
        finally:
            ltrace.set_eq_streak(True)
            ltrace.set_unit_streak(True)
        return {k: np.ascontiguousarray(out[k]).tobytes() for k in ARRAYS}, out["stats"], out["status"].copy()

    report = {}
    fov = np.radians(40.0)
    for name, (M, a, r_obs, tho) in CASES.items():
        for W, H in SIZES:
            cam = ltrace.Camera(W, H, 2 * np.arctan(np.tan(fov / 2) * W / H), fov, 0.0, 0.0, r_obs, tho)
            met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
            bg = np.random.default_rng(W).integers(0, 256, size=(H, W, 3), dtype=np.uint8).astype(np.float32) / 255.0
            ref, ref_st, status = frame(cam, met, bg, "queue")                      # constants in vector registers
            runs = {"direct": frame(cam, met, bg, "direct"),                        # constants in scalar registers
                    "direct_eq_off": frame(cam, met, bg, "direct", eq=False),
                    "direct_unit_off": frame(cam, met, bg, "direct", unit=False),
                    "queue_eq_off": frame(cam, met, bg, "queue", eq=False)}
            d_st = runs["direct"][1]
            differ = {}
            for run, (arrs, st, _) in runs.items():
                differ[run] = [k for k in ARRAYS if arrs[k] != ref[k]] + [k for k in COUNTERS if st[k] != ref_st[k]]
                if run.startswith("direct"):
                    differ[run] += [k for k in DIRECT_COUNTERS if st[k] != d_st[k]]
            report[f"{name}|{W}x{H}"] = dict(
                differ=differ, rays=ref_st["rays"], escaped=int((status == 1).sum()), captured=int((status == -1).sum()),
                refine_columns=int(ltrace.pixel_angles(cam, want_theta=False)[2].sum()), wave_iters=d_st["wave_iters"],
                eq_iters=d_st["eq_iters"], eq_iters_off=runs["direct_eq_off"][1]["eq_iters"])
    print("report", json.dumps(report), flush=True)
    return 0


def report(phase):
    if phase not in _reports:
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **PHASES[phase]), check=True,
                             capture_output=True, text=True, timeout=300).stdout
        lines = [ln for ln in out.splitlines() if ln.startswith("report ")]
        assert len(lines) == 1, out
        _reports[phase] = json.loads(lines[0][len("report "):])
    return _reports[phase]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("phase", list(PHASES))
def test_scalar_and_vector_operands_give_the_same_bits(phase, case):
    rep = report(phase)
    assert sorted(rep) == sorted(f"{c}|{w}x{h}" for c in CASES for w, h in SIZES)
    for w, h in SIZES:
        r = rep[f"{case}|{w}x{h}"]
        print(phase, case, f"{w}x{h}", r)
        assert r["differ"] == {"direct": [], "direct_eq_off": [], "direct_unit_off": [], "queue_eq_off": []}, r["differ"]
        # the case reached the code it is there for: rays of both endings, real iterations, the fixed-quadrant loop taken
        # where the camera is on the equator and not taken with the switch off, refine lanes in the view along the axis
        assert r["rays"] == w * h and r["escaped"] > 0 and r["captured"] > 0 and r["wave_iters"] > 0
        assert r["eq_iters_off"] == 0
        if case in ("a0_kerr", "a0.9", "M2") and phase == "as_is":
            assert 0 < r["eq_iters"] <= r["wave_iters"], r
        if case == "a0.998_axis":
            assert r["refine_columns"] > 0, r


if __name__ == "__main__":
    sys.exit(main())
