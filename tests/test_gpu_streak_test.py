"""The far-field streak's per-step test (kerr_rk4_streak_loop) against a yardstick that never runs the
streak: ltrace.trace_batch_kerr_general_probe traces every ray by the general iteration alone.  "Which of the two paths
took a step does not matter" is what the loop's comment claims, so the production batch path must give the same bits --
final_alpha (NaN where the ray did not escape), winding, status -- and the same number of right-hand-side evaluations,
ray by ray.  All comparisons are equalities: no tolerance.

The ray sets (tests/streak_test_check.py), 4096 rays = 64 wavefronts each, float32 and float64, both schedules:
A the default camera on the equator; B the camera at 1.0 and 0.3 rad, where angles leave the fixed-quadrant loop's band
in mid-streak; C the camera at r = 12, next to 4 r_capture; D an affine range that ends inside a streak; E a = 0.99 and
the camera 0.005 rad from the spin axis with axis-refine rays, where attempts come out non-finite and are retried.
Each environment is a process of its own: the switches are read once."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETS = ("A", "B_th1.0", "B_th0.3", "C", "D_lam37.25", "D_lam60.5", "E")
CASES = [f"{s}|f{p}|{sched}" for s in SETS for p in (32, 64) for sched in ("direct", "queue")]
ENVS = {"default": {}, "ghost_lanes_from_the_start": {"LT_D_LONG": "1"}, "fixed_quadrant_loop_off": {"LT_EQ_STREAK": "0"}}
_reports = {}


def report(env_id):
    if env_id not in _reports:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "streak_test_check.py")],
                             env=dict(os.environ, **ENVS[env_id]), check=True, capture_output=True, text=True, timeout=600).stdout
        lines = [ln for ln in out.splitlines() if ln.startswith("report ")]
        assert len(lines) == 1, out
        _reports[env_id] = json.loads(lines[0][len("report "):])
    return _reports[env_id]


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", list(ENVS))
def test_batch_path_equals_the_general_iteration_alone(env_id):
    rep = report(env_id)
    assert sorted(k for k in rep if k != "frame_A") == sorted(CASES)
    for name in CASES:
        r = rep[name]
        print(name, r)
        assert r["rays"] == 4096
        assert r["differ"] == {"fa": 0, "winding": 0, "status": 0, "evals": 0}, (name, r["differ"])
        assert r["fa_nan_where_not_escaped"], name
        assert r["escaped"] > 0 and r["evals_total"] > 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", list(ENVS))
def test_the_sets_reach_what_they_are_there_for(env_id):
    rep = report(env_id)
    for prec in (32, 64):
        for sched in ("direct", "queue"):
            # D: from r = 50 a ray needs an affine range of ~48 to be captured and of more than 50 to escape at r = 100
            # (|dr/dlambda| <= 1), so with 37.25 every ray ends at the range limit: 37 base steps of 1 and one of 0.25 -- 38
            # steps, 152 evaluations -- or 74 of 0.5 and one of 0.25 on an axis-refine ray.  With 60.5 the inner rays are
            # captured, and the rays that never come inside 4 r_capture take 60 base steps and one of 0.5: 61 steps.
            d = rep[f"D_lam37.25|f{prec}|{sched}"]
            assert d["captured"] == 0 and d["invalid"] == 0
            assert d["evals_hist"]["152"] > 0 and d["evals_hist_refine"]["300"] > 0
            assert d["evals_hist"]["152"] + d["evals_hist_refine"]["300"] == 4096
            d = rep[f"D_lam60.5|f{prec}|{sched}"]
            assert d["captured"] > 0 and d["evals_hist"]["244"] > 0
            # E: rays that became invalid after taking steps -- a non-finite attempt, retried with halved steps down to the floor
            assert rep[f"E|f{prec}|{sched}"]["invalid_in_flight"] > 0
    f = rep["frame_A"]
    if env_id == "default":
        assert 0 < f["eq_iters"] <= f["wave_iters"], f   # the fixed-quadrant loop was really taken
    if env_id == "fixed_quadrant_loop_off":
        assert f["eq_iters"] == 0, f
