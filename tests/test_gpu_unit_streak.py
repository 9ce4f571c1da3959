"""The unit-step form of the float32 streak's fixed-quadrant loop (kerr_rk4_streak): a wavefront whose rays
all step by exactly 1 and start a streak call far from the end of the affine range takes its steps with h, h / 2 and h / 6
as literals and without the per-step range test.  Multiplying by 1 is exact and the dropped test was true, so the switch
(ltrace.set_unit_streak / LT_UNIT_STREAK) may change NOTHING: every comparison here is an equality.

tests/unit_streak_check.py, one process per environment:
  frames   128 x 128, float32 RK4, both schedules, switch on against off: final_alpha, winding, status and steps of every
           pixel bit for bit, and the counters -- rays, steps, right-hand-side evaluations, endings, and in the direct
           schedule wave iterations and fixed-quadrant iterations (the queue schedule's grouping of rays into wavefronts
           varies from run to run).  Cameras: a = 0.9 from r = 50 on the equator, at theta 1.0 and 0.3 (angles leave the
           band in mid-streak), from r = 12 (next to 4 r_capture), and a = 0.99 from 0.005 rad off the spin axis.  The
           axis-refine columns cut through two columns of tiles: wavefronts that mix base steps of 1 and 0.5 must stay on the old loops.
  ray sets 4096 rays = 64 wavefronts, both schedules, switch on and off against the general iteration alone
           (ltrace.trace_batch_kerr_general_probe): final_alpha, winding, status, right-hand-side evaluations of every ray.
           The cameras above, with the frames' refine rule, all rays refined and none, and affine ranges of 37.25, 60.5 and
           100.5: rays end inside a streak and the hoisted range test fails -- at once, or after one call in the unit-step form.
Environments: ghost lanes from the first iteration (LT_D_LONG=0), at the default iteration, and never."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CAMERAS = ("equator", "th1.0", "th0.3", "r12", "axis_a0.99")
SETS = CAMERAS + ("axis_a0.99_refine", "no_refine", "lam37.25", "lam60.5", "lam100.5")
SCHEDULES = ("direct", "queue")
ENVS = {"default": {}, "ghost_lanes_from_the_start": {"LT_D_LONG": "0"}, "ghost_lanes_never": {"LT_D_LONG": "1000000000"}}
_reports = {}


def report(env_id):
    if env_id not in _reports:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "unit_streak_check.py")],
                             env=dict(os.environ, **ENVS[env_id]), check=True, capture_output=True, text=True, timeout=600).stdout
        lines = [ln for ln in out.splitlines() if ln.startswith("report ")]
        assert len(lines) == 1, out
        _reports[env_id] = json.loads(lines[0][len("report "):])
    return _reports[env_id]


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", list(ENVS))
def test_the_switch_changes_no_output_and_no_counter_of_a_frame(env_id):
    rep = report(env_id)
    assert sorted(k for k in rep if k.startswith("frame|")) == sorted(f"frame|{c}|{s}" for c in CAMERAS for s in SCHEDULES)
    for cam in CAMERAS:
        for sched in SCHEDULES:
            r = rep[f"frame|{cam}|{sched}"]
            print(cam, sched, r)
            assert r["differ"] == [], (cam, sched, r["differ"])
            assert r["rays"] == 128 * 128 and r["steps"] > 0 and r["escaped"] > 0
            # wavefronts of both kinds: with axis-refine rays next to others, and with a base step of 1 in every lane
            assert r["tile_columns_mixed"] == 2 and r["tile_columns_unit"] == 14
        d = rep[f"frame|{cam}|direct"]
        assert d["wave_iters"] > 0
        if cam in ("equator", "r12"):
            assert 0 < d["eq_iters"] <= d["wave_iters"], d   # the loop that carries the unit-step form was really taken


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", list(ENVS))
def test_either_setting_equals_the_general_iteration_alone(env_id):
    rep = report(env_id)
    assert sorted(k for k in rep if k.startswith("batch|")) == sorted(f"batch|{c}|{s}" for c in SETS for s in SCHEDULES)
    none = {"fa": 0, "winding": 0, "status": 0, "evals": 0}
    for name in SETS:
        for sched in SCHEDULES:
            r = rep[f"batch|{name}|{sched}"]
            print(name, sched, r)
            assert r["rays"] == 4096
            assert r["differ"] == {"on": none, "off": none}, (name, sched, r["differ"])
            assert r["evals_total"] > 0
    for sched in SCHEDULES:
        # from r = 50 a ray needs an affine range of more than 50 to escape at r = 100 and of ~48 to be captured: with 37.25
        # every ray ends at the range limit (which the status counts with the escapes), the unrefined ones after 37 steps of 1
        # and one of 0.25; with 60.5 and 100.5 the rays that stay outside 4 r_capture and do not escape in time end there
        # after 61 and 101 steps
        assert rep[f"batch|lam37.25|{sched}"]["escaped"] == 4096 and rep[f"batch|lam37.25|{sched}"]["captured"] == 0
        for name in ("lam37.25", "lam60.5", "lam100.5"):
            assert rep[f"batch|{name}|{sched}"]["full_range_unit"] > 0, name
        assert rep[f"batch|equator|{sched}"]["escaped"] > 0 and rep[f"batch|equator|{sched}"]["captured"] > 0
