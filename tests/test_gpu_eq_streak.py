"""The float32 far-field streak's fixed-quadrant loop (kerr_rk4_streak) changes no result.

Its sincos is compared with the general one on the device for every float32 of the band, and whole frames are rendered
with the loop enabled and disabled: every output and every counter the rays determine must be byte-equal, while the
counter of fixed-quadrant iterations shows that the loop did run.  All comparisons are equalities: no tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "light-path-tracer_amd"))

import ltrace  # noqa: E402


def _bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.mark.gpu
def test_both_sincos_forms_agree_on_every_float32_of_the_band():
    lo, hi = np.float32(0.80), np.float32(2.34)
    got = ltrace.sincos_q1_probe(_bits(lo), _bits(hi))
    assert got["band"] == (float(lo), float(hi))               # the band the kernels use is the one probed
    assert got["compared"] == _bits(hi) - _bits(lo) + 1 == 13170115
    assert got["differing"] == 0, f"first differing x has bits {got['first_differing_bits']:#010x}"
    assert got["outside_k1"] == 0


def test_band_bounds_reduce_to_quadrant_one():
    two_over_pi = np.float32(0.636619772367581343)
    for x in (np.float32(0.80), np.float32(2.34)):
        assert np.rint(x * two_over_pi) == 1.0
    # ... with margins far above an ulp of the product (6e-8): the product stays 0.009 away from the rounding boundaries
    assert np.float32(0.80) * two_over_pi > 0.5 + 9e-3 and np.float32(2.34) * two_over_pi < 1.5 - 9e-3


def _report(**env):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eq_streak_check.py")], env=dict(os.environ, **env),
                         check=True, capture_output=True, text=True, timeout=600).stdout
    lines = [ln for ln in out.splitlines() if ln.startswith("report ")]
    assert len(lines) == 1, out
    return json.loads(lines[0][len("report "):])


F32_FRAMES = [f"plain192_th{th}_a{a}|{s}" for th, a in ((90.0, 0.9), (60.0, 0.9), (25.0, 0.9), (135.0, -0.9)) for s in ("direct", "queue")] + \
             ["plain768_th90_a0.9|direct", "disk96|direct", "disk_images96|direct"]
F64_FRAMES = ["plain96_th90_a0.9_f64|direct", "plain96_th90_a0.9_f64|queue"]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"LT_D_PERSIST": "0"}, {"LT_D_PERSIST": "1", "LT_D_LONG": "1", "LT_Q_LONG": "0"}],
                         ids=["default", "one_workgroup_per_tile", "ghost_lanes_from_the_start"])
def test_switch_changes_no_output(env):
    rep = _report(**env)
    assert sorted(rep) == sorted(F32_FRAMES + F64_FRAMES)
    for name, r in rep.items():
        assert set(r["outputs"]) >= {"fa", "winding", "steps", "status", "rgba"}, name
        assert r["differ"] == [], (name, r["differ"])
        assert r["eq_iters_off"] == 0, name                   # switch off: the loop is never entered
    ghosts = "LT_D_LONG" in env
    for name in F32_FRAMES:
        # the variant runs: a test that passes with the loop never entered proves nothing.  (With every wavefront in its
        # ghost-lane phase from the start the direct schedule takes its steps in the lone-wave form, which has no such loop.)
        if ghosts and name.endswith("|direct"):
            continue
        assert 0 < rep[name]["eq_iters_on"] <= rep[name]["wave_iters"], (name, rep[name])
    for name in F64_FRAMES:
        assert rep[name]["eq_iters_on"] == 0, name             # float64 has no such loop
    if not ghosts:
        # the camera on the equator: most iterations of a bulk wave are fixed-quadrant ones
        r = rep["plain192_th90.0_a0.9|direct"]
        assert r["eq_iters_on"] > 0.25 * r["wave_iters"], r
