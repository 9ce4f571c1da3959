"""The host side of tests/ray_replay.py: the case builders, what each case contains according to the float64 oracle, the
domain cap of the one-step bound on the oracle's own rays, and the comparison function on planted differences.  No GPU:
the rays come from the oracle's pixel angles (the device's lt_pixel_angles agrees with them to 1e-12, test_gpu_pipeline.py).
"""
import numpy as np
import pytest

import ray_replay as rr
from oracle import oracle

SIZES = {"wide": (72 * 40, 37), "near_axis": (40 * 40, 63), "critical_curve": (64 * 48, 1), "retrograde": (48 * 40, 29),
         "close": (40 * 40, 5), "far_observer": (48 * 24, 17), "schw_r12": (40 * 40, 11), "schw_r50": (40 * 40, 50)}
CUTS = {"ragged_1": 1, "ragged_63": 63, "ragged_65": 65, "ragged_1000": 1000}


def test_cases_have_the_advertised_sizes_and_remainders():
    assert sorted(rr.CASES) == sorted(list(SIZES) + list(CUTS))
    for name, (pixels, rem) in SIZES.items():
        c = rr.CASES[name]
        idx = rr.ray_index(c)
        assert c.W * c.H == pixels and pixels % 64 == 0            # whole wavefronts ...
        assert idx.size == pixels + rem and idx.size % 64 == rem and 0 < rem < 64   # ... plus a ragged remainder
        assert np.array_equal(np.unique(idx), np.arange(pixels))   # every pixel of the frame is in the set
        assert 1000 < idx.size < 4000
    for name, n in CUTS.items():
        c = rr.CASES[name]
        assert np.array_equal(rr.ray_index(c), np.arange(n))
        assert c._replace(name="wide", rem=rr.CASES["wide"].rem, cut=None) == rr.CASES["wide"]   # wide's camera, cut to n
    assert {n % 64 for n in CUTS.values()} == {1, 63, 1, 1000 % 64} and 1000 // 64 > 1


def test_case_builders_are_deterministic():
    for name, c in rr.CASES.items():
        first = rr.rays(c, "oracle")
        rr._pixels.cache_clear()
        again = rr.rays(c, "oracle")
        for x, y in zip(first, again):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
        al, th, rf = first
        assert al.shape == th.shape == rf.shape == rr.ray_index(c).shape and rf.dtype == np.uint8
        assert np.array_equal(al, al.astype(np.float32).astype(np.float64))   # alpha is the reference's float32 lookup
        wide = rr.rays(rr.CASES["wide"], "oracle")
        if c.cut is not None:
            assert all(np.array_equal(x, y[:c.cut]) for x, y in zip(first, wide))


@pytest.mark.parametrize("name", rr.FRAME_CASES)
def test_every_case_holds_every_class_of_ray(name):
    """Counted with the float64 oracle: escaped and captured rays in every case, refine-flagged rays in every Kerr case (the
    axis-refine columns of a camera that looks at the hole), rays of both endings among the refine-flagged ones where the
    geometry allows."""
    c = rr.CASES[name]
    al, th, rf = rr.rays(c, "oracle")
    if c.kind == rr.KERR:
        _, _, st, _ = oracle.trace_batch_kerr(rr.M, c.a, c.r_obs, al, th, c.theta_obs, rr.lambda_max(c), rf, integrator="rk4")
        assert 0 < rf.sum() < rf.size
        assert (st[rf != 0] == -1).any()
        if name in ("wide", "near_axis", "retrograde", "far_observer"):   # (seen from r = 12, or zoomed in, the hole fills the refine columns)
            assert (st[rf != 0] == 1).any()
    else:
        _, _, st, _ = oracle.trace_batch_schw(rr.M, c.r_obs, al)
        assert (st == 0).sum() == 1   # the axis pixel: alpha = 0, no impact parameter
    print(name, "escaped", int((st == 1).sum()), "captured", int((st == -1).sum()), "invalid", int((st == 0).sum()), "refine", int(rf.sum()))
    assert (st == 1).sum() >= 50 and (st == -1).sum() >= 50


def test_ragged_cuts_hold_rays():
    wide = rr.CASES["wide"]
    al, th, rf = rr.rays(wide, "oracle")
    _, _, st, _ = oracle.trace_batch_kerr(rr.M, wide.a, wide.r_obs, al, th, wide.theta_obs, rr.lambda_max(wide), rf, integrator="rk4")
    assert (st[:1000] == 1).any() and rf[:1000].any() and rf[:63].any()   # (a cut of the first rows: the hole is further down)


@pytest.mark.parametrize("name", rr.BOUND_CASES)
def test_domain_cap_holds_on_the_oracles_rays(name):
    """The states the oracle's float64 rays hold after every 32nd iteration: at most 5 % lie outside the domain of the
    one-step bound (ray_replay.step_domain) -- the cap test_gpu_ray_replay.py allows the float32 rays."""
    c = rr.CASES[name]
    o = rr.oracle_rays(c)
    s = o["samples"]
    d = rr.step_domain(c, s["state"], s["L"], s["refine"], s["lam"])
    m = s["ray"].size
    outside = int((~d["inside"]).sum())
    print(name, "rays", int(o["ok"].sum()), "iterations", int(o["iters"].sum()), "sampled states", m, "outside the domain", outside,
          "not ordinary", int((~d["ordinary"]).sum()), "excluded by the unit", int((~d["keep"]).sum()), "below the classes' radii", int((~d["covered"]).sum()))
    assert m > 1000 and outside <= rr.DOMAIN_CAP * m
    assert (o["attempts"] >= o["iters"]).all() and np.isin(o["event"][o["ok"]], (-1, 0, 1, 2)).all()


def test_only_the_far_observers_rays_reach_the_ghost_lane_phase():
    """RK4 steps of the oracle's rays against the thresholds at which a wavefront turns long (384 iterations in the direct
    schedule, a lane past 600 steps in the queue schedule): far_observer has wavefronts -- 64 consecutive rays of a batch call,
    8 x 8 tiles of a frame -- in which two rays of different length both run past either; no other case has a ray that long."""
    for name in rr.KERR_CASES:
        c = rr.CASES[name]
        al, th, rf = rr.rays(c, "oracle")
        steps = oracle.trace_batch_kerr(rr.M, c.a, c.r_obs, al, th, c.theta_obs, rr.lambda_max(c), rf, integrator="rk4")[3] // 4
        if name != "far_observer":
            assert steps.max() < 384, name
            continue
        batch, tiles = steps[:steps.size // 64 * 64].reshape(-1, 64), rr.frame_waves(c, steps)
        for long_steps in (384, 600):
            got = int(rr.ghost_phase_waves(batch, long_steps).sum()), int(rr.ghost_phase_waves(tiles, long_steps).sum())
            print("far_observer: wavefronts past", long_steps, "with lanes ending inside the phase:", got, "of", (batch.shape[0], tiles.shape[0]))
            assert min(got) > 0
    w = np.array([[700] * 63 + [100], [700] * 62 + [650, 100], [300] * 64, [700] * 64])
    assert rr.ghost_phase_waves(w, 600).tolist() == [False, True, False, False]
    t = rr.frame_waves(rr.CASES["far_observer"], np.arange(48 * 24))
    assert t.shape == (18, 64) and t[0, :9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 48] and t[1, 0] == 8 and t[6, 0] == 8 * 48


def test_dropped_refine_flags_are_reported_on_the_refine_rays():
    """The comparison on two oracle traces of near_axis, with and without the axis-refine flags: every refine ray differs (its
    base step halves), no other ray does."""
    c = rr.CASES["near_axis"]
    al, th, rf = rr.rays(c, "oracle")
    keys = ("fa", "winding", "status", "rhs_evals")
    run = lambda flags: dict(zip(keys, oracle.trace_batch_kerr(rr.M, c.a, c.r_obs, al, th, c.theta_obs, rr.lambda_max(c), flags, integrator="rk4")))  # noqa: E731
    bad = rr.differing(run(np.zeros_like(rf)), run(rf), count="rhs_evals")
    assert np.array_equal(bad, rf != 0) and bad.sum() == 126


def test_near_axis_has_retried_steps_in_the_oracle():
    o = rr.oracle_rays(rr.CASES["near_axis"])
    assert (o["attempts"] > o["iters"]).sum() >= 10


def _result(n=1000, seed=0):
    rng = np.random.default_rng(seed)
    status = rng.choice([-1, 0, 1], n).astype(np.int8)
    fa = np.where(status == 1, rng.uniform(0.0, np.pi, n), np.nan)
    steps = rng.integers(1, 5000, n)
    return dict(fa=fa, winding=rng.integers(0, 4, n), status=status, steps=steps, rhs_evals=(4 * steps).astype(np.uint32))


def test_comparison_reports_planted_differences():
    case = rr.CASES["ragged_1000"]
    want = _result()
    same = {k: v.copy() for k, v in want.items()}
    assert rr.explain(case, same, want, source="oracle") is None and not rr.differing(same, want).any()
    esc = np.nonzero(want["status"] == 1)[0]
    # one bit of fa, in float64 and in a frame's float32
    for dtype in (np.float64, np.float32):
        got = {k: v.copy() for k, v in want.items()}
        got["fa"] = got["fa"].astype(dtype)
        got["fa"][esc[7]] = np.nextafter(got["fa"][esc[7]], dtype(4.0))
        bad = rr.differing(got, want)
        assert bad.sum() == 1 and bad[esc[7]]
        msg = rr.explain(case, got, want, source="oracle")
        assert msg is not None and "1 of 1000 rays differ" in msg and f"entry {esc[7]}" in msg and "alpha=" in msg and "refine=" in msg
        assert f"steps={int(want['steps'][esc[7]])}" in msg
    # a float32 frame equals the replay rounded to float32
    got = dict({k: v.copy() for k, v in want.items()}, fa=want["fa"].astype(np.float32))
    assert not rr.differing(got, want).any()
    # off by one in steps / rhs_evals; status; winding; an angle on a ray that did not escape
    for key, count in (("steps", "steps"), ("rhs_evals", "rhs_evals"), ("winding", "steps"), ("status", "steps")):
        got = {k: v.copy() for k, v in want.items()}
        got[key][3] += 1
        bad = rr.differing(got, want, count=count)
        assert bad[3] and bad.sum() == 1, key
        assert "entry 3" in rr.explain(case, got, want, count=count, source="oracle")
    got = {k: v.copy() for k, v in want.items()}
    got["steps"][5] -= 1
    assert not rr.differing(got, want, count="rhs_evals").any() and rr.differing(got, want, count="steps")[5]
    cap = np.nonzero(want["status"] != 1)[0][0]
    both = {k: v.copy() for k, v in want.items()}
    both["fa"][cap] = 1.0
    got = {k: v.copy() for k, v in both.items()}
    assert rr.differing(got, both)[cap]     # not a NaN although the ray did not escape: both sides agreeing does not help
    # NaN payloads do not matter, signed zeros do
    got = {k: v.copy() for k, v in want.items()}
    got["fa"][cap] = -np.nan
    assert not rr.differing(got, want).any()
    z = dict(want, fa=np.where(np.arange(1000) == esc[0], 0.0, want["fa"]))
    got = dict({k: v.copy() for k, v in z.items()}, fa=np.where(np.arange(1000) == esc[0], -0.0, want["fa"]))
    assert rr.differing(got, z).sum() == 1
