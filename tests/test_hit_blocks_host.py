"""The units and bounds of tests/hit_blocks.py, derived on the CPU from the reference alone: every K the GPU tests of the hit
times hold the device to (tests/test_gpu_hit_blocks.py), the bound on the two-term sum, and the conditions on the inputs."""
import numpy as np
import pytest

import disk
import disk_blocks as dk
import hit_blocks as hb
import step_blocks as sb
from oracle import oracle


def test_the_restatement_in_float64_is_the_reference_bit_for_bit():
    for spin, name, c in hb.rate_classes():
        y = c["y"]
        ref = disk.time_rates(c["M"], c["a"], c["L"], y[:, 0], y[:, 1], y[:, 2], y[:, 3])
        got = hb.rates_T(c["M"], c["a"], c["L"], y[:, 0], y[:, 1], y[:, 2], y[:, 3], np.float64)
        for g, r in zip(got, ref):
            assert np.array_equal(g, r, equal_nan=True), (spin, name)
    for spin, name, c in hb.step_classes(64):
        with np.errstate(all="ignore"):
            ref = disk.step_time(c["M"], c["a"], c["L"], c["y0"], c["y1"], c["h"], c["tau"])
        got = hb.step_time_T(c["M"], c["a"], c["L"], c["y0"], c["y1"], c["h"], c["tau"], np.float64)
        assert np.array_equal(got, ref, equal_nan=True), (spin, name)


@pytest.mark.parametrize("precision", [32, 64])
def test_k_of_the_rates(precision):
    T = hb.dtype_of(precision)
    worst = np.zeros(3)
    for spin, name, c in hb.rate_classes():
        y = c["y"]
        unit, keep = hb.rate_units(c["M"], c["a"], c["L"], y, precision)
        assert (~keep).mean() <= hb.EXCLUDED_CAP, (spin, name, (~keep).mean())
        ref = hb.rates_ld(c["M"], c["a"], c["L"], y)
        with np.errstate(all="ignore"):
            got = np.stack(hb.rates_T(c["M"], c["a"], c["L"], y[:, 0], y[:, 1], y[:, 2], y[:, 3], T), axis=1)
        e = (np.abs(got.astype(hb.LD) - ref).astype(np.float64) / unit)[keep]
        print(f"float{precision} rates, a = {spin:6}, {name:8s}: {np.round(e.max(axis=0), 2)} units; relative t' {np.max(np.abs(got[keep, 0] / ref[keep, 0].astype(np.float64) - 1)):.1e}")
        worst = np.maximum(worst, e.max(axis=0))
    print(f"float{precision} rates: worst {np.round(worst, 3)} units")
    assert int(np.ceil(worst.max())) == hb.k_rate(precision), worst


@pytest.mark.parametrize("precision", [32, 64])
def test_k_of_the_step_rule(precision):
    T = hb.dtype_of(precision)
    worst, rows = 0.0, 0
    for spin, name, c in hb.step_classes(precision):
        ref = c["ref"]
        keep = ref["keep"]
        out = ~keep
        print(f"float{precision} step rule, a = {spin:6}, {name:22s}: {int(out.sum())} of {out.size} rows left out")
        if name in hb.STARTS_INSIDE:
            # the one exemption, checked row by row: what these two classes lose beyond the cap is exactly the rows whose START
            # lies at or inside 1.001 r_plus (hit_blocks.STARTS_INSIDE says why they exist); every other row is under the cap
            inside = c["y0"][:, 0] <= 1.001 * dk.r_plus(c["M"], c["a"])
            assert inside.mean() <= hb.STARTS_INSIDE[name], (spin, name, inside.mean())
            assert (out & ~inside).sum() <= hb.EXCLUDED_CAP * out.size, (spin, name, int((out & ~inside).sum()))
        else:
            assert name.split("/")[1] in dk.UNSTABLE_CLASSES or out.mean() <= hb.EXCLUDED_CAP, (spin, name, out.mean())
        assert out.size == hb.N
        got = hb.step_time_T(c["M"], c["a"], c["L"], c["y0"], c["y1"], c["h"], c["tau"], T)
        e = (np.abs(got.astype(hb.LD) - ref["dt"]).astype(np.float64) / ref["unit"])[keep]
        by_tau = [e[(np.arange(keep.size) % 4 == k)[keep]].max() for k in range(4)]
        print(f"float{precision} step rule, a = {spin:6}, {name:22s}: {e.max():.2f} units (tau = {hb.TAUS}: {np.round(by_tau, 2)})")
        worst, rows = max(worst, float(e.max())), rows + int(keep.sum())
    print(f"float{precision} step rule: worst {worst:.3f} units on {rows} rows")
    assert rows > 18000
    assert int(np.ceil(worst)) == hb.k_dt(precision), worst


def test_edge_rows_of_the_reference():
    """h = 0 is 0 whatever the states (disk.step_time says so explicitly: 0 x NaN would be NaN); NaN in, NaN out."""
    c = hb.step_class("crossing", "ordinary", 0.9, 64)
    y0, y1 = c["y0"][:8].copy(), c["y1"][:8].copy()
    assert (disk.step_time(1.0, 0.9, c["L"][:8], y0, y1, 0.0, c["tau"][:8]) == 0.0).all()
    y0[::2, 0] = np.nan
    y1[1::2, 1] = np.nan
    with np.errstate(all="ignore"):
        assert np.isnan(disk.step_time(1.0, 0.9, c["L"][:8], y0, y1, c["h"][:8], c["tau"][:8])).all()
        assert (disk.step_time(1.0, 0.9, c["L"][:8], y0, y1, 0.0, c["tau"][:8]) == 0.0).all()


def test_rule_is_fifth_order():
    """The unit bounds rounding, not truncation: halving h divides the rule's distance from a fine quadrature of the same cubic
    path by ~32, and at the tracer's own h that distance is orders of magnitude above the float64 unit."""
    c = hb.step_class("step", "mid", 0.9, 64)
    M, a, L = c["M"], c["a"], c["L"]
    st = np.stack([c["y0"][:, 0], c["y0"][:, 1], np.zeros(hb.N), c["y0"][:, 2], c["y0"][:, 3]], axis=1)[:64]
    L = L[:64]

    def err(h):
        y1 = oracle.rk4_step_kerr(st, L, h, M, a)[0]
        fine, y = np.zeros(64, dtype=hb.LD), st
        for _ in range(16):  # the same step as 16 of h / 16: truncation 16 / 16^5 of the one step's
            yn = oracle.rk4_step_kerr(y, L, h / 16, M, a)[0]
            fine += hb.step_time_ld(M, a, L, y[:, [0, 1, 3, 4]], yn[:, [0, 1, 3, 4]], h / 16, 1.0, 64)["dt"]
            y = yn
        one = hb.step_time_ld(M, a, L, st[:, [0, 1, 3, 4]], y1[:, [0, 1, 3, 4]], h, 1.0, 64)
        return np.abs(one["dt"] - fine).astype(np.float64), one["unit"]

    e1, unit = err(1.0)
    e2, _ = err(0.5)
    ratio = np.median(e1 / e2)
    print(f"truncation at h = 1: median {np.median(e1):.2e} = {np.median(e1 / unit):.1e} float64 units; h -> h / 2 divides it by {ratio:.1f}")
    assert 20.0 < ratio < 48.0
    assert np.median(e1 / unit) > 1e3


# ---- the two-term sum -------------------------------------------------------------------------------------------------------------------
_RAYS = {}


def oracle_ray_terms(a, n_rays=64, n_steps=700, r_obs=600.0):
    """float32 RK4 rays of the oracle from r_obs toward the hole, iteration by iteration (oracle.rk4_iteration, float32), and
    the float32 terms the rule adds per counted step (hb.step_time_T on the step's ends): -> (terms (k, n) float64 of float32
    values, NaN where nothing was counted; counted (n,))."""
    if a in _RAYS:
        return _RAYS[a]
    b = np.linspace(3.0, 14.0, n_rays)
    st = np.zeros((n_rays, 5))
    L = np.empty(n_rays)
    for i, bi in enumerate(b):
        ok, s, _, pp = oracle.kerr_ic(1.0, a, r_obs, np.arctan(bi / r_obs), 0.3 + 0.09 * i, 1.4)
        assert ok
        st[i], L[i] = s, pp
    st, L = sb.f32(st), sb.f32(L)
    lam = np.zeros(n_rays)
    terms = np.full((n_steps, n_rays), np.nan)
    alive = np.ones(n_rays, dtype=bool)
    for k in range(n_steps):
        o = oracle.rk4_iteration(st, L, lam, 1.0, a, r_obs=r_obs, lambda_max=5000.0, f32=True)
        new = o["state"].astype(np.float64)
        moved = alive & (o["event"] == 4) & (o["lam"] != lam.astype(np.float32))
        h = (o["lam"].astype(np.float64) - lam)
        cols = [0, 1, 3, 4]
        with np.errstate(all="ignore"):
            dt = hb.step_time_T(1.0, a, L, st[:, cols], new[:, cols], sb.f32(h), 1.0, np.float32).astype(np.float64)
        terms[k] = np.where(moved, dt, np.nan)
        alive &= o["event"] == 4
        st, lam = np.where(alive[:, None], new, st), np.where(alive, o["lam"].astype(np.float64), lam)
    _RAYS[a] = terms, (~np.isnan(terms)).sum(axis=0)
    return _RAYS[a]


@pytest.mark.parametrize("a", [0.9, 0.998])
def test_two_term_sum_is_within_its_bound_and_the_plain_sum_is_not(a):
    terms, counted = oracle_ray_terms(a)
    assert (counted >= hb.MIN_SUM_STEPS).all(), counted.min()   # what test_gpu_hit_blocks.py's sum rays rely on
    hi, lo = hb.two_sum_replay(terms, np.float32)
    part = terms[-1] * 0.0
    part = np.where(np.isnan(part), 0.0, part)
    stored = (hi + (lo + part.astype(np.float32))).astype(np.float64)
    exact = np.nansum(terms.astype(hb.LD), axis=0)
    bound = hb.sum_bound(terms, part, 32)
    e2 = np.abs(stored.astype(hb.LD) - exact).astype(np.float64)
    e1 = np.abs(hb.plain_sum_replay(terms, np.float32).astype(hb.LD) - exact).astype(np.float64)
    u_tot = hb.U32 * np.abs(exact).astype(np.float64)
    print(f"a = {a}: {counted.min()} ... {counted.max()} counted steps; two-term sum {np.max(e2 / u_tot):.2f} u |total| worst "
          f"(bound {np.max(bound / u_tot):.3f}), plain sum median {np.median(e1 / u_tot):.2f}, misses the bound on {int((e1 > bound).sum())} of {e1.size}")
    assert (e2 <= bound).all()
    assert (e1 > bound).mean() >= 0.5
    # a dropped t_lo is the plain sum of the hi parts: it misses the bound where the plain sum does
    assert (np.abs(hi.astype(hb.LD) - exact).astype(np.float64) > bound).mean() >= 0.5


# ---- the polarization rule where it is hardest --------------------------------------------------------------------------------------------
def test_float64_error_of_the_polarization_rule_per_class():
    """What numpy's float64 is off from the same statement in longdouble, per class: the figures hit_blocks.POL_F64_ERR writes
    down (this machine's libm may move them a little: within a factor 2 either way), and what the classes have to contain."""
    for name in hb.POL_CLASSES:
        c = hb.pol_class(name)
        assert c["hit"].shape == (hb.N, 3) and np.isfinite(c["hit"]).all() and np.isfinite(c["cam"]).all()
        ref = hb.pol_reference(c, hb.LD)
        assert np.isfinite(ref.astype(np.float64)).all(), name
        e = float(np.max(np.abs(hb.pol_reference(c).astype(hb.LD) - ref)))
        print(f"{name:10s}: numpy float64 against longdouble {e:.2e} (written down {hb.POL_F64_ERR[name]:.2e})")
        assert hb.POL_F64_ERR[name] / 2 <= e <= 2 * hb.POL_F64_ERR[name], (name, e)
    ri = dk.isco(1.0, 0.998)
    r = hb.pol_class("isco_band")["hit"][:, 0]
    assert (r >= ri).all() and (r <= 1.001 * ri).all()
    assert (hb.pol_class("pth0")["hit"][:, 2] == 0).all() and (hb.pol_class("pr0")["hit"][:, 1] == 0).all() and (hb.pol_class("L0")["L"] == 0).all()
    assert hb.pol_class("mass")["M"] == 2.5 and hb.pol_class("obs_far")["r_obs"] == 1e4 and hb.pol_class("obs_near")["r_obs"] < 4.4


def test_the_switch_rows_sit_a_factor_four_either_side():
    c = hb.pol_class("a998")
    rows = np.arange(64)
    for delta, lit in ((2e-12, True), (5e-13, False)):
        _, s2 = hb.tilted_fields(c, rows, np.full(64, delta))
        s2 = s2.astype(np.float64)
        assert (s2 >= 3.9 * hb.POL_S2_SWITCH).all() if lit else (s2 <= hb.POL_S2_SWITCH / 3.9).all(), (delta, s2.min(), s2.max())
