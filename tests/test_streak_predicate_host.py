"""The far-field streak's per-step test (kerr_rk4_streak_loop, lt_device.hpp) sums fewer magnitudes for its
finiteness test than the predicate it replaced: the components that a range test of the same mask covers are left out.
Both forms are restated here in numpy float32 -- its add is the device's v_add_f32 rounding, and nothing contracts in
these sums -- and evaluated on a grid of edge values of the five components.  They must agree everywhere, in the
continue condition of both loops and in the per-lane `good` that the keep/discard selects and the return value use.
The parts of the predicate that did not change (lam <= lam_limit, min_r > r_cut, !(max_d > 0.25)) are ANDed into both
forms alike and are left out.  No GPU."""
import numpy as np
import pytest

F = np.float32
FLT_MAX = np.finfo(F).max
# a = 0.9, M = 1, r_obs = 50: 4 r_capture, 2 r_obs, and the band of the fixed-quadrant loop (M<float>::EQ_BAND_LO / HI)
RC4 = F(4 * 1.01 * (1 + np.sqrt(1 - 0.81)))
R_ESCAPE = F(100.0)
EQ_LO, EQ_HI = F(0.80), F(2.34)


def around(x, n=1):
    """x and its n float32 neighbours on either side"""
    out, lo, hi = [F(x)], F(x), F(x)
    for _ in range(n):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return out


def below(x, n):
    out = [F(x)]
    for _ in range(n):
        out.append(np.nextafter(out[-1], F(0)))
    return out


EDGES = [F(0.0), F(-0.0), F(1e-45), F(-1e-40), F(1.0), F(-1.0)] + around(2.0 ** 31) + [-F(2.0 ** 31)] + below(FLT_MAX, 3) + \
        [-FLT_MAX, F(FLT_MAX / 2), -F(FLT_MAX / 2), F(FLT_MAX / 3), F(np.inf), F(-np.inf), F(np.nan)]
# r and theta: inside and outside their ranges, on and next to every bound, and the edge values again
R_VALUES = around(RC4) + around(R_ESCAPE) + [F(6.0), F(50.0), F(99.0), F(5.0), F(150.0), -F(50.0)] + EDGES
TH_VALUES = around(EQ_LO) + around(EQ_HI) + [F(np.pi / 2), F(1.0), F(2.0), F(0.5), F(2.5), F(3.2), -F(1.5)] + EDGES


@pytest.fixture(scope="module")
def grid():
    r, th, ph, pr, pth = np.meshgrid(*(np.array(v, dtype=F) for v in (R_VALUES, TH_VALUES, EDGES, EDGES, EDGES)), indexing="ij")
    with np.errstate(over="ignore", invalid="ignore"):
        a = lambda x: np.abs(x)
        f5 = np.isfinite((((a(r) + a(th)) + a(ph)) + a(pr)) + a(pth))              # the replaced test: all five, left to right
        f4 = (((a(th) + a(ph)) + a(pr)) + a(pth)) <= FLT_MAX                       # general loop
        f3 = ((a(ph) + a(pr)) + a(pth)) <= FLT_MAX                                 # fixed-quadrant loop
        in_range = (r >= RC4) & (r < R_ESCAPE)
        band = (th > EQ_LO) & (th < EQ_HI)
    assert f5.dtype == bool and f5.size == len(R_VALUES) * len(TH_VALUES) * len(EDGES) ** 3
    return dict(f5=f5, f4=f4, f3=f3, in_range=in_range, band=band)


def test_grid_reaches_both_sides_of_every_test(grid):
    # the comparison below is empty talk unless each form is true somewhere and false somewhere, inside the ranges too
    g = grid
    for name in ("f5", "f4", "f3", "in_range", "band"):
        assert g[name].any() and not g[name].all(), name
    inside = g["in_range"] & g["band"]
    assert (inside & g["f5"]).any() and (inside & ~g["f5"]).any()
    # an angle that the band test rejects and the shorter sum does not see: the case the exit's full sum exists for
    assert (g["in_range"] & g["f3"] & ~g["f5"]).any()


def test_general_loop_predicate_is_the_old_one(grid):
    g = grid
    old = g["f5"] & g["in_range"]
    new = g["f4"] & g["in_range"]          # continue condition and per-lane `good` alike
    assert np.array_equal(old, new), np.argwhere(old != new)[:5]


def test_fixed_quadrant_loop_predicates_are_the_old_ones(grid):
    g = grid
    old_good = g["f5"] & g["in_range"]
    mask = g["f3"] & g["in_range"]
    # the continue condition: every lane good and inside the band
    assert np.array_equal(old_good & g["band"], mask & g["band"]), np.argwhere((old_good & g["band"]) != (mask & g["band"]))[:5]
    # the lane's `good` on leaving: the mask and the full sum
    assert np.array_equal(old_good, mask & g["f5"])
    # ... which the mask alone would not be
    assert not np.array_equal(old_good, mask)
