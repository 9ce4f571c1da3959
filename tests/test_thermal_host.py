"""The thermal continuum on the CPU: the Novikov-Thorne flux against quadrature of its defining integral, the numpy
statements of the rule (disk.thermal_coeffs / thermal_spectrum / shade_thermal) against a longdouble reference, the table,
the struct, the bindings, the command line and the refusals that need no device.  tests/test_gpu_thermal.py holds the
kernels to the same reference with the same bounds; the cases, records, emitters, frequencies and the reference are here.

The flux's bound, derived.  novikov_thorne_flux adds the six terms of Page & Thorne's bracket (disk.novikov_thorne_terms);
towards the ISCO they cancel, so the sum's relative error is the terms' absolute errors over the bracket.  A term is a
product of a coefficient -- a handful of operations on the roots, each within a few ulp -- and a logarithm within an ulp, so
each term is within 64 ulp of itself with room, the prefactor's few ulp included:
    |F - F_ref| / F_ref <= 64 2^-53 sum|terms| / |bracket| + the quadrature's own relative error estimate.
The reference is F = (1 / (4 pi r)) (-Omega,r) (E - Omega L)^-2 int_{r_isco}^{r} (E - Omega L) L,r dr with E, L, Omega of the
circular equatorial orbit in +phi and their derivatives in closed form, in 30-digit arithmetic (mpmath).

The numpy statements' bound, derived (the GPU section's).  The reference takes c of every emitting slot from
disk.thermal_coeffs -- steps 1 to 4 are IEEE-exact operations, held to the bit on the GPU -- and x = nu c rounded to float64,
and computes A / expm1(x), the sums and nu^3 in longdouble.  A float64 term differs from it by expm1's E ulp, the division's
half and the rounding of A (its own half ulp: 2 covers both); a sum of n non-negative terms adds n 2^-53 of itself; nu^3
adds three roundings.  Terms with x >= 700 count in full: float64 expm1 may overflow there and a tiny quotient may flush,
where longdouble does neither.  E = 2: no documentation of the device library's expm1 is installed with it, and glibc's is
within 1 ulp.
    |S - S_ref| <= nu^3 ((E + 2) 2^-53 sum_{x < 700} t + sum_{x >= 700} t + n 2^-53 sum t) + 3 2^-53 S_ref.

F at a = 1e-9 against a = 0.  The flux depends on the spin to first order (6e-9 relative between the two at r = 7 M), so the
two are not within the rounding bound of each other; what the bound does cover is the x2 term, which is 0 at a = 0 and
a* / 6 ln(...) near it.  The test takes the mean of F at a = +1e-9 and a = -1e-9, which removes the first order, and holds it
against F at a = 0 to twice the bound (both sides are rounded) plus the second order in the spin, written out in the test.

Steps 1 to 4 on their own (test_coefficients_against_an_independent_restatement).  coefficients_ref restates them in plain
longdouble from the header's words, not from disk.thermal_coeffs: the node spacing h = (r_max - r_min) / (n_r - 1), the
interval by floor((r - r_min) / h), F by the chord, T = t_max F^0.25 by a power, c = 1 / (g f_col T).  The float64 statement
rounds inv_dr twice and v twice, so w is off by at most 4 u v <= 4 u n_r and F by dF = u (4 n_r |f1 - f0| + 2 (|f0| + |f1|))
(the subtraction and the fma included); the two square roots pass a quarter of dF / F on and add one u, t_max T one, g f_col,
its product with T and the quotient three:  |c - c_ref| / c_ref <= 8 u + dF / (4 F) to first order, taken with a factor
1.01 where dF / F < 1e-3.  Slots whose F lies within dF of 0 may emit in one statement and not in the other and are left
out of both comparisons; everywhere else the two must agree on which slots emit.  The reference, the closure's
temperatures and the GPU tests' closure all take T from this restatement, so a misreading of the rule shared by the numpy
statement and the kernel fails here.

MEASURED here, the figures the tests print:
    flux against quadrature: worst 0.019 of the bound, at a / M = 0.998, M = 2.5, r = 3 r_isco (bound 9.4e-14); the
        quadrature's own estimate is below 2e-35 everywhere;
    efficiency: 0.057190958418 at a = 0 and 0.155752991994 at a / M = 0.9, within 1.1e-16 of 1 - E(r_isco) (tolerances 5e-15, 2e-14);
    interpolation of the 4096-node table at mid-nodes: worst relative error 0.985 at the first interval (F is quadratic there
        and 0 at the node, so the chord is twice the curve), 0.999 of h^2 max|F''| / 8; beyond the 16th interval 5.2e-4;
    steps 1 to 4 against the independent restatement: c within 0.37 of its bound on strip, mid, big and one, coarse and
        4096-node tables (largest bound 1.8e-10, at the table's foot); the same slots emit;
    numpy statements against longdouble: at most 0.38 of the bound (spectra; the single pixel) and 0.998 (band images: the
        float32 rounding is most of that bound);
    Stefan-Boltzmann closure on a 400-point grid: 2.2e-16 relative (bound 1e-9).
"""
import ctypes

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES, records
from test_hotspot_records_host import synth

LD = np.longdouble
U = LD(2.0) ** -53
E_EXPM1 = 2                     # ulp of the float64 expm1 under test (header above)
T_MAX, F_COL, EXPOSURE = 0.75, 1.7, 0.05
_THERMAL_RECORDS, _REFERENCES = {}, {}


# ---- cases: records, emitters, frequencies ---------------------------------------------------------------------------------------
def thermal_records(name):
    """(hits, n_hits) of a case of test_diskmap_host: a copy of its records in which about one stored slot in 16 has a g
    that emits nothing -- 0, negative, NaN, in turn -- so that every pixel walk meets them.  Made once."""
    if name not in _THERMAL_RECORDS:
        hits, n_hits, _ = records(name)
        hits = hits.copy()
        c = CASES[name]
        pick = np.random.default_rng(c.seed + 7).random(hits.shape[:3]) < (1 / 16 if hits.size > 4 else 0)
        kind = np.arange(pick.sum()) % 3
        g = hits[..., 2]
        g[pick] = np.choose(kind, [0.0, -0.5, np.nan]).astype(np.float32)
        _THERMAL_RECORDS[name] = (hits, n_hits)
    return _THERMAL_RECORDS[name]


def make_thermal(name, split=False, n_r=37, zero=(9, 14), exposure=EXPOSURE):
    """The emitter of a case: the Novikov-Thorne profile of the case's hole on n_r nodes over a range strictly inside the
    records' [r_isco, r_out], so that slots fall off both ends, with the nodes zero[0] ... zero[1] set to 0 -- a stretch
    without light, whose neighbouring intervals interpolate towards 0 -- and one node negative."""
    c = CASES[name]
    r_in = float(diskmod.isco(c.M, c.a))
    lo, hi = r_in + 0.5 * c.M, c.r_out - 3.0 * c.M
    nodes = lo + np.arange(n_r) * (hi - lo) / (n_r - 1)
    flux = diskmod.novikov_thorne_flux(c.M, c.a, nodes)
    flux = flux / flux.max()
    flux[zero[0]:zero[1]] = 0.0
    flux[zero[0] + 1] = -0.25
    return diskmod.ThermalDisk(flux, lo, hi, t_max=T_MAX, f_col=F_COL, exposure=exposure, split_orders=split)


def frequencies(n, seed=3):
    """n frequencies, log-spaced from 1e-3 t_max to 600 t_max and shuffled: nu c reaches several hundred on the emitting slots
    (c >= 1 / (1.4 f_col t_max)), and beyond 700 on the cool ones."""
    nu = T_MAX * np.exp(np.linspace(np.log(1e-3), np.log(600.0), n)) if n > 1 else np.array([T_MAX * 40.0])
    return np.random.default_rng(seed).permutation(nu)


class ThermalReference:
    """The longdouble reference and its bound (header above) for one set of records and one emitter."""

    def __init__(self, hits, n_hits, thermal):
        self.A, self.c, self.emits = diskmod.thermal_coeffs(hits, n_hits, thermal)
        self.m = self.c.shape[-1]

    def _terms(self, nu, c):
        x = np.float64(nu) * c                                            # rounded to float64, as the rule says
        with np.errstate(over="ignore"):
            t = LD(self.A) / np.expm1(x.astype(LD))
        return x, t

    @staticmethod
    def _sum_and_bound(nu, x, t, axis=None):
        """nu^3 sum t and its bound, over all entries or along `axis` (entries that do not emit carry t = 0)."""
        n3 = LD(nu) ** 3
        total = t.sum(axis=axis)
        n = t.size if axis is None else t.shape[axis]
        warm = np.where(x < 700.0, t, LD(0)).sum(axis=axis)
        bound = n3 * ((E_EXPM1 + 2) * U * warm + (total - warm) + n * U * total) + 3 * U * n3 * total
        return n3 * total, bound

    def spectrum(self, nu, split):
        """-> (value, bound), each (planes, n_freq) longdouble."""
        planes = self.m if split else 1
        val, bnd = np.zeros((planes, len(nu)), dtype=LD), np.zeros((planes, len(nu)), dtype=LD)
        for p in range(planes):
            c = self.c[..., p][self.emits[..., p]] if split else self.c[self.emits]
            for k, f in enumerate(nu):
                val[p, k], bnd[p, k] = self._sum_and_bound(f, *self._terms(f, c))
        return val, bnd

    def bands(self, nu):
        """-> (value, bound), each (n_bands, R, W) longdouble; the bound without the float32 rounding."""
        val, bnd = [], []
        for f in nu:
            x, t = self._terms(f, np.where(self.emits, self.c, 1.0))
            v, b = self._sum_and_bound(f, x, np.where(self.emits, t, LD(0)), axis=-1)
            val.append(v)
            bnd.append(b)
        return np.stack(val), np.stack(bnd)


def coefficients_ref(hits, n_hits, td):
    """Steps 1 to 4 restated from the header in plain longdouble, independently of disk.thermal_coeffs -> (T, c, emits, F, dF),
    each (..., max_images): the physical temperature t_max F^(1/4) (a frequency), c = 1 / (g f_col T), which slots emit, the
    interpolated flux and the float64 statement's error bound on it (header above).  T and c are 0 where nothing emits."""
    h32 = np.asarray(hits, dtype=np.float32)
    m = h32.shape[-2]
    r, g = h32[..., 0].astype(LD), h32[..., 2].astype(LD)
    stored = (np.cumprod(~np.isnan(h32[..., 0]), axis=-1).sum(axis=-1) if n_hits is None else np.minimum(np.asarray(n_hits, dtype=np.int64), m))
    with np.errstate(invalid="ignore"):
        on = (stored[..., None] > np.arange(m)) & (g > 0) & (r >= LD(td.r_min)) & (r <= LD(td.r_max))
    spacing = (LD(td.r_max) - LD(td.r_min)) / LD(td.n_r - 1)
    at = np.where(on, (r - LD(td.r_min)) / spacing, LD(0))
    i0 = np.minimum(np.floor(at).astype(np.int64), td.n_r - 2)
    f0, f1 = td.flux[i0].astype(LD), td.flux[i0 + 1].astype(LD)
    F = f0 + (at - i0) * (f1 - f0)
    dF = U * (4 * td.n_r * np.abs(f1 - f0) + 2 * (np.abs(f0) + np.abs(f1)))
    on = on & (F > 0)
    T = np.where(on, LD(td.t_max) * np.where(on, F, LD(1)) ** LD(0.25), LD(0))
    c = np.where(on, 1 / np.where(on, g * LD(td.f_col) * T, LD(1)), LD(0))
    return T, c, on, F, dF


def reference(name, counts=True):
    """The ThermalReference of a case's records and its unsplit emitter (the planes only select), made once."""
    if (name, counts) not in _REFERENCES:
        hits, n_hits = thermal_records(name)
        _REFERENCES[name, counts] = ThermalReference(hits, n_hits if counts else None, make_thermal(name))
    return _REFERENCES[name, counts]


def excess(got, want, bound):
    """The largest |got - want| in units of its bound (0 where both the difference and the bound are 0)."""
    d = np.abs(np.asarray(got).astype(LD) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(d == 0, LD(0), d / bound)
    return float(q.max())


# ---- 1. the Novikov-Thorne flux ------------------------------------------------------------------------------------------------
SPINS = (0.0, 1e-9, 0.5, 0.9, 0.998, -0.7)


def nt_quadrature(M, astar, r):
    """(F, relative error estimate) of the defining integral in 30-digit arithmetic, derivatives in closed form."""
    import mpmath as mp
    with mp.workdps(30):
        M, a, r = mp.mpf(M), mp.mpf(astar) * mp.mpf(M), mp.mpf(r)
        sM = mp.sqrt(M)
        x = abs(a) / M
        z1 = 1 + mp.cbrt(1 - x * x) * (mp.cbrt(1 + x) + mp.cbrt(1 - x))
        z2 = mp.sqrt(3 * x * x + z1 * z1)
        r_in = M * (3 + z2 - (-1 if a < 0 else 1) * mp.sqrt((3 - z1) * (3 + z1 + 2 * z2)))
        P = lambda s: s ** mp.mpf(1.5) - 3 * M * mp.sqrt(s) + 2 * a * sM
        dP = lambda s: mp.mpf(1.5) * mp.sqrt(s) - mp.mpf(1.5) * M / mp.sqrt(s)
        D = lambda s: s ** mp.mpf(0.75) * mp.sqrt(P(s))
        dD = lambda s: mp.mpf(0.75) * s ** mp.mpf(-0.25) * mp.sqrt(P(s)) + s ** mp.mpf(0.75) * dP(s) / (2 * mp.sqrt(P(s)))
        E = lambda s: (s ** mp.mpf(1.5) - 2 * M * mp.sqrt(s) + a * sM) / D(s)
        N = lambda s: s * s - 2 * a * sM * mp.sqrt(s) + a * a
        L = lambda s: sM * N(s) / D(s)
        dL = lambda s: sM * ((2 * s - a * sM / mp.sqrt(s)) * D(s) - N(s) * dD(s)) / D(s) ** 2
        Om = lambda s: sM / (s ** mp.mpf(1.5) + a * sM)
        dOm = lambda s: -mp.mpf(1.5) * sM * mp.sqrt(s) / (s ** mp.mpf(1.5) + a * sM) ** 2
        integral, err = mp.quad(lambda s: (E(s) - Om(s) * L(s)) * dL(s), [r_in, r], error=True)
        F = -dOm(r) / (4 * mp.pi * r) / (E(r) - Om(r) * L(r)) ** 2 * integral
        return F, err / abs(integral)


def flux_bound(M, a, r):
    """64 2^-53 sum|terms| / |bracket| at radii r (header above), float64."""
    terms = diskmod.novikov_thorne_terms(M, a, r)
    return 64.0 * 2.0 ** -53 * np.abs(terms).sum(axis=0) / np.abs(terms.sum(axis=0))


def test_flux_against_the_defining_integral():
    worst, where, worst_quad = 0.0, None, 0.0
    for M in (1.0, 2.5):
        for astar in SPINS:
            a = astar * M
            r_in = float(diskmod.isco(M, a))
            for r in (1.001 * r_in, 1.3 * r_in, 3.0 * r_in, 50.0 * M):
                want, quad_err = nt_quadrature(M, astar, r)
                got = float(diskmod.novikov_thorne_flux(M, a, r))
                bound = float(flux_bound(M, a, np.float64(r))) + float(quad_err)
                q = abs(float((got - want) / want)) / bound
                worst_quad = max(worst_quad, float(quad_err))
                if q > worst:
                    worst, where = q, (astar, M, r / r_in, bound)
                assert want > 0 and q <= 1, (astar, M, r, got, float(want), bound)
    print(f"flux against quadrature: worst {worst:.3f} of the bound at a/M = {where[0]}, M = {where[1]}, r = {where[2]:.4g} r_isco "
          f"(bound {where[3]:.2e}); largest quadrature estimate {worst_quad:.1e}")


def test_flux_is_continuous_in_the_spin_at_zero():
    """The x2 term near a = 0 (header: the mean of +-1e-9 against 0, to the flux's own bound)."""
    for M in (1.0, 2.5):
        r = diskmod.isco(M, 0.0) * np.array([1.001, 1.3, 3.0, 50.0 / 6.0])
        mean = 0.5 * (diskmod.novikov_thorne_flux(M, 1e-9 * M, r) + diskmod.novikov_thorne_flux(M, -1e-9 * M, r))
        zero = diskmod.novikov_thorne_flux(M, 0.0, r)
        # (r is 1.001 r_isco of a = 0 and within 1e-9 of that for the neighbours: all three lie outside their ISCO.)
        # Rounding: the mean's two evaluations are each within the bound, so is their mean, and F(0) is: twice the bound.
        # What the mean leaves of the physics is second order in the spin: near the ISCO F goes as (r - r_isco)^2 and r_isco
        # moves by 3.27 M per unit a*, so F changes by (3.27e-9 M / (r - r_isco))^2 of itself; elsewhere by some 1e-18.
        second = (3.27e-9 * M / (r - diskmod.isco(M, 0.0))) ** 2 + 1e-17
        assert np.all(zero > 0) and np.all(np.abs(mean - zero) <= (2 * flux_bound(M, 0.0, r) + second) * zero)
        assert diskmod.novikov_thorne_terms(M, 0.0, r)[4].tolist() == [0.0] * 4       # the x2 term itself, at its limit


def test_flux_edges_and_far_field():
    for M in (1.0, 2.5):
        for astar in SPINS:
            a = astar * M
            r_in = float(diskmod.isco(M, a))
            assert diskmod.novikov_thorne_flux(M, a, r_in) == 0.0 and diskmod.novikov_thorne_flux(M, a, 0.5 * r_in) == 0.0
            r = r_in * np.exp(np.linspace(0.0, np.log(1e4), 2001))
            F = diskmod.novikov_thorne_flux(M, a, r)
            assert np.all(F >= 0.0) and np.all(F[1:] > 0.0)
            far = M * np.array([100.0, 1e3, 1e5])
            left = 1.0 - diskmod.novikov_thorne_flux(M, a, far) * 8.0 * np.pi * far ** 3 / (3.0 * M)
            assert np.all(left > 0.0) and np.all(left <= 3.0 * np.sqrt(r_in / far)), (astar, left / np.sqrt(r_in / far))


@pytest.mark.parametrize("astar,eta", [(0.0, 0.0572), (0.9, 0.1558)])
def test_flux_radiates_the_binding_energy(astar, eta):
    """int 4 pi r^2 E F d ln r = 1 - E(r_isco): both faces' luminosity at infinity per unit accretion rate.  In s = r^-1/2 the
    integrand is smooth down to s = 0 (it tends to 3 M s); the tolerance is the quadrature's stated error plus the flux's
    own bound carried through the same integral."""
    from scipy.integrate import quad
    M = 1.0
    a = astar * M
    r_in = float(diskmod.isco(M, a))
    E = lambda r: (r ** 1.5 - 2 * M * r ** 0.5 + a) / (r ** 0.75 * np.sqrt(r ** 1.5 - 3 * M * r ** 0.5 + 2 * a))

    def integrand(s, err=False):
        r = 1.0 / (s * s)
        if r <= r_in:
            return 0.0
        F = float(diskmod.novikov_thorne_flux(M, a, r))
        if err:
            F *= float(flux_bound(M, a, np.float64(r)))
        return 4.0 * np.pi * r * r * E(r) * F * 2.0 / s

    s_in = r_in ** -0.5
    total, est = quad(integrand, 0.0, s_in, epsabs=0, epsrel=1e-13, limit=400)
    carried, _ = quad(lambda s: integrand(s, True), 0.0, s_in * (1 - 1e-9), epsabs=0, epsrel=1e-6, limit=400)
    want = 1.0 - E(r_in)
    print(f"a/M = {astar}: efficiency {total:.12f}, 1 - E_isco {want:.12f}, difference {total - want:.1e}, tolerance {est + carried:.1e}")
    assert abs(total - want) <= est + carried and abs(want - eta) < 5e-5


# ---- 2. the table ----------------------------------------------------------------------------------------------------------------
def test_novikov_thorne_table():
    M, a, r_out = 1.0, 0.9, 20.0
    td = diskmod.ThermalDisk.novikov_thorne(M, a, r_out, t_max=0.75, f_col=1.7)
    assert td.n_r == 4096 and td.flux[0] == 0.0 and td.flux.max() == 1.0 and (td.t_max, td.f_col, td.exposure) == (0.75, 1.7, 1.0)
    assert td.r_min == float(diskmod.isco(M, a)) and td.r_max == r_out and td.nodes()[0] == td.r_min and abs(td.nodes()[-1] - r_out) < 1e-12
    peak = int(np.argmax(td.flux))
    assert 0 < peak < td.n_r - 1 and np.all(np.diff(td.flux[:peak + 1]) > 0) and np.all(np.diff(td.flux[peak:]) < 0)
    # interpolation at the mid-nodes against the closed form: the linear-interpolation bound h^2 max|F''| / 8 per interval,
    # F'' from the closed form by a central second difference at a sixteenth of the node spacing, the maximum over the
    # interval's ends, middle and quarter points (F'' is monotone on an interval except around its zero, where it is small)
    norm = diskmod.novikov_thorne_flux(M, a, td.nodes()).max()
    F = lambda r: diskmod.novikov_thorne_flux(M, a, r) / norm
    h = (td.r_max - td.r_min) / (td.n_r - 1)
    mid = td.nodes()[:-1] + 0.5 * h
    interp = diskmod.fma(0.5, td.flux[1:] - td.flux[:-1], td.flux[:-1])   # step 3 of the rule at w = 1/2
    e = h / 16.0
    pts = np.stack([td.nodes()[:-1] + k * h / 4.0 for k in range(5)])
    pts = np.clip(pts, td.r_min + 2 * e, None)
    second = np.abs((F(pts + e) - 2.0 * F(pts) + F(pts - e)) / (e * e)).max(axis=0)
    bound = h * h * second / 8.0 * (1 + 1e-3) + 1e-15
    err = np.abs(interp - F(mid))
    rel = err / F(mid)
    print(f"4096-node table at mid-nodes: worst relative error {rel.max():.2e} at interval {int(np.argmax(rel))}, {float((err / bound).max()):.3f} of "
          f"h^2 max|F''| / 8; beyond the 16th interval {rel[16:].max():.1e}")
    assert np.all(err <= bound)
    for bad in (dict(flux=[1.0]), dict(r_min=0.0), dict(r_max=2.0), dict(t_max=0.0), dict(f_col=-1.0), dict(exposure=float("nan")),
                dict(flux=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            diskmod.ThermalDisk(**{**dict(flux=[0.0, 1.0], r_min=3.0, r_max=9.0), **bad})


def test_fma_is_one_rounding():
    """disk.fma against exact rational arithmetic, on products that nearly cancel their addend and on plain ones."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    a, b, c = rng.uniform(-1, 1, (3, 6000))
    c[:3000] = -(a * b)[:3000] * (1 + rng.uniform(-4e-16, 4e-16, 3000))
    c[3000:3500] = (a * b)[3000:3500] * 2.0 ** 53                          # the product decides a tie
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(diskmod.fma(a, b, c), want) and np.count_nonzero(a * b + c != want) > 1000


# ---- 3. the numpy statements against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_freq,split,counts", [("big", 5, True, True), ("mid", 16, False, True), ("strip", 64, True, False),
                                                      ("strip", 257, False, True), ("one", 1, False, True), ("one", 64, True, False)])
def test_numpy_spectrum_against_the_reference(name, n_freq, split, counts):
    hits, n_hits = thermal_records(name)
    nu = frequencies(n_freq)
    got = diskmod.thermal_spectrum(hits, n_hits if counts else None, make_thermal(name, split), nu)
    want, bound = reference(name, counts).spectrum(nu, split)
    assert got.shape == want.shape == (CASES[name].m if split else 1, n_freq)
    q = excess(got, want, bound)
    print(f"{name} {n_freq} frequencies, split {split}: numpy statement against longdouble, largest difference {q:.3f} of its bound")
    assert q <= 1 and np.all(want[:, np.argsort(nu)[:n_freq // 2 + 1]].sum(axis=0) > 0)


@pytest.mark.parametrize("name,n_bands", [("mid", 3), ("strip", 16), ("one", 2)])
def test_numpy_bands_against_the_reference(name, n_bands):
    hits, n_hits = thermal_records(name)
    nu = frequencies(n_bands, seed=5)
    got = diskmod.shade_thermal(hits, n_hits, make_thermal(name), nu)
    want, bound = reference(name).bands(nu)
    assert got.shape == (n_bands, CASES[name].R, CASES[name].W) and got.dtype == np.float32
    q = excess(got, want, bound + LD(2.0) ** -24 * want + LD(1e-45))      # (one rounding to float32; its subnormal step)
    dark = ~reference(name).emits.any(axis=-1)
    print(f"{name} {n_bands} bands: numpy statement against longdouble, largest difference {q:.3f} of its bound; {int(dark.sum())} dark pixels")
    assert q <= 1
    assert np.all(got[:, dark] == 0.0) and not np.any(np.signbit(got)) and not np.any(np.isnan(got))


@pytest.mark.parametrize("name,table", [("strip", "coarse"), ("mid", "coarse"), ("mid", "fine"), ("big", "fine"), ("one", "coarse")])
def test_coefficients_against_an_independent_restatement(name, table):
    """disk.thermal_coeffs -- which the reference above and the kernels are held to -- against coefficients_ref, at the records'
    own off-node radii, g from 0.15 to 1.4 and f_col = 1.7 (header: the bound, and the slots left out)."""
    c_ = CASES[name]
    hits, n_hits = thermal_records(name)
    td = make_thermal(name) if table == "coarse" else diskmod.ThermalDisk.novikov_thorne(c_.M, c_.a, c_.r_out - c_.M, t_max=T_MAX, f_col=F_COL,
                                                                                         exposure=EXPOSURE)
    for counts in (n_hits, None):
        A, c, emits = diskmod.thermal_coeffs(hits, counts, td)
        T, c_ref, on, F, dF = coefficients_ref(hits, counts, td)
        assert A == EXPOSURE / F_COL ** 4 or abs(A / (EXPOSURE / F_COL ** 4) - 1) <= 4 * float(U)
        sure = np.abs(F) > dF                                             # (elsewhere F's sign is within the statement's rounding)
        assert np.array_equal(emits[sure], on[sure]) and (~sure & (emits | on)).sum() <= 0.01 * (emits | on).sum()
        both = emits & on & (dF < 1e-3 * F)
        rel = np.abs(c[both].astype(LD) - c_ref[both]) / c_ref[both]
        bound = 8 * U + 1.01 * dF[both] / (4 * F[both])
        assert both.sum() >= (1 if hits.size == 4 else 0.2 * emits.size) and both.sum() >= 0.99 * (emits & on).sum()
        print(f"{name}, {table} table, counts {counts is not None}: c of {int(both.sum())} slots against the restatement, largest difference "
              f"{float((rel / bound).max()):.3f} of its bound (largest bound {float(bound.max()):.1e})")
        assert np.all(rel <= bound)
        g = hits[..., 2].astype(LD)[both]
        assert np.all(np.abs(1 / (c[both].astype(LD) * g * LD(F_COL)) - T[both]) <= bound * T[both])    # c carries the temperature


def test_slots_that_emit_nothing_are_exact_zeros():
    hits, n_hits = synth(6, 9, 3, 5, 2.4, 20.0)
    n_hits[:] = 3
    hits[..., 0] = np.random.default_rng(1).uniform(4.0, 12.0, hits.shape[:3])
    hits[..., 2] = 0.8
    td = diskmod.ThermalDisk([0.5, 1.0, 0.0, 0.0, -1.0, 0.25], 4.0, 12.0, t_max=T_MAX)
    nu = frequencies(7)
    warm = nu < 10 * T_MAX                                                # (beyond, the quotients underflow)
    assert np.all(diskmod.thermal_spectrum(hits, n_hits, td, nu)[:, warm] > 0)
    for change in ("g0", "gneg", "gnan", "rlow", "rhigh", "rnan", "dark"):
        h = hits.copy()
        if change == "g0": h[..., 2] = 0.0
        if change == "gneg": h[..., 2] = -0.8
        if change == "gnan": h[..., 2] = np.nan
        if change == "rlow": h[..., 0] = np.nextafter(np.float32(4.0), np.float32(0.0))
        if change == "rhigh": h[..., 0] = np.nextafter(np.float32(12.0), np.float32(99.0))
        if change == "rnan": h[..., 0] = np.nan
        if change == "dark": h[..., 0] = np.random.default_rng(2).uniform(7.2, 10.4, hits.shape[:3])   # the zero stretch and the negative node
        for out in (diskmod.thermal_spectrum(h, n_hits, td, nu), diskmod.shade_thermal(h, n_hits, td, nu[:3])):
            assert np.all(out == 0.0) and not np.any(np.signbit(out)), change
    # the ends themselves emit: r_min and r_max as float32 compare equal to the doubles
    h = hits.copy()
    h[..., 0] = 4.0
    assert np.all(diskmod.thermal_spectrum(h, n_hits, td, nu)[:, warm] > 0)
    h[..., 0] = 12.0
    assert np.all(diskmod.thermal_spectrum(h, n_hits, td, nu)[:, warm] > 0)
    assert np.all(diskmod.thermal_spectrum(hits, np.zeros_like(n_hits), td, nu) == 0.0)


def test_planes_hold_their_slot_and_add_up():
    name = "strip"
    hits, n_hits = thermal_records(name)
    m = CASES[name].m
    nu = frequencies(9)
    whole = diskmod.thermal_spectrum(hits, n_hits, make_thermal(name), nu)
    planes = diskmod.thermal_spectrum(hits, n_hits, make_thermal(name, True), nu)
    assert whole.shape == (1, 9) and planes.shape == (m, 9)
    n = int(reference(name).emits.sum())
    assert np.all(np.abs(planes.astype(LD).sum(axis=0) - whole[0]) <= 2 * n * U * whole[0])
    for j in range(m):
        only = hits.copy()
        only[:, :, np.arange(m) != j, 2] = np.nan                         # every other slot emits nothing
        assert np.array_equal(diskmod.thermal_spectrum(only, n_hits, make_thermal(name, True), nu)[j], planes[j])
        assert np.array_equal(diskmod.thermal_spectrum(only, n_hits, make_thermal(name), nu)[0], planes[j])
        assert np.all(planes[j][nu < 10 * T_MAX] > 0)


def test_a_permuted_list_gives_the_permuted_row():
    hits, n_hits = thermal_records("strip")
    nu = frequencies(21)
    td = make_thermal("strip", True)
    row = diskmod.thermal_spectrum(hits, n_hits, td, nu)
    perm = np.random.default_rng(9).permutation(21)
    assert np.array_equal(diskmod.thermal_spectrum(hits, n_hits, td, nu[perm]), row[:, perm])
    assert np.array_equal(diskmod.thermal_spectrum(hits, n_hits, td, nu[::-1]), row[:, ::-1])
    assert np.array_equal(diskmod.thermal_spectrum(hits, n_hits, td, nu[4:5]), row[:, 4:5])


def closure(spectrum, nu, hits, n_hits, td):
    """(trapezoid in ln nu of the spectrum, (pi^4 / 15) exposure sum g^4 T^4) for records whose frequencies are ascending."""
    T, _, emits, _, _ = coefficients_ref(hits, n_hits, td)               # the physical temperatures, not the statement's c
    g = np.asarray(hits, dtype=np.float32)[..., 2].astype(LD)[emits]
    y = spectrum * nu
    return float(np.sum(0.5 * (y[1:] + y[:-1]) * np.diff(np.log(nu)))), float(np.pi ** 4 / 15 * LD(td.exposure) * np.sum(g ** 4 * T[emits] ** 4))


def closure_grid(td, g_max, n=400):
    """1e-5 t_max ... 100 f_col t_max g_max, log-spaced.  400 points: the trapezoid in ln nu converges geometrically for this
    analytic, doubly decaying integrand, and the numpy statement alone closes to 3e-13 with them (3e-6 with 64 over this
    many decades)."""
    return np.exp(np.linspace(np.log(1e-5 * td.t_max), np.log(100.0 * td.f_col * td.t_max * g_max), n))


def test_stefan_boltzmann_closure():
    hits, n_hits = synth(40, 50, 3, 21, 2.4, 20.0)
    td = diskmod.ThermalDisk.novikov_thorne(1.0, 0.9, 20.0, n_r=512, t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE)
    nu = closure_grid(td, float(np.nanmax(hits[..., 2])))
    got, want = closure(diskmod.thermal_spectrum(hits, n_hits, td, nu)[0], nu, hits, n_hits, td)
    print(f"Stefan-Boltzmann closure on {nu.size} points: {got:.12e} against {want:.12e}, relative {abs(got / want - 1):.1e}")
    assert want > 0 and abs(got / want - 1) <= 1e-9


# ---- 4. the struct, exports and bindings, the command line, refusals ----------------------------------------------------------------
def test_struct_layout_defaults_and_constants():
    assert ctypes.sizeof(ltrace.Thermal) == 5 * 8 + 2 * 4 == 48
    d = ltrace.default_thermal()
    assert (d.r_min, d.r_max, d.t_max, d.f_col, d.exposure, d.n_r, d.split_orders) == (6.0, 20.0, 1.0, 1.0, 1.0, 2, 0)
    lt = diskmod.ThermalDisk([0.0, 1.0, 0.5], 3.0, 9.0, t_max=0.5, f_col=1.7, exposure=0.25, split_orders=True).to_lt()
    assert (lt.r_min, lt.r_max, lt.t_max, lt.f_col, lt.exposure, lt.n_r, lt.split_orders) == (3.0, 9.0, 0.5, 1.7, 0.25, 3, 1)
    assert (ltrace.THERMAL_MAX_NODES, ltrace.THERMAL_MAX_FREQS, ltrace.THERMAL_MAX_BANDS) == (65536, 1024, 16)
    assert (diskmod.THERMAL_MAX_NODES, diskmod.THERMAL_MAX_FREQS, diskmod.THERMAL_MAX_BANDS) == (65536, 1024, 16)
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(ltrace.__file__)), "..", "include", "ltrace.h")).read()
    for text in ("#define LT_THERMAL_MAX_NODES 65536", "#define LT_THERMAL_MAX_FREQS 1024", "#define LT_THERMAL_MAX_BANDS 16", "thermal continuum",
                 "#define LT_VERSION 200"):
        assert text in header


def test_the_c_compiler_gives_the_struct_the_same_layout(tmp_path):
    import os
    import subprocess
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ltrace.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(lt_thermal), offsetof(lt_thermal, t_max), offsetof(lt_thermal, exposure),\n'
                   '  offsetof(lt_thermal, n_r), offsetof(lt_thermal, split_orders)); return 0; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()]
    assert got == [ctypes.sizeof(ltrace.Thermal), ltrace.Thermal.t_max.offset, ltrace.Thermal.exposure.offset, ltrace.Thermal.n_r.offset,
                   ltrace.Thermal.split_orders.offset]


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    th, spec = ctypes.POINTER(ltrace.Thermal), ctypes.POINTER(ltrace.Spectrum)
    for suffix in ("", "_dev"):
        res, args = ltrace.SIGNATURES["lt_disk_spectrum" + suffix]
        at = args.index(spec)
        for name in ("lt_disk_thermal_spectrum", "lt_shade_thermal"):
            assert hasattr(lib, name + suffix) and name + suffix in ltrace.SIGNATURES, name + suffix
            # the disk spectrum's arguments with (thermal, flux, nu, n_freq) in the grid's place
            assert ltrace.SIGNATURES[name + suffix] == (res, args[:at] + [th, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + args[at + 1:])
    assert hasattr(lib, "lt_default_thermal") and ltrace.SIGNATURES["lt_default_thermal"] == (None, [th])
    for fn in (ltrace.thermal_spectrum, ltrace.thermal_spectrum_dev, ltrace.shade_thermal, ltrace.shade_thermal_dev, ltrace.default_thermal):
        assert callable(fn)
    assert ltrace.load().lt_version() == 200
    hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
    met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
    td = diskmod.ThermalDisk([0.0, 1.0, 0.5], 3.0, 9.0)
    with pytest.raises(ValueError, match="flux"):              # a table that is not the struct's n_r never reaches the library
        ltrace.thermal_spectrum(hits, n_hits, met, d, td.to_lt(), [0.0, 1.0], [1.0])
    with pytest.raises(ValueError, match="frequencies"):
        ltrace.thermal_spectrum(hits, n_hits, met, d, td.to_lt(), td.flux, np.ones(1025))
    with pytest.raises(ValueError, match="frequencies"):
        ltrace.shade_thermal(hits, n_hits, met, d, td.to_lt(), td.flux, np.ones(17))
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        calls = (lambda: ltrace.thermal_spectrum(hits, n_hits, met, d, td.to_lt(), td.flux, [1.0, 2.0]),
                 lambda: ltrace.shade_thermal(hits, n_hits, met, d, td.to_lt(), td.flux, [1.0, 2.0]),
                 lambda: ltrace.thermal_spectrum_dev(8, 0, 4, 4, 2, met, d, td.to_lt(), 8, 8, 2, 8),
                 lambda: ltrace.shade_thermal_dev(8, 0, 4, 4, 2, met, d, td.to_lt(), 8, 8, 2, 8),
                 lambda: ltrace.thermal_spectrum(hits, n_hits, met, d, ltrace.default_thermal(n_r=3, t_max=-1.0), td.flux, [1.0]))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE       # the first refusal of all, whatever else is wrong


SEQUENCE = ["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"]
SPOT = ["--hotspot", "8", "0", "1.5"]


@pytest.mark.parametrize("argv,match", [(["--thermal", "0.5", "--thermal-frequencies", "0.01", "10", "8"], "--thermal"),
                                        (SEQUENCE + ["--thermal", "0.5", "--thermal-bands", "1.0"], "--thermal"),
                                        (SEQUENCE + SPOT + ["--thermal-frequencies", "0.01", "10", "8"], "need --thermal"),
                                        (SEQUENCE + SPOT + ["--thermal-bands", "1.0"], "need --thermal"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5"], "--thermal-frequencies"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "1.7", "3"], "T_MAX"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-frequencies", "0.01", "10", "8.5"], "whole number"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-frequencies", "0.01", "10", "1025"], "1024"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-frequencies", "10", "0.01", "8"], "NU_MIN"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-bands"] + ["1.0"] * 17, "16"),
                                        (SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-bands", "-1.0"], "> 0"),
                                        (SEQUENCE + ["--disk-map", "spiral", "--thermal", "-0.5", "--thermal-bands", "1.0"], "t_max")])
def test_cli_refusals(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    thin = diskmod.TransparentDisk(max_images=3)
    with pytest.raises(ValueError, match=match):
        image_lens.thermal_from_args(args, thin, 1.0, 0.9)
    if args.hotspot is not None or args.disk_map is not None:
        with pytest.raises(ValueError, match=match):
            image_lens.main_sequence(args, thin)


def test_cli_needs_the_optically_thin_disk():
    import image_lens
    args = image_lens.build_parser().parse_args(["--a", "0.9", "--disk", "--synthetic", "16", "12"] + SPOT + ["--thermal", "0.5", "--thermal-bands", "1.0"])
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.thermal_from_args(args, diskmod.ThinDisk(), 1.0, 0.9)
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.main_sequence(args, diskmod.ThinDisk())
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.main_sequence(args, None)


def test_cli_builds_the_emitter():
    import image_lens
    thin = diskmod.TransparentDisk(max_images=3, r_out=18.0)
    args = image_lens.build_parser().parse_args(SEQUENCE + SPOT + ["--thermal", "0.5", "1.7", "--thermal-frequencies", "0.01", "10", "7",
                                                                   "--thermal-bands", "0.3", "2.5"])
    td, nu, bands = image_lens.thermal_from_args(args, thin, 1.0, 0.9)
    assert (td.t_max, td.f_col, td.r_min, td.r_max, td.n_r) == (0.5, 1.7, float(diskmod.isco(1.0, 0.9)), 18.0, 4096) and td.flux.max() == 1.0
    assert nu.shape == (7,) and nu[0] == 0.01 and nu[-1] == 10.0 and np.allclose(np.diff(np.log(nu)), np.log(1000.0) / 6)
    assert bands.tolist() == [0.3, 2.5]
    args = image_lens.build_parser().parse_args(SEQUENCE + SPOT + ["--thermal", "0.5", "--thermal-bands", "0.3"])
    td, nu, bands = image_lens.thermal_from_args(args, thin, 1.0, 0.9)
    assert td.f_col == 1.0 and nu is None and bands.tolist() == [0.3]
    assert image_lens.thermal_from_args(image_lens.build_parser().parse_args(SEQUENCE + SPOT)) is None
    for kw in (dict(thermal=td), dict(frequencies=[1.0]), dict(bands=[1.0])):
        with pytest.raises(ValueError, match="thermal"):       # render_sequence's own refusals of the three arguments come first
            image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8), **kw)
