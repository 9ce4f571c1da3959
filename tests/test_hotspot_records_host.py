"""Synthetic hit records for the hot spot's shading and light curve, an extended-precision reference of both, and the
CPU tests that hold disk.shade_hotspot / disk.lightcurve to it.  tests/test_gpu_hotspot_records.py imports the generator,
the reference and the bounds from here and holds the kernels (lt_hotspot.hpp) to them.

The shading and light-curve kernels are functions of the caller's records alone, so the records need no trace: synth()
draws them at whatever size reaches an edge of the kernels (a second pass of the light curve's grid-stride loop, counts
above max_images, one pixel).  Reference is written from the formulas of include/ltrace.h ("hot spot") in np.longdouble
(64-bit mantissa here), sums included; it calls nothing of disk.py.

Bounds, derived and not measured:
    frames: float32 output of a value good to ~1e-12 relative -- 1 ulp of float32 for the numpy statement (two roundings
        of the same number), 2 ulp for the kernel (the existing GPU test's bound);
    light curve: every term is non-negative, so the order of summation costs at most n_terms 2^-53 relative; what is left
        is the phase Omega (t - dt), rounded in float64 and amplified by the Gaussian's exponent:
            rel <= 1e-12 + 8 2^-53 max|Omega (t - dt)| r_out r_spot / sigma^2                      (lc_bound)
        about 2e-12 for |t| <= 500 and sigma = 1.5, about 2.5e-10 at t = 1e5; a phase kept in float32 would be off by ~1e-2.

MEASURED here, disk.lightcurve / disk.shade_hotspot against the reference (the cases of NUMPY_CASES):
    light curve, largest |lc - ref| / |ref| over the three columns, at t = 5 ... 42.5 / 1e5 ... / -3e4 ...:
        257 x 331 x 8 (a = 0.9):        4.0e-16 / 6.9e-14 / 2.7e-14   (bounds 2.0e-12 / 2.6e-10 / 7.8e-11);
        260 x 300 x 3 (a = -0.7):       5.4e-16 / 5.2e-14 / 1.2e-14   (bounds 2.1e-12 / 2.7e-10 / 8.3e-11);
        3 x 70 x 5 (M = 2, a = 1.2):    5.6e-15 / 2.1e-12 / 9.8e-13   (bounds 1.5e-12 / 1.3e-10 / 4.0e-11);
    frames: at most 1.00 ulp of float32 on the two large frames, no bit on the small one.
"""
import numpy as np
import pytest

import disk as diskmod

LD = np.longdouble
TWO_PI_LD = 2 * np.arccos(LD(-1))
DT_RANGE = (30.0, 400.0)
G_RANGE = (0.15, 1.4)


# ---- the generator ----------------------------------------------------------------------------------------------------
def synth(R, W, max_images, seed, r_in, r_out, n_max=12):
    """Deterministic hit records -> (hits float32 (R, W, max_images, 4), n_hits uint8 (R, W)).  Uniform r in [r_in, r_out],
    phi in [0, 2 pi), g in [0.15, 1.4] (all three branches of the ramp clamp(2 g - 0.5 i, 0, 1)), dt in [30, 400] M.
    n_hits: 0 for about 55 % of the pixels, else uniform in 1 ... n_max, so counts exceed max_images as the timed trace's
    do.  Slots j >= n_hits are NaN in all four components."""
    rng = np.random.default_rng(seed)
    shape = (R, W, max_images)
    hits = np.stack([rng.uniform(r_in, r_out, shape), rng.uniform(0.0, 2 * np.pi, shape), rng.uniform(*G_RANGE, shape),
                     rng.uniform(*DT_RANGE, shape)], axis=-1).astype(np.float32)
    n_hits = np.where(rng.random((R, W)) < 0.55, 0, rng.integers(1, n_max + 1, (R, W))).astype(np.uint8)
    hits[np.arange(max_images)[None, None, :] >= n_hits[..., None]] = np.nan
    return hits, n_hits


# ---- the reference ----------------------------------------------------------------------------------------------------
def omega_ref(M, a, r):
    """Omega = sqrt(M) / (r^1.5 + a sqrt(M)) of the circular equatorial orbit in +phi, longdouble."""
    M, a, r = LD(M), LD(a), LD(r)
    return np.sqrt(M) / (r * np.sqrt(r) + a * np.sqrt(M))


def isco_ref(M, a):
    """Bardeen-Press-Teukolsky ISCO of the orbit in +phi (retrograde for a < 0), longdouble."""
    M, a = LD(M), LD(a)
    x = abs(a) / M
    z1 = 1 + np.cbrt(1 - x * x) * (np.cbrt(1 + x) + np.cbrt(1 - x))
    z2 = np.sqrt(3 * x * x + z1 * z1)
    return M * (3 + z2 - (-1 if a < 0 else 1) * np.sqrt((3 - z1) * (3 + z1 + 2 * z2)))


def _ramp(s):
    return np.stack([np.clip(2 * s - LD(0.5) * i, LD(0), LD(1)) for i in range(3)], axis=-1)


class Reference:
    """The stored slots of one record buffer -- slot j of a pixel is stored where j < min(n_hits, max_images) -- as flat
    longdouble arrays, and the frame / light curve of a spot over them.  spot: (r_spot, phi0, sigma, exposure, with_disk)."""

    def __init__(self, hits, n_hits):
        self.R, self.W, self.m = hits.shape[:3]
        ns = np.minimum(n_hits.astype(np.int64), self.m).reshape(-1)
        self.lit = (ns > 0).reshape(self.R, self.W)
        self.pix, self.slot = np.nonzero(np.arange(self.m)[None, :] < ns[:, None])
        rec = hits.reshape(-1, self.m, 4)[self.pix, self.slot]
        assert not np.isnan(rec).any()
        self.r, self.ph, self.g, self.dt = (rec[:, c].astype(LD) for c in range(4))
        self._last = (None, None)     # the emission of the last (metric, spot, time): a frame's variants share it

    def spot_emission(self, M, a, spot, t_obs):
        """(n_stored, 3): exposure g^4 exp(-d^2 / 2 sigma^2) ramp(g), d the distance in the plane to the spot at t_obs - dt."""
        key = (M, a, tuple(spot), float(t_obs))
        if self._last[0] != key:
            r_s, phi0, sigma, exposure = (LD(x) for x in spot[:4])
            phi_s = phi0 + omega_ref(M, a, r_s) * (LD(t_obs) - self.dt)
            d2 = self.r * self.r + r_s * r_s - 2 * self.r * r_s * np.cos(self.ph - phi_s)
            inten = exposure * self.g ** 4 * np.exp(-d2 / (2 * sigma * sigma))
            self._last = (key, inten[:, None] * _ramp(self.g))
        return self._last[1]

    def disk_emission(self, r_in, q, exposure):
        """(n_stored, 3): exposure g^4 (r_in / r)^q ramp(g (r_in / r)^0.75), the thin disk's light."""
        x = LD(r_in) / self.r
        return (LD(exposure) * self.g ** 4 * x ** LD(q))[:, None] * _ramp(self.g * x ** LD(0.75))

    def frame(self, M, a, spot, t_obs, r_in, q=3.0, disk_exposure=1.0, base=None, channels=3):
        """clamp(base + sum_j (with_disk E_j^disk + E_j^spot), 0, 1) in longdouble, (R, W, 3) or (R, W) for channels = 1
        (the mean of the three); a pixel without a stored hit keeps base.  Not yet rounded to float32."""
        e = self.spot_emission(M, a, spot, t_obs)
        if spot[4]:
            e = e + self.disk_emission(r_in, q, disk_exposure)
        if channels == 1:
            e = (e[:, 0] + e[:, 1] + e[:, 2]) / 3
        shape = (self.R * self.W,) if channels == 1 else (self.R * self.W, 3)
        acc = np.zeros(shape, dtype=LD) if base is None else np.asarray(base, dtype=np.float32).astype(LD).reshape(shape)
        start = acc.copy()
        for j in range(self.m):     # (a pixel occurs once per slot, so the indexed add sees no index twice)
            sel = self.slot == j
            acc[self.pix[sel]] += e[sel]
        lit = self.lit.reshape(-1) if channels == 1 else self.lit.reshape(-1)[:, None]
        out = np.where(lit, np.clip(acc, LD(0), LD(1)), start)
        return out.reshape((self.R, self.W) if channels == 1 else (self.R, self.W, 3))

    def lightcurve(self, M, a, spot, times):
        """(len(times), 3) longdouble: per time the sums of e, e ix, e iy over the stored slots, e the mean of the spot's
        three channels; column ix = p mod W and row iy = p div W of pixel p."""
        ix, iy = (self.pix % self.W).astype(LD), (self.pix // self.W).astype(LD)
        out = np.empty((len(times), 3), dtype=LD)
        for i, t in enumerate(times):
            es = self.spot_emission(M, a, spot, t)
            e = (es[:, 0] + es[:, 1] + es[:, 2]) / 3
            out[i] = e.sum(), (e * ix).sum(), (e * iy).sum()
        return out


# ---- bounds and comparisons ---------------------------------------------------------------------------------------------
def lc_bound(M, a, spot, times, r_out):
    """The light curve's relative bound (header) over `times`, dt anywhere in the generator's range."""
    r_s, sigma = float(spot[0]), float(spot[2])
    t = np.asarray(times, dtype=np.float64)
    phase = float(abs(omega_ref(M, a, r_s))) * max(np.max(np.abs(t - DT_RANGE[0])), np.max(np.abs(t - DT_RANGE[1])))
    return 1e-12 + 8 * 2.0 ** -53 * phase * r_out * r_s / sigma ** 2


def lc_excess(lc, ref, bound):
    """Largest |lc - ref| / (bound |ref|) (<= 1: inside the bound); a reference of exactly 0 -- the centroid sums of a
    one-pixel frame -- wants exactly 0.  Also returns the largest relative difference itself, for the record."""
    diff = np.abs(np.asarray(lc).astype(LD) - ref)
    assert np.all(diff[ref == 0] == 0)
    rel = np.max(np.where(ref == 0, LD(0), diff / np.where(ref == 0, LD(1), np.abs(ref))))
    return float(rel / LD(bound)), float(rel)


def ulps(x, ref):
    """|x - ref| in units of float32's spacing at ref (ref the reference, longdouble or already float32)."""
    r32 = np.asarray(ref).astype(np.float32)
    return np.abs(np.asarray(x).astype(np.float64) - r32.astype(np.float64)) / np.spacing(np.maximum(np.abs(r32), np.float32(1e-30)))


# ---- CPU tests ----------------------------------------------------------------------------------------------------------
# (R, W, max_images, M, a, r_out, seed); the spot is "the spot of the existing GPU test" scaled with M
NUMPY_CASES = [(257, 331, 8, 1.0, 0.9, 20.0, 21), (260, 300, 3, 1.0, -0.7, 20.0, 22), (3, 70, 5, 2.0, 1.2, 40.0, 23)]
NUMPY_IDS = [f"{c[0]}x{c[1]}x{c[2]}-M{c[3]:g}-a{c[4]:g}" for c in NUMPY_CASES]
LC_TIMES = np.concatenate([5.0 + 7.5 * np.arange(6), 1e5 + 11.0 * np.arange(5), -3e4 + 13.0 * np.arange(5)])   # 16 times
_CASE = {}


def numpy_case(i):
    if i not in _CASE:
        R, W, m, M, a, r_out, seed = NUMPY_CASES[i]
        hits, n_hits = synth(R, W, m, seed, float(diskmod.isco(M, a)), r_out)
        _CASE[i] = (hits, n_hits, Reference(hits, n_hits))
    return _CASE[i]


def test_generator():
    R, W, m = 57, 64, 5
    hits, n_hits = synth(R, W, m, 3, 2.32, 20.0)
    again = synth(R, W, m, 3, 2.32, 20.0)
    assert hits.tobytes() == again[0].tobytes() and n_hits.tobytes() == again[1].tobytes()
    assert synth(R, W, m, 4, 2.32, 20.0)[0].tobytes() != hits.tobytes()
    assert hits.shape == (R, W, m, 4) and hits.dtype == np.float32 and n_hits.shape == (R, W) and n_hits.dtype == np.uint8
    stored = np.arange(m) < n_hits[..., None]
    assert np.array_equal(np.isnan(hits), np.repeat(~stored[..., None], 4, axis=-1))
    assert 0.50 <= np.mean(n_hits == 0) <= 0.60 and n_hits.max() == 12 and (n_hits > m).sum() > 0.15 * n_hits.size
    r, ph, g, dt = (hits[..., c][stored] for c in range(4))
    one = np.float32(1 + 1e-6)
    assert r.min() >= np.float32(2.32) / one and r.max() <= 20.0 and r.min() < 2.6 and r.max() > 19.5
    assert ph.min() >= 0 and ph.max() <= np.float32(2 * np.pi) and g.min() >= np.float32(0.15) and g.max() <= np.float32(1.4)
    assert dt.min() >= 30 and dt.max() <= 400
    # the ramp's three branches: 0 (blue below g = 0.5), in between, and 1 (red above g = 0.5)
    assert (g < 0.5).any() and ((g > 0.5) & (g < 1.0)).any() and (g > 1.0).any()


@pytest.mark.parametrize("M,a", [(1.0, 0.9), (1.0, -0.7), (1.0, 0.0), (2.0, 1.2)])
def test_reference_orbit_and_isco(M, a):
    """The reference's own Omega and ISCO against disk.py's and the library's host function: what the GPU test takes as
    r_in and as the period is one number in all three."""
    import ltrace
    assert abs(float(isco_ref(M, a)) - float(diskmod.isco(M, a))) <= 1e-14 * float(isco_ref(M, a))
    assert abs(float(isco_ref(M, a)) - ltrace.kerr_isco(M, a)) <= 1e-14 * float(isco_ref(M, a))
    for r in (6.5, 9.0, 23.0):
        assert abs(float(omega_ref(M, a, r)) - float(diskmod.omega(M, a, r))) <= 4e-16 * float(omega_ref(M, a, r))
    # Kepler far out, dragged by the hole's spin close in; all lengths and times scale with M
    assert float(omega_ref(M, a, 1e6)) == pytest.approx(np.sqrt(M) * 1e-9, rel=1e-6)
    assert (float(omega_ref(M, a, 9.0)) < float(omega_ref(M, 0.0, 9.0))) == (a > 0)
    assert float(omega_ref(2 * M, 2 * a, 18.0)) == pytest.approx(float(omega_ref(M, a, 9.0)) / 2, rel=1e-15)


@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_numpy_lightcurve_against_the_reference(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, ref = numpy_case(ci)
    spot = (9.0 * M, 0.5, 1.5 * M, 2.0, True)
    lc = diskmod.lightcurve(M, a, hits, n_hits, diskmod.HotSpot(*spot), LC_TIMES)
    want = ref.lightcurve(M, a, spot, LC_TIMES)
    assert np.all(want[:, 0] > 0)
    for name, sel in (("t = 5 ... 42.5", slice(0, 6)), ("t = 1e5", slice(6, 11)), ("t = -3e4", slice(11, 16))):
        bound = lc_bound(M, a, spot, LC_TIMES[sel], r_out)
        excess, rel = lc_excess(lc[sel], want[sel], bound)
        print(f"{NUMPY_IDS[ci]} {name}: disk.lightcurve against longdouble, largest relative difference {rel:.2e}, bound {bound:.2e}")
        assert excess <= 1


@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_numpy_frames_against_the_reference(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, ref = numpy_case(ci)
    r_in = float(diskmod.isco(M, a))
    dk = diskmod.ThinDisk(r_out=r_out, exposure=0.25)
    rng = np.random.default_rng(seed)
    worst, inside = 0.0, 0
    for with_disk, channels, with_base, t_obs in ((True, 3, True, 333.25), (True, 1, False, 1e5), (False, 3, False, -3e4), (False, 1, True, 0.0)):
        spot = (9.0 * M, 0.5, 1.5 * M, 2.0, with_disk)
        base = rng.uniform(0.0, 0.5, (R, W) + ((3,) if channels == 3 else ())).astype(np.float32) if with_base else None
        got = diskmod.shade_hotspot(M, a, hits, n_hits, dk, diskmod.HotSpot(*spot), t_obs, base=base, channels=channels)
        want = ref.frame(M, a, spot, t_obs, r_in, dk.q, dk.exposure, base=base, channels=channels)
        assert got.shape == want.shape and got.dtype == np.float32
        worst = max(worst, float(np.max(ulps(got, want))))
        w32 = want.astype(np.float32)
        inside += int(((w32 > (0 if base is None else base)) & (w32 < 1)).sum())
    print(f"{NUMPY_IDS[ci]}: disk.shade_hotspot against longdouble, largest difference {worst:.2f} ulp of float32")
    assert worst <= 1
    assert inside > 0.2 * R * W        # lit and not saturated: pixels that say something


@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_stored_slots_without_counts(ci):
    """The NaN padding makes the rule without n_hits (leading non-NaN slots) pick min(n_hits, max_images)."""
    hits, n_hits, ref = numpy_case(ci)
    m = hits.shape[2]
    want = np.minimum(n_hits.astype(np.int64), m)
    assert (n_hits > m).any()
    assert np.array_equal(diskmod._stored(hits, None), want) and np.array_equal(diskmod._stored(hits, n_hits), want)
    assert ref.pix.size == int(want.sum()) and np.array_equal(ref.lit, want > 0)
