"""The rotating emissivity map (include/ltrace.h, "a rotating emissivity map"): an extended-precision reference of the
rule, the CPU tests that hold disk.shade_diskmap / disk.diskmap_lightcurve / disk.sample_map to it, the library's exports
and bindings, and the refusals that need no GPU.  tests/test_gpu_diskmap.py imports the cases, the reference and the
bounds from here and holds the kernels (lt_diskmap.hpp) to them.

Records come from test_hotspot_records_host.synth (the shading is a function of the caller's records alone).
MapReference is written from the header's six steps in np.longdouble (64-bit mantissa here), sums included, with the
true 2 pi; it calls nothing of disk.py.

Bounds, derived and not measured:
    frames: float32 output of a value good to ~1e-12 relative -- 1 ulp of float32 for the numpy statement (two roundings
        of the same number), 2 ulp for the kernel (two roundings plus contraction, the existing kernels' bound);
    light curve: every term is non-negative (texels in [0.5, 1.5]), so the order of summation costs at most n_terms 2^-53
        relative; what is left is the phase Omega (t - dt), rounded in float64 (and wrapped with the float64 2 pi, which
        is 0.35 2^-53 relative off: inside the factor 8) and amplified by the table's slope -- a step of du in the
        azimuthal coordinate u = psi n_phi / 2 pi moves the bilinear value by at most du (T_max - T_min), relative to a
        value of at least T_min:
            rel <= 1e-12 + 8 2^-53 max|Omega (t - dt)| (n_phi / 2 pi) (T_max - T_min) / T_min             (map_lc_bound)
        Omega at the records' inner radius for Keplerian rotation (the largest there is), |omega_p| for rigid.

MEASURED here, disk.py against the reference (the cases and variants below):
    frames: no float32 differs (0.00 ulp) on any of the four cases;
    light curve, largest |lc - ref| / |ref| over the three columns, and its bound there (the 37 x 64 table at
        t = 1e5 ..., Keplerian but for mid): big 2.0e-14 (bound 4.1e-10), mid 9.4e-15 (5.5e-11, rigid), strip 1.8e-13 (1.1e-10),
        one 1.6e-12 (4.1e-10).
"""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_hotspot_records_host import DT_RANGE, isco_ref, lc_excess, synth, ulps

LD = np.longdouble
TWO_PI_LD = 2 * np.arccos(LD(-1))

# ---- cases: records, tables, variants -----------------------------------------------------------------------------------
Case = namedtuple("Case", "R W m M a r_out seed")
CASES = {"big": Case(257, 331, 8, 1.0, 0.9, 20.0, 51),      # a second, partial pass of the light curve's 65 536-pixel stride; W odd
         "mid": Case(260, 300, 3, 1.0, -0.7, 20.0, 52),
         "strip": Case(3, 70, 5, 2.0, 1.2, 40.0, 53),       # less than one block
         "one": Case(1, 1, 1, 1.0, 0.9, 20.0, 67)}          # (a seed whose pixel holds a hit, at r = 9.6 M)
TABLES = [(1, 1), (2, 3), (5, 1), (37, 64)]
# table, rotation, t_obs, with n_hits, with base, channels, with_disk, range strictly inside the records' r range
Variant = namedtuple("Variant", "table rotation t_obs counts base channels with_disk inside")
VARIANTS = [Variant(3, "kepler", 333.25, True, True, 3, True, False), Variant(3, "rigid", 1e5, False, False, 1, False, False),
            Variant(1, "kepler", -3e4, True, False, 3, False, True), Variant(1, "rigid", 333.25, False, True, 1, True, True),
            Variant(2, "kepler", 1e5, True, True, 1, False, False), Variant(0, "rigid", -3e4, True, False, 3, True, False),
            Variant(0, "kepler", 333.25, False, False, 1, False, True), Variant(2, "rigid", 333.25, True, True, 3, False, False)]
LC_GRIDS = [(5.0, 7.5, 6), (1e5, 11.0, 5), (-3e4, 13.0, 5), (333.25, 0.0, 1)]
DISK_EXPOSURE, MAP_EXPOSURE = 0.25, 0.05
_RECORDS = {}


def records(name):
    """(hits, n_hits, MapReference) of a case, made once."""
    if name not in _RECORDS:
        c = CASES[name]
        hits, n_hits = synth(c.R, c.W, c.m, c.seed, float(diskmod.isco(c.M, c.a)), c.r_out)
        _RECORDS[name] = (hits, n_hits, MapReference(hits, n_hits))
    return _RECORDS[name]


def table(shape, seed=7):
    """Texels uniform in [0.5, 1.5], float32."""
    return np.random.default_rng(seed + 1000 * shape[0] + shape[1]).uniform(0.5, 1.5, shape).astype(np.float32)


def make_map(c, v, exposure=MAP_EXPOSURE):
    """The disk.DiskMap of variant v on case c's records.  Its range exceeds the records' r range [isco, r_out], or lies
    strictly inside it, so that slots fall outside; the rigid pattern speed is the Keplerian one near r = 10 M."""
    r_in = float(diskmod.isco(c.M, c.a))
    lo, hi = (r_in + 2.0 * c.M, c.r_out - 5.0 * c.M) if v.inside else (0.5 * r_in, c.r_out + c.M)
    return diskmod.DiskMap(table(TABLES[v.table]), r_min=lo, r_max=hi, rotation=v.rotation, omega_p=0.03 / c.M, exposure=exposure,
                           with_disk=v.with_disk)


def base_of(c, v, seed=0):
    if not v.base:
        return None
    return np.random.default_rng(c.seed + seed).uniform(0.0, 0.5, (c.R, c.W) + ((3,) if v.channels == 3 else ())).astype(np.float32)


# ---- the reference ------------------------------------------------------------------------------------------------------
def _ramp(s):
    return np.stack([np.clip(2 * s - LD(0.5) * i, LD(0), LD(1)) for i in range(3)], axis=-1)


class MapReference:
    """The stored slots of one record buffer -- slot j of a pixel is stored where j < min(n_hits, max_images) -- as flat
    longdouble arrays, and the frame / light curve of a map over them, by the header's steps 1 to 6."""

    def __init__(self, hits, n_hits):
        self.R, self.W, self.m = hits.shape[:3]
        ns = np.minimum(n_hits.astype(np.int64), self.m).reshape(-1)
        self.lit = (ns > 0).reshape(self.R, self.W)
        self.pix, self.slot = np.nonzero(np.arange(self.m)[None, :] < ns[:, None])
        rec = hits.reshape(-1, self.m, 4)[self.pix, self.slot]
        assert not np.isnan(rec).any()
        self.r32 = rec[:, 0]
        self.r, self.ph, self.g, self.dt = (rec[:, c].astype(LD) for c in range(4))

    def weight(self, M, a, dmap, t_obs):
        """(n_stored,): the table's bilinear value m of every stored slot at observer time t_obs (steps 1 to 5)."""
        T = dmap.texels.astype(LD)
        n_r, n_phi = T.shape
        r_min, r_max = LD(dmap.r_min), LD(dmap.r_max)
        t_em = LD(t_obs) - self.dt
        if dmap.rotation == "rigid":
            om = LD(dmap.omega_p)
        else:
            om = np.sqrt(LD(M)) / (self.r * np.sqrt(self.r) + LD(a) * np.sqrt(LD(M)))
        x = self.ph - om * t_em
        psi = x - TWO_PI_LD * np.floor(x / TWO_PI_LD)
        psi = np.where((psi >= TWO_PI_LD) | (psi < 0), LD(0), psi)
        v = np.clip((self.r - r_min) / (r_max - r_min) * n_r - LD(0.5), LD(0), LD(n_r - 1))
        i0 = np.minimum(np.floor(v).astype(np.int64), n_r - 1)
        i1 = np.minimum(i0 + 1, n_r - 1)
        f_r = v - i0
        u = psi * (n_phi / TWO_PI_LD) - LD(0.5)
        fl = np.floor(u)
        k0 = np.mod(fl.astype(np.int64), n_phi)
        k1 = np.mod(k0 + 1, n_phi)
        f_p = u - fl
        m = (1 - f_r) * ((1 - f_p) * T[i0, k0] + f_p * T[i0, k1]) + f_r * ((1 - f_p) * T[i1, k0] + f_p * T[i1, k1])
        # exact comparisons of the float32 r against the doubles
        inside = (self.r32.astype(np.float64) >= np.float64(dmap.r_min)) & (self.r32.astype(np.float64) <= np.float64(dmap.r_max))
        return np.where(inside, m, LD(0))

    def map_emission(self, M, a, dmap, t_obs):
        """(n_stored, 3): exposure g^4 m ramp(g)."""
        return (LD(dmap.exposure) * self.g ** 4 * self.weight(M, a, dmap, t_obs))[:, None] * _ramp(self.g)

    def disk_emission(self, r_in, q, exposure):
        """(n_stored, 3): exposure g^4 (r_in / r)^q ramp(g (r_in / r)^0.75), the thin disk's light."""
        x = LD(r_in) / self.r
        return (LD(exposure) * self.g ** 4 * x ** LD(q))[:, None] * _ramp(self.g * x ** LD(0.75))

    def frame(self, M, a, dmap, t_obs, r_in, q=3.0, disk_exposure=1.0, base=None, channels=3, clamp=True):
        """clamp(base + sum_j (with_disk E_j^disk + E_j^map), 0, 1) in longdouble, (R, W, 3) or (R, W) for channels = 1
        (the mean of the three); a pixel without a stored hit keeps base.  Not yet rounded to float32."""
        e = self.map_emission(M, a, dmap, t_obs)
        if dmap.with_disk:
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
        out = np.where(lit, np.clip(acc, LD(0), LD(1)) if clamp else acc, start)
        return out.reshape((self.R, self.W) if channels == 1 else (self.R, self.W, 3))

    def lightcurve(self, M, a, dmap, times):
        """(len(times), 3) longdouble: per time the sums of e, e ix, e iy over the stored slots, e the mean of the map's
        three channels; column ix = p mod W and row iy = p div W of pixel p."""
        ix, iy = (self.pix % self.W).astype(LD), (self.pix // self.W).astype(LD)
        out = np.empty((len(times), 3), dtype=LD)
        for i, t in enumerate(times):
            es = self.map_emission(M, a, dmap, t)
            e = (es[:, 0] + es[:, 1] + es[:, 2]) / 3
            out[i] = e.sum(), (e * ix).sum(), (e * iy).sum()
        return out


def map_lc_bound(M, a, dmap, times, r_in, dt_range=DT_RANGE):
    """The light curve's relative bound (header) over `times`, dt anywhere in dt_range, Omega at r_in for Keplerian rotation."""
    t = np.asarray(times, dtype=np.float64)
    om = abs(dmap.omega_p) if dmap.rotation == "rigid" else float(np.sqrt(M) / (r_in ** 1.5 + a * np.sqrt(M)))
    phase = om * max(np.max(np.abs(t - dt_range[0])), np.max(np.abs(t - dt_range[1])))
    T = dmap.texels.astype(np.float64)
    return 1e-12 + 8 * 2.0 ** -53 * phase * (T.shape[1] / (2 * np.pi)) * (T.max() - T.min()) / T.min()


def grid_times(grid):
    return grid[0] + grid[1] * np.arange(grid[2])


# ---- CPU tests: the numpy statement against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_numpy_frames_against_the_reference(name):
    c = CASES[name]
    hits, n_hits, ref = records(name)
    r_in = float(isco_ref(c.M, c.a))
    dk = diskmod.ThinDisk(r_out=c.r_out, exposure=DISK_EXPOSURE)
    worst, inside, outside_slots = 0.0, 0, 0
    for v in VARIANTS:
        dmap, base = make_map(c, v), base_of(c, v)
        got = diskmod.shade_diskmap(c.M, c.a, hits, n_hits if v.counts else None, dk, dmap, v.t_obs, base=base, channels=v.channels)
        want = ref.frame(c.M, c.a, dmap, v.t_obs, r_in, dk.q, dk.exposure, base=base, channels=v.channels)
        assert got.shape == want.shape and got.dtype == np.float32
        worst = max(worst, float(np.max(ulps(got, want))))
        w32 = want.astype(np.float32)
        inside += int(((w32 > (0 if base is None else base)) & (w32 < 1)).sum())
        if v.inside:
            outside_slots += int(((ref.r32 < dmap.r_min) | (ref.r32 > dmap.r_max)).sum())
    print(f"{name}: disk.shade_diskmap against longdouble, largest difference {worst:.2f} ulp of float32; {inside} lit, unsaturated values")
    assert worst <= 1
    if c.R * c.W > 1:
        assert inside >= 0.2 * c.R * c.W       # lit and not saturated: pixels that say something
        assert outside_slots > 0               # and slots outside the map's annulus
    else:
        assert inside >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_lightcurve_against_the_reference(name):
    c = CASES[name]
    hits, n_hits, ref = records(name)
    r_in = float(diskmod.isco(c.M, c.a))
    for v in VARIANTS[:2] if c.R * c.W > 1000 else VARIANTS:
        dmap = make_map(c, v)
        for grid in LC_GRIDS:
            times = grid_times(grid)
            lc = diskmod.diskmap_lightcurve(c.M, c.a, hits, n_hits if v.counts else None, dmap, times)
            want = ref.lightcurve(c.M, c.a, dmap, times)
            bound = map_lc_bound(c.M, c.a, dmap, times, r_in)
            excess, rel = lc_excess(lc, want, bound)
            print(f"{name} {v.rotation} {TABLES[v.table]} t = {grid[0]:g} ...: disk.diskmap_lightcurve against longdouble, largest "
                  f"relative difference {rel:.2e}, bound {bound:.2e}")
            assert np.all(want[:, 0] > 0)
            assert excess <= 1


@pytest.mark.parametrize("S", [1, 2, 3])
def test_numpy_aa_is_the_resolve_of_the_fine_frame(S):
    """disk.shade_diskmap_aa is aa.resolve of disk.shade_diskmap on the fine records; on records repeated S times per axis
    it is the one-sample frame of the unrepeated records (S^2 equal float32 add up exactly in float64)."""
    import aa
    c, v = CASES["strip"], VARIANTS[0]
    hits, n_hits, _ = records("strip")
    dk, dmap, base = diskmod.ThinDisk(r_out=c.r_out, exposure=DISK_EXPOSURE), make_map(c, v), base_of(c, v)
    one = diskmod.shade_diskmap(c.M, c.a, hits, n_hits, dk, dmap, v.t_obs, base=base)
    rep = lambda x: np.repeat(np.repeat(x, S, axis=0), S, axis=1)
    assert np.array_equal(diskmod.shade_diskmap_aa(c.M, c.a, rep(hits), rep(n_hits), dk, dmap, v.t_obs, S, base=rep(base)), one)
    fh, fn = synth(c.R * S, 10 * S, c.m, 90 + S, float(diskmod.isco(c.M, c.a)), c.r_out)
    fine = diskmod.shade_diskmap(c.M, c.a, fh, fn, dk, dmap, v.t_obs, channels=1)
    got = diskmod.shade_diskmap_aa(c.M, c.a, fh, fn, dk, dmap, v.t_obs, S, channels=1)
    assert got.shape == (c.R, 10) and got.dtype == np.float32 and np.array_equal(got, aa.resolve(fine, S))
    assert S == 1 or not np.array_equal(got, fine[::S, ::S])


# ---- CPU tests: sampling properties ---------------------------------------------------------------------------------------
def _map(texels, r_min=4.0, r_max=12.0):
    return diskmod.DiskMap(np.asarray(texels, dtype=np.float32), r_min=r_min, r_max=r_max)


def test_texel_centres_return_the_texel():
    T = table((5, 8))
    dm = _map(T)
    r = dm.r_min + (np.arange(5) + 0.5) * (dm.r_max - dm.r_min) / 5          # exact in float64: (i + 1/2) 1.6 + 4 is not, hence ulps
    psi = (np.arange(8) + 0.5) * 2 * np.pi / 8
    got = diskmod.sample_map(dm, r[:, None], psi[None, :])
    assert np.max(np.abs(got - T)) <= 8 * np.spacing(1.5)


def test_radial_ramp_is_reproduced_and_constant_beyond_the_centres():
    n_r = 9
    T = np.repeat((3.0 + 0.25 * np.arange(n_r))[:, None], 4, axis=1)          # linear in the radial index, exact in float32
    dm = _map(T)
    h = (dm.r_max - dm.r_min) / n_r
    first, last = dm.r_min + 0.5 * h, dm.r_max - 0.5 * h
    r = np.linspace(first, last, 257)
    want = 3.0 + 0.25 * ((r - dm.r_min) / h - 0.5)
    assert np.max(np.abs(diskmod.sample_map(dm, r, 1.0) - want)) <= 16 * np.spacing(5.0)
    assert np.all(diskmod.sample_map(dm, np.linspace(dm.r_min, first, 33)[:-1], 2.0) == 3.0)
    assert np.all(diskmod.sample_map(dm, np.linspace(last, dm.r_max, 33)[1:], 2.0) == 3.0 + 0.25 * (n_r - 1))


def test_the_seam_is_periodic():
    T = table((3, 7))
    dm = _map(T)
    hits = np.empty((1, 64, 1, 4), dtype=np.float32)
    rng = np.random.default_rng(3)
    hits[0, :, 0, 0], hits[0, :, 0, 2], hits[0, :, 0, 3] = rng.uniform(4.0, 12.0, 64), 1.0, 50.0
    hits[0, :, 0, 1] = rng.uniform(0.0, 2 * np.pi, 64)
    there = diskmod.map_emission(1.0, 0.9, hits, dm, 100.0)
    # a hit at psi and at psi + 2 pi: the unwound azimuth of the first, then shifted by one turn, through wrap_2pi
    psi = diskmod.wrap_2pi(np.linspace(0.0, 2 * np.pi, 97)[:-1])
    a, b = diskmod.sample_map(dm, 7.0, psi), diskmod.sample_map(dm, 7.0, diskmod.wrap_2pi(psi + 2 * np.pi))
    assert np.max(np.abs(a - b)) <= 7 / (2 * np.pi) * 8 * np.spacing(4 * np.pi) * 1.0      # d(psi) n_phi / 2 pi (T_max - T_min)
    # across the seam: psi just below 2 pi and just above 0 interpolate between the last and the first texel of a row
    eps = 1e-9
    lo, hi = diskmod.sample_map(dm, 7.0, 2 * np.pi - eps), diskmod.sample_map(dm, 7.0, eps)
    assert abs(lo - hi) <= 4 * eps * 7 / (2 * np.pi)
    one_row = _map(T[1:2])
    assert abs(diskmod.sample_map(one_row, 7.0, 0.0) - 0.5 * (float(T[1, 6]) + float(T[1, 0]))) <= 4 * np.spacing(1.5)
    assert there.shape == (1, 64, 1, 3) and np.all(there >= 0)


def test_a_single_texel_is_everywhere_inside():
    dm = _map([[0.8125]])
    r = np.linspace(dm.r_min, dm.r_max, 41)
    psi = np.linspace(0.0, 2 * np.pi, 50)[:-1]
    assert np.all(diskmod.sample_map(dm, r[:, None], psi[None, :]) == 0.8125)


def test_outside_the_annulus_is_dark():
    dm = _map(table((4, 4)))
    lo, hi = np.float32(dm.r_min), np.float32(dm.r_max)
    r = np.array([np.nextafter(lo, np.float32(0)), lo, hi, np.nextafter(hi, np.float32(np.inf)), np.nan], dtype=np.float32)
    got = diskmod.sample_map(dm, r, 1.0)
    assert got[0] == 0 and got[3] == 0 and got[4] == 0 and got[1] > 0 and got[2] > 0
    hits = np.zeros((1, 5, 1, 4), dtype=np.float32)
    hits[0, :, 0, 0], hits[0, :, 0, 2] = r, 1.0
    e = diskmod.map_emission(1.0, 0.0, hits[:, :4], dm, 0.0)
    assert np.all(e[0, [0, 3]] == 0) and np.all(e[0, [1, 2], 0, 0] > 0)


def test_generators():
    sp = diskmod.spiral_map(16, 64, arms=2, pitch=0.35, contrast=0.8, r_min=4.0, r_max=12.0)
    assert sp.shape == (16, 64) and sp.dtype == np.float32 and sp.min() >= 0.2 - 1e-6 and sp.max() <= 1.8 + 1e-6
    assert np.allclose(sp[:, :32], sp[:, 32:], atol=1e-5)                      # two arms: period pi
    with pytest.raises(ValueError):
        diskmod.spiral_map(4, 4, contrast=1.5)
    gs = diskmod.spots_map(64, 256, 4.0, 12.0, [(9.0, 0.5, 1.5), (6.0, 4.0, 0.5, 2.0)])
    assert gs.shape == (64, 256) and gs.dtype == np.float32
    i, k = np.unravel_index(np.argmax(gs), gs.shape)
    assert abs(4.0 + (i + 0.5) / 8 - 6.0) < 0.2 and abs((k + 0.5) * 2 * np.pi / 256 - 4.0) < 0.05 and 1.9 < gs.max() <= 2.0 + 1e-3
    # the first spot alone is the hot spot's profile at t = 0
    one = diskmod.spots_map(64, 256, 4.0, 12.0, [(9.0, 0.5, 1.5)])
    r, ph = 4.0 + (40 + 0.5) / 8, (20 + 0.5) * 2 * np.pi / 256
    assert one[40, 20] == np.float32(np.exp(-(r * r + 81.0 - 18.0 * r * np.cos(ph - 0.5)) / 4.5))


# ---- exports, bindings, the struct ------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(ltrace.DiskMap) == 4 * 8 + 4 * 4 == 48
    d = ltrace.default_diskmap()
    assert (d.r_min, d.r_max, d.omega_p, d.exposure, d.n_r, d.n_phi, d.rotation, d.with_disk) == (6.0, 20.0, 0.0, 1.0, 1, 1, 0, 1)
    d = ltrace.default_diskmap(rotation="rigid", n_phi=7)
    assert d.rotation == ltrace.MAP_RIGID == 1 and d.n_phi == 7 and ltrace.MAP_KEPLERIAN == 0
    lt = diskmod.DiskMap(table((5, 3)), r_min=3.0, r_max=9.0, rotation="rigid", omega_p=0.02, exposure=0.5, with_disk=False).to_lt()
    assert (lt.r_min, lt.r_max, lt.omega_p, lt.exposure, lt.n_r, lt.n_phi, lt.rotation, lt.with_disk) == (3.0, 9.0, 0.02, 0.5, 5, 3, 1, 0)


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    mapargs = [ctypes.POINTER(ltrace.DiskMap), ctypes.c_void_p]
    spot = [ctypes.POINTER(ltrace.HotSpot)]
    for name, twin in (("lt_shade_diskmap", "lt_shade_hotspot"), ("lt_shade_diskmap_aa", "lt_shade_hotspot_aa"),
                       ("lt_diskmap_lightcurve", "lt_hotspot_lightcurve")):
        for suffix in ("", "_dev"):
            assert hasattr(lib, name + suffix) and name + suffix in ltrace.SIGNATURES, name + suffix
            res, args = ltrace.SIGNATURES[name + suffix]
            tres, targs = ltrace.SIGNATURES[twin + suffix]
            at = targs.index(spot[0])
            assert res == tres and args == targs[:at] + mapargs + targs[at + 1:], name + suffix
    assert hasattr(lib, "lt_default_diskmap") and ltrace.SIGNATURES["lt_default_diskmap"] == (None, [ctypes.POINTER(ltrace.DiskMap)])
    for fn in (ltrace.shade_diskmap, ltrace.shade_diskmap_dev, ltrace.shade_diskmap_aa, ltrace.shade_diskmap_aa_dev,
               ltrace.diskmap_lightcurve, ltrace.diskmap_lightcurve_dev, ltrace.default_diskmap):
        assert callable(fn)
    assert ltrace.load().lt_version() == 200
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
        met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
        dm = diskmod.DiskMap(table((2, 3)))
        calls = (lambda: ltrace.shade_diskmap(hits, n_hits, met, d, dm.to_lt(), dm.texels, 0.0),
                 lambda: ltrace.shade_diskmap_aa(hits, n_hits, 2, met, d, dm.to_lt(), dm.texels, 0.0),
                 lambda: ltrace.diskmap_lightcurve(hits, n_hits, met, d, dm.to_lt(), dm.texels, 0.0, 1.0, 4),
                 lambda: ltrace.shade_diskmap_dev(8, 0, 4, 4, 2, met, d, dm.to_lt(), 8, 0.0),
                 lambda: ltrace.shade_diskmap_aa_dev(8, 0, 2, 2, 2, 2, met, d, dm.to_lt(), 8, 0.0),
                 lambda: ltrace.diskmap_lightcurve_dev(8, 0, 4, 4, 2, met, d, dm.to_lt(), 8, 0.0, 1.0, 4, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE


# ---- refusals that need no device ---------------------------------------------------------------------------------------------
def test_argument_errors():
    import image_lens
    from metrics import Kerr
    metric = Kerr(M=1.0, a=0.9, integrator="rk4", precision=32)
    fov = (np.radians(40.0), np.radians(40.0))
    dm = diskmod.DiskMap(table((2, 3)))
    td = diskmod.TransparentDisk(max_images=3)
    with pytest.raises(ValueError, match="hot spot"):
        image_lens.render_sequence(None, metric, 50.0, fov, td, diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8), diskmap=dm)
    with pytest.raises(ValueError, match="not polarized"):
        image_lens.render_sequence(None, metric, 50.0, fov, td, None, [0.0, 10.0], shape=(8, 8), bfield=diskmod.BField(), diskmap=dm)
    with pytest.raises(ValueError, match="samples"):
        image_lens.render_sequence(None, metric, 50.0, fov, td, None, [0.0, 10.0], shape=(8, 8), samples=9, diskmap=dm)
    hits, n_hits = synth(6, 9, 2, 5, 2.4, 20.0)
    met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
    for fn in (lambda t: ltrace.shade_diskmap(hits, n_hits, met, d, dm.to_lt(), t, 0.0),
               lambda t: ltrace.shade_diskmap_aa(hits, n_hits, 3, met, d, dm.to_lt(), t, 0.0),
               lambda t: ltrace.diskmap_lightcurve(hits, n_hits, met, d, dm.to_lt(), t, 0.0, 1.0, 2)):
        with pytest.raises(ValueError, match="texels"):       # a table that is not the struct's (n_r, n_phi) never reaches the library
            fn(np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="samples per pixel"):
        ltrace.shade_diskmap_aa(hits, n_hits, 2, met, d, dm.to_lt(), dm.texels, 0.0)
    with pytest.raises(ValueError, match="base"):
        ltrace.shade_diskmap(hits, n_hits, met, d, dm.to_lt(), dm.texels, 0.0, base=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError):
        diskmod.DiskMap(np.zeros((2, 3, 4)))
    with pytest.raises(ValueError):
        diskmod.DiskMap(np.zeros((2, 3)), rotation="solid")


@pytest.mark.parametrize("extra,match", [(["--hotspot", "8", "0", "1.5"], "--hotspot"), (["--bfield", "0", "0", "1"], "--bfield"),
                                         (["--samples", "4", "--adaptive", "2"], "not adaptively sampled")])
def test_cli_refusals(extra, match):
    import image_lens
    args = image_lens.build_parser().parse_args(["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12", "--disk-map", "spiral"] + extra)
    with pytest.raises(ValueError, match=match):
        image_lens.main_sequence(args, diskmod.TransparentDisk(max_images=3))


def test_cli_builds_the_map():
    import image_lens
    td = diskmod.TransparentDisk(max_images=3, r_out=18.0)
    args = image_lens.build_parser().parse_args(["--disk-images", "3", "--disk-map", "spiral"])
    dm = image_lens.diskmap_from_args(args, td, 1.0, 0.9)
    assert dm.texels.shape == (256, 1024) and dm.rotation == "kepler" and (dm.r_min, dm.r_max) == (td.inner_edge(1.0, 0.9), 18.0)
    args = image_lens.build_parser().parse_args(["--disk-images", "3", "--disk-map", "spiral", "--disk-map-range", "5", "15", "--disk-map-rotation",
                                                 "rigid", "--disk-map-omega", "0.02", "--disk-map-exposure", "0.5"])
    dm = image_lens.diskmap_from_args(args, td, 1.0, 0.9)
    assert (dm.r_min, dm.r_max, dm.rotation, dm.omega_p, dm.exposure) == (5.0, 15.0, "rigid", 0.02, 0.5)
