"""Energy-resolved light (include/ltrace.h, "energy-resolved light"): the bin rule at exact edges, an extended-precision
reference of the three spectra, the CPU tests that hold disk.disk_spectrum / disk.hotspot_spectrum /
disk.diskmap_spectrum to it, the grid's validation, the library's exports and bindings, and the CLI's refusals.
tests/test_gpu_spectrum.py imports the grids, the reference and the bounds from here and holds the kernels
(lt_spectrum.hpp) to them.

Records come from test_hotspot_records_host.synth; the map's tables and variants from test_diskmap_host.
SpectrumReference holds a Reference and a MapReference of the same records (composition; neither is edited) and is
written from the header's formulas: weights and sums in np.longdouble, the bin index by the float64 rule, because the
rule defines it so (formula_bin below, one scalar at a time with math.floor; bins_f64 is its vectorised twin, and both are
independent of disk.spectrum_bin).

Bounds, derived and not measured.  Every bin is a sum of non-negative terms, so its relative error is at most the largest
relative error of a term plus n_terms 2^-53 (n_terms: the entries of that bin; the bound of a sum of non-negative float64
in ANY order, so it covers numpy's running sum and the kernel's partials alike):
    the spot: lc_bound (test_hotspot_records_host: the phase Omega (t - dt) rounded in float64, amplified by the Gaussian);
    the map:  map_lc_bound (test_diskmap_host: the phase amplified by the table's slope);
    the disk: 1e-12, the floor of those bounds: pow and g^4 in float64.
A bin that is empty in the reference must be exactly 0.0.
"""
import ctypes
import math

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import LC_GRIDS, VARIANTS, Case, MapReference, grid_times, make_map, map_lc_bound
from test_hotspot_records_host import NUMPY_CASES, NUMPY_IDS, Reference, isco_ref, lc_bound, omega_ref, synth

LD = np.longdouble
U = 2.0 ** -53
# (g_min, g_max, n_bins): inv_dg no power of two and both out-of-range columns in use (synth's g spans 0.15 ... 1.4); the
# default grid; one bin; the most bins there are
GRIDS = [(0.3, 1.2, 7), (0.0625, 1.5625, 96), (0.25, 1.25, 1), (0.15, 1.4, 512)]
EDGE_GRID = (0.25, 1.25, 8)          # inv_dg = 8.0 exactly, every multiple of 0.125 exact in float32
DISK_EXPOSURE = 0.25
SPOT = lambda M: (9.0 * M, 0.5, 1.5 * M, 2.0, True)      # "the spot of the existing GPU test" scaled with M
MAP_VARIANTS = (VARIANTS[0], VARIANTS[1])                 # Keplerian and rigid, the 37 x 64 table, t = 333.25 / 1e5
f32 = np.float32


def edge_values():
    """(g float32, column or -1 for skipped) on EDGE_GRID."""
    g = np.array([0.25, 1.125, 1.25, np.nextafter(f32(0.25), f32(0)), np.nextafter(f32(0.375), f32(0)), np.nextafter(f32(1.25), f32(0)),
                  np.nan], dtype=np.float32)
    return g, np.array([1, 8, 9, 0, 1, 8, -1])


def formula_bin(g32, g_min, g_max, n_bins):
    """The header's rule for one stored float32 g, in Python floats (float64): the column, or -1 for a NaN."""
    x = float(f32(g32))
    if x != x:
        return -1
    inv_dg = n_bins / (g_max - g_min)
    if x < g_min:
        return 0
    if x >= g_max:
        return n_bins + 1
    return 1 + min(int(math.floor((x - g_min) * inv_dg)), n_bins - 1)


def bins_f64(g32, g_min, g_max, n_bins):
    """formula_bin for an array of finite float32 g."""
    x = np.asarray(g32, dtype=np.float32).astype(np.float64)
    inv_dg = n_bins / (g_max - g_min)
    k = 1 + np.minimum(np.floor((x - g_min) * inv_dg).astype(np.int64), n_bins - 1)
    return np.where(x < g_min, 0, np.where(x >= g_max, n_bins + 1, k))


# ---- the reference ------------------------------------------------------------------------------------------------------
class SpectrumReference:
    """The three spectra of one record buffer in longdouble.  spot: (r_spot, phi0, sigma, exposure, with_disk)."""

    def __init__(self, hits, n_hits):
        self.spot_ref, self.map_ref = Reference(hits, n_hits), MapReference(hits, n_hits)
        s = self.spot_ref
        self.m, self.slot, self.r, self.ph, self.g, self.dt = s.m, s.slot, s.r, s.ph, s.g, s.dt
        assert np.array_equal(s.pix, self.map_ref.pix) and np.array_equal(s.slot, self.map_ref.slot)
        self.g32 = hits.reshape(-1, self.m, 4)[s.pix, s.slot, 2]
        self._keys = {}

    def keys(self, grid, split):
        """(order, starts, keys present, counts (planes, cols)) of the stored slots under a grid: sorted once."""
        if (grid, split) not in self._keys:
            cols, planes = grid[2] + 2, self.m if split else 1
            key = (self.slot * cols if split else 0) + bins_f64(self.g32, *grid)
            order = np.argsort(key, kind="stable")
            present, starts, counts = np.unique(key[order], return_index=True, return_counts=True)
            full = np.zeros(planes * cols, dtype=np.int64)
            full[present] = counts
            self._keys[(grid, split)] = (order, starts, present, full.reshape(planes, cols))
        return self._keys[(grid, split)]

    def bin(self, weights, grid, split):
        """(planes, n_bins + 2) longdouble: the weights (n_stored,) summed per key."""
        order, starts, present, counts = self.keys(grid, split)
        out = np.zeros(counts.size, dtype=LD)
        if present.size:
            out[present] = np.add.reduceat(weights[order], starts)
        return out.reshape(counts.shape)

    def disk_weights(self, r_in, q, exposure):
        return LD(exposure) * self.g ** 4 * (LD(r_in) / self.r) ** LD(q)

    def spot_weights(self, M, a, spot, t_obs):
        r_s, phi0, sigma, exposure = (LD(x) for x in spot[:4])
        phi_s = phi0 + omega_ref(M, a, r_s) * (LD(t_obs) - self.dt)
        d2 = self.r * self.r + r_s * r_s - 2 * self.r * r_s * np.cos(self.ph - phi_s)
        return exposure * self.g ** 4 * np.exp(-d2 / (2 * sigma * sigma))

    def map_weights(self, M, a, dmap, t_obs):
        return LD(dmap.exposure) * self.g ** 4 * self.map_ref.weight(M, a, dmap, t_obs)


def check_spectrum(got, want, counts, term_bound):
    """got (..., planes, cols) float64 against want longdouble of the same shape: empty bins exactly 0, every other within
    (term_bound + n_terms 2^-53) relative.  -> the largest difference in units of its bound, and itself."""
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.float64 and got.shape[-2:] == counts.shape
    assert np.all(got[..., counts == 0] == 0.0) and not np.any(np.signbit(got[..., counts == 0]))
    diff = np.abs(got.astype(LD) - want)
    assert np.all(diff[want == 0] == 0)
    rel = np.where(want == 0, LD(0), diff / np.where(want == 0, LD(1), want))
    bound = term_bound + counts * U
    return float(np.max(rel / bound)), float(np.max(rel))


def as_case(c):
    return Case(*c)


_CASE = {}


def spectrum_case(i):
    """(hits, n_hits, SpectrumReference) of NUMPY_CASES[i], made once."""
    if i not in _CASE:
        R, W, m, M, a, r_out, seed = NUMPY_CASES[i]
        hits, n_hits = synth(R, W, m, seed, float(diskmod.isco(M, a)), r_out)
        _CASE[i] = (hits, n_hits, SpectrumReference(hits, n_hits))
    return _CASE[i]


def short_times(grid):
    """The first two times of a light-curve grid (the reference's longdouble exp and cos are what a test's time goes to)."""
    return grid_times(grid)[:2]


# ---- 1. the bin rule ------------------------------------------------------------------------------------------------------
def test_bin_rule_at_exact_edges():
    spec = diskmod.Spectrum(*EDGE_GRID)
    assert spec.n_bins / (spec.g_max - spec.g_min) == 8.0
    g, want = edge_values()
    assert all(float(x) == float(f32(x)) for x in np.arange(2, 11) * 0.125)
    got = diskmod.spectrum_bin(g, spec)
    assert got.tolist() == want.tolist()
    assert [formula_bin(x, *EDGE_GRID) for x in g] == want.tolist()
    # every edge of the grid, the float32 just below and just above it
    edges = (0.25 + 0.125 * np.arange(9)).astype(np.float32)
    assert diskmod.spectrum_bin(edges, spec).tolist() == list(range(1, 10))
    assert diskmod.spectrum_bin(np.nextafter(edges, f32(0)), spec).tolist() == list(range(0, 9))
    assert diskmod.spectrum_bin(np.nextafter(edges, f32(2)), spec).tolist() == list(range(1, 9)) + [9]
    assert diskmod.spectrum_bin(np.array([0.0, -1.0, np.inf, -np.inf], dtype=np.float32), spec).tolist() == [0, 0, 9, 0]


def test_bin_rule_is_the_formula_element_by_element():
    grid = GRIDS[0]                                           # inv_dg = 7 / 0.9, no power of two
    spec = diskmod.Spectrum(*grid)
    rng = np.random.default_rng(11)
    edges = spec.edges().astype(np.float32)
    g = np.concatenate([rng.uniform(0.1, 1.5, 4000).astype(np.float32), edges, np.nextafter(edges, f32(0)), np.nextafter(edges, f32(2)),
                        np.array([np.nan, 0.0, np.inf], dtype=np.float32)])
    got = diskmod.spectrum_bin(g, spec)
    assert got.tolist() == [formula_bin(x, *grid) for x in g]
    assert set(got.tolist()) == set(range(-1, 9))           # skipped, underflow, the seven bins, overflow
    finite = np.isfinite(g)
    assert np.array_equal(bins_f64(g[finite], *grid), got[finite])


# ---- 2. the numpy statements against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_numpy_spectra_against_the_reference(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, ref = spectrum_case(ci)
    c = as_case(NUMPY_CASES[ci])
    r_in = float(isco_ref(M, a))
    dk = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE)
    spot = SPOT(M)
    worst = dict(disk=(0.0, 0.0), spot=(0.0, 0.0), map=(0.0, 0.0))
    note = lambda who, pair: worst.__setitem__(who, max(worst[who], pair))
    disk_w = ref.disk_weights(r_in, dk.q, dk.exposure)
    spot_w = {(gi, float(t)): ref.spot_weights(M, a, spot, t) for gi, grid in enumerate(LC_GRIDS) for t in short_times(grid)}
    maps = [make_map(c, v) for v in MAP_VARIANTS]
    map_w = {(vi, gi, float(t)): ref.map_weights(M, a, dm, t) for vi, dm in enumerate(maps) for gi, grid in enumerate(LC_GRIDS[:2])
             for t in short_times(grid)}
    for grid in GRIDS:
        for split in (False, True):
            spec = diskmod.Spectrum(*grid, split_orders=split)
            counts = ref.keys(grid, split)[3]
            assert counts.shape == (m if split else 1, grid[2] + 2) and counts.sum() == ref.g.size
            nh = n_hits if split else None                   # with the counts and with the NaN padding
            got = diskmod.disk_spectrum(M, a, hits, nh, dk, spec)
            want = ref.bin(disk_w, grid, split)
            note("disk", check_spectrum(got, want, counts, 1e-12))
            assert np.all(want[counts > 0] > 0)
            for gi, lcg in enumerate(LC_GRIDS):
                times = short_times(lcg)
                got = diskmod.hotspot_spectrum(M, a, hits, nh, diskmod.HotSpot(*spot), spec, times)
                want = np.stack([ref.bin(spot_w[(gi, float(t))], grid, split) for t in times])
                note("spot", check_spectrum(got, want, counts, lc_bound(M, a, spot, times, r_out)))
            for vi, dm in enumerate(maps):
                for gi, lcg in enumerate(LC_GRIDS[:2]):
                    times = short_times(lcg)
                    got = diskmod.diskmap_spectrum(M, a, hits, nh, dm, spec, times)
                    want = np.stack([ref.bin(map_w[(vi, gi, float(t))], grid, split) for t in times])
                    note("map", check_spectrum(got, want, counts, map_lc_bound(M, a, dm, times, float(diskmod.isco(M, a)))))
            # the grids do what they are for
            if grid == GRIDS[0]:
                assert np.all(counts.sum(axis=0)[[0, -1]] > 0) and np.all(got.sum(axis=(0, 1))[[0, -1]] > 0)
                assert np.all(ref.bin(disk_w, grid, split).sum(axis=0)[[0, -1]] > 0)
            if grid == GRIDS[1] and R * W > 1000:
                assert (counts.sum(axis=0)[1:-1] > 0).sum() >= 48
    for who, (excess, rel) in worst.items():
        print(f"{NUMPY_IDS[ci]} {who}: numpy spectrum against longdouble, largest relative difference {rel:.2e}, {excess:.3f} of its bound")
        assert excess <= 1


def test_rows_sum_to_the_bolometric_light():
    """A row summed over all columns and planes is the light curve's column 0 with the ramp taken out: checked against
    the reference's plain sum of the weights."""
    R, W, m, M, a, r_out, seed = NUMPY_CASES[2]
    hits, n_hits, ref = spectrum_case(2)
    spot = SPOT(M)
    for grid in GRIDS:
        got = diskmod.hotspot_spectrum(M, a, hits, n_hits, diskmod.HotSpot(*spot), diskmod.Spectrum(*grid, split_orders=True), [333.25])
        total = ref.spot_weights(M, a, spot, 333.25).sum()
        assert abs(got.astype(LD).sum() - total) <= (lc_bound(M, a, spot, [333.25], r_out) + ref.g.size * U) * total


# ---- 3. planes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_planes_add_up_to_the_unsplit_spectrum(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, ref = spectrum_case(ci)
    dk, spot = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE), diskmod.HotSpot(*SPOT(M))
    for grid in GRIDS:
        one, per = diskmod.Spectrum(*grid), diskmod.Spectrum(*grid, split_orders=True)
        counts = ref.keys(grid, False)[3]
        pairs = [(diskmod.disk_spectrum(M, a, hits, n_hits, dk, one), diskmod.disk_spectrum(M, a, hits, n_hits, dk, per)),
                 (diskmod.hotspot_spectrum(M, a, hits, n_hits, spot, one, [5.0])[0], diskmod.hotspot_spectrum(M, a, hits, n_hits, spot, per, [5.0])[0])]
        for whole, planes in pairs:
            assert whole.shape == (1, grid[2] + 2) and planes.shape == (m, grid[2] + 2)
            assert np.all(np.abs(planes.sum(axis=0) - whole[0]) <= counts[0] * U * whole[0])
            assert m == 1 or np.count_nonzero(planes.sum(axis=1)) == m                # every order holds light


# ---- 4. the grid, the struct, exports and bindings, the CLI ---------------------------------------------------------------------
def test_spectrum_validation_and_edges():
    for bad in ((0.0, 1.0, 4), (-0.5, 1.0, 4), (1.0, 1.0, 4), (1.2, 0.3, 4), (0.3, float("inf"), 4), (float("nan"), 1.0, 4), (0.3, 1.2, 0),
                (0.3, 1.2, 513), (0.3, 1.2, 2.5)):
        with pytest.raises(ValueError):
            diskmod.Spectrum(*bad)
    s = diskmod.Spectrum(0.25, 1.25, 8)
    assert np.array_equal(s.edges(), 0.25 + 0.125 * np.arange(9)) and not s.split_orders and s.planes(5) == 1
    assert np.array_equal(s.energies(6.4), 6.4 * (0.3125 + 0.125 * np.arange(8)))
    d = diskmod.Spectrum()
    assert (d.g_min, d.g_max, d.n_bins, d.split_orders) == (0.0625, 1.5625, 96, False)
    e = diskmod.Spectrum(0.3, 1.2, 7, split_orders=True).edges()
    assert e.shape == (8,) and e[0] == 0.3 and e[-1] == 1.2 and np.all(np.diff(e) > 0)
    assert diskmod.Spectrum(0.3, 1.2, 512, split_orders=True).planes(8) == 8


def test_struct_layout_defaults_and_constants():
    assert ctypes.sizeof(ltrace.Spectrum) == 2 * 8 + 2 * 4 == 24
    d = ltrace.default_spectrum()
    assert (d.g_min, d.g_max, d.n_bins, d.split_orders) == (0.0625, 1.5625, 96, 0)
    lt = diskmod.Spectrum(0.3, 1.2, 7, split_orders=True).to_lt()
    assert (lt.g_min, lt.g_max, lt.n_bins, lt.split_orders) == (0.3, 1.2, 7, 1)
    assert (ltrace.SPECTRUM_MAX_BINS, ltrace.SPECTRUM_BLOCKS, ltrace.SPECTRUM_WORKSPACE_BYTES) == (512, 256, 64 << 20)
    assert diskmod.SPECTRUM_MAX_BINS == ltrace.SPECTRUM_MAX_BINS
    # the largest key count: 8 planes of 514 columns, 256 partial histograms of float64 per time
    big = diskmod.Spectrum(0.15, 1.4, 512, split_orders=True).to_lt()
    assert ltrace.spectrum_planes(big, 8) == 8 and ltrace.spectrum_batch_times(big, 8) == (64 << 20) // (256 * 4112 * 8) == 7
    assert ltrace.spectrum_batch_times(ltrace.default_spectrum(), 3) == (64 << 20) // (256 * 98 * 8)
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(ltrace.__file__)), "..", "include", "ltrace.h")).read()
    for text in ("#define LT_SPECTRUM_MAX_BINS 512", "#define LT_SPECTRUM_BLOCKS 256", "#define LT_SPECTRUM_WORKSPACE_BYTES (64 << 20)",
                 "energy-resolved light"):
        assert text in header


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    spec, spot, dmap = ctypes.POINTER(ltrace.Spectrum), ctypes.POINTER(ltrace.HotSpot), ctypes.POINTER(ltrace.DiskMap)
    for suffix in ("", "_dev"):
        for name in ("lt_disk_spectrum", "lt_hotspot_spectrum", "lt_diskmap_spectrum"):
            assert hasattr(lib, name + suffix) and name + suffix in ltrace.SIGNATURES, name + suffix
        # the light curves' arguments with the grid before the times
        res, args = ltrace.SIGNATURES["lt_hotspot_lightcurve" + suffix]
        at = args.index(spot) + 1
        assert ltrace.SIGNATURES["lt_hotspot_spectrum" + suffix] == (res, args[:at] + [spec] + args[at:])
        res, args = ltrace.SIGNATURES["lt_diskmap_lightcurve" + suffix]
        at = args.index(dmap) + 2
        assert ltrace.SIGNATURES["lt_diskmap_spectrum" + suffix] == (res, args[:at] + [spec] + args[at:])
        assert ltrace.SIGNATURES["lt_disk_spectrum" + suffix] == (res, args[:args.index(dmap)] + [spec, ctypes.c_void_p])
    assert hasattr(lib, "lt_default_spectrum") and ltrace.SIGNATURES["lt_default_spectrum"] == (None, [spec])
    for fn in (ltrace.disk_spectrum, ltrace.disk_spectrum_dev, ltrace.hotspot_spectrum, ltrace.hotspot_spectrum_dev, ltrace.diskmap_spectrum,
               ltrace.diskmap_spectrum_dev, ltrace.default_spectrum):
        assert callable(fn)
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
        met, d, sp = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(), ltrace.default_spectrum()
        dm = diskmod.DiskMap(np.ones((2, 3), np.float32))
        calls = (lambda: ltrace.disk_spectrum(hits, n_hits, met, d, sp),
                 lambda: ltrace.hotspot_spectrum(hits, n_hits, met, d, ltrace.default_hotspot(), sp, 0.0, 1.0, 4),
                 lambda: ltrace.diskmap_spectrum(hits, n_hits, met, d, dm.to_lt(), dm.texels, sp, 0.0, 1.0, 4),
                 lambda: ltrace.disk_spectrum_dev(8, 0, 4, 4, 2, met, d, sp, 8),
                 lambda: ltrace.hotspot_spectrum_dev(8, 0, 4, 4, 2, met, d, ltrace.default_hotspot(), sp, 0.0, 1.0, 4, 8),
                 lambda: ltrace.diskmap_spectrum_dev(8, 0, 4, 4, 2, met, d, dm.to_lt(), 8, sp, 0.0, 1.0, 4, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE


SEQUENCE = ["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"]


@pytest.mark.parametrize("argv,match", [(["--spectrum", "0.3", "1.2", "7"], "--spectrum"),
                                        (SEQUENCE + ["--spectrum", "0.3", "1.2", "7"], "--spectrum"),
                                        (SEQUENCE + ["--hotspot", "8", "0", "1.5", "--spectrum-orders"], "--spectrum-orders"),
                                        (SEQUENCE + ["--hotspot", "8", "0", "1.5", "--spectrum", "0.3", "1.2", "7.5"], "N_BINS"),
                                        (SEQUENCE + ["--hotspot", "8", "0", "1.5", "--spectrum", "1.2", "0.3", "7"], "g_min"),
                                        (SEQUENCE + ["--disk-map", "spiral", "--spectrum", "0.3", "1.2", "600"], "n_bins")])
def test_cli_refusals(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    with pytest.raises(ValueError, match=match):
        image_lens.spectrum_from_args(args)
    if args.hotspot is not None or args.disk_map is not None:
        with pytest.raises(ValueError, match=match):
            image_lens.main_sequence(args, diskmod.TransparentDisk(max_images=3))


def test_cli_builds_the_grid():
    import image_lens
    args = image_lens.build_parser().parse_args(SEQUENCE + ["--hotspot", "8", "0", "1.5", "--spectrum", "0.3", "1.2", "7", "--spectrum-orders"])
    s = image_lens.spectrum_from_args(args)
    assert (s.g_min, s.g_max, s.n_bins, s.split_orders) == (0.3, 1.2, 7, True)
    assert image_lens.spectrum_from_args(image_lens.build_parser().parse_args(SEQUENCE + ["--hotspot", "8", "0", "1.5"])) is None
    with pytest.raises(ValueError, match="hot spot"):         # render_sequence's own refusals come first, the grid changes none
        image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8),
                                   diskmap=diskmod.DiskMap(np.ones((2, 3), np.float32)), spectrum=s)
