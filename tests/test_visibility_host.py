"""Visibilities (include/ltrace.h, "visibilities"): an extended-precision reference of the three emitters' complex
visibilities, the CPU tests that hold disk.disk_visibility / disk.hotspot_visibility / disk.diskmap_visibility to it,
disk.Baselines' validation, constructors and recentring, the library's exports and bindings, and the CLI's refusals.
tests/test_gpu_visibility.py imports the baselines, the reference and the bounds from here and holds the kernels
(lt_visibility.hpp) to them.

VisibilityReference stands on a SpectrumReference of the same records (composition; nothing of it is edited): its
longdouble weights and its pix / slot arrays.  The phase is evaluated in longdouble from the float64 (u, v): x = u ix + v iy
(errors of 2^-64 relative, nothing next to the bounds), f = x - rint(x), cos and sin of 2 pi f.

Bounds, derived and not measured.  A component of V[plane, b] is a sum of n_terms terms w cos / -w sin of magnitude at
most w, so its error is at most (largest relative error of a weight + largest error of a phase factor + n_terms 2^-53)
times the sum of the weights, the plane's flux -- relative to the flux and not to |V|, which can be as near to zero as it
likes:
    term_bound   as the spectrum's: lc_bound for the spot, map_lc_bound for the map, 1e-12 for the disk;
    phase_bound  the rule's x = fl(fl(u ix) + fl(v iy)): |u ix| <= W / 2 and |v iy| <= H / 2, so the two products are off
                 by at most 2^-53 (W / 2 + H / 2) together and the sum by as much again, (W + H) 2^-53 cycles in all, times
                 2 pi in the factor; sincospi itself is held to 4 ulp (the bound OpenCL sets for sinpi / cospi in double,
                 which the device library implements; numpy's sin and cos of pi r are within one), 4 x 2^-52 for values up
                 to 1; and the product w c is rounded once where it is not fused, 2^-53:
                 (2 pi (W + H) + 8 + 1) 2^-53;
    n_terms      the plane's stored slots: the bound of a float64 sum of n numbers in ANY order, n 2^-53 sum |terms|, so it
                 covers numpy's pairwise sums, the kernel's chunks and the 256 partials alike.  Without split_orders the
                 slots of a pixel are added before the phase is applied: the same count.
A plane that is empty in the reference must be exactly 0 + 0i.
"""
import ctypes
import math

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import LC_GRIDS, make_map, map_lc_bound
from test_hotspot_records_host import NUMPY_CASES, NUMPY_IDS, isco_ref, lc_bound
from test_spectrum_host import DISK_EXPOSURE, MAP_VARIANTS, SPOT, U, as_case, short_times, spectrum_case

LD = np.longdouble
TWO_PI_LD = 2 * np.arccos(LD(-1))
# (0, 0); the Nyquist limit on either axis; a quarter cycle on both; five generic ones (one with a negative component,
# one with both)
BASELINES = np.array([(0.0, 0.0), (0.5, 0.0), (0.0, -0.5), (0.25, 0.25), (0.013, 0.0071), (0.11, -0.37), (0.3141, 0.2718), (0.49, 0.003),
                      (-0.2, -0.05)])


def phase_bound(R, W):
    """The header's phase rule against the exact phase, per unit weight (derived above)."""
    return (2 * math.pi * (W + R) + 9) * U


# ---- the reference ------------------------------------------------------------------------------------------------------
class VisibilityReference:
    """The visibilities of one record buffer in longdouble, on the weights of a SpectrumReference."""

    def __init__(self, spec_ref, W):
        self.ref, self.m = spec_ref, spec_ref.m
        pix = spec_ref.spot_ref.pix
        self.slot = spec_ref.slot
        self.ix, self.iy = (pix % W).astype(LD), (pix // W).astype(LD)
        self._phase = {}

    def phase(self, uv):
        """(cos, sin) of 2 pi (u ix + v iy), each (n_baselines, n_stored) longdouble; the last set of baselines is kept."""
        uv = np.ascontiguousarray(uv, dtype=np.float64)
        key = uv.tobytes()
        if key not in self._phase:
            x = uv[:, 0].astype(LD)[:, None] * self.ix + uv[:, 1].astype(LD)[:, None] * self.iy
            th = TWO_PI_LD * (x - np.rint(x))
            self._phase = {key: (np.cos(th), np.sin(th))}
        return self._phase[key]

    def counts(self, split):
        """(planes,) stored slots of every plane."""
        return np.bincount(self.slot, minlength=self.m) if split else np.array([self.slot.size])

    def planes(self, weights, split):
        """(planes, n_stored) longdouble: the weights of every plane's slots, 0 elsewhere."""
        if not split:
            return weights[None, :]
        return np.where(self.slot[None, :] == np.arange(self.m)[:, None], weights[None, :], LD(0))

    def visibility(self, weights, uv, split):
        """-> (re, im, flux): (planes, n_baselines) twice and (planes,), longdouble."""
        c, s = self.phase(uv)
        w = self.planes(weights, split)
        return w @ c.T, -(w @ s.T), w.sum(axis=1)


def check_visibility(got, want, counts, term_bound, ph_bound):
    """got complex128 (..., planes, n_b) against want = (re, im, flux) longdouble of (..., planes, n_b) and (..., planes):
    a plane without a stored slot exactly 0 + 0i, every component within (term_bound + ph_bound + n_terms 2^-53) flux.
    -> the largest difference in units of its bound."""
    re, im, flux = want
    got = np.asarray(got)
    assert got.dtype == np.complex128 and got.shape == re.shape and got.shape[-2] == counts.size
    assert np.all(got[..., counts == 0, :] == 0)
    bound = np.broadcast_to((term_bound + ph_bound + counts * U)[:, None] * flux[..., None], re.shape)
    diff = np.maximum(np.abs(got.real.astype(LD) - re), np.abs(got.imag.astype(LD) - im))
    assert np.all(diff[bound == 0] == 0)
    return float(np.max(np.where(bound == 0, LD(0), diff / np.where(bound == 0, LD(1), bound))))


_VREF = {}


def visibility_case(ci):
    """(hits, n_hits, SpectrumReference, VisibilityReference) of NUMPY_CASES[ci], made once."""
    if ci not in _VREF:
        hits, n_hits, ref = spectrum_case(ci)
        _VREF[ci] = (hits, n_hits, ref, VisibilityReference(ref, NUMPY_CASES[ci][1]))
    return _VREF[ci]


# ---- 1. the phase rule ------------------------------------------------------------------------------------------------------
def test_phase_rule_is_exact_at_quarter_cycles():
    s, c = diskmod.sincospi_reduced(np.array([0.0, 0.25, 0.5, 0.75, 1.0, -0.25, -0.5, 300.25, -77.75, 12345.5]))
    assert s.tolist() == [0, 1, 0, -1, 0, -1, 0, 1, 1, 0] and c.tolist() == [1, 0, -1, 0, 1, 0, -1, 0, 0, -1]
    ph = diskmod.visibility_phase([(0.25, 0.0), (0.5, 0.5), (0.0, -0.25)], np.arange(4), np.array([0, 0, 1, 3]))
    assert ph.shape == (3, 4) and ph.dtype == np.complex128
    assert np.array_equal(ph[0], [1, -1j, -1, 1j]) and np.array_equal(ph[1], [1, -1, -1, 1]) and np.array_equal(ph[2], [1, 1, 1j, -1j])
    # odd / even: V(-u, -v) is the conjugate, to the bit
    rng = np.random.default_rng(3)
    uv, ix, iy = rng.uniform(-0.5, 0.5, (64, 2)), rng.integers(0, 331, 500), rng.integers(0, 257, 500)
    assert np.array_equal(diskmod.visibility_phase(-uv, ix, iy), np.conj(diskmod.visibility_phase(uv, ix, iy)))
    # against longdouble, within the phase bound
    x = uv[:, :1].astype(LD) * ix + uv[:, 1:].astype(LD) * iy
    th = TWO_PI_LD * (x - np.rint(x))
    got = diskmod.visibility_phase(uv, ix, iy)
    assert np.max(np.abs(got.real - np.cos(th))) <= phase_bound(257, 331) and np.max(np.abs(got.imag + np.sin(th))) <= phase_bound(257, 331)


# ---- 2. the numpy statements against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_numpy_visibilities_against_the_reference(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, ref, vref = visibility_case(ci)
    c = as_case(NUMPY_CASES[ci])
    dk = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE)
    spot = SPOT(M)
    pb = phase_bound(R, W)
    worst = dict(disk=0.0, spot=0.0, map=0.0)
    disk_w = ref.disk_weights(float(isco_ref(M, a)), dk.q, dk.exposure)
    for split in (False, True):
        nh = n_hits if split else None                   # with the counts and with the NaN padding
        counts = vref.counts(split)
        assert counts.sum() == ref.g.size and counts.size == (m if split else 1)
        got = diskmod.disk_visibility(M, a, hits, nh, dk, BASELINES, split)
        want = vref.visibility(disk_w, BASELINES, split)
        worst["disk"] = max(worst["disk"], check_visibility(got, want, counts, 1e-12, pb))
        assert np.all(want[2][counts > 0] > 0) and np.all(got[:, 0].imag == 0)
        for gi, lcg in enumerate(LC_GRIDS[:2]):
            times = short_times(lcg)
            got = diskmod.hotspot_visibility(M, a, hits, nh, diskmod.HotSpot(*spot), BASELINES, split, times)
            want = tuple(np.stack(x) for x in zip(*[vref.visibility(ref.spot_weights(M, a, spot, t), BASELINES, split) for t in times]))
            worst["spot"] = max(worst["spot"], check_visibility(got, want, counts, lc_bound(M, a, spot, times, r_out), pb))
            dm = make_map(c, MAP_VARIANTS[gi])
            got = diskmod.diskmap_visibility(M, a, hits, nh, dm, BASELINES, split, times)
            want = tuple(np.stack(x) for x in zip(*[vref.visibility(ref.map_weights(M, a, dm, t), BASELINES, split) for t in times]))
            worst["map"] = max(worst["map"], check_visibility(got, want, counts, map_lc_bound(M, a, dm, times, float(diskmod.isco(M, a))), pb))
    for who, excess in worst.items():
        print(f"{NUMPY_IDS[ci]} {who}: numpy visibility against longdouble, {excess:.3f} of its bound")
        assert excess <= 1


def test_planes_add_up_and_zero_baseline_is_the_flux():
    R, W, m, M, a, r_out, seed = NUMPY_CASES[2]
    hits, n_hits, ref, vref = visibility_case(2)
    spot = diskmod.HotSpot(*SPOT(M))
    whole = diskmod.hotspot_visibility(M, a, hits, n_hits, spot, BASELINES, False, [333.25])[0]
    per = diskmod.hotspot_visibility(M, a, hits, n_hits, spot, BASELINES, True, [333.25])[0]
    flux = ref.spot_weights(M, a, SPOT(M), 333.25).sum()
    assert whole.shape == (1, 9) and per.shape == (m, 9) and np.count_nonzero(per[:, 0]) == m
    bound = (lc_bound(M, a, SPOT(M), [333.25], r_out) + phase_bound(R, W) + ref.g.size * U) * float(flux)
    assert np.all(np.abs(per.sum(axis=0) - whole[0]) <= 2 * bound)
    assert abs(LD(whole[0, 0].real) - flux) <= bound and whole[0, 0].imag == 0
    assert np.all(np.abs(whole[0]) <= whole[0, 0].real * (1 + 1e-12))          # the triangle inequality on non-negative weights


# ---- 3. the baselines ---------------------------------------------------------------------------------------------------------
def test_baselines_validation_and_constructors():
    for bad in (np.zeros((0, 2)), np.zeros((1025, 2)), np.zeros(4), np.zeros((3, 3)), [(0.5000001, 0.0)], [(0.0, -0.5000001)],
                [(float("nan"), 0.0)], [(0.0, float("inf"))]):
        with pytest.raises(ValueError):
            diskmod.Baselines(bad)
    b = diskmod.Baselines([(0.5, -0.5), (0, 0)])
    assert len(b) == 2 and b.uv.dtype == np.float64 and b.uv.flags.c_contiguous and not b.split_orders and b.planes(5) == 1
    assert diskmod.Baselines(np.zeros((1024, 2)), split_orders=True).planes(8) == 8
    r = diskmod.Baselines.radial(5, 0.4, 90.0)
    assert len(r) == 5 and np.allclose(r.uv[:, 1], [0, 0.1, 0.2, 0.3, 0.4]) and np.all(np.abs(r.uv[:, 0]) < 1e-16)
    assert np.array_equal(diskmod.Baselines.radial(3, 0.5, 0.0).uv, [(0, 0), (0.25, 0), (0.5, 0)])
    assert np.array_equal(diskmod.Baselines.radial(1, 0.5, 10.0).uv, [(0, 0)])
    g = diskmod.Baselines.grid(3, 2, 0.5, split_orders=True)
    assert g.split_orders and np.array_equal(g.uv, [(-0.5, -0.5), (0, -0.5), (0.5, -0.5), (-0.5, 0.5), (0, 0.5), (0.5, 0.5)])
    assert np.array_equal(g.fine(4), g.uv / 4)
    for bad in (lambda: diskmod.Baselines.radial(4, 0.6, 0.0), lambda: diskmod.Baselines.radial(0, 0.5, 0.0), lambda: diskmod.Baselines.grid(33, 32, 0.5)):
        with pytest.raises(ValueError):
            bad()
    assert diskmod.VISIBILITY_MAX_BASELINES == ltrace.VISIBILITY_MAX_BASELINES == 1024


def test_recentre():
    M, a = 1.0, 0.9
    dk = diskmod.ThinDisk(r_out=20.0, exposure=1.0)
    b = diskmod.Baselines(BASELINES)
    rec = np.array([8.0, 1.0, 0.75, 100.0], dtype=np.float32)
    w = (0.75 * 0.75) ** 2 * (float(diskmod.isco(M, a)) / 8.0) ** dk.q
    # a one-pixel frame: the centre is the pixel, nothing moves
    V = diskmod.disk_visibility(M, a, rec.reshape(1, 1, 1, 4), None, dk, b.uv)
    assert np.array_equal(b.recentre(V, (1, 1)), V) and np.all(np.abs(V - w) <= 4 * U * w)
    # an odd frame with one lit pixel at its centre: V is real and equal to w
    for H, W in ((5, 7), (81, 97), (257, 331)):
        hits = np.full((H, W, 1, 4), np.nan, dtype=np.float32)
        hits[H // 2, W // 2, 0] = rec
        V = b.recentre(diskmod.disk_visibility(M, a, hits, None, dk, b.uv), (H, W))
        assert V.shape == (1, 9)
        assert np.all(np.abs(V.real - w) <= 4 * U * w) and np.all(np.abs(V.imag) <= 4 * U * w), (H, W)
    # S x S equal fine pixels under one output pixel at the centre of an odd frame, (u / S, v / S): real again, S^2 w / S^2
    S, H, W = 2, 3, 5
    hits = np.full((H * S, W * S, 1, 4), np.nan, dtype=np.float32)
    hits[S * (H // 2):S * (H // 2) + S, S * (W // 2):S * (W // 2) + S, 0] = rec
    V = b.recentre(diskmod.disk_visibility(M, a, hits, None, dk, b.fine(S)), (H, W), S)
    assert abs(V[0, 0] - w) <= 8 * U * w and np.all(np.abs(V.imag) <= 8 * U * w) and np.all(V.real <= w * (1 + 8 * U))


# ---- 4. constants, exports and bindings, the CLI ------------------------------------------------------------------------------
def test_constants_and_batch():
    assert (ltrace.VISIBILITY_MAX_BASELINES, ltrace.VISIBILITY_BLOCKS, ltrace.VISIBILITY_BATCH_TERMS, ltrace.VISIBILITY_WORKSPACE_BYTES) == (
        1024, 256, 16, 64 << 20)
    assert [ltrace.visibility_batch_times(True, m) for m in range(1, 9)] == [16, 8, 5, 4, 3, 2, 2, 2]
    assert all(ltrace.visibility_batch_times(False, m) == 16 for m in (1, 3, 8))
    assert ltrace.visibility_planes(True, 5) == 5 and ltrace.visibility_planes(False, 5) == 1
    # one batch of the most terms at the most baselines fills the workspace exactly
    assert 256 * 16 * 1024 * 16 == ltrace.VISIBILITY_WORKSPACE_BYTES
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(ltrace.__file__)), "..", "include", "ltrace.h")).read()
    for text in ("#define LT_VISIBILITY_MAX_BASELINES 1024", "#define LT_VISIBILITY_BLOCKS 256", "#define LT_VISIBILITY_BATCH_TERMS 16",
                 "#define LT_VISIBILITY_WORKSPACE_BYTES (64 << 20)", "visibilities"):
        assert text in header


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    spec = ctypes.POINTER(ltrace.Spectrum)
    uv = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32]
    for suffix in ("", "_dev"):
        for name in ("lt_disk_visibility", "lt_hotspot_visibility", "lt_diskmap_visibility"):
            assert hasattr(lib, name + suffix) and name + suffix in ltrace.SIGNATURES, name + suffix
            # the spectrum's arguments with (uv, n_baselines, split_orders) in the grid's place
            res, args = ltrace.SIGNATURES[name.replace("visibility", "spectrum") + suffix]
            at = args.index(spec)
            assert ltrace.SIGNATURES[name + suffix] == (res, args[:at] + uv + args[at + 1:])
    assert hasattr(lib, "lt_visibility_batch_times")
    for fn in (ltrace.disk_visibility, ltrace.disk_visibility_dev, ltrace.hotspot_visibility, ltrace.hotspot_visibility_dev,
               ltrace.diskmap_visibility, ltrace.diskmap_visibility_dev, ltrace.visibility_batch_times):
        assert callable(fn)
    with pytest.raises(ValueError):
        ltrace._uv_array(np.zeros(4))
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        from test_hotspot_records_host import synth
        hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
        met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
        dm = diskmod.DiskMap(np.ones((2, 3), np.float32))
        b = BASELINES
        calls = (lambda: ltrace.disk_visibility(hits, n_hits, met, d, b),
                 lambda: ltrace.hotspot_visibility(hits, n_hits, met, d, ltrace.default_hotspot(), b, True, 0.0, 1.0, 4),
                 lambda: ltrace.diskmap_visibility(hits, n_hits, met, d, dm.to_lt(), dm.texels, b, False, 0.0, 1.0, 4),
                 lambda: ltrace.disk_visibility_dev(8, 0, 4, 4, 2, met, d, b, False, 8),
                 lambda: ltrace.hotspot_visibility_dev(8, 0, 4, 4, 2, met, d, ltrace.default_hotspot(), b, False, 0.0, 1.0, 4, 8),
                 lambda: ltrace.diskmap_visibility_dev(8, 0, 4, 4, 2, met, d, dm.to_lt(), 8, b, True, 0.0, 1.0, 4, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE


SEQUENCE = ["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"]
SPOT_ARGS = ["--hotspot", "8", "0", "1.5"]


@pytest.mark.parametrize("argv,match", [(["--visibility", "8", "0.5", "0"], "--visibility"),
                                        (SEQUENCE + ["--visibility", "8", "0.5", "0"], "--visibility"),
                                        (SEQUENCE + SPOT_ARGS + ["--visibility-orders"], "--visibility-orders"),
                                        (SEQUENCE + SPOT_ARGS + ["--visibility", "7.5", "0.5", "0"], "N must"),
                                        (SEQUENCE + SPOT_ARGS + ["--visibility", "8", "0.6", "0"], "0.5"),
                                        (SEQUENCE + ["--disk-map", "spiral", "--visibility", "1025", "0.5", "0"], "1024"),
                                        (SEQUENCE + ["--disk-map", "spiral", "--visibility", "0", "0.5", "0"], "1024")])
def test_cli_refusals(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    with pytest.raises(ValueError, match=match):
        image_lens.baselines_from_args(args)
    if args.hotspot is not None or args.disk_map is not None:
        with pytest.raises(ValueError, match=match):
            image_lens.main_sequence(args, diskmod.TransparentDisk(max_images=3))


def test_cli_builds_the_baselines():
    import image_lens
    args = image_lens.build_parser().parse_args(SEQUENCE + SPOT_ARGS + ["--visibility", "3", "0.5", "0", "--visibility-orders"])
    b = image_lens.baselines_from_args(args)
    assert b.split_orders and np.array_equal(b.uv, [(0, 0), (0.25, 0), (0.5, 0)])
    assert image_lens.baselines_from_args(image_lens.build_parser().parse_args(SEQUENCE + SPOT_ARGS)) is None
    with pytest.raises(ValueError, match="hot spot"):         # render_sequence's own refusals come first, the baselines change none
        image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8),
                                   diskmap=diskmod.DiskMap(np.ones((2, 3), np.float32)), baselines=b)
