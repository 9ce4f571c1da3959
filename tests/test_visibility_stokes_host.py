"""Polarized visibilities (include/ltrace.h, "polarized visibilities"): an extended-precision reference of Stokes I, Q, U on
every baseline, the CPU tests that hold disk.disk_visibility_stokes / disk.hotspot_visibility_stokes to it, the exact
properties of the numpy statement, disk.fractional_polarization, the library's constants, exports and bindings, and the
CLI.  tests/test_gpu_visibility_stokes.py imports the reference and the bounds from here and holds the kernels
(lt_visibility_stokes.hpp) to them.

StokesVisibilityReference stands on a VisibilityReference and its SpectrumReference (composition; nothing of either is
edited): their longdouble weights w_I, pix / slot arrays and phases.  Its Q and U weights are w_I times the longdouble
products Pi sz sz q and Pi sz sz u of the float32 polarization records (test_polarization_host.synth_pol), exact to 2^-64.

Bounds, derived and not measured.  As test_visibility_host.py's, a component of V[plane, stokes, b] is a sum of n_terms
terms w cos / -w sin, and its error is bounded relative to the plane's FLUX, the sum of w_I -- not relative to |Q~| or to the
sum of |w_Q|: Q and U are signed and cancel, the flux does not.
    I            test_visibility_host.py's bound unchanged: (term_bound + phase_bound + n_terms 2^-53) flux.
    Q, U         |w_Q| = Pi sz^2 |q| w_I <= (1 + 2^-22) w_I: Pi <= 1, sz <= 1, and |q|, |u| <= 1 up to the float32 rounding
                 of a cosine (2^-24 relative, 2^-22 with room for sz and the product).  So a relative error e of w_Q is
                 at most e (1 + 2^-22) w_I in absolute terms, and the spectrum's term_bound (the relative error of the
                 float64 w_I) carries over.  The float64 statement evaluates four more products, each rounded once --
                 Pi sz, (Pi sz) sz, (Pi sz sz) q and ((Pi sz sz) q) w_I -- 2^-53 each: term_bound + 4 x 2^-53.  Then the phase
                 and the sum as before:
                 (term_bound + 4 x 2^-53 + phase_bound + n_terms 2^-53) (1 + 2^-22) flux.
A plane that is empty in the reference must be exactly 0 + 0i in all three.
"""
import ctypes
import os

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import LC_GRIDS
from test_hotspot_records_host import NUMPY_CASES, NUMPY_IDS, isco_ref, lc_bound, synth
from test_polarization_host import synth_pol
from test_spectrum_host import DISK_EXPOSURE, SPOT, U, short_times
from test_visibility_host import BASELINES, VisibilityReference, check_visibility, phase_bound, visibility_case

LD = np.longdouble
FIELD = diskmod.BField(0.3, -0.5, 1.0, pol_frac=0.6)
QU_SLACK = 1.0 + 2.0 ** -22                                  # |w_Q|, |w_U| <= QU_SLACK w_I (derived above)
QU_PRODUCTS = 4 * U                                          # the four extra rounded products of w_Q and w_U


# ---- the reference ------------------------------------------------------------------------------------------------------
class StokesVisibilityReference:
    """I, Q and U visibilities of one record buffer in longdouble, on a VisibilityReference of the same hits."""

    def __init__(self, vref, pol, pol_frac):
        self.vref = vref
        s = vref.ref.spot_ref
        rec = np.asarray(pol, dtype=np.float32).reshape(-1, vref.m, 4)[s.pix, s.slot].astype(LD)
        pw = LD(pol_frac) * rec[:, 2] * rec[:, 2]
        self.factors = (None, pw * rec[:, 0], pw * rec[:, 1])

    def visibility(self, weights, uv, split):
        """-> [(re, im, flux)] for I, Q, U: (planes, n_baselines) twice and the plane's flux of w_I (planes,), longdouble."""
        i = self.vref.visibility(weights, uv, split)
        return [i] + [self.vref.visibility(weights * f, uv, split)[:2] + (i[2],) for f in self.factors[1:]]


def check_visibility_stokes(got, wants, counts, term_bound, ph_bound):
    """got complex128 (..., planes, 3, n_b) against wants = [(re, im, flux)] of I, Q, U: check_visibility per Stokes plane
    with the bounds derived above.  -> the largest difference in units of its bound, per Stokes parameter."""
    got = np.asarray(got)
    assert got.dtype == np.complex128 and got.shape[-2] == 3
    out = [check_visibility(got[..., 0, :], wants[0], counts, term_bound, ph_bound)]
    for c in (1, 2):
        re, im, flux = wants[c]
        out.append(check_visibility(got[..., c, :], (re, im, flux * LD(QU_SLACK)), counts, term_bound + QU_PRODUCTS, ph_bound))
    return out


def stack_stokes(per_time):
    """[[(re, im, flux)] x 3 per time] -> [(re, im, flux)] x 3 with a leading time axis."""
    return [tuple(np.stack(x) for x in zip(*[w[c] for w in per_time])) for c in range(3)]


_SREF = {}


def stokes_case(ci):
    """(hits, n_hits, pol, SpectrumReference, StokesVisibilityReference) of NUMPY_CASES[ci], made once."""
    if ci not in _SREF:
        R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
        hits, n_hits, ref, vref = visibility_case(ci)
        pol = synth_pol((R, W, m), seed + 100)
        _SREF[ci] = (hits, n_hits, pol, ref, StokesVisibilityReference(vref, pol, FIELD.pol_frac))
    return _SREF[ci]


# ---- 1. the numpy statements against the reference -------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(NUMPY_CASES)), ids=NUMPY_IDS)
def test_numpy_polarized_visibilities_against_the_reference(ci):
    R, W, m, M, a, r_out, seed = NUMPY_CASES[ci]
    hits, n_hits, pol, ref, sref = stokes_case(ci)
    dk = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE)
    spot = SPOT(M)
    pb = phase_bound(R, W)
    worst = dict(disk=[0.0] * 3, spot=[0.0] * 3)
    disk_w = ref.disk_weights(float(isco_ref(M, a)), dk.q, dk.exposure)
    for split in (False, True):
        nh = n_hits if split else None                   # with the counts and with the NaN padding
        counts = sref.vref.counts(split)
        got = diskmod.disk_visibility_stokes(M, a, hits, nh, pol, dk, BASELINES, FIELD, split)
        assert got.shape == (m if split else 1, 3, len(BASELINES))
        assert np.array_equal(got[:, 0], diskmod.disk_visibility(M, a, hits, nh, dk, BASELINES, split))      # the I plane, exactly
        worst["disk"] = np.maximum(worst["disk"], check_visibility_stokes(got, sref.visibility(disk_w, BASELINES, split), counts, 1e-12, pb))
        assert np.all(got[:, :, 0].imag == 0)                                # the zero baseline is a real sum, Q and U included
        times = short_times(LC_GRIDS[int(split)])
        got = diskmod.hotspot_visibility_stokes(M, a, hits, nh, pol, diskmod.HotSpot(*spot), BASELINES, FIELD, split, times)
        assert got.shape == (len(times), m if split else 1, 3, len(BASELINES))
        assert np.array_equal(got[:, :, 0], diskmod.hotspot_visibility(M, a, hits, nh, diskmod.HotSpot(*spot), BASELINES, split, times))
        want = stack_stokes([sref.visibility(ref.spot_weights(M, a, spot, t), BASELINES, split) for t in times])
        worst["spot"] = np.maximum(worst["spot"], check_visibility_stokes(got, want, counts, lc_bound(M, a, spot, times, r_out), pb))
    for who, excess in worst.items():
        print(f"{NUMPY_IDS[ci]} {who}: numpy I, Q, U against longdouble, {excess[0]:.3f}, {excess[1]:.3f}, {excess[2]:.3f} of their bounds")
        assert max(excess) <= 1


# ---- 2. exact properties of the numpy statement --------------------------------------------------------------------------
def test_unpolarized_light_has_no_q_and_u():
    R, W, m, M, a, r_out, seed = NUMPY_CASES[2]
    hits, n_hits, pol, ref, sref = stokes_case(2)
    dark = diskmod.BField(0.3, -0.5, 1.0, pol_frac=0.0)
    dk, spot = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE), diskmod.HotSpot(*SPOT(M))
    for split in (False, True):
        V = diskmod.disk_visibility_stokes(M, a, hits, n_hits, pol, dk, BASELINES, dark, split)
        assert np.all(V[:, 1:] == 0) and np.array_equal(V[:, 0], diskmod.disk_visibility(M, a, hits, n_hits, dk, BASELINES, split))
        V = diskmod.hotspot_visibility_stokes(M, a, hits, n_hits, pol, spot, BASELINES, dark, split, [333.25, 340.0])
        assert np.all(V[:, :, 1:] == 0) and np.array_equal(V[:, :, 0], diskmod.hotspot_visibility(M, a, hits, n_hits, spot, BASELINES, split, [333.25, 340.0]))
        assert np.any(V[:, :, 0] != 0)


def test_planes_add_up_to_the_unsplit_result():
    R, W, m, M, a, r_out, seed = NUMPY_CASES[2]
    hits, n_hits, pol, ref, sref = stokes_case(2)
    spot = diskmod.HotSpot(*SPOT(M))
    whole = diskmod.hotspot_visibility_stokes(M, a, hits, n_hits, pol, spot, BASELINES, FIELD, False, [333.25])
    per = diskmod.hotspot_visibility_stokes(M, a, hits, n_hits, pol, spot, BASELINES, FIELD, True, [333.25])
    assert whole.shape == (1, 1, 3, 9) and per.shape == (1, m, 3, 9)
    scale = np.abs(whole[:, :, :1, :1])                                     # the flux: I at the zero baseline
    assert np.all(scale > 0) and np.all(np.abs(per.sum(axis=1, keepdims=True) - whole) <= 1e-12 * scale)
    assert np.all(np.abs(per[0, :, 1:]).sum(axis=(1, 2)) > 0)               # every order holds polarized light


def test_fractional_polarization():
    R, W, m, M, a, r_out, seed = NUMPY_CASES[2]
    hits, n_hits, pol, ref, sref = stokes_case(2)
    aligned = pol.copy()
    aligned[..., 0], aligned[..., 1] = 1.0, 0.0                             # every q = 1: m(0, 0) = sum Pi sz^2 w / sum w <= Pi
    dk = diskmod.ThinDisk(r_out=r_out, exposure=DISK_EXPOSURE)
    for split in (False, True):
        V = diskmod.disk_visibility_stokes(M, a, hits, n_hits, aligned, dk, BASELINES, FIELD, split)
        frac = diskmod.fractional_polarization(V)
        assert frac.shape == (m if split else 1, 9) and frac.dtype == np.complex128
        assert np.all(np.abs(frac[:, 0]) <= FIELD.pol_frac * (1 + 1e-12)) and np.all(frac[:, 0].real > 0) and np.all(frac[:, 0].imag == 0)
        assert np.array_equal(frac, (V[:, 1] + 1j * V[:, 2]) / V[:, 0])
    V = np.zeros((2, 3, 4), dtype=np.complex128)
    V[0] = [[2, 2j, 0, 1], [1, 1, 5, 0], [0, 1, 5, 0]]                      # (1 + i) / 2i = (1 - i) / 2
    frac = diskmod.fractional_polarization(V)
    assert np.array_equal(frac[0, [0, 1, 3]], [0.5, 0.5 - 0.5j, 0]) and np.isnan(frac[0, 2]) and np.all(np.isnan(frac[1]))
    with np.errstate(all="raise"):                                            # (no warning where I~ is 0)
        diskmod.fractional_polarization(V)


def test_skipped_slots_and_records_that_are_not_numbers():
    """A slot whose g is NaN is skipped in all three planes; a NaN in the polarization record of a kept slot is the record's
    answer and reaches Q and U, not I."""
    M, a = 1.0, 0.9
    dk = diskmod.ThinDisk(r_out=20.0, exposure=1.0)
    hits, n_hits = synth(4, 6, 2, 5, float(diskmod.isco(M, a)), 20.0)
    hits, n_hits = synth_filled(hits), np.full_like(n_hits, 2)
    pol = synth_pol((4, 6, 2), 9)
    want = diskmod.disk_visibility_stokes(M, a, hits, n_hits, pol, dk, BASELINES, FIELD, True)
    holed, hpol = hits.copy(), pol.copy()
    holed[1, 2, 0, 2] = np.nan                                              # g of one slot: skipped
    hpol[1, 2, 0] = np.nan                                                  # (its record does not matter then)
    got = diskmod.disk_visibility_stokes(M, a, holed, n_hits, hpol, dk, BASELINES, FIELD, True)
    assert not np.isnan(got).any() and np.array_equal(got[1], want[1]) and not np.array_equal(got[0], want[0])
    hpol = pol.copy()
    hpol[3, 5, 1, 0] = np.nan                                               # q of a kept slot of order 1
    got = diskmod.disk_visibility_stokes(M, a, hits, n_hits, hpol, dk, BASELINES, FIELD, True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1, 0], want[1, 0]) and np.array_equal(got[1, 2], want[1, 2])
    assert np.all(np.isnan(got[1, 1].real))


def synth_filled(hits):
    """hits with every slot stored: the NaN padding replaced by a valid record."""
    out = hits.copy()
    out[np.isnan(out[..., 0])] = np.array([8.0, 1.0, 0.75, 100.0], dtype=np.float32)
    return out


# ---- 3. constants, exports and bindings, the CLI ------------------------------------------------------------------------------
def test_constants_and_the_workspace():
    assert ltrace.visibility_stokes_batch_pairs() == ltrace.VISIBILITY_STOKES_BATCH_PAIRS == 5
    assert 3 * ltrace.VISIBILITY_STOKES_BATCH_PAIRS <= ltrace.VISIBILITY_BATCH_TERMS
    # the partials of one batch of pairs at the most baselines: 60 MiB of the workspace's 64
    one_batch = ltrace.VISIBILITY_BLOCKS * 3 * ltrace.VISIBILITY_STOKES_BATCH_PAIRS * ltrace.VISIBILITY_MAX_BASELINES * 16
    assert one_batch == 60 << 20 and one_batch <= ltrace.VISIBILITY_WORKSPACE_BYTES
    header = open(os.path.join(os.path.dirname(os.path.abspath(ltrace.__file__)), "..", "include", "ltrace.h")).read()
    for text in ("#define LT_VISIBILITY_STOKES_BATCH_PAIRS 5", "polarized visibilities", "lt_visibility_stokes_batch_pairs"):
        assert text in header


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    field = ctypes.POINTER(ltrace.BField)
    for suffix in ("", "_dev"):
        for name, emitter in (("lt_disk_visibility", ltrace.Disk), ("lt_hotspot_visibility", ltrace.HotSpot)):
            new = name + "_stokes" + suffix
            assert hasattr(lib, new) and new in ltrace.SIGNATURES, new
            # the unpolarized arguments with pol after n_hits and the field after the emitter
            res, args = ltrace.SIGNATURES[name + suffix]
            at = args.index(ctypes.POINTER(emitter)) + 1
            assert ltrace.SIGNATURES[new] == (res, args[:2] + [ctypes.c_void_p] + args[2:at] + [field] + args[at:])
    assert hasattr(lib, "lt_visibility_stokes_batch_pairs") and "lt_visibility_stokes_batch_pairs" in ltrace.SIGNATURES
    for fn in (ltrace.disk_visibility_stokes, ltrace.disk_visibility_stokes_dev, ltrace.hotspot_visibility_stokes,
               ltrace.hotspot_visibility_stokes_dev, ltrace.visibility_stokes_batch_pairs):
        assert callable(fn)
    hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
    pol = synth_pol((4, 4, 2), 6)
    met, d, f = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(), FIELD.to_lt()
    with pytest.raises(ValueError):
        ltrace.disk_visibility_stokes(hits, n_hits, pol[:3], met, d, f, BASELINES)
    with pytest.raises(ValueError):
        ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, d, ltrace.default_hotspot(), f, np.zeros(4), False, 0.0, 1.0, 2)
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        b = BASELINES
        calls = (lambda: ltrace.disk_visibility_stokes(hits, n_hits, pol, met, d, f, b),
                 lambda: ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, d, ltrace.default_hotspot(), f, b, True, 0.0, 1.0, 4),
                 lambda: ltrace.disk_visibility_stokes_dev(8, 0, 8, 4, 4, 2, met, d, f, b, False, 8),
                 lambda: ltrace.hotspot_visibility_stokes_dev(8, 0, 8, 4, 4, 2, met, d, ltrace.default_hotspot(), f, b, False, 0.0, 1.0, 4, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE


SEQUENCE = ["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"]
SPOT_ARGS = ["--hotspot", "8", "0", "1.5"]
FIELD_ARGS = ["--bfield", "0", "0", "1", "--pol-frac", "0.5"]


def test_cli_builds_the_call_and_writes_the_files(tmp_path, monkeypatch):
    """--visibility with --bfield: render_sequence gets both, and the two new files are written next to the old ones."""
    import image_lens
    seen = {}

    def fake(source_image, metric, r_obs, fov, tdisk, hotspot, times, **kw):
        seen.update(kw, times=times, hotspot=hotspot)
        n, planes, nb = len(times), kw["baselines"].planes(tdisk.max_images), len(kw["baselines"])
        out = dict(rgba=np.zeros((n, 12, 16, 4), np.uint8), lightcurve=np.zeros((n, 3)), stats=dict(integrate_ms=0.0),
                   visibility=np.full((n, planes, nb), 1 + 0j), disk_visibility=np.full((planes, nb), 2 + 0j))
        if kw["bfield"] is not None:
            out.update(stokes=np.zeros((n, 12, 16, 3), np.float32), stokes_lightcurve=np.zeros((n, 3)),
                       visibility_stokes=np.full((n, planes, 3, nb), 3 + 0j), disk_visibility_stokes=np.full((planes, 3, nb), 4 + 0j))
        return out

    monkeypatch.setattr(image_lens, "render_sequence", fake)
    stem = str(tmp_path / "ring")
    argv = SEQUENCE + SPOT_ARGS + FIELD_ARGS + ["--times", "0", "10", "2", "--visibility", "3", "0.5", "0", "--visibility-orders", "--output", stem + ".png"]
    image_lens.main_sequence(image_lens.build_parser().parse_args(argv), diskmod.TransparentDisk(max_images=3))
    assert seen["bfield"].pol_frac == 0.5 and seen["baselines"].split_orders and np.array_equal(seen["baselines"].uv, [(0, 0), (0.25, 0), (0.5, 0)])
    assert np.load(stem + "_visibility_stokes.npy").shape == (2, 3, 3, 3) and np.load(stem + "_disk_visibility_stokes.npy").shape == (3, 3, 3)
    assert np.load(stem + "_visibility.npy").shape == (2, 3, 3) and os.path.exists(stem + "_baselines.npy")
    # without a field the old files alone
    stem = str(tmp_path / "plain")
    argv = SEQUENCE + SPOT_ARGS + ["--times", "0", "10", "2", "--visibility", "3", "0.5", "0", "--output", stem + ".png"]
    image_lens.main_sequence(image_lens.build_parser().parse_args(argv), diskmod.TransparentDisk(max_images=3))
    assert seen["bfield"] is None and os.path.exists(stem + "_visibility.npy") and not os.path.exists(stem + "_visibility_stokes.npy")
    # a field without a spot is a sequence too: the baselines are built
    args = image_lens.build_parser().parse_args(SEQUENCE + FIELD_ARGS + ["--visibility", "3", "0.5", "0"])
    assert len(image_lens.baselines_from_args(args)) == 3


@pytest.mark.parametrize("argv,match", [(SEQUENCE + FIELD_ARGS + ["--visibility-orders"], "--visibility-orders"),
                                        (SEQUENCE + FIELD_ARGS + ["--visibility", "7.5", "0.5", "0"], "N must"),
                                        (SEQUENCE + FIELD_ARGS + ["--visibility", "8", "0.6", "0"], "0.5"),
                                        (SEQUENCE + FIELD_ARGS + ["--disk-map", "spiral", "--visibility", "8", "0.5", "0"], "not polarized")])
def test_cli_refusals_are_unchanged(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    with pytest.raises(ValueError, match=match):
        image_lens.main_sequence(args, diskmod.TransparentDisk(max_images=3))
    with pytest.raises(ValueError, match="not polarized"):     # render_sequence keeps refusing a map with a field
        image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), None, [0.0, 10.0], shape=(8, 8), bfield=FIELD,
                                   diskmap=diskmod.DiskMap(np.ones((2, 3), np.float32)), baselines=diskmod.Baselines(BASELINES))
