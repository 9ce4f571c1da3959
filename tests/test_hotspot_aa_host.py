"""Host-side checks of the supersampled hot-spot and Stokes frames (include/ltrace.h, "supersampled hot-spot and Stokes
frames"): the numpy statements disk.shade_hotspot_aa / disk.stokes_frame_aa, the argument errors that need no GPU, and
the library's exports.  tests/test_gpu_hotspot_aa.py imports replicate() and the cases from here.

Nothing here has a tolerance.  On records repeated S times per axis every sub-sample of a pixel is the same float32 x;
k x for k <= 64 is exact in float64 (a 24-bit mantissa times a 7-bit integer), so the ordered sum is S^2 x exactly and
(S^2 x) / S^2 rounds back to x: the resolved frame IS the one-sample frame of the unrepeated records."""
import ctypes

import numpy as np
import pytest

import aa
import disk as diskmod
import ltrace
from test_hotspot_records_host import synth
from test_polarization_host import FIELD, synth_pol

SPOT = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5, exposure=2.0, with_disk=True)
DISK = diskmod.ThinDisk(r_out=20.0, exposure=0.25)
M, A = 1.0, 0.9


def replicate(a, S):
    """Records (R, W, ...) -> (R S, W S, ...): every pixel repeated S times per axis."""
    return np.repeat(np.repeat(a, S, axis=0), S, axis=1)


def records(R, W, m, seed, M_=M, a=A, r_out=20.0):
    hits, n_hits = synth(R, W, m, seed, float(diskmod.isco(M_, a)), r_out)
    return hits, n_hits, synth_pol((R, W, m), seed + 100)


@pytest.mark.parametrize("S", [2, 3, 8])
def test_replicated_records(S):
    hits, n_hits, pol = records(9, 11, 4, 61)
    rng = np.random.default_rng(S)
    for channels, with_base, use_counts, t_obs in ((3, True, True, 333.25), (1, False, False, 1e5), (1, True, True, 0.0)):
        base = rng.uniform(0.0, 0.5, (9, 11) + ((3,) if channels == 3 else ())).astype(np.float32) if with_base else None
        nh = n_hits if use_counts else None
        one = diskmod.shade_hotspot(M, A, hits, nh, DISK, SPOT, t_obs, base=base, channels=channels)
        got = diskmod.shade_hotspot_aa(M, A, replicate(hits, S), None if nh is None else replicate(nh, S), DISK, SPOT, t_obs, S,
                                       base=None if base is None else replicate(base, S), channels=channels)
        assert got.dtype == np.float32 and got.shape == one.shape
        assert np.array_equal(got, one)
        assert (one > 0).sum() > 20
    one = diskmod.stokes_frame(M, A, hits, n_hits, pol, DISK, SPOT, 333.25, FIELD)
    got = diskmod.stokes_frame_aa(M, A, replicate(hits, S), replicate(n_hits, S), replicate(pol, S), DISK, SPOT, 333.25, FIELD, S)
    assert got.dtype == np.float32 and np.array_equal(got, one) and (one[..., 1] != 0).sum() > 20


@pytest.mark.parametrize("S,R,W,m", [(1, 4, 6, 3), (2, 5, 7, 3), (3, 7, 13, 3), (5, 3, 4, 8)])
def test_random_records(S, R, W, m):
    hits, n_hits, pol = records(R * S, W * S, m, 70 + S)
    base = np.random.default_rng(S).uniform(0.0, 0.5, (R * S, W * S, 3)).astype(np.float32)
    fine = diskmod.shade_hotspot(M, A, hits, n_hits, DISK, SPOT, 333.25, base=base)
    got = diskmod.shade_hotspot_aa(M, A, hits, n_hits, DISK, SPOT, 333.25, S, base=base)
    assert got.shape == (R, W, 3) and np.array_equal(got, aa.resolve(fine, S))
    if S == 1:
        assert np.array_equal(got, fine)
    else:
        assert not np.array_equal(got, fine[::S, ::S])          # the sub-samples differ: a mean, not a pick
    gray = diskmod.shade_hotspot_aa(M, A, hits, None, DISK, SPOT, 0.0, S, channels=1)
    assert gray.shape == (R, W) and np.array_equal(gray, aa.resolve(diskmod.shade_hotspot(M, A, hits, None, DISK, SPOT, 0.0, channels=1), S))
    iqu = diskmod.stokes_frame_aa(M, A, hits, n_hits, pol, DISK, SPOT, 333.25, FIELD, S)
    assert iqu.shape == (R, W, 3) and np.array_equal(iqu, aa.resolve(diskmod.stokes_frame(M, A, hits, n_hits, pol, DISK, SPOT, 333.25, FIELD), S))


def test_argument_errors():
    import image_lens
    from metrics import Kerr
    metric = Kerr(M=M, a=A, integrator="rk4", precision=32)
    fov = (np.radians(40.0), np.radians(40.0))
    for S in (0, 9, -2):
        with pytest.raises(ValueError, match="samples"):
            image_lens.render_sequence(None, metric, 50.0, fov, diskmod.TransparentDisk(max_images=3), SPOT, [0.0, 10.0], shape=(8, 8),
                                       samples=S)
    with pytest.raises(ValueError, match="samples"):           # a background that is not the fine frame
        image_lens.render_sequence(np.zeros((9, 8, 3), np.float32), metric, 50.0, fov, diskmod.TransparentDisk(max_images=3), SPOT,
                                   [0.0], samples=2)
    hits, n_hits, pol = records(6, 9, 2, 5)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, A)
    d, s, b = ltrace.default_disk(), ltrace.default_hotspot(), ltrace.default_bfield()
    for S in (2, 4, 0):                                        # 6 x 9 is 3 x 3 samples per pixel and nothing else
        with pytest.raises(ValueError, match="samples per pixel"):
            ltrace.shade_hotspot_aa(hits, n_hits, S, met, d, s, 0.0)
        with pytest.raises(ValueError, match="samples per pixel"):
            ltrace.shade_stokes_aa(hits, n_hits, pol, S, met, d, s, b, 0.0)
    with pytest.raises(ValueError, match="base"):
        ltrace.shade_hotspot_aa(hits, n_hits, 3, met, d, s, 0.0, base=np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError):
        diskmod.shade_hotspot_aa(M, A, hits, n_hits, DISK, SPOT, 0.0, 2)


def test_cli_refuses_adaptive_sequences():
    import image_lens
    args = image_lens.build_parser().parse_args(["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12", "--hotspot", "8", "0", "1.5",
                                                 "--samples", "4", "--adaptive", "2"])
    with pytest.raises(ValueError, match="not adaptively sampled"):
        image_lens.main_sequence(args, diskmod.TransparentDisk(max_images=3))


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    for name in ("lt_shade_hotspot_aa", "lt_shade_hotspot_aa_dev", "lt_shade_stokes_aa", "lt_shade_stokes_aa_dev"):
        assert hasattr(lib, name) and name in ltrace.SIGNATURES, name
        twin = ltrace.SIGNATURES[name.replace("_aa", "")]
        res, args = ltrace.SIGNATURES[name]
        at = 4 if "hotspot" in name else 5                      # samples follows (R, W)
        assert res == twin[0] and args == twin[1][:at] + [ctypes.c_int32] + twin[1][at:], name
    for fn in (ltrace.shade_hotspot_aa, ltrace.shade_hotspot_aa_dev, ltrace.shade_stokes_aa, ltrace.shade_stokes_aa_dev):
        assert callable(fn)
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        hits, n_hits, pol = records(4, 4, 2, 5)
        met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, A)
        with pytest.raises(ltrace.LtraceError) as ei:
            ltrace.shade_hotspot_aa(hits, n_hits, 2, met, ltrace.default_disk(), ltrace.default_hotspot(), 0.0)
        assert ei.value.code == ltrace.ERR_NO_DEVICE
        with pytest.raises(ltrace.LtraceError) as ei:
            ltrace.shade_stokes_aa(hits, n_hits, pol, 2, met, ltrace.default_disk(), ltrace.default_hotspot(), ltrace.default_bfield(), 0.0)
        assert ei.value.code == ltrace.ERR_NO_DEVICE
