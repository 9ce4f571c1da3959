"""Host-side checks of the supersampled frame: aa.py (the numpy statement of the resolve rule of include/ltrace.h,
"supersampled frames") against loops written out pixel by pixel, the bindings, the plan (lt_aa_band_bytes: pure host
arithmetic) and the entry points' answer on a machine without a GPU."""
import ctypes

import numpy as np
import pytest

import aa
import ltrace


def _resolve_loop(fine, S):
    """The rule of include/ltrace.h written out: per pixel and channel, float64 from 0.0, j outer, i inner."""
    fine3 = fine if fine.ndim == 3 else fine[..., None]
    H, W, C = fine3.shape[0] // S, fine3.shape[1] // S, fine3.shape[2]
    out = np.empty((H, W, C), dtype=np.float32)
    for y in range(H):
        for x in range(W):
            for c in range(C):
                acc = 0.0
                for j in range(S):
                    for i in range(S):
                        acc = acc + float(fine3[y * S + j, x * S + i, c])
                out[y, x, c] = np.float32(acc / float(S * S))
    return out if fine.ndim == 3 else out[..., 0]


@pytest.mark.parametrize("S", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("channels", [1, 3])
def test_resolve_is_the_ordered_float64_mean(S, channels):
    rng = np.random.default_rng(100 * S + channels)
    shape = (5 * S, 7 * S) if channels == 1 else (5 * S, 7 * S, 3)
    # magnitudes from 1e-30 to 1: the order of the additions decides the last bits of the float64 sum
    fine = (10.0 ** rng.uniform(-30.0, 0.0, size=shape)).astype(np.float32)
    got = aa.resolve(fine, S)
    assert got.dtype == np.float32 and got.shape == (5, 7) + shape[2:]
    np.testing.assert_array_equal(got, _resolve_loop(fine, S))


def test_resolve_of_one_sample_is_the_frame():
    fine = np.random.default_rng(1).random((6, 9, 3), dtype=np.float32)
    fine[0, 0] = (np.float32(1e-38), np.float32(0.0), np.float32(np.nextafter(np.float32(1), np.float32(0))))
    assert aa.resolve(fine, 1).tobytes() == fine.tobytes()
    assert aa.resolve(fine[..., 0].copy(), 1).tobytes() == fine[..., 0].tobytes()


def test_hand_built_cases():
    block = np.array([[1, 0], [0, 0]], dtype=np.float32)
    r = aa.resolve(block, 2)
    assert r.shape == (1, 1) and r[0, 0] == np.float32(0.25)
    assert aa.to_rgba8(r).tolist() == [[[63, 63, 63, 255]]]                     # 0.25 * 255 = 63.75, truncated
    rgb = np.zeros((2, 4, 3), dtype=np.float32)
    rgb[0, 0] = (1, 0.5, 0)
    rgb[1, 3] = (0, 0, 1)
    r = aa.resolve(rgb, 2)
    assert r.shape == (1, 2, 3) and r[0, 0].tolist() == [0.25, 0.125, 0.0] and r[0, 1].tolist() == [0.0, 0.0, 0.25]
    assert aa.to_rgba8(r)[0].tolist() == [[63, 31, 0, 255], [0, 0, 63, 255]]
    assert aa.to_rgba8(np.array([[1.0, 0.999]], dtype=np.float32)).tolist() == [[[255, 255, 255, 255], [254, 254, 254, 255]]]
    thirds = aa.resolve(np.array([[1, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.float32), 3)
    assert thirds[0, 0] == np.float32(1.0 / 9.0)
    with pytest.raises(ValueError):
        aa.resolve(np.zeros((5, 4), dtype=np.float32), 2)
    with pytest.raises(ValueError):
        aa.resolve(np.zeros((4, 4), dtype=np.float64), 2)


@pytest.mark.parametrize("mode", [aa.PLAIN, aa.DISK, aa.DISK_IMAGES])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_cover_counts_the_classes(mode, S):
    rng = np.random.default_rng(10 * S + mode)
    H, W = 4, 5
    classes = [1, -1, 0] + ([2] if mode == aa.DISK else [])
    status = rng.choice(classes, size=(H * S, W * S)).astype(np.int8)
    n_hits = rng.integers(0, 3, size=(H * S, W * S)).astype(np.uint8)
    got = aa.cover(status, n_hits if mode == aa.DISK_IMAGES else None, S, mode)
    assert got.dtype == np.uint8 and got.shape == (H, W, 4)
    for y in range(H):
        for x in range(W):
            n = [0, 0, 0, 0]
            for j in range(S):
                for i in range(S):
                    st = status[y * S + j, x * S + i]
                    n[0] += st == 1
                    n[1] += st == -1
                    n[2] += st == 0
                    if mode == aa.DISK:
                        n[3] += st == 2
                    elif mode == aa.DISK_IMAGES:
                        n[3] += n_hits[y * S + j, x * S + i] > 0
            assert got[y, x].tolist() == n
    assert np.all(got[..., :3 if mode != aa.DISK else 4].astype(int).sum(axis=2) == S * S)
    if mode == aa.PLAIN:
        assert not got[..., 3].any()


def test_bindings_are_present():
    lib = ltrace.load()
    for name in ("lt_default_aa", "lt_render_aa", "lt_render_aa_dev", "lt_aa_band_bytes"):
        assert hasattr(lib, name) and name in ltrace.SIGNATURES, name
    for fn in (ltrace.default_aa, ltrace.render_aa, ltrace.render_aa_dev, ltrace.aa_band_bytes):
        assert callable(fn)
    assert (ltrace.AA_PLAIN, ltrace.AA_DISK, ltrace.AA_DISK_IMAGES) == (aa.PLAIN, aa.DISK, aa.DISK_IMAGES) == (0, 1, 2)
    a = ltrace.default_aa()
    assert (a.samples, a.mode, a.max_images, a.band_rows) == (2, ltrace.AA_PLAIN, 3, 0)
    a = ltrace.default_aa(samples=4, mode="disk_images", max_images=5, band_rows=32)
    assert (a.samples, a.mode, a.max_images, a.band_rows) == (4, ltrace.AA_DISK_IMAGES, 5, 32)
    assert ctypes.sizeof(ltrace.AA) == 16


def _cam(W=1024, H=1024):
    fov = np.radians(40.0)
    return ltrace.Camera(W, H, fov, fov, 0.0, 0.0, 50.0, np.radians(80.0)), ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)


def test_plan_is_host_arithmetic():
    """Bands: the automatic band is the largest whose records fit LT_AA_BAND_BYTES; the refusals need no device."""
    cam, met = _cam()
    # 1024^2 x 4^2 rays x three float4: 0.75 GiB, one band
    n, rows, bands = ltrace.aa_band_bytes(cam, met, ltrace.default_opts(), ltrace.default_aa(samples=4))
    assert (rows, bands) == (1024, 1) and 4096 * 4096 * 48 <= n <= 4096 * 4096 * 48 + 8192
    # x 8^2: 3 GiB, more than one band, each within the budget and a multiple of the row block
    n, rows, bands = ltrace.aa_band_bytes(cam, met, ltrace.default_opts(), ltrace.default_aa(samples=8))
    assert bands == -(-1024 // rows) > 1 and rows % 16 == 0 and n <= ltrace.AA_BAND_BYTES
    assert (rows + 16) * 8 * 8192 * 48 > ltrace.AA_BAND_BYTES            # one more row block would not fit
    # float64 and the thin disk's slots make a ray's records larger
    n64, rows64, _ = ltrace.aa_band_bytes(cam, met, ltrace.default_opts(precision=64, integrator="dp45_exact"),
                                          ltrace.default_aa(samples=8, mode="disk_images", max_images=3), disk=ltrace.default_disk())
    assert rows64 < rows and n64 <= ltrace.AA_BAND_BYTES
    # an explicit band, a partition
    n, rows, bands = ltrace.aa_band_bytes(cam, met, ltrace.default_opts(n_parts=4, part=1), ltrace.default_aa(samples=2, band_rows=64))
    assert (rows, bands) == (64, 4) and n >= 64 * 2 * 2048 * 48

    def code(opts, a, disk=None, metric=met):
        with pytest.raises(ltrace.LtraceError) as ei:
            ltrace.aa_band_bytes(cam, metric, opts, a, disk=disk)
        return ei.value.code

    assert code(ltrace.default_opts(), ltrace.default_aa(samples=0)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ltrace.default_aa(samples=9)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ltrace.default_aa(band_rows=24)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ltrace.default_aa(mode="disk")) == ltrace.ERR_INVALID_ARG                  # no disk
    assert code(ltrace.default_opts(schedule="queue"), ltrace.default_aa(mode="disk"), ltrace.default_disk()) == ltrace.ERR_UNSUPPORTED
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    assert code(ltrace.default_opts(), ltrace.default_aa(mode="disk_images"), ltrace.default_disk(), schw) == ltrace.ERR_UNSUPPORTED


@pytest.mark.skipif(ltrace.device_count() > 0, reason="GPU present")
def test_no_gpu_means_no_device():
    cam, met = _cam(64, 48)
    lib = ltrace.load()
    a, o = ltrace.default_aa(), ltrace.default_opts()
    rgb = np.zeros((48, 64, 3), dtype=np.float32)
    st = ltrace.Stats()
    rc = lib.lt_render_aa(ctypes.byref(cam), ctypes.byref(met), ctypes.byref(o), ctypes.byref(a), None, None, 3,
                          ctypes.c_void_p(rgb.ctypes.data), None, None, ctypes.byref(st))
    assert rc == ltrace.ERR_NO_DEVICE
    rc = lib.lt_render_aa_dev(ctypes.byref(cam), ctypes.byref(met), ctypes.byref(o), ctypes.byref(a), None, None, 3, None, None,
                              None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    bad = ltrace.default_aa(samples=0)      # no device comes first, as for every compute entry point
    assert lib.lt_render_aa_dev(ctypes.byref(cam), ctypes.byref(met), ctypes.byref(o), ctypes.byref(bad), None, None, 3, None,
                                None, None, None) == ltrace.ERR_NO_DEVICE
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.render_aa(cam, met, o, a)
    assert ei.value.code == ltrace.ERR_NO_DEVICE
    assert not rgb.any()


def test_image_lens_accepts_samples():
    import image_lens
    ap = image_lens.build_parser()
    assert ap.parse_args([]).samples is None
    args = ap.parse_args(["--a", "0.9", "--synthetic", "256", "192", "--disk-images", "3", "--samples", "4"])
    assert args.samples == 4 and args.disk_images == 3 and args.synthetic == [256, 192]
    with pytest.raises(ValueError):         # the background must be the fine frame
        import metrics
        image_lens.render_frame(np.zeros((9, 8, 3), dtype=np.float32), metrics.Kerr(1.0, 0.9), 50.0, (0.7, 0.7), samples=2)
