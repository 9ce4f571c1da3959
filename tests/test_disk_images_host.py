"""CPU tests of the optically thin disk: the colour rule of disk.shade_images, TransparentDisk, the bindings of
lt_render_disk_images / lt_trace_batch_kerr_disk_images and their answer on a machine without a GPU
(include/ltrace.h, "optically thin disk")."""
import ctypes as C

import numpy as np
import pytest

import disk
import ltrace
import metrics


def _hits(rng, shape, m):
    """Random stored hits: r in [r_in, 20], phi in [0, 2 pi), g in [0.3, 1.6]."""
    r = rng.uniform(2.3209, 20.0, shape + (m,))
    ph = rng.uniform(0.0, 2 * np.pi, shape + (m,))
    g = rng.uniform(0.3, 1.6, shape + (m,))
    return np.stack([r, ph, g], axis=-1).astype(np.float32)


@pytest.mark.parametrize("channels", [1, 3])
def test_one_hit_on_black_equals_opaque_shade(channels):
    rng = np.random.default_rng(1)
    r_in = 2.3209
    img = _hits(rng, (400,), 3)
    n_hits = np.ones(400, dtype=np.uint8)
    img[:, 1:] = np.nan
    for q, exposure in ((3.0, 1.0), (2.0, 0.3)):
        ref = disk.shade(img[:, 0, 0], img[:, 0, 2], r_in, q=q, exposure=exposure, channels=channels)
        # below saturation: every channel of the unclamped emission is <= 1
        x = r_in / img[:, 0, 0].astype(np.float64)
        g = img[:, 0, 2].astype(np.float64)
        below = exposure * g ** 4 * x ** q <= 1.0
        assert below.sum() > 50
        base = np.zeros((400, 3) if channels == 3 else (400,), np.float32)
        got = disk.shade_images(base, img, n_hits, r_in, q=q, exposure=exposure, channels=channels)
        assert got.dtype == np.float32 and got.shape == base.shape
        np.testing.assert_array_equal(got[below], ref[below])


def _reference(base, img, n_hits, r_in, q, exposure, channels):
    """The rule of include/ltrace.h written out pixel by pixel."""
    out = np.array(base, dtype=np.float32, copy=True)
    for p in np.ndindex(*np.shape(n_hits)):
        ns = min(int(n_hits[p]), img.shape[-2])
        if ns == 0:
            continue
        acc = np.array(base[p], dtype=np.float64).reshape(-1)
        for j in range(ns):
            r, g = float(img[p][j, 0]), float(img[p][j, 2])
            x = r_in / r
            intensity = exposure * g ** 4 * x ** q
            s = g * x ** 0.75
            e = np.array([intensity * min(max(2 * s - 0.5 * i, 0.0), 1.0) for i in range(3)])
            acc = acc + ((e[0] + e[1] + e[2]) / 3.0 if channels == 1 else e)
        out[p] = np.clip(acc, 0.0, 1.0).astype(np.float32).reshape(np.shape(out[p]))
    return out


@pytest.mark.parametrize("channels", [1, 3])
def test_sum_and_clamp(channels):
    rng = np.random.default_rng(7)
    r_in, m = 6.0, 3
    shape = (9, 11)
    img = _hits(rng, shape, m)
    img[..., 0] = rng.uniform(6.0, 20.0, shape + (m,))
    n_hits = rng.integers(0, 6, shape).astype(np.uint8)      # 0 ... 5: beyond max_images too
    for p in np.ndindex(*shape):                             # slots at or beyond n_hits are NaN, as the renderer writes
        img[p][min(int(n_hits[p]), m):] = np.nan
    base = rng.uniform(0.0, 1.0, shape + ((3,) if channels == 3 else ())).astype(np.float32)
    for q, exposure in ((3.0, 1.0), (3.0, 8.0), (1.5, 0.05)):
        got = disk.shade_images(base, img, n_hits, r_in, q=q, exposure=exposure, channels=channels)
        np.testing.assert_array_equal(got, _reference(base, img, n_hits, r_in, q, exposure, channels))
    # no stored hit: the base, bit for bit
    none = disk.shade_images(base, img, np.zeros(shape, np.uint8), r_in, channels=channels)
    assert none.tobytes() == base.tobytes()


def test_hand_built_cases():
    r_in = 6.0
    nan = np.nan
    # r = r_in, g = 0.5: I = g^4 = 0.0625, s = 0.5, ramp = (1, 0.5, 0)
    one = [6.0, 1.0, 0.5]
    img = np.array([[one, [nan] * 3, [nan] * 3],
                    [one, one, [nan] * 3],
                    [one, one, one],
                    [one, one, one]], np.float32)
    n_hits = np.array([1, 2, 3, 200], np.uint8)
    base = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, 1.0], [0.9, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    got = disk.shade_images(base, img, n_hits, r_in)
    e = np.array([0.0625, 0.03125, 0.0])
    want = np.array([e, [0.25, 0.5, 1.0] + 2 * e, [0.9, 0.0, 0.0] + 3 * e, 3 * e]).clip(0, 1).astype(np.float32)
    np.testing.assert_array_equal(got, want)
    assert got[1, 2] == 1.0                                  # clamped after the sum
    # exposure large enough to saturate: clamp to 1, and the unclamped terms add before the clamp
    got = disk.shade_images(np.zeros((1, 3), np.float32), img[:1, :1], np.array([1]), r_in, exposure=32.0)
    np.testing.assert_array_equal(got, np.array([[1.0, 1.0, 0.0]], np.float32))
    # 1 channel: the mean of the three channels of each E_j
    got = disk.shade_images(np.array([0.1, 0.0], np.float32), img[1:3, :, :], np.array([2, 3]), r_in, channels=1)
    m = e.sum() / 3.0
    np.testing.assert_array_equal(got, np.array([float(np.float32(0.1)) + m + m, m + m + m], np.float32))


def test_transparent_disk():
    t = disk.TransparentDisk()
    assert isinstance(t, disk.ThinDisk)
    assert (t.r_in, t.r_out, t.q, t.exposure, t.max_images) == (None, 20.0, 3.0, 1.0, 3)
    lt = disk.TransparentDisk(r_in=3.0, r_out=15.0, q=2.5, exposure=0.5, max_images=5).to_lt()
    assert isinstance(lt, ltrace.Disk)
    assert (lt.r_in, lt.r_out, lt.q, lt.exposure, lt.flags) == (3.0, 15.0, 2.5, 0.5, 0)
    assert disk.TransparentDisk().to_lt().r_in == 0.0


def test_bindings():
    lib = ltrace.load()
    for name in ("lt_render_disk_images", "lt_render_disk_images_dev", "lt_trace_batch_kerr_disk_images"):
        assert hasattr(lib, name), name
        assert name in ltrace.SIGNATURES
    assert ltrace.STAT_DISK_HITS == 13 and ltrace.STAT_DISK_HITS < ltrace.STAT_WORDS
    assert ltrace.DISK_MAX_IMAGES == 8
    assert callable(metrics.Kerr.trace_rays_batch_disk_images)
    for f in (ltrace.render_disk_images, ltrace.render_disk_images_dev, ltrace.trace_batch_kerr_disk_images):
        assert callable(f)


def test_no_device_answers():
    if ltrace.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device answer is for machines without one")
    lib = ltrace.load()
    cam = ltrace.Camera(16, 16, 0.5, 0.5, 0.0, 0.0, 50.0, 1.4)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    o = ltrace.default_opts()
    d = ltrace.default_disk()
    rc = lib.lt_render_disk_images(C.byref(cam), C.byref(met), C.byref(o), C.byref(d), 3, None, 3, None, None, None,
                                   None, None, None, None, None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    rc = lib.lt_render_disk_images_dev(C.byref(cam), C.byref(met), C.byref(o), C.byref(d), 3, None, 3, None, None,
                                       None, None, None, None, None, None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    al = np.zeros(4)
    rc = lib.lt_trace_batch_kerr_disk_images(1.0, 0.9, 50.0, al.ctypes.data, al.ctypes.data, 1.4, 5000.0, None, 1, 32,
                                             C.byref(d), 3, 4, None, None, None, None, None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    with pytest.raises(ltrace.LtraceError):
        ltrace.trace_batch_kerr_disk_images(1.0, 0.9, 50.0, al, al, 1.4, 5000.0, d)
