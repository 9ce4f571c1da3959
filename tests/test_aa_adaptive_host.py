"""Host-side checks of adaptive supersampling (include/ltrace.h, "adaptive supersampling"): aa.refine_mask and aa.compose
(the numpy statement of the rule) on hand-made arrays, the struct and its defaults, the plan (lt_aa_adaptive_plan: pure
host arithmetic) with every refusal, the header's prototypes against the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import aa
import ltrace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ESC, CAP = (1, 0, 0, 0), (0, 1, 0, 0)


def _cover(H, W, fill):
    c = np.zeros((H, W, 4), dtype=np.uint8)
    c[:] = fill
    return c


def _mask_loop(cover, rgb, S_lo, mode, contrast):
    """The definition pixel by pixel."""
    H, W = cover.shape[:2]
    out = np.zeros((H, W), dtype=bool)
    col = None if rgb is None else rgb.reshape(H, W, -1)
    for y in range(H):
        for x in range(W):
            c = cover[y, x]
            if mode == aa.DISK_IMAGES:
                f = sum(int(v != 0) for v in c[:3]) > 1 or 0 < c[3] < S_lo * S_lo
            else:
                f = sum(int(v != 0) for v in c) > 1
            for ny in range(max(0, y - 1), min(H, y + 2)):
                for nx in range(max(0, x - 1), min(W, x + 2)):
                    if (ny, nx) == (y, x):
                        continue
                    f = f or bool(np.any(cover[ny, nx] != c))
                    if contrast >= 0:
                        f = f or any(np.float32(abs(np.float32(col[y, x, ch] - col[ny, nx, ch]))) > np.float32(contrast)
                                     for ch in range(col.shape[2]))
            out[y, x] = f
    return out


def test_mixed_alone():
    cover = _cover(5, 6, (4, 0, 0, 0))
    mask = aa.refine_mask(cover, None, 2, aa.PLAIN, -1.0)
    assert not mask.any()
    for mode, px, want in ((aa.PLAIN, (3, 1, 0, 0), True), (aa.DISK, (3, 0, 0, 1), True), (aa.DISK, (0, 0, 0, 4), False),
                           (aa.PLAIN, (0, 4, 0, 0), False), (aa.DISK_IMAGES, (2, 2, 0, 0), True)):
        cover = _cover(5, 6, px)                      # every pixel the same: no edge anywhere
        mask = aa.refine_mask(cover, None, 2, mode, -1.0)
        assert mask.all() == want and mask.any() == want, (mode, px)


def test_thin_disk_slot_three():
    """DISK_IMAGES: slot 3 overlaps the others -- (4, 0, 0, 4) is uniform, (4, 0, 0, 2) is partly on the disk."""
    for px, S_lo, want in (((4, 0, 0, 4), 2, False), ((4, 0, 0, 2), 2, True), ((4, 0, 0, 0), 2, False), ((1, 0, 0, 1), 1, False),
                           ((9, 0, 0, 4), 3, True), ((4, 0, 0, 4), 3, True)):
        mask = aa.refine_mask(_cover(3, 3, px), None, S_lo, aa.DISK_IMAGES, -1.0)
        assert mask.all() == want and mask.any() == want, (px, S_lo)
    # the same bytes in the opaque disk's mode are two non-zero slots
    assert aa.refine_mask(_cover(3, 3, (4, 0, 0, 4)), None, 2, aa.DISK, -1.0).all()


def test_edge_alone_and_frame_corners():
    cover = _cover(6, 7, ESC)
    cover[0, 0] = CAP                                  # a corner: three neighbours
    mask = aa.refine_mask(cover, None, 1, aa.PLAIN, -1.0)
    want = np.zeros((6, 7), dtype=bool)
    want[0:2, 0:2] = True
    assert np.array_equal(mask, want)
    cover = _cover(6, 7, ESC)
    cover[5, 6] = CAP
    cover[3, 0] = CAP                                  # an edge pixel: five neighbours
    mask = aa.refine_mask(cover, None, 1, aa.PLAIN, -1.0)
    want = np.zeros((6, 7), dtype=bool)
    want[4:6, 5:7] = True
    want[2:5, 0:2] = True
    assert np.array_equal(mask, want)
    assert np.array_equal(mask, _mask_loop(cover, None, 1, aa.PLAIN, -1.0))
    # a one-pixel frame has no neighbour; a one-row frame only left and right ones
    assert not aa.refine_mask(_cover(1, 1, ESC), None, 1, aa.PLAIN, -1.0).any()
    row = _cover(1, 5, ESC)
    row[0, 2] = CAP
    assert aa.refine_mask(row, None, 1, aa.PLAIN, -1.0).tolist() == [[False, True, True, True, False]]
    # bytes that differ only in slot 3 are an edge too
    cover = _cover(3, 4, (1, 0, 0, 0))
    cover[1, 3] = (1, 0, 0, 1)
    assert aa.refine_mask(cover, None, 1, aa.DISK_IMAGES, -1.0).tolist() == [[False, False, True, True]] * 3


def test_contrast_on_off_and_exactly_equal():
    cover = _cover(4, 6, ESC)
    rgb = np.zeros((4, 6, 3), dtype=np.float32)
    rgb[:, 3:, 1] = np.float32(0.25)                   # a step of exactly 0.25 in one channel between columns 2 and 3
    assert not aa.refine_mask(cover, rgb, 1, aa.PLAIN, -1.0).any()
    assert not aa.refine_mask(cover, None, 1, aa.PLAIN, -0.5).any()
    assert not aa.refine_mask(cover, rgb, 1, aa.PLAIN, 0.25).any()          # equal to the difference: not flagged
    below = np.nextafter(np.float32(0.25), np.float32(0))
    mask = aa.refine_mask(cover, rgb, 1, aa.PLAIN, below)
    want = np.zeros((4, 6), dtype=bool)
    want[:, 2:4] = True
    assert np.array_equal(mask, want)
    assert np.array_equal(aa.refine_mask(cover, rgb, 1, aa.PLAIN, 0.0), want)
    # the comparison is float32's: 0.1f + 0.2f - 0.1f against 0.2f
    a, b = np.float32(0.1) + np.float32(0.2), np.float32(0.1)
    rgb = np.zeros((1, 2, 3), dtype=np.float32)
    rgb[0, 0, 2], rgb[0, 1, 2] = a, b
    d = np.float32(a - b)
    assert not aa.refine_mask(_cover(1, 2, ESC), rgb, 1, aa.PLAIN, d).any()
    assert aa.refine_mask(_cover(1, 2, ESC), rgb, 1, aa.PLAIN, np.nextafter(d, np.float32(0))).all()


def test_contrast_on_one_channel():
    cover = _cover(3, 5, CAP)
    gray = np.zeros((3, 5), dtype=np.float32)
    gray[1, 4] = 0.5
    mask = aa.refine_mask(cover, gray, 1, aa.PLAIN, 0.0625)
    want = np.zeros((3, 5), dtype=bool)
    want[:, 3:] = True
    assert np.array_equal(mask, want)
    assert np.array_equal(mask, _mask_loop(cover, gray, 1, aa.PLAIN, 0.0625))


@pytest.mark.parametrize("mode", [aa.PLAIN, aa.DISK, aa.DISK_IMAGES])
@pytest.mark.parametrize("contrast", [-1.0, 0.3])
def test_mask_against_the_definition_written_out(mode, contrast):
    rng = np.random.default_rng(17 + mode)
    H, W, S_lo = 7, 9, 2
    cover = np.zeros((H, W, 4), dtype=np.uint8)
    cover[..., 0] = 4
    for _ in range(6):                                  # a few pixels of other classes in a uniform frame
        y, x = rng.integers(0, H), rng.integers(0, W)
        cover[y, x] = [(0, 4, 0, 0), (2, 2, 0, 0), (4, 0, 0, 3) if mode == aa.DISK_IMAGES else (1, 0, 0, 3), (3, 0, 1, 0)][rng.integers(0, 4)]
    rgb = (rng.random((H, W, 3)) * 0.4).astype(np.float32)
    got = aa.refine_mask(cover, rgb, S_lo, mode, contrast)
    assert got.dtype == bool and np.array_equal(got, _mask_loop(cover, rgb, S_lo, mode, contrast))
    assert got.any() and not got.all()


def test_refine_mask_refuses_other_arrays():
    with pytest.raises(ValueError):
        aa.refine_mask(np.zeros((3, 3, 4), dtype=np.int32), None, 1, aa.PLAIN, -1.0)
    with pytest.raises(ValueError):
        aa.refine_mask(_cover(3, 3, ESC), np.zeros((3, 3, 3), dtype=np.float64), 1, aa.PLAIN, 0.1)
    with pytest.raises(ValueError):
        aa.refine_mask(_cover(3, 3, ESC), np.zeros((3, 4, 3), dtype=np.float32), 1, aa.PLAIN, 0.1)


def test_compose():
    mask = np.array([[True, False, False], [False, False, True]])
    lo = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    hi = -lo - 1
    out = aa.compose(mask, lo, hi)
    assert out.dtype == np.float32 and out.shape == lo.shape
    for y in range(2):
        for x in range(3):
            assert out[y, x].tolist() == (hi if mask[y, x] else lo)[y, x].tolist()
    lo2, hi2 = np.zeros((2, 3), dtype=np.uint8), np.full((2, 3), 7, dtype=np.uint8)
    assert aa.compose(mask, lo2, hi2).tolist() == [[7, 0, 0], [0, 0, 7]]
    lo4 = np.zeros((2, 3, 4), dtype=np.uint8)
    assert aa.compose(mask, lo4, lo4 + 9)[..., 3].tolist() == [[9, 0, 0], [0, 0, 9]]
    assert aa.compose(np.zeros((2, 3), dtype=bool), lo, hi).tobytes() == lo.tobytes()
    assert aa.compose(np.ones((2, 3), dtype=bool), lo, hi).tobytes() == hi.tobytes()
    with pytest.raises(ValueError):
        aa.compose(mask, lo, hi[:1])
    with pytest.raises(ValueError):
        aa.compose(mask, lo, hi.astype(np.float64))


def test_struct_and_defaults():
    assert ctypes.sizeof(ltrace.AAAdaptive) == 32
    assert ltrace.STAT_AA_REFINED == 14 < ltrace.STAT_WORDS
    a = ltrace.default_aa_adaptive()
    assert (a.samples_lo, a.samples_hi, a.mode, a.max_images, a.band_rows, a.chunk_pixels, a.reserved) == (1, 4, ltrace.AA_PLAIN, 3, 0, 0, 0)
    assert a.contrast == np.float32(0.0625)
    a = ltrace.default_aa_adaptive(samples_lo=2, samples_hi=8, mode="disk_images", max_images=5, band_rows=32, chunk_pixels=100, contrast=-1.0)
    assert (a.samples_lo, a.samples_hi, a.mode, a.max_images, a.band_rows, a.chunk_pixels, a.contrast) == (2, 8, ltrace.AA_DISK_IMAGES, 5, 32, 100, -1.0)
    lib = ltrace.load()
    for name in ("lt_default_aa_adaptive", "lt_render_aa_adaptive", "lt_render_aa_adaptive_dev", "lt_aa_adaptive_plan"):
        assert hasattr(lib, name) and name in ltrace.SIGNATURES, name
    for fn in (ltrace.default_aa_adaptive, ltrace.render_aa_adaptive, ltrace.render_aa_adaptive_dev, ltrace.aa_adaptive_plan):
        assert callable(fn)


def test_header_prototypes_match_the_bindings():
    """Every parameter of the header's four prototypes against the argtypes of ltrace.SIGNATURES, and the struct's
    members against ltrace.AAAdaptive."""
    hdr = open(os.path.join(ROOT, "include", "ltrace.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    P = ctypes.POINTER
    ctype = {"const lt_camera *": P(ltrace.Camera), "const lt_metric *": P(ltrace.Metric), "const lt_opts *": P(ltrace.Opts),
             "const lt_aa_adaptive *": P(ltrace.AAAdaptive), "lt_aa_adaptive *": P(ltrace.AAAdaptive), "const lt_disk *": P(ltrace.Disk),
             "const float *": ctypes.c_void_p, "float *": ctypes.c_void_p, "uint8_t *": ctypes.c_void_p, "uint64_t *": ctypes.c_void_p,
             "int32_t": ctypes.c_int32, "lt_stats *": P(ltrace.Stats), "int64_t *": P(ctypes.c_int64)}
    for name, res in (("lt_default_aa_adaptive", None), ("lt_render_aa_adaptive_dev", ctypes.c_int), ("lt_render_aa_adaptive", ctypes.c_int),
                      ("lt_aa_adaptive_plan", ctypes.c_int)):
        m = re.search(r"\b(void|int)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        params = [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")]
        types = [re.sub(r"\s*\w+$", "", p) if not p.endswith("*") else p for p in params]      # drop the parameter's name
        got_res, got_args = ltrace.SIGNATURES[name]
        assert got_res == res and (m.group(1) == "void") == (res is None), name
        assert [ctype[t] for t in types] == got_args, (name, types)
    m = re.search(r"typedef struct lt_aa_adaptive \{(.*?)\} lt_aa_adaptive;", hdr, flags=re.S)
    members = [tuple(ln.split()) for ln in m.group(1).replace(";", "").strip().splitlines()]
    ct = {"int32_t": ctypes.c_int32, "float": ctypes.c_float}
    assert [(n, ct[t]) for t, n in members] == list(ltrace.AAAdaptive._fields_)
    assert re.search(r"#define LT_STAT_AA_REFINED 14\b", hdr)


def _cam(W=1024, H=1024):
    fov = np.radians(40.0)
    return ltrace.Camera(W, H, fov, fov, 0.0, 0.0, 50.0, np.radians(80.0)), ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)


def test_plan_is_host_arithmetic():
    cam, met = _cam()
    # the base pass is lt_render_aa's at samples_lo; a float32 ray's records are 48 bytes, 4^2 rays per refined pixel
    nbytes, chunk = ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive())
    assert nbytes == ltrace.aa_band_bytes(cam, met, ltrace.default_opts(), ltrace.default_aa(samples=1))[0]
    assert chunk == 1024 * 1024                                    # the whole frame's refined rays would fit: 0.75 GiB
    nbytes, chunk = ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive(samples_lo=2, samples_hi=8))
    assert nbytes == ltrace.aa_band_bytes(cam, met, ltrace.default_opts(), ltrace.default_aa(samples=2))[0]
    assert chunk * 64 * 48 <= ltrace.AA_BAND_BYTES < (chunk + 1) * 64 * 48
    # float64 and the thin disk's slots make a ray's records larger: 96 + 3 * 16 + 4 bytes
    o64 = ltrace.default_opts(precision=64, integrator="dp45_exact")
    _, chunk64 = ltrace.aa_adaptive_plan(cam, met, o64, ltrace.default_aa_adaptive(samples_hi=8, mode="disk_images"), disk=ltrace.default_disk())
    assert chunk64 < chunk and chunk64 * 64 * 148 <= ltrace.AA_BAND_BYTES < (chunk64 + 1) * 64 * 148
    # an explicit chunk is taken as it is, up to the frame
    assert ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive(chunk_pixels=7))[1] == 7
    assert ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive(chunk_pixels=2 ** 30))[1] == 1024 * 1024


def test_every_refusal_through_the_plan():
    cam, met = _cam()
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)

    def code(opts, a, disk=None, metric=met, camera=cam):
        with pytest.raises(ltrace.LtraceError) as ei:
            ltrace.aa_adaptive_plan(camera, metric, opts, a, disk=disk)
        return ei.value.code

    ad = ltrace.default_aa_adaptive
    for lo in (0, 5, -1):
        assert code(ltrace.default_opts(), ad(samples_lo=lo, samples_hi=8)) == ltrace.ERR_INVALID_ARG
    for lo, hi in ((1, 1), (2, 2), (3, 2), (1, 9), (4, 4), (1, 0)):
        assert code(ltrace.default_opts(), ad(samples_lo=lo, samples_hi=hi)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(contrast=float("nan"))) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(chunk_pixels=-1)) == ltrace.ERR_INVALID_ARG
    # partitions: the 3 x 3 test reads rows a partition does not own
    assert code(ltrace.default_opts(n_parts=2), ad()) == ltrace.ERR_UNSUPPORTED
    assert code(ltrace.default_opts(n_parts=2, part=1), ad()) == ltrace.ERR_UNSUPPORTED
    assert code(ltrace.default_opts(block_owner=np.zeros(64, dtype=np.uint16)), ad()) == ltrace.ERR_UNSUPPORTED
    # as lt_render_aa refuses: the mode, a disk mode without a disk, band_rows, the mode's own refusals, the options
    assert code(ltrace.default_opts(), ad(mode=7)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(mode="disk")) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(mode="disk_images")) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(mode="disk_images", max_images=9), ltrace.default_disk()) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(band_rows=24)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(), ad(band_rows=-16)) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(schedule="queue"), ad(mode="disk"), ltrace.default_disk()) == ltrace.ERR_UNSUPPORTED
    assert code(ltrace.default_opts(), ad(mode="disk_images"), ltrace.default_disk(), schw) == ltrace.ERR_UNSUPPORTED
    assert code(ltrace.default_opts(precision=16), ad()) == ltrace.ERR_INVALID_ARG
    assert code(ltrace.default_opts(integrator="dp45", precision=32), ad()) == ltrace.ERR_UNSUPPORTED
    assert code(ltrace.default_opts(), ad(), camera=_cam(0, 16)[0]) == ltrace.ERR_INVALID_ARG
    # what is accepted: the plain mode takes what lt_render_dev takes
    assert ltrace.aa_adaptive_plan(cam, schw, ltrace.default_opts(), ad())[1] > 0
    assert ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(schedule="queue"), ad(samples_lo=4, samples_hi=5, contrast=-1.0))[1] > 0


@pytest.mark.skipif(ltrace.device_count() > 0, reason="GPU present")
def test_no_gpu_means_no_device():
    cam, met = _cam(64, 48)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.render_aa_adaptive(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive())
    assert ei.value.code == ltrace.ERR_NO_DEVICE
    with pytest.raises(ltrace.LtraceError) as ei:      # no device comes first, as for every compute entry point
        ltrace.render_aa_adaptive_dev(cam, met, ltrace.default_opts(), ltrace.default_aa_adaptive(samples_lo=0))
    assert ei.value.code == ltrace.ERR_NO_DEVICE


def test_image_lens_accepts_adaptive():
    import image_lens
    import metrics
    ap = image_lens.build_parser()
    args = ap.parse_args([])
    assert args.adaptive is None and args.contrast is None
    args = ap.parse_args(["--a", "0.9", "--synthetic", "256", "192", "--samples", "4", "--adaptive", "1", "--contrast", "0.1"])
    assert (args.samples, args.adaptive, args.contrast) == (4, 1, 0.1)
    kerr = metrics.Kerr(1.0, 0.9)
    lo, hi = np.zeros((8, 8, 3), dtype=np.float32), np.zeros((32, 32, 3), dtype=np.float32)
    with pytest.raises(ValueError):         # adaptive needs the pair of backgrounds
        image_lens.render_frame(hi, kerr, 50.0, (0.7, 0.7), samples=4, adaptive=1)
    with pytest.raises(ValueError):         # ... of the two fine sizes
        image_lens.render_frame((lo, hi[:30]), kerr, 50.0, (0.7, 0.7), samples=4, adaptive=1)
    with pytest.raises(ValueError):         # ... and samples
        image_lens.render_frame((lo, hi), kerr, 50.0, (0.7, 0.7), adaptive=1)
