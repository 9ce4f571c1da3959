"""GPU tests of adaptive supersampling (lt_render_aa_adaptive, lt_render_aa_adaptive_dev; include/ltrace.h, "adaptive
supersampling").

The feature traces no new ray: every pixel of its result is, by definition, a pixel of one of two lt_render_aa frames --
LO (samples_lo) where the pixel is not refined, HI (samples_hi) where it is -- and which pixels are refined follows from
LO alone.  So it is checked by identity: render LO and HI with ltrace.render_aa, compute the mask with aa.refine_mask
(numpy, written from the definition), compose with aa.compose and require rgb, rgba, cover, level and the counters of the
new call to be identical to that, byte for byte.  Every case also asserts that its frame can tell a wrong answer from a
right one: some but not most pixels are refined, LO and HI differ on both sides of the mask, and the mask holds pixels
that only the 3 x 3 neighbourhood finds.

The reference frames are rendered once per (integrator, precision, mode, samples, size, background) and shared."""
import functools

import numpy as np
import pytest

import aa as aamod
import ltrace
from test_gpu_aa import _bg, _scene

pytestmark = pytest.mark.gpu

MODES = ("plain", "disk", "disk_images")
MAX_IMAGES = 3
COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "disk", "disk_hits", "refined")   # words 0-5, 12, 13, 14
KERR, SCHW = ltrace.METRIC_KERR, ltrace.METRIC_SCHWARZSCHILD


def _opts(integ, prec, **kw):
    return ltrace.default_opts(integrator=integ, precision=prec, **kw)


def _disk(mode):
    return None if mode == "plain" else ltrace.default_disk()


def _cam(W, H, kind):
    cam, _, met = _scene(W, H, 1, kind=kind, theta_deg=80.0 if kind == KERR else 90.0)
    return cam, met


def _background(bg, W, H, S):
    """bg: None, "noise1" / "noise3" (test_gpu_aa's), "step" (the smooth background of the contrast test)."""
    if bg is None:
        return None
    if bg == "step":
        u = (np.arange(W * S, dtype=np.float64) + 0.5) / (W * S)
        row = (0.4 * u + 0.5 * (u >= 0.5)).astype(np.float32)       # a horizontal ramp with one vertical step of height 0.5
        img = np.empty((H * S, W * S, 3), dtype=np.float32)
        img[...] = row[None, :, None]
        return img
    return _bg(W, H, S, channels=int(bg[-1]))


def _frozen(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def _aa_frame(integ, prec, mode, S, W, H, bg, kind=KERR):
    """LO or HI: lt_render_aa with samples = S and the background at (H S, W S)."""
    cam, met = _cam(W, H, kind)
    out = ltrace.render_aa(cam, met, _opts(integ, prec), ltrace.default_aa(samples=S, mode=mode, max_images=MAX_IMAGES), disk=_disk(mode),
                           background=_background(bg, W, H, S))
    return _frozen({k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in out.items()})


@functools.lru_cache(maxsize=None)
def _fine_frame(integ, prec, mode, S, W, H, kind=KERR):
    """steps (and n_hits in thin-disk mode) of the S fine frame through the mode's EXISTING entry point."""
    _, fine, met = _scene(W, H, S, kind=kind, theta_deg=80.0 if kind == KERR else 90.0)
    if mode == "plain":
        out = ltrace.render(fine, met, _opts(integ, prec), background=None, want=("steps",))
    elif mode == "disk":
        out = ltrace.render_disk(fine, met, _opts(integ, prec), ltrace.default_disk(), background=None, want=("steps",))
    else:
        out = ltrace.render_disk_images(fine, met, _opts(integ, prec), ltrace.default_disk(), max_images=MAX_IMAGES, background=None,
                                        want=("steps", "n_hits"))
    return _frozen({k: np.array(v) for k, v in out.items() if isinstance(v, np.ndarray)})


def _adaptive(mode, S_lo, S_hi, contrast=-1.0, **kw):
    return ltrace.default_aa_adaptive(samples_lo=S_lo, samples_hi=S_hi, mode=mode, max_images=MAX_IMAGES, contrast=contrast, **kw)


def _expected(integ, prec, mode, S_lo, S_hi, W, H, bg, contrast, kind=KERR):
    """The numpy composition and the exact counters, from LO, HI and the S_hi fine frame."""
    lo, hi = _aa_frame(integ, prec, mode, S_lo, W, H, bg, kind), _aa_frame(integ, prec, mode, S_hi, W, H, bg, kind)
    mask = aamod.refine_mask(lo["cover"], lo["rgb"], S_lo, ltrace.AA_MODES[mode], contrast)
    exp = {k: aamod.compose(mask, lo[k], hi[k]) for k in ("rgb", "rgba", "cover")}
    exp["level"] = np.where(mask, S_hi, S_lo).astype(np.uint8)
    N = int(mask.sum())
    hc = hi["cover"][mask].astype(np.int64).sum(axis=0)        # the refined pixels' S_hi^2 rays by class
    fine = _fine_frame(integ, prec, mode, S_hi, W, H, kind)
    mask_fine = np.repeat(np.repeat(mask, S_hi, axis=0), S_hi, axis=1)
    ls = lo["stats"]
    c = dict(refined=N, rays=S_lo * S_lo * W * H + S_hi * S_hi * N, escaped=ls["escaped"] + int(hc[0]), captured=ls["captured"] + int(hc[1]),
             invalid=ls["invalid"] + int(hc[2]), disk=ls["disk"] + int(hc[3]),
             steps=ls["steps"] + int(fine["steps"][mask_fine].astype(np.int64).sum()),
             disk_hits=ls["disk_hits"] + (int(fine["n_hits"][mask_fine].astype(np.int64).sum()) if mode == "disk_images" else 0))
    # the header's rule: RK4 4 evaluations per step, DP45 1 per ray + 6 per attempt (Schwarzschild is RK4)
    c["rhs_evals"] = 4 * c["steps"] if integ == "rk4" or kind == SCHW else c["rays"] + 6 * c["steps"]
    exp["counters"] = c
    return exp, mask, lo, hi


def _same(got, exp, what=""):
    for k in ("rgb", "rgba", "cover", "level"):
        if k not in got:
            continue
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert np.asarray(got[k]).tobytes() == exp[k].tobytes(), (what, k, int(np.sum(np.asarray(got[k]) != exp[k])))
    assert {k: got["stats"][k] for k in COUNTERS} == exp["counters"], (what, {k: got["stats"][k] for k in COUNTERS}, exp["counters"])


def _uniform(cover, mode, S):
    """Pixels whose own cover is not mixed (one class; thin disk: and all or none of the rays with a hit)."""
    if mode == "disk_images":
        return ((cover[..., :3] != 0).sum(axis=2) == 1) & ((cover[..., 3] == 0) | (cover[..., 3] == S * S))
    return (cover != 0).sum(axis=2) == 1


def _can_fail(mode, S_lo, S_hi, mask, lo, hi, what=""):
    """Conditions, not measurements: without them an implementation that refines nothing, everything or only the mixed
    pixels could pass the identity."""
    H, W = mask.shape
    N = int(mask.sum())
    print(f"{what}: N = {N} of {W * H} ({N / (W * H):.3f})")
    assert 0 < N < W * H / 2, (what, N)
    differ = np.any((lo["rgb"] != hi["rgb"]).reshape(H, W, -1), axis=2)
    assert np.any(differ & ~mask), (what, "LO == HI on every unrefined pixel")
    assert np.any(differ & mask), (what, "LO == HI on every refined pixel")
    assert np.any(mask & _uniform(lo["cover"], mode, S_lo)), (what, "no pixel flagged by its neighbourhood alone")
    if mode != "plain":
        on = hi["cover"][..., 3].astype(int)
        assert np.any(mask & (on > 0) & (on < S_hi * S_hi)), (what, "no refined pixel partly on the disk")
    if mode == "disk_images" and S_lo > 1:
        # the thin disk's slot-3 rule on the base pass itself: one class among slots 0-2, some but not all rays with a hit
        lc = lo["cover"].astype(int)
        by_slot3 = ((lc[..., :3] != 0).sum(axis=2) == 1) & (lc[..., 3] > 0) & (lc[..., 3] < S_lo * S_lo)
        assert np.any(by_slot3) and np.all(mask[by_slot3]), (what, "no pixel that 0 < cover[3] < S_lo^2 alone calls mixed")
    tot = hi["cover"][..., :3 if mode == "disk_images" else 4].astype(int).sum(axis=2)
    assert np.all(tot == S_hi * S_hi)


def _run(integ, prec, mode, S_lo, S_hi, W, H, bg="noise3", contrast=-1.0, kind=KERR, **ad_kw):
    cam, met = _cam(W, H, kind)
    return ltrace.render_aa_adaptive(cam, met, _opts(integ, prec), _adaptive(mode, S_lo, S_hi, contrast, **ad_kw), disk=_disk(mode),
                                     background_lo=_background(bg, W, H, S_lo), background_hi=_background(bg, W, H, S_hi))


# ---- 1, 2: identity, and that it can fail ----------------------------------------------------------------------------
def _size(S_hi):
    return (48, 40) if S_hi == 8 else (96, 80)


IDENTITY = ([("rk4", 32, m, lo, hi) for m in MODES for lo, hi in ((1, 4), (2, 4), (1, 3), (2, 3), (1, 8))] +
            [("dp45_exact", 64, m, lo, hi) for m in MODES for lo, hi in ((1, 4), (2, 3))] + [("rk4", 64, "disk_images", 2, 4)])


@pytest.mark.parametrize("integ,prec,mode,S_lo,S_hi", IDENTITY)
def test_identity_with_the_two_supersampled_frames(integ, prec, mode, S_lo, S_hi):
    W, H = _size(S_hi)
    exp, mask, lo, hi = _expected(integ, prec, mode, S_lo, S_hi, W, H, "noise3", -1.0)
    got = _run(integ, prec, mode, S_lo, S_hi, W, H)
    _same(got, exp, (integ, prec, mode, S_lo, S_hi))
    assert got["stats"]["rays"] == S_lo * S_lo * W * H + S_hi * S_hi * int(mask.sum())
    lv = got["level"].astype(int)
    assert np.all(got["cover"][..., :3 if mode == "disk_images" else 4].astype(int).sum(axis=2) == lv * lv)
    _can_fail(mode, S_lo, S_hi, mask, lo, hi, (integ, prec, mode, S_lo, S_hi))


@pytest.mark.parametrize("mode", MODES)
def test_one_base_sample_leaves_the_modes_own_pixel(mode):
    """S_lo = 1: an unrefined pixel is exactly the pixel the mode's existing entry point renders."""
    W, H = 96, 80
    cam, met = _cam(W, H, KERR)
    bg = _background("noise3", W, H, 1)
    if mode == "plain":
        own = ltrace.render(cam, met, ltrace.default_opts(), background=bg, want=("rgb", "rgba"))
    elif mode == "disk":
        own = ltrace.render_disk(cam, met, ltrace.default_opts(), ltrace.default_disk(), background=bg, want=("rgb", "rgba"))
    else:
        own = ltrace.render_disk_images(cam, met, ltrace.default_opts(), ltrace.default_disk(), max_images=MAX_IMAGES, background=bg,
                                        want=("rgb", "rgba"))
    got = _run("rk4", 32, mode, 1, 4, W, H)
    keep = got["level"] == 1
    assert keep.any() and not keep.all()
    for k in ("rgb", "rgba"):
        assert np.asarray(got[k])[keep].tobytes() == np.asarray(own[k])[keep].tobytes(), k


# ---- 3: the colour test ----------------------------------------------------------------------------------------------
def test_contrast_finds_what_cover_cannot_see():
    W, H, S_lo, S_hi = 96, 80, 1, 4
    exp, mask, lo, hi = _expected("rk4", 32, "plain", S_lo, S_hi, W, H, "step", 0.25)
    got = _run("rk4", 32, "plain", S_lo, S_hi, W, H, bg="step", contrast=0.25)
    _same(got, exp, "contrast 0.25")
    off = aamod.refine_mask(lo["cover"], None, S_lo, ltrace.AA_PLAIN, -1.0)
    print(f"contrast: N = {int(mask.sum())}, without the colour test {int(off.sum())}")
    assert np.all(mask[off]) and mask.sum() > off.sum(), "the mask is not a strict superset of the cover tests' mask"
    assert mask.sum() < W * H / 2
    _same(_run("rk4", 32, "plain", S_lo, S_hi, W, H, bg="step", contrast=-1.0), _expected("rk4", 32, "plain", S_lo, S_hi, W, H, "step", -1.0)[0],
          "contrast off")


# ---- 4: the photon ring is found by colour ---------------------------------------------------------------------------
def test_thin_disk_without_background_finds_the_photon_ring_by_colour():
    W, H, S_lo, S_hi = 96, 80, 1, 4
    exp, mask, lo, hi = _expected("rk4", 32, "disk_images", S_lo, S_hi, W, H, None, 0.0625)
    got = _run("rk4", 32, "disk_images", S_lo, S_hi, W, H, bg=None, contrast=0.0625)
    _same(got, exp, "thin disk, no background")
    by_cover = aamod.refine_mask(lo["cover"], None, S_lo, ltrace.AA_DISK_IMAGES, -1.0)
    nh = _fine_frame("rk4", 32, "disk_images", S_lo, W, H)["n_hits"].astype(int)
    most = np.zeros((H, W), dtype=int)                    # the most hits among a pixel's S_lo^2 rays
    for j in range(S_lo):
        for i in range(S_lo):
            most = np.maximum(most, nh[j::S_lo, i::S_lo])
    ring = mask & ~by_cover & (most >= 2)                 # cover equals all the neighbours', and is not mixed
    print(f"photon ring: N = {int(mask.sum())}, by cover {int(by_cover.sum())}, 2-hit pixels found by colour alone {int(ring.sum())}")
    assert ring.any(), "no pixel with a second image of the disk that only the colour test finds"
    assert mask.sum() < W * H / 2


# ---- 5, 6: nothing and everything --------------------------------------------------------------------------------------
def _yawed(W, H):
    """The demo camera turned away so that the hole is outside the frame."""
    cam, met = _cam(W, H, KERR)
    cam.psi_x = 1.0
    return cam, met


def test_nothing_flagged_launches_nothing_further():
    W, H = 96, 80
    cam, met = _yawed(W, H)
    lo = ltrace.render_aa(cam, met, ltrace.default_opts(), ltrace.default_aa(samples=1))
    got = ltrace.render_aa_adaptive(cam, met, ltrace.default_opts(), _adaptive("plain", 1, 4))      # returns OK: no zero-sized launch
    assert not aamod.refine_mask(np.asarray(lo["cover"]), None, 1, ltrace.AA_PLAIN, -1.0).any()
    assert got["stats"]["refined"] == 0 and got["stats"]["rays"] == W * H
    for k in ("rgb", "rgba", "cover"):
        assert got[k].tobytes() == lo[k].tobytes(), k
    assert np.all(got["level"] == 1)
    for k in COUNTERS[:-1]:
        assert got["stats"][k] == lo["stats"][k], k


def test_everything_flagged_is_the_fine_pass():
    W, H, S_lo, S_hi = 96, 80, 1, 3
    cam, met = _yawed(W, H)
    opts = ltrace.default_opts(loop_around=1)             # every pixel shows a texel of the noise
    bg_lo, bg_hi = _bg(W, H, S_lo), _bg(W, H, S_hi)
    lo = ltrace.render_aa(cam, met, opts, ltrace.default_aa(samples=S_lo), background=bg_lo)
    hi = ltrace.render_aa(cam, met, opts, ltrace.default_aa(samples=S_hi), background=bg_hi)
    assert aamod.refine_mask(np.asarray(lo["cover"]), np.asarray(lo["rgb"]), S_lo, ltrace.AA_PLAIN, 0.0).all()
    got = ltrace.render_aa_adaptive(cam, met, opts, _adaptive("plain", S_lo, S_hi, contrast=0.0), background_lo=bg_lo, background_hi=bg_hi)
    assert got["stats"]["refined"] == W * H and got["stats"]["rays"] == (S_lo * S_lo + S_hi * S_hi) * W * H
    for k in ("rgb", "rgba", "cover"):
        assert got[k].tobytes() == hi[k].tobytes(), k
    assert np.all(got["level"] == S_hi)
    for k in COUNTERS[:-1]:
        assert got["stats"][k] == lo["stats"][k] + hi["stats"][k], k


# ---- 7: chunks and bands -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, -1])
def test_results_do_not_depend_on_chunks_and_bands(chunk):
    W, H, S_lo, S_hi = 96, 80, 1, 3
    exp, mask, lo, hi = _expected("rk4", 32, "disk_images", S_lo, S_hi, W, H, "noise3", -1.0)
    N = int(mask.sum())
    assert N > 8
    cam, met = _cam(W, H, KERR)
    kw = dict(chunk_pixels=chunk if chunk > 0 else N - 1, band_rows=16)
    assert ltrace.aa_adaptive_plan(cam, met, ltrace.default_opts(), _adaptive("disk_images", S_lo, S_hi, **kw), disk=ltrace.default_disk())[1] == kw["chunk_pixels"]
    _same(_run("rk4", 32, "disk_images", S_lo, S_hi, W, H, **kw), exp, kw)
    _same(_run("rk4", 32, "disk_images", S_lo, S_hi, W, H), exp, "automatic")


# ---- 8, 9: device pointers, the stream's workspace ---------------------------------------------------------------------
def _upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return d


def _launch_dev(stream_ptr, cam, met, mode, S_lo, S_hi, W, H, outputs, contrast=-1.0):
    import hipmini
    o = ltrace.default_opts()
    o.stream = stream_ptr
    shapes = dict(rgb=((H, W, 3), np.float32), rgba=((H, W, 4), np.uint8), cover=((H, W, 4), np.uint8), level=((H, W), np.uint8))
    bufs = {k: hipmini.DeviceArray(*shapes[k]) for k in outputs}
    bufs["stats"] = _upload(np.zeros(ltrace.STAT_WORDS, dtype=np.uint64))
    bufs["bg_lo"], bufs["bg_hi"] = _upload(_bg(W, H, S_lo)), _upload(_bg(W, H, S_hi))
    ptr = lambda k: bufs[k].ptr if k in bufs else 0
    ltrace.render_aa_adaptive_dev(cam, met, o, _adaptive(mode, S_lo, S_hi, contrast), disk=_disk(mode), d_bg_lo=bufs["bg_lo"].ptr,
                                  d_bg_hi=bufs["bg_hi"].ptr, bg_channels=3, d_rgb=ptr("rgb"), d_rgba=ptr("rgba"), d_cover=ptr("cover"),
                                  d_level=ptr("level"), d_stats=bufs["stats"].ptr)
    return bufs


def _read_dev(bufs, outputs):
    out = {k: bufs[k].get() for k in outputs}
    c = bufs["stats"].get()
    words = (0, 1, 2, 3, 4, 5, ltrace.STAT_DISK, ltrace.STAT_DISK_HITS, ltrace.STAT_AA_REFINED)
    out["stats"] = dict(zip(COUNTERS, [int(c[i]) for i in words]))
    return out


@pytest.mark.parametrize("mode,outputs,contrast", [("disk_images", ("rgb", "rgba", "cover", "level"), -1.0), ("disk", ("rgba",), 0.5),
                                                   ("plain", ("cover", "level"), 0.5), ("disk_images", ("rgba",), -1.0)])
def test_host_and_device_pointer_variants_agree(mode, outputs, contrast):
    import hipmini
    W, H, S_lo, S_hi = 96, 80, 2, 4
    cam, met = _cam(W, H, KERR)
    host = _run("rk4", 32, mode, S_lo, S_hi, W, H, contrast=contrast)
    exp = dict(host, counters={k: host["stats"][k] for k in COUNTERS})
    assert 0 < host["stats"]["refined"] < W * H          # (with the colour test on, the noise background flags many pixels)
    st = hipmini.Stream()
    for rep in range(2):                                   # the repeated call finds list, count and scratch grown
        bufs = _launch_dev(st.ptr, cam, met, mode, S_lo, S_hi, W, H, outputs, contrast)
        st.synchronize()
        _same(_read_dev(bufs, outputs), exp, (mode, outputs, rep))
    ltrace.release_stream(st.ptr)


def test_an_ordinary_frame_after_an_adaptive_one_is_unchanged():
    """lt_render_dev, lt_render_aa_adaptive_dev, the same lt_render_dev on ONE stream: the third frame must not reuse the
    records the refined pass left in the stream's workspace, and gives the bytes it gives on a fresh stream."""
    import hipmini
    from test_gpu_aa import _launch_plain
    W, H = 96, 80
    cam, met = _cam(W, H, KERR)
    bg = _bg(W, H, 1)
    frames = []
    fresh = hipmini.Stream()
    b = _launch_plain(fresh.ptr, cam, met, bg)
    fresh.synchronize()
    frames.append({k: v.get().tobytes() for k, v in b.items() if k != "bg"})
    ltrace.release_stream(fresh.ptr)
    st = hipmini.Stream()
    adaptive = []
    for what in ("plain", "adaptive", "plain", "adaptive-1", "plain"):
        if what == "plain":
            b = _launch_plain(st.ptr, cam, met, bg)
            st.synchronize()
            frames.append({k: v.get().tobytes() for k, v in b.items() if k != "bg"})
        else:                                              # S_lo = 1: the base pass renders the very camera of the plain frame
            S_lo = 1 if what == "adaptive-1" else 2
            b = _launch_dev(st.ptr, cam, met, "plain", S_lo, 4, W, H, ("rgba", "level"))
            st.synchronize()
            adaptive.append(_read_dev(b, ("rgba", "level")))
    ltrace.release_stream(st.ptr)
    assert all(f == frames[0] for f in frames[1:])
    assert all(0 < a["stats"]["refined"] < W * H / 2 for a in adaptive)


# ---- 10: Schwarzschild, one channel ----------------------------------------------------------------------------------
def test_identity_schwarzschild_plain():
    W, H, S_lo, S_hi = 96, 80, 1, 2
    exp, mask, lo, hi = _expected("rk4", 32, "plain", S_lo, S_hi, W, H, "noise3", -1.0, kind=SCHW)
    got = _run("rk4", 32, "plain", S_lo, S_hi, W, H, kind=SCHW)
    _same(got, exp, "schwarzschild")
    _can_fail("plain", S_lo, S_hi, mask, lo, hi, "schwarzschild")


def test_identity_one_channel_background():
    W, H, S_lo, S_hi = 96, 80, 1, 4
    exp, mask, lo, hi = _expected("rk4", 32, "disk", S_lo, S_hi, W, H, "noise1", -1.0)
    got = _run("rk4", 32, "disk", S_lo, S_hi, W, H, bg="noise1")
    assert got["rgb"].shape == (H, W)
    _same(got, exp, "one channel")
    _can_fail("disk", S_lo, S_hi, mask, lo, hi, "one channel")
    # ... and the colour test on one channel
    exp, mask_c, _, _ = _expected("rk4", 32, "disk", S_lo, S_hi, W, H, "noise1", 0.9)
    _same(_run("rk4", 32, "disk", S_lo, S_hi, W, H, bg="noise1", contrast=0.9), exp, "one channel, contrast")
    assert mask_c.sum() > mask.sum()


# ---- 11: image_lens --------------------------------------------------------------------------------------------------
def test_render_frame_with_adaptive_is_the_library_call():
    import image_lens
    import metrics
    from disk import TransparentDisk
    W, H, S_lo, S_hi = 96, 80, 1, 4
    cam, met = _cam(W, H, KERR)
    bg_lo, bg_hi = _bg(W, H, S_lo), _bg(W, H, S_hi)
    kerr = metrics.Kerr(M=1.0, a=0.9, integrator="rk4", precision=32, schedule="direct")
    out = image_lens.render_frame((bg_lo, bg_hi), kerr, 50.0, (cam.hfov, cam.vfov), theta_obs=np.radians(80.0), want=("rgb", "rgba"), samples=S_hi,
                                  adaptive=S_lo, disk=TransparentDisk(max_images=3))
    lib = ltrace.render_aa_adaptive(cam, met, ltrace.default_opts(axis_refine_frac=image_lens.Y_AXIS_REFINE_FRAC),
                                    ltrace.default_aa_adaptive(samples_lo=S_lo, samples_hi=S_hi, mode="disk_images", max_images=3),
                                    disk=ltrace.default_disk(), background_lo=bg_lo, background_hi=bg_hi)
    for k in ("rgb", "rgba", "cover", "level"):
        assert out[k].shape == lib[k].shape and out[k].tobytes() == lib[k].tobytes(), k
    assert out["stats"]["refined"] == lib["stats"]["refined"] > 0
    assert out["rgb"].shape == (H, W, 3)
    off = image_lens.render_frame((bg_lo, bg_hi), kerr, 50.0, (cam.hfov, cam.vfov), theta_obs=np.radians(80.0), want=("rgba",), samples=S_hi,
                                  adaptive=S_lo, contrast=-1.0, disk=TransparentDisk(max_images=3))
    assert 0 < off["stats"]["refined"] < out["stats"]["refined"]
