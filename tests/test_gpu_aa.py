"""GPU tests of the supersampled frame (lt_render_aa, lt_render_aa_dev; include/ltrace.h, "supersampled frames").

The feature changes no ray: a supersampled frame is by definition the box filter of the FINE frame (the same camera
with W S x H S pixels) that the mode's existing entry point renders.  So it is checked by identity: render the fine
frame with lt_render / lt_render_disk / lt_render_disk_images, resolve it in numpy (aa.resolve, aa.to_rgba8, aa.cover)
and require rgb, rgba, cover and the counters of the new call to be byte-identical to that.  Every test also asserts
that its frame exercises the feature (pixels of mixed classes, pixels partly on the disk, rays with two hits)."""
import numpy as np
import pytest

import aa as aamod
import ltrace

pytestmark = pytest.mark.gpu

MODES = ("plain", "disk", "disk_images")
MAX_IMAGES = 3
COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "disk", "disk_hits")   # words 0-5, 12, 13


def _scene(W, H, S, kind=ltrace.METRIC_KERR, theta_deg=80.0):
    """The README's demo view (a = 0.9, r_obs = 50, theta_obs = 80 deg, vertical fov 40 deg, r_out = 20) at W x H."""
    vfov = np.radians(40.0)
    hfov = 2 * np.arctan(np.tan(vfov / 2) * W / H)
    cam = ltrace.Camera(W, H, hfov, vfov, 0.0, 0.0, 50.0, np.radians(theta_deg))
    fine = ltrace.Camera(W * S, H * S, hfov, vfov, 0.0, 0.0, 50.0, np.radians(theta_deg))
    met = ltrace.Metric(kind, 0, 1.0, 0.9 if kind == ltrace.METRIC_KERR else 0.0)
    return cam, fine, met


def _bg(W, H, S, channels=3, seed=5):
    shape = (H * S, W * S) if channels == 1 else (H * S, W * S, 3)
    return np.random.default_rng(seed + 1000 * S + W).random(shape, dtype=np.float32)


def _fine_frame(mode, fine, met, opts, bg):
    """The fine frame through the mode's EXISTING entry point: rgb, rgba, status, n_hits (thin mode), counters."""
    want = ("status", "rgb", "rgba")
    if mode == "plain":
        out = ltrace.render(fine, met, opts, background=bg, want=want)
        out["stats"]["disk"] = out["stats"]["disk_hits"] = 0
    elif mode == "disk":
        out = ltrace.render_disk(fine, met, opts, ltrace.default_disk(), background=bg, want=want)
        out["stats"]["disk_hits"] = 0
    else:
        out = ltrace.render_disk_images(fine, met, opts, ltrace.default_disk(), max_images=MAX_IMAGES, background=bg,
                                        want=want + ("n_hits",))
    return out


def _expected(mode, fine_out, S):
    mode_id = ltrace.AA_MODES[mode]
    rgb = aamod.resolve(np.asarray(fine_out["rgb"]), S)
    return dict(rgb=rgb, rgba=aamod.to_rgba8(rgb), cover=aamod.cover(fine_out["status"], fine_out.get("n_hits"), S, mode_id),
                counters={k: fine_out["stats"][k] for k in COUNTERS})


def _aa(mode, S, band_rows=0):
    return ltrace.default_aa(samples=S, mode=mode, max_images=MAX_IMAGES, band_rows=band_rows)


def _disk(mode):
    return None if mode == "plain" else ltrace.default_disk()


def _same(got, exp, what=""):
    for k in ("rgb", "rgba", "cover"):
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k, int(np.sum(got[k] != exp[k])))
    assert {k: got["stats"][k] for k in COUNTERS} == exp["counters"], what


def _exercised(mode, S, cover, fine_out):
    """The frame shows what the feature is for: a resolve of equal sub-samples would pass any identity."""
    esc = cover[..., 0].astype(int)
    assert np.any((esc > 0) & (esc < S * S)), "no pixel with both escaped and other sub-rays"
    total = cover[..., :4].astype(int).sum(axis=2) if mode != "disk_images" else cover[..., :3].astype(int).sum(axis=2)
    assert np.all(total == S * S)
    if mode == "plain":
        assert not cover[..., 3].any()
    else:
        on = cover[..., 3].astype(int)
        assert np.any((on > 0) & (on < S * S)), "no pixel partly on the disk"
    if mode == "disk_images":
        assert np.any(np.asarray(fine_out["n_hits"]) >= 2), "no ray with two hits: the photon ring is not in the frame"


IDENTITY = ([("rk4", 32, m, S, 96, 80) for m in MODES for S in (2, 3, 4)] + [("rk4", 32, m, 8, 48, 40) for m in MODES] +
            [("dp45_exact", 64, m, S, 96, 80) for m in MODES for S in (2, 3)] + [("rk4", 64, "disk_images", 2, 96, 80),
                                                                                   ("rk4", 64, "plain", 3, 96, 80)])


@pytest.mark.parametrize("integ,prec,mode,S,W,H", IDENTITY)
def test_identity_with_the_fine_frame(integ, prec, mode, S, W, H):
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    exp_fine = _fine_frame(mode, fine, met, ltrace.default_opts(integrator=integ, precision=prec), bg)
    exp = _expected(mode, exp_fine, S)
    got = ltrace.render_aa(cam, met, ltrace.default_opts(integrator=integ, precision=prec), _aa(mode, S), disk=_disk(mode),
                           background=bg)
    _same(got, exp, (integ, prec, mode, S))
    assert got["stats"]["rays"] == S * S * W * H
    _exercised(mode, S, got["cover"], exp_fine)


def test_identity_schwarzschild_plain():
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S, kind=ltrace.METRIC_SCHWARZSCHILD, theta_deg=90.0)
    bg = _bg(W, H, S)
    exp_fine = _fine_frame("plain", fine, met, ltrace.default_opts(), bg)
    got = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa("plain", S), background=bg)
    _same(got, _expected("plain", exp_fine, S), "schwarzschild")
    _exercised("plain", S, got["cover"], exp_fine)


@pytest.mark.parametrize("mode", MODES)
def test_shadow_render_without_background(mode):
    S, W, H = 3, 96, 80
    cam, fine, met = _scene(W, H, S)
    exp_fine = _fine_frame(mode, fine, met, ltrace.default_opts(), None)
    got = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa(mode, S), disk=_disk(mode), background=None)
    _same(got, _expected(mode, exp_fine, S), mode)
    _exercised(mode, S, got["cover"], exp_fine)
    frac = got["rgb"][..., 0]
    assert np.any((frac > 0) & (frac < 1)), "no anti-aliased edge"


@pytest.mark.parametrize("mode", MODES)
def test_one_channel_background(mode):
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S, channels=1)
    exp_fine = _fine_frame(mode, fine, met, ltrace.default_opts(), bg)
    got = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa(mode, S), disk=_disk(mode), background=bg)
    assert got["rgb"].shape == (H, W)
    _same(got, _expected(mode, exp_fine, S), mode)
    _exercised(mode, S, got["cover"], exp_fine)


@pytest.mark.parametrize("mode", MODES)
def test_one_sample_is_the_family_itself(mode):
    W, H = 96, 80
    cam, fine, met = _scene(W, H, 1)
    bg = _bg(W, H, 1)
    ref = _fine_frame(mode, fine, met, ltrace.default_opts(), bg)
    got = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa(mode, 1), disk=_disk(mode), background=bg)
    assert got["rgb"].tobytes() == np.asarray(ref["rgb"]).tobytes() and got["rgba"].tobytes() == np.asarray(ref["rgba"]).tobytes()


@pytest.mark.parametrize("mode,prec", [("plain", 32), ("disk_images", 32), ("disk", 64)])
def test_results_do_not_depend_on_the_banding(mode, prec):
    S, W, H = 3, 96, 80                        # five row blocks of 16 rows
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    opts = ltrace.default_opts(precision=prec)
    exp_fine = _fine_frame(mode, fine, met, opts, bg)
    exp = _expected(mode, exp_fine, S)
    bands = {}
    for band_rows in (16, 48, 0):
        nbytes, rows, n = ltrace.aa_band_bytes(cam, met, opts, _aa(mode, S, band_rows), disk=_disk(mode))
        bands[band_rows] = (rows, n, nbytes)
        _same(ltrace.render_aa(cam, met, opts, _aa(mode, S, band_rows), disk=_disk(mode), background=bg), exp, (mode, band_rows))
    assert [bands[b][:2] for b in (16, 48, 0)] == [(16, 5), (48, 2), (80, 1)]
    assert bands[16][2] < bands[48][2] < bands[0][2] <= ltrace.AA_BAND_BYTES
    _exercised(mode, S, exp["cover"], exp_fine)


@pytest.mark.parametrize("mode,n_parts,table,band_rows", [("plain", 2, False, 0), ("disk", 3, False, 16), ("disk_images", 2, True, 0),
                                                          ("plain", 3, True, 16), ("disk_images", 3, False, 32)])
def test_partitions_reassemble_to_the_whole_frame(mode, n_parts, table, band_rows):
    S, W, H, rb = 2, 96, 88, 16                # 88 rows: the last row block has 8
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    whole = ltrace.render_aa(cam, met, ltrace.default_opts(row_block=rb), _aa(mode, S), disk=_disk(mode), background=bg)
    _exercised(mode, S, whole["cover"], _fine_frame(mode, fine, met, ltrace.default_opts(), bg))
    owner = np.random.default_rng(7).integers(0, n_parts, size=(H + rb - 1) // rb).astype(np.uint16) if table else None
    if table:
        owner[:n_parts] = np.arange(n_parts)   # every partition owns something
    full = {k: np.zeros_like(whole[k]) for k in ("rgb", "rgba", "cover")}
    seen = np.zeros(H, dtype=int)
    counters = dict.fromkeys(COUNTERS, 0)
    for part in range(n_parts):
        opts = ltrace.default_opts(row_block=rb, n_parts=n_parts, part=part, block_owner=owner)
        rows = ltrace.owned_rows(H, rb, owner, part) if table else ltrace.global_rows(H, rb, n_parts, part)
        got = ltrace.render_aa(cam, met, opts, _aa(mode, S, band_rows), disk=_disk(mode), background=bg)
        assert got["rgb"].shape[0] == len(rows)
        for k in full:
            full[k][rows] = got[k]
        seen[rows] += 1
        for k in COUNTERS:
            counters[k] += got["stats"][k]
    assert np.all(seen == 1)
    for k in full:
        assert full[k].tobytes() == whole[k].tobytes(), k
    assert counters == {k: whole["stats"][k] for k in COUNTERS}


# ---- device pointers, streams -----------------------------------------------------------------------------------------
def _upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return d


def _launch_aa(stream_ptr, cam, met, mode, S, bg, band_rows=0):
    """Enqueues lt_render_aa_dev on the stream; returns its device buffers (read them once the stream has drained)."""
    import hipmini
    o = ltrace.default_opts()
    o.stream = stream_ptr
    bufs = dict(rgb=hipmini.DeviceArray((cam.height, cam.width, 3), np.float32), rgba=hipmini.DeviceArray((cam.height, cam.width, 4), np.uint8),
                cover=hipmini.DeviceArray((cam.height, cam.width, 4), np.uint8), stats=_upload(np.zeros(ltrace.STAT_WORDS, dtype=np.uint64)),
                bg=_upload(bg))
    ltrace.render_aa_dev(cam, met, o, _aa(mode, S, band_rows), disk=_disk(mode), d_bg=bufs["bg"].ptr, bg_channels=3, d_rgb=bufs["rgb"].ptr,
                         d_rgba=bufs["rgba"].ptr, d_cover=bufs["cover"].ptr, d_stats=bufs["stats"].ptr)
    return bufs


def _read(bufs):
    out = {k: bufs[k].get() for k in ("rgb", "rgba", "cover")}
    c = bufs["stats"].get()
    out["stats"] = dict(zip(COUNTERS, [int(c[i]) for i in (0, 1, 2, 3, 4, 5, ltrace.STAT_DISK, ltrace.STAT_DISK_HITS)]))
    return out


def _launch_plain(stream_ptr, cam, met, bg):
    import hipmini
    o = ltrace.default_opts()
    o.stream = stream_ptr
    bufs = dict(fa=hipmini.DeviceArray((cam.height, cam.width), np.float32), status=hipmini.DeviceArray((cam.height, cam.width), np.int8),
                rgba=hipmini.DeviceArray((cam.height, cam.width, 4), np.uint8), bg=_upload(bg))
    ltrace.render_dev(cam, met, o, d_bg=bufs["bg"].ptr, bg_channels=3, d_fa=bufs["fa"].ptr, d_status=bufs["status"].ptr, d_rgba=bufs["rgba"].ptr)
    return bufs


@pytest.mark.parametrize("mode,band_rows", [("plain", 0), ("disk", 16), ("disk_images", 0)])
def test_host_and_device_pointer_variants_agree(mode, band_rows):
    import hipmini
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    host = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa(mode, S, band_rows), disk=_disk(mode), background=bg)
    st = hipmini.Stream()
    bufs = _launch_aa(st.ptr, cam, met, mode, S, bg, band_rows)
    st.synchronize()
    dev = _read(bufs)
    ltrace.release_stream(st.ptr)
    _same(dev, dict(host, counters={k: host["stats"][k] for k in COUNTERS}), mode)


def test_an_ordinary_frame_after_a_supersampled_one_is_unchanged():
    """lt_render_dev, lt_render_aa_dev, the same lt_render_dev on ONE stream: the third frame must not reuse records the
    supersampled call left in the stream's workspace."""
    import hipmini
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    st = hipmini.Stream()
    frames = []
    for what in ("plain", "aa", "plain", "aa-bands", "plain", "fine", "plain"):
        if what == "plain":
            b = _launch_plain(st.ptr, cam, met, _bg(W, H, 1))
        elif what == "fine":    # the fine frame itself through lt_render_dev: the very camera a one-band call renders
            b = _launch_plain(st.ptr, fine, met, _bg(W, H, S))
        else:
            b = _launch_aa(st.ptr, cam, met, "disk_images", S, _bg(W, H, S), band_rows=32 if what == "aa-bands" else 0)
        st.synchronize()
        frames.append({k: v.get().tobytes() for k, v in b.items() if k != "bg"})
    ltrace.release_stream(st.ptr)
    assert frames[0] == frames[2] == frames[4] == frames[6]
    assert {k: frames[1][k] for k in ("rgb", "rgba", "cover")} == {k: frames[3][k] for k in ("rgb", "rgba", "cover")}


def test_two_supersampled_frames_in_flight_on_two_streams():
    import hipmini
    S, W, H = 2, 96, 80
    specs = [("disk_images", _scene(W, H, S, theta_deg=80.0)), ("disk", _scene(W, H, S, theta_deg=70.0))]
    bg = _bg(W, H, S)
    alone = []
    for mode, (cam, fine, met) in specs:
        alone.append(ltrace.render_aa(cam, met, ltrace.default_opts(), _aa(mode, S), disk=_disk(mode), background=bg))
    streams = [hipmini.Stream(), hipmini.Stream()]
    bufs = [[], []]
    for rep in range(3):                        # frames of both streams enqueued before anything is waited for
        for i, (mode, (cam, fine, met)) in enumerate(specs):
            bufs[i].append(_launch_aa(streams[i].ptr, cam, met, mode, S, bg))
    for s in streams:
        s.synchronize()
    for i in range(2):
        for b in bufs[i]:
            _same(_read(b), dict(alone[i], counters={k: alone[i]["stats"][k] for k in COUNTERS}), i)
        ltrace.release_stream(streams[i].ptr)


def test_a_repeated_one_band_call_reuses_its_records():
    import hipmini
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    st = hipmini.Stream()
    outs, deltas = [], []
    for rep in range(3):
        before = ltrace.ic_reuse_counts()
        b = _launch_aa(st.ptr, cam, met, "disk_images", S, bg)
        st.synchronize()
        after = ltrace.ic_reuse_counts()
        deltas.append((after[0] - before[0], after[1] - before[1]))
        outs.append(_read(b))
    before = ltrace.ic_reuse_counts()
    b = _launch_aa(st.ptr, cam, met, "disk_images", S, bg, band_rows=32)      # three bands: three prologues, none reused
    st.synchronize()
    after = ltrace.ic_reuse_counts()
    outs.append(_read(b))
    ltrace.release_stream(st.ptr)
    assert deltas == [(0, 1), (1, 0), (1, 0)], deltas      # (LT_IC_REUSE=0 in the environment switches the reuse off: not here)
    assert (after[0] - before[0], after[1] - before[1]) == (0, 3)
    for o in outs[1:]:
        _same(o, dict(outs[0], counters=outs[0]["stats"]), "repeat")


def test_refusals():
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    bg = _bg(W, H, S)

    def code(met_, opts, aa_, disk):
        with pytest.raises(ltrace.LtraceError) as ei:
            ltrace.render_aa(cam, met_, opts, aa_, disk=disk, background=bg)
        return ei.value.code

    for bad in (0, 9, -1):
        assert code(met, ltrace.default_opts(), ltrace.default_aa(samples=bad), None) == ltrace.ERR_INVALID_ARG
    assert code(met, ltrace.default_opts(), ltrace.default_aa(mode=7), None) == ltrace.ERR_INVALID_ARG
    for mode in ("disk", "disk_images"):
        assert code(schw, ltrace.default_opts(), _aa(mode, S), ltrace.default_disk()) == ltrace.ERR_UNSUPPORTED
        assert code(met, ltrace.default_opts(schedule="queue"), _aa(mode, S), ltrace.default_disk()) == ltrace.ERR_UNSUPPORTED
        assert code(met, ltrace.default_opts(), _aa(mode, S), None) == ltrace.ERR_INVALID_ARG
    assert code(met, ltrace.default_opts(), ltrace.default_aa(mode="disk_images", max_images=9), ltrace.default_disk()) == ltrace.ERR_INVALID_ARG
    assert code(met, ltrace.default_opts(), _aa("plain", S, band_rows=24), None) == ltrace.ERR_INVALID_ARG     # not a multiple of 16
    # the plain mode accepts what lt_render_dev accepts: the queue schedule, Schwarzschild
    q = ltrace.render_aa(cam, met, ltrace.default_opts(schedule="queue"), _aa("plain", S), background=bg)
    d = ltrace.render_aa(cam, met, ltrace.default_opts(), _aa("plain", S), background=bg)
    assert q["rgb"].tobytes() == d["rgb"].tobytes() and q["cover"].tobytes() == d["cover"].tobytes()


def test_render_frame_with_samples_is_the_library_call():
    import image_lens
    import metrics
    from disk import TransparentDisk
    S, W, H = 2, 96, 80
    cam, fine, met = _scene(W, H, S)
    bg = _bg(W, H, S)
    kerr = metrics.Kerr(M=1.0, a=0.9, integrator="rk4", precision=32, schedule="direct")
    out = image_lens.render_frame(bg, kerr, 50.0, (cam.hfov, cam.vfov), theta_obs=np.radians(80.0), want=("rgb", "rgba"), samples=S,
                                  disk=TransparentDisk(max_images=3))
    lib = ltrace.render_aa(cam, met, ltrace.default_opts(axis_refine_frac=image_lens.Y_AXIS_REFINE_FRAC), _aa("disk_images", S),
                           disk=ltrace.default_disk(), background=bg)
    for k in ("rgb", "rgba", "cover"):
        assert out[k].shape == lib[k].shape and out[k].tobytes() == lib[k].tobytes(), k
    assert out["rgb"].shape == (H, W, 3)
