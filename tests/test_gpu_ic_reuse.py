"""Reuse of the camera prologue's ray records: a frame whose camera, metric, row partition and precision
equal those of the frame before it on the same stream skips k_prologue_camera.  Every output of lt_render_dev must
be byte-identical to a cold render of the same inputs (a stream the library has never seen), every change of an input
the prologue reads must run the prologue again, and so must everything else that writes or moves the records."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ltrace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

OUTPUTS = (("d_fa", np.float32, ()), ("d_w", np.uint16, ()), ("d_status", np.int8, ()), ("d_steps", np.uint32, ()),
           ("d_rgba", np.uint8, (4,)))
BASE = dict(width=256, height=192, hfov=np.radians(48.0), vfov=np.radians(37.0), psi_y=0.0, psi_x=0.0, r_obs=50.0,
            theta_obs=np.pi / 2, a=0.9, kind=ltrace.METRIC_KERR, precision=32, tb_symmetry=0, loop_around=0, row_block=16,
            n_parts=1, part=0, block_owner=None)
NB = 192 // 16
OWNER_A = np.arange(NB) % 2                      # two tables of the same length, each giving partition 0 six blocks
OWNER_B = (np.arange(NB) // 2) % 2


def _upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return d


def _background(H, W):
    return np.random.default_rng(H * 10007 + W).random((H, W, 3), dtype=np.float32)


def _scene(spec):
    s = dict(BASE, **spec)
    cam = ltrace.Camera(s["width"], s["height"], s["hfov"], s["vfov"], s["psi_y"], s["psi_x"], s["r_obs"], s["theta_obs"])
    met = ltrace.Metric(s["kind"], 0, 1.0, s["a"] if s["kind"] == ltrace.METRIC_KERR else 0.0)
    o = ltrace.default_opts(precision=s["precision"], tb_symmetry=s["tb_symmetry"], loop_around=s["loop_around"],
                            row_block=s["row_block"], n_parts=s["n_parts"], part=s["part"], block_owner=s["block_owner"])
    if s["block_owner"] is not None:
        rows = len(ltrace.owned_rows(s["height"], s["row_block"], s["block_owner"], s["part"]))
    else:
        rows = ltrace.local_rows(s["height"], s["row_block"], s["n_parts"], s["part"])
    return cam, met, o, rows


def _launch(stream_ptr, spec, how="plain"):
    """Enqueues one frame on the stream; returns its device buffers (read them after the stream has drained)."""
    import hipmini
    cam, met, o, rows = _scene(spec)
    o.stream = stream_ptr
    bufs = {k: hipmini.DeviceArray((rows, cam.width) + tail, dt) for k, dt, tail in OUTPUTS}
    bufs["bg"] = _upload(_background(cam.height, cam.width))
    ptrs = {k: bufs[k].ptr for k, _, _ in OUTPUTS}
    if how == "plain":
        ltrace.render_dev(cam, met, o, d_bg=bufs["bg"].ptr, bg_channels=3, **ptrs)
    elif how == "disk":
        bufs["d_disk"] = hipmini.DeviceArray((rows, cam.width, 3), np.float32)
        ltrace.render_disk_dev(cam, met, o, ltrace.default_disk(), d_bg=bufs["bg"].ptr, bg_channels=3,
                               d_disk=bufs["d_disk"].ptr, **ptrs)
    else:
        bufs["d_images"] = hipmini.DeviceArray((rows, cam.width, 2, 3), np.float32)
        bufs["d_n_hits"] = hipmini.DeviceArray((rows, cam.width), np.uint8)
        ltrace.render_disk_images_dev(cam, met, o, ltrace.default_disk(), max_images=2, d_bg=bufs["bg"].ptr, bg_channels=3,
                                      d_images=bufs["d_images"].ptr, d_n_hits=bufs["d_n_hits"].ptr, **ptrs)
    return bufs


def _bytes(bufs):
    return {k: v.get().tobytes() for k, v in bufs.items() if k != "bg"}


class Counted:
    """One frame at a time on a stream, with what lt_ic_reuse_counts said about it: 'hit' or 'miss'."""

    def __init__(self, stream=None):
        import hipmini
        self.stream = hipmini.Stream() if stream is None else stream     # 0: the default stream

    @property
    def ptr(self):
        return self.stream.ptr if self.stream else None

    def frame(self, spec, how="plain"):
        import hipmini
        before = ltrace.ic_reuse_counts()
        bufs = _launch(self.ptr, spec, how)
        self.stream.synchronize() if self.stream else hipmini.device_synchronize()
        after = ltrace.ic_reuse_counts()
        delta = (after[0] - before[0], after[1] - before[1])
        assert delta in ((1, 0), (0, 1)), delta
        return _bytes(bufs), "hit" if delta == (1, 0) else "miss"

    def close(self):
        if self.stream:
            ltrace.release_stream(self.ptr)


def _cold(spec, how="plain"):
    """The frame on a stream the library has never seen: nothing to reuse."""
    c = Counted()
    out, what = c.frame(spec, how)
    c.close()
    assert what == "miss"
    return out


def _digest(switch):
    env = dict(os.environ)
    env.pop("LT_IC_REUSE", None)
    if switch is not None:
        env["LT_IC_REUSE"] = switch
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ic_reuse_check.py")], env=env, check=True,
                         capture_output=True, text=True, timeout=600).stdout
    lines = [ln for ln in out.splitlines() if ln.startswith("digest ")]
    assert len(lines) == 1, out
    _, digest, hits, misses = lines[0].split()
    return digest, int(hits), int(misses)


def test_switch_off_gives_the_same_bytes():
    """Frames A, A, B, A, A on one stream, float32 / float64, both schedules, in fresh processes: LT_IC_REUSE=0 (the
    prologue runs every frame) and the default give the same bytes; the default reuses the records of the repeated
    frames only."""
    off, on, dflt = _digest("0"), _digest("1"), _digest(None)
    assert off[0] == on[0] == dflt[0]
    assert off[1:] == (0, 20)
    assert on[1:] == dflt[1:] == (8, 12)


def test_repeated_frame_reuses_and_equals_cold():
    c = Counted()
    first, what = c.frame({})
    assert what == "miss"
    assert first == _cold({})
    for _ in range(3):
        again, what = c.frame({})
        assert what == "hit"
        assert again == first
    c.close()
    again, what = c.frame({})                                      # the slot and its key went with lt_release_stream
    assert what == "miss" and again == first
    c.close()


CHANGES = [
    ("width", {}, dict(width=248)),
    ("height", {}, dict(height=176)),
    ("hfov", {}, dict(hfov=np.radians(47.0))),
    ("vfov", {}, dict(vfov=np.radians(38.0))),
    ("psi_x", {}, dict(psi_x=0.02)),
    ("psi_y", {}, dict(psi_y=-0.015)),
    ("r_obs", {}, dict(r_obs=40.0)),
    ("theta_obs", {}, dict(theta_obs=1.2)),
    ("spin", {}, dict(a=0.5)),
    ("spin_sign", {}, dict(a=-0.9)),
    ("metric_kind", {}, dict(kind=ltrace.METRIC_SCHWARZSCHILD)),
    ("precision", {}, dict(precision=64)),
    ("tb_symmetry", {}, dict(tb_symmetry=1)),
    ("loop_around", {}, dict(loop_around=1)),
    ("row_block", dict(n_parts=2), dict(n_parts=2, row_block=8)),
    ("n_parts", {}, dict(n_parts=2)),
    ("part", dict(n_parts=2, part=0), dict(n_parts=2, part=1)),
    ("block_owner_contents", dict(n_parts=2, block_owner=OWNER_A), dict(n_parts=2, block_owner=OWNER_B)),
    ("block_owner_vs_cyclic", dict(n_parts=2), dict(n_parts=2, block_owner=OWNER_A)),
]


@pytest.mark.parametrize("name,base,changed", CHANGES, ids=[c[0] for c in CHANGES])
def test_one_changed_input_runs_the_prologue_again(name, base, changed):
    """base, base, changed, changed, base on one stream: the first frame after each change runs the prologue and
    equals a cold render of its inputs; so does the frame that goes back."""
    cold_base, cold_changed = _cold(base), _cold(changed)
    if name not in ("loop_around", "block_owner_vs_cyclic"):       # (these two need not move a pixel: no source leaves
        assert cold_base != cold_changed                           # this frame / the table deals the rows out alike)
    c = Counted()
    for spec, want, cold in ((base, "miss", cold_base), (base, "hit", cold_base), (changed, "miss", cold_changed),
                             (changed, "hit", cold_changed), (base, "miss", cold_base)):
        out, what = c.frame(spec)
        assert what == want, (name, what, want)
        assert out == cold, name
    c.close()


def test_batch_twin_between_two_frames():
    """The batch twins write their records into the default stream's workspace: the frame after one runs the prologue."""
    c = Counted(stream=0)
    first, _ = c.frame({})
    again, what = c.frame({})
    assert what == "hit" and again == first
    al = np.linspace(0.05, 0.3, 3000)
    fa, w = np.full(al.size, np.nan), np.zeros(al.size, dtype=np.int64)
    ltrace.trace_batch_kerr(1.0, 0.9, 50.0, al, np.full(al.size, 0.7), np.pi / 2, 5000.0, None, fa, w, precision=32)
    after, what = c.frame({})
    assert what == "miss"
    assert after == first == _cold({})
    fa2, w2 = np.full(al.size, np.nan), np.zeros(al.size, dtype=np.int64)
    ltrace.trace_batch_kerr(1.0, 0.9, 50.0, al, np.full(al.size, 0.7), np.pi / 2, 5000.0, None, fa2, w2, precision=32)
    assert fa.tobytes() == fa2.tobytes() and w.tobytes() == w2.tobytes()


def test_workspace_growth():
    small, big = dict(width=256, height=256), dict(width=512, height=512)
    c = Counted()
    first, what = c.frame(small)
    assert what == "miss"
    grown, what = c.frame(big)                                     # a new, larger buffer
    assert what == "miss" and grown == _cold(big)
    back, what = c.frame(small)                                    # same buffer; its records are the large frame's
    assert what == "miss" and back == first
    again, what = c.frame(small)
    assert what == "hit" and again == first
    c.close()


def test_disk_and_plain_frames_share_the_records():
    """One camera through lt_render_disk_dev, lt_render_dev, lt_render_disk_dev and lt_render_disk_images_dev: the same
    records serve all of them (without tb_symmetry, which the disks never apply), each frame equal to its cold render."""
    cold = {how: _cold({}, how) for how in ("disk", "plain", "images")}
    c = Counted()
    for how, want in (("disk", "miss"), ("plain", "hit"), ("disk", "hit"), ("images", "hit"), ("plain", "hit")):
        out, what = c.frame({}, how)
        assert what == want, (how, what)
        assert out == cold[how], how
    # with tb_symmetry the plain frame traces half the rows: other records
    tb = dict(tb_symmetry=1)
    cold_tb = {how: _cold(tb, how) for how in ("disk", "plain")}
    for how, want in (("plain", "miss"), ("disk", "miss"), ("disk", "hit"), ("plain", "miss")):
        out, what = c.frame(tb, how)
        assert what == want, (how, what)
        assert out == cold_tb[how], how
    c.close()


def test_two_streams_keep_their_own_records():
    """Two streams alternating two cameras, frames in flight together: each stream reuses its own records."""
    specs = [dict(width=320, height=240), dict(width=240, height=320, psi_x=0.05, psi_y=0.02)]
    cold = [_cold(s) for s in specs]
    streams = [Counted(), Counted()]
    before = ltrace.ic_reuse_counts()
    frames = [[], []]
    for rep in range(3):
        for i in (0, 1):
            frames[i].append(_launch(streams[i].ptr, specs[i]))
    for s in streams:
        s.stream.synchronize()
    after = ltrace.ic_reuse_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (4, 2)
    for i in (0, 1):
        for bufs in frames[i]:
            assert _bytes(bufs) == cold[i]
        streams[i].close()


def test_timing_counts_a_frame_that_reused_its_records():
    """lt_timing_collect still counts the call, and reports the time between two event records, not a stale one."""
    import hipmini
    c = Counted()
    ltrace.timing_collect()
    cam, met, o, rows = _scene(dict(width=512, height=512))
    o.stream, o.timing = c.ptr, 1
    fa = hipmini.DeviceArray((rows, cam.width), np.float32)
    times = []
    for _ in range(3):
        ltrace.render_dev(cam, met, o, d_fa=fa.ptr)
        c.stream.synchronize()
        times.append(ltrace.timing_collect())
    assert [t["calls"] for t in times] == [1, 1, 1]
    for t in times:
        assert t["prologue_ms"] >= 0.0 and t["integrate_ms"] > 0.0 and t["epilogue_ms"] > 0.0
    print("prologue_ms first / reused:", [t["prologue_ms"] for t in times])
    c.close()
