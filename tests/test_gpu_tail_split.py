"""The tail split of the frame path (ltrace.set_tail_split / LT_TAIL_SPLIT): the last tile rows of a
frame's tile queue are integrated by a second launch on a side stream of the library's, and the rows above are shaded
while it ends.  The same rays are traced by the same code and the same pixels shaded by the same kernel, so the switch
may change NOTHING: every comparison here is of bytes -- final_alpha, winding, status, steps, rgb and rgba of every pixel
-- and of every counter of lt_stats but the two clock samples (rays, steps, right-hand-side evaluations, escaped /
captured / invalid, wave iterations, waves, background tiles, fixed-quadrant iterations), split on against split off.
Sizes of the second part: 1 and 3 tile rows, as many as fit (a request the library clamps), and the automatic size.
Whether a frame was split is read from ltrace.tail_split_counts.

A partition taller than 65535 rows -- what the epilogue's row slices are for -- is not a test of a few seconds and is
left out; the slicing code runs in every split frame (rows of part A, then the rest)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":   # (test_record_reuse_off's process: no conftest has set the path)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "light-path-tracer_amd"), os.path.join(ROOT, "tests")]

import ltrace

pytestmark = pytest.mark.gpu

OUTPUTS = (("d_fa", np.float32, ()), ("d_w", np.uint16, ()), ("d_status", np.int8, ()), ("d_steps", np.uint32, ()),
           ("d_rgb", np.float32, (3,)), ("d_rgba", np.uint8, (4,)))
COUNTERS = [i for i in range(ltrace.STAT_WORDS) if i not in (ltrace.STAT_CLK_CYCLES, ltrace.STAT_CLK_TICKS)]
BASE = dict(width=256, height=192, hfov=np.radians(48.0), vfov=np.radians(37.0), psi_y=0.0, psi_x=0.0, r_obs=50.0,
            theta_obs=np.pi / 2, a=0.9, kind=ltrace.METRIC_KERR, precision=32, integrator="rk4", schedule="direct",
            tb_symmetry=0, bg_sampling=ltrace.BG_GLOBAL, row_block=16, n_parts=1, part=0, block_owner=None, bg=False, timing=0)
ALL = 1 << 20   # "as many tile rows as fit"
SIZES = (1, 3, ALL, -1)


def _upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return d


def _scene(spec):
    s = dict(BASE, **spec)
    cam = ltrace.Camera(s["width"], s["height"], s["hfov"], s["vfov"], s["psi_y"], s["psi_x"], s["r_obs"], s["theta_obs"])
    met = ltrace.Metric(s["kind"], 0, 1.0, s["a"] if s["kind"] == ltrace.METRIC_KERR else 0.0)
    o = ltrace.default_opts(precision=s["precision"], integrator=s["integrator"], schedule=s["schedule"],
                            tb_symmetry=s["tb_symmetry"], bg_sampling=s["bg_sampling"], row_block=s["row_block"],
                            n_parts=s["n_parts"], part=s["part"], block_owner=s["block_owner"], timing=s["timing"])
    if s["block_owner"] is not None:
        rows = len(ltrace.owned_rows(s["height"], s["row_block"], s["block_owner"], s["part"]))
    else:
        rows = ltrace.local_rows(s["height"], s["row_block"], s["n_parts"], s["part"])
    bg = np.random.default_rng(s["height"] * 10007 + s["width"]).random((s["height"], s["width"], 3), dtype=np.float32) if s["bg"] else None
    return cam, met, o, rows, bg


def enqueue(stream_ptr, spec):
    """One frame on the stream; returns its device buffers (to be read once the stream has drained)."""
    import hipmini
    cam, met, o, rows, bg = _scene(spec)
    o.stream = stream_ptr
    bufs = {k: hipmini.DeviceArray((rows, cam.width) + tail, dt) for k, dt, tail in OUTPUTS}
    bufs["d_stats"] = _upload(np.zeros(ltrace.STAT_WORDS, dtype=np.uint64))
    keep = _upload(bg) if bg is not None else None
    ltrace.render_dev(cam, met, o, d_bg=keep.ptr if keep else 0, bg_channels=3, **{k: v.ptr for k, v in bufs.items()})
    bufs["_bg"] = keep
    return bufs


def collect(bufs):
    out = {k: bufs[k].get().tobytes() for k, _, _ in OUTPUTS}
    st = bufs["d_stats"].get()
    out["counters"] = tuple(int(st[i]) for i in COUNTERS)
    return out


class OnStream:
    """Frames on one stream of the test's own, one at a time; each with what tail_split_counts said about it."""

    def __init__(self):
        import hipmini
        self.stream = hipmini.Stream()

    def frame(self, spec, size):
        before = ltrace.tail_split_counts()
        prev = ltrace.set_tail_split(size)
        try:
            bufs = enqueue(self.stream.ptr, spec)
        finally:
            ltrace.set_tail_split(prev)
        self.stream.synchronize()
        after = ltrace.tail_split_counts()
        return collect(bufs), (after[0] - before[0], after[1] - before[1])

    def close(self):
        ltrace.release_stream(self.stream.ptr)


def frame(spec, size):
    s = OnStream()
    try:
        return s.frame(spec, size)
    finally:
        s.close()


SPLIT, WHOLE = (1, 0), (0, 1)


def check(spec, sizes=SIZES, expect=None, rays=None):
    """The frame with the split off and with every size: equal bytes and counters.  expect: what the counts must say of
    the forced sizes (default: split) -- the automatic size may decline a frame this small."""
    off, what = frame(spec, 0)
    assert what == WHOLE
    s = dict(BASE, **spec)
    if rays is None:
        rays = _scene(spec)[3] * s["width"]
    assert off["counters"][ltrace.STAT_RAYS] == rays and off["counters"][ltrace.STAT_STEPS] > 0
    for size in sizes:
        on, what = frame(spec, size)
        assert what == (expect or SPLIT) or (size == -1 and what == WHOLE), (size, what)
        for k in off:
            assert on[k] == off[k], (spec, size, k, on["counters"], off["counters"])
    return off


def test_persistent_grid_more_than_one_fill_of_the_chip():
    """1024 x 640: 10 240 tiles, handed out from the two head words."""
    off = check(dict(width=1024, height=640))
    c = off["counters"]
    assert c[COUNTERS.index(ltrace.STAT_WAVES)] == 10240 and c[COUNTERS.index(ltrace.STAT_EQ_ITERS)] > 0


def test_automatic_size_splits_a_frame_of_several_fills():
    """2048 x 1024, 32 768 tiles on 5 120 wave slots: 21 tile rows of 252 tiles are one fill, 41 rows lie below the rectangle."""
    spec = dict(width=2048, height=1024, hfov=np.radians(90.0), vfov=np.radians(53.13))
    off, _ = frame(spec, 0)
    on, what = frame(spec, -1)
    assert what == SPLIT
    assert on == off


def test_one_workgroup_per_tile():
    """200 x 136: 425 tiles, either part fits the chip and runs without a head word."""
    check(dict(width=200, height=136), sizes=(1, 3, ALL))


def test_pad_lanes():
    """203 x 141: neither dimension a multiple of 8, the last tile row and column carry pad lanes."""
    check(dict(width=203, height=141), sizes=(1, 3, ALL))
    check(dict(width=203, height=141, bg=True), sizes=(1, ALL))


def test_hot_rectangle_at_either_edge_and_cameras_off_the_hole():
    # the hole near the last row: the rectangle reaches the last tile row, nothing lies below it -- no split
    check(dict(psi_y=-0.3), sizes=(1, ALL), expect=WHOLE)
    # near the first row: the rectangle starts at tile row 0
    check(dict(psi_y=0.3), sizes=(1, 3, ALL))
    # looking away from the hole: no strip, no rectangle; "as many as fit" is every tile row but the first, 1 all but the last
    check(dict(psi_y=np.pi), sizes=(1, ALL))
    check(dict(psi_x=0.2), sizes=(1, ALL))        # the hole off the frame's middle column: the strip off centre
    check(dict(theta_obs=1.0), sizes=(1, 3, ALL))


@pytest.mark.parametrize("spec", [dict(kind=ltrace.METRIC_SCHWARZSCHILD), dict(schedule="queue"), dict(tb_symmetry=1),
                                  dict(bg=True, bg_sampling=ltrace.BG_LDS_TILES)],
                         ids=["schwarzschild", "queue_schedule", "tb_symmetry", "lds_background"])
def test_paths_that_are_never_split(spec):
    off, what = frame(spec, 0)
    assert what == WHOLE
    for size in (3, -1):
        on, what = frame(spec, size)
        assert what == WHOLE
        if spec.get("schedule") == "queue":   # (the queue schedule groups rays into wavefronts differently from run to run)
            per_wave = [COUNTERS.index(i) for i in (ltrace.STAT_WAVE_ITERS, ltrace.STAT_WAVES, ltrace.STAT_EQ_ITERS)]
            on["counters"] = tuple(v for n, v in enumerate(on["counters"]) if n not in per_wave)
            ref = dict(off, counters=tuple(v for n, v in enumerate(off["counters"]) if n not in per_wave))
            assert on == ref
        else:
            assert on == off


def test_global_gather_background_splits():
    check(dict(bg=True, bg_sampling=ltrace.BG_GLOBAL), sizes=(1, 3, ALL))


@pytest.mark.parametrize("spec", [dict(precision=32, integrator="rk4"), dict(precision=64, integrator="rk4"),
                                  dict(precision=64, integrator="dp45_exact")], ids=["f32_rk4", "f64_rk4", "f64_dp45_exact"])
def test_precisions_and_integrators(spec):
    check(dict(spec, width=200, height=136), sizes=(1, ALL))


def test_block_cyclic_partitions():
    """384 rows in three parts of 128 local rows = 16 tile rows each; a partition's rectangle covers about a third of the
    frame's plus a row block, so the frame is tall and its field of view wide enough to leave three tile rows below it."""
    for part in range(3):
        check(dict(height=384, hfov=np.radians(75.0), vfov=np.radians(60.0), n_parts=3, part=part), sizes=(1, ALL))


def test_block_owner_table_with_unequal_shares_and_an_empty_partition():
    # 8, 0 and 4 of the 12 row blocks; either partition's last block lies below the rows the hole's rectangle touches
    owner = np.array([0, 0, 0, 2, 2, 0, 0, 2, 0, 0, 0, 2], dtype=np.uint16)
    for part in (0, 2):
        check(dict(n_parts=3, part=part, block_owner=owner), sizes=(1, ALL))
    for size in (0, 3):   # the partition without rows: nothing is launched, nothing is counted
        out, what = frame(dict(n_parts=3, part=1, block_owner=owner), size)
        assert what == (0, 0) and out["counters"] == (0,) * len(COUNTERS)


def _first_and_repeated(size):
    s = OnStream()
    try:
        hits0 = ltrace.ic_reuse_counts()[0]
        first, w1 = s.frame({}, size)
        again, w2 = s.frame({}, size)
        return first, again, (w1, w2), ltrace.ic_reuse_counts()[0] - hits0
    finally:
        s.close()


def test_record_reuse_on():
    f0, a0, w0, hits0 = _first_and_repeated(0)
    f3, a3, w3, hits3 = _first_and_repeated(3)
    assert w0 == (WHOLE, WHOLE) and w3 == (SPLIT, SPLIT)
    assert hits0 == hits3 == 1          # the repeated frame skipped the prologue, split or not
    assert f0 == a0 == f3 == a3


def test_record_reuse_off():
    """LT_IC_REUSE is read once per process: the same two frames in a process of their own."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, LT_IC_REUSE="0"), check=True,
                         capture_output=True, text=True, timeout=300).stdout
    assert "reuse_off equal=True hits=0 split=True" in out, out


def test_workspace_growth_on_one_stream_with_stats():
    """A small frame, then one that replaces the stream's workspace (control words, head words and partial counters
    with it), then the small one again: each equals its frame on a stream of its own, split off."""
    small, large = dict(width=200, height=136), dict(width=512, height=384)
    ref = {k: frame(spec, 0)[0] for k, spec in (("small", small), ("large", large))}
    s = OnStream()
    try:
        for k, spec in (("small", small), ("large", large), ("small", small)):
            got, what = s.frame(spec, 3)
            assert what == SPLIT and got == ref[k], k
    finally:
        s.close()


def test_two_streams_in_flight():
    """Two user streams, different frames enqueued turn by turn without waiting, then both released."""
    specs = (dict(width=256, height=192), dict(width=203, height=141, theta_obs=1.0))
    ref = [frame(spec, 0)[0] for spec in specs]
    streams = [OnStream(), OnStream()]
    prev = ltrace.set_tail_split(3)
    try:
        before = ltrace.tail_split_counts()
        pending = [[enqueue(st.stream.ptr, spec) for st, spec in zip(streams, specs)] for _ in range(3)]
        for st in streams:
            st.stream.synchronize()
        after = ltrace.tail_split_counts()
        assert (after[0] - before[0], after[1] - before[1]) == (6, 0)
        for turn in pending:
            for bufs, want in zip(turn, ref):
                assert collect(bufs) == want
    finally:
        ltrace.set_tail_split(prev)
        for st in streams:
            st.close()


def test_timing_marks_tile_the_call():
    """With timing on, the three times are non-negative and their sum is at most the wall time of the call (enqueue to
    drained stream) plus 2 %."""
    spec = dict(width=1024, height=640, timing=1)
    s = OnStream()
    try:
        s.frame(spec, 3)                # (first use of the stream: allocations, the side stream)
        ltrace.timing_collect()
        for size in (3, ALL, 0):
            prev = ltrace.set_tail_split(size)
            try:
                t0 = time.perf_counter()
                bufs = enqueue(s.stream.ptr, spec)
                s.stream.synchronize()
                wall_ms = (time.perf_counter() - t0) * 1e3
            finally:
                ltrace.set_tail_split(prev)
            t = ltrace.timing_collect()
            print(size, t, wall_ms)
            assert t["calls"] == 1
            assert t["prologue_ms"] >= 0 and t["integrate_ms"] > 0 and t["epilogue_ms"] >= 0
            assert t["prologue_ms"] + t["integrate_ms"] + t["epilogue_ms"] <= wall_ms * 1.02
            del bufs
    finally:
        s.close()


def test_the_switch_returns_the_previous_setting():
    prev = ltrace.set_tail_split(5)
    assert ltrace.set_tail_split(-7) == 5
    assert ltrace.set_tail_split(prev) == -1      # anything below -1 is the automatic size


if __name__ == "__main__":   # test_record_reuse_off's process
    f0, a0, w0, hits0 = _first_and_repeated(0)
    f3, a3, w3, hits3 = _first_and_repeated(3)
    print(f"reuse_off equal={f0 == a0 == f3 == a3} hits={hits0 + hits3} split={w3 == (SPLIT, SPLIT) and w0 == (WHOLE, WHOLE)}")
