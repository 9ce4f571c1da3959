"""Where the tail split cuts a frame's tile queue (tail_split_plan, lt_api.hip), against a brute-force
enumeration of the queue order: queue_pos_to_tile (lt_kernels.hpp) restated here in Python, position by position.  For
every shape, strip, rectangle, slot count and requested size of the grid below, a split must give
  * every queue position >= pos_split a tile with ty >= ty_split that lies outside the strip,
  * every tile with ty < ty_split a queue position < pos_split,
  * every strip tile a queue position < pos_split,
and a non-empty part on either side; a frame that is not split reports (tiles_y, n_tiles).  Forced sizes are clamped to
the rows below the rectangle, the automatic size is one fill of the slots and declines where the frame has no room for
it.  lt_tail_split_plan is host arithmetic: no GPU."""
import itertools

import pytest

import ltrace


def queue_pos_to_tile(pos, tiles_x, tiles_y, strip_x0, strip_x1, hot_x0, hot_x1, hot_y0, hot_y1):
    """(tx, ty) of queue position pos: the strip's columns row by row, the rectangle, then everything else row-major on the
    grid with the strip's columns removed (hot_x0 / hot_x1 are columns of that grid)."""
    sw = strip_x1 - strip_x0
    n_strip = sw * tiles_y
    if pos < n_strip:
        return strip_x0 + pos % sw, pos // sw
    pos -= n_strip
    cw = tiles_x - sw
    hw, hh = hot_x1 - hot_x0, hot_y1 - hot_y0
    if pos < hw * hh:
        ty, cx = hot_y0 + pos // hw, hot_x0 + pos % hw
    else:
        p = pos - hw * hh
        top, side = hot_y0 * cw, cw - hw
        mid = hh * side
        if p < top:
            ty, cx = p // cw, p % cw
        elif p < top + mid:
            p -= top
            ty, o = hot_y0 + p // side, p % side
            cx = o if o < hot_x0 else o + hw
        else:
            p -= top + mid
            ty, cx = hot_y1 + p // cw, p % cw
    return (cx if cx < strip_x0 else cx + sw), ty


def frames():
    """(tiles_x, tiles_y, strip_x0, strip_x1, hot_x0, hot_x1, hot_y0, hot_y1): no strip and no rectangle, a strip alone, a
    rectangle in the middle, at the top, reaching the last tile row, as wide as the compacted grid; the strip at either
    edge; one tile row, one tile column."""
    out = []
    for tx, ty in ((1, 1), (1, 9), (9, 1), (7, 5), (26, 18), (25, 17), (64, 40)):
        out.append((tx, ty, 0, 0, 0, 0, 0, 0))
        for s0, s1 in ((0, min(2, tx)), (tx // 2, min(tx // 2 + 4, tx)), (max(tx - 3, 0), tx)):
            cw = tx - (s1 - s0)
            out.append((tx, ty, s0, s1, 0, 0, 0, 0))
            if cw <= 0:
                continue
            for hx0, hx1 in ((0, cw), (cw // 3, max(cw // 3 + 1, 2 * cw // 3))):
                for hy0, hy1 in ((0, max(1, ty // 2)), (ty // 3, max(ty // 3 + 1, 2 * ty // 3)), (ty // 2, ty)):
                    if hx1 <= cw and hy1 <= ty and hx0 < hx1 and hy0 < hy1:
                        out.append((tx, ty, s0, s1, hx0, hx1, hy0, hy1))
    return sorted(set(out))


FRAMES = frames()
SLOTS = (0, 1, 7, 60, 400, 5120)
REQUESTS = (-1, 0, 1, 2, 3, 10, 1 << 20)


def test_the_restated_queue_order_is_a_permutation_of_the_tiles():
    for f in FRAMES:
        tx, ty = f[:2]
        seen = {queue_pos_to_tile(p, *f) for p in range(tx * ty)}
        assert seen == set(itertools.product(range(tx), range(ty))), f


@pytest.mark.parametrize("request_rows", REQUESTS)
def test_the_cut_separates_the_queue_as_the_launches_and_the_epilogue_assume(request_rows):
    n_split = 0
    for f in FRAMES:
        tx, ty, s0, s1, _, _, _, hy1 = f
        n_tiles, cw = tx * ty, tx - (s1 - s0)
        order = [queue_pos_to_tile(p, *f) for p in range(n_tiles)]
        for slots in SLOTS:
            split, ty_split, pos_split = ltrace.tail_split_plan(tx, ty, s0, s1, hy1, slots, request_rows)
            if not split:
                assert (ty_split, pos_split) == (ty, n_tiles), (f, slots)
                continue
            n_split += 1
            rows_b = ty - ty_split
            assert request_rows != 0 and 1 <= rows_b <= ty - hy1 and 0 < pos_split < n_tiles, (f, slots, ty_split, pos_split)
            assert pos_split == n_tiles - rows_b * cw
            for pos, (x, y) in enumerate(order):
                in_strip = s0 <= x < s1
                if pos >= pos_split:
                    assert y >= ty_split and not in_strip, (f, slots, pos, x, y)
                if y < ty_split or in_strip:
                    assert pos < pos_split, (f, slots, pos, x, y)
            if request_rows > 0:   # clamped to the rows below the rectangle, and part A keeps a tile
                avail = ty - hy1 - (1 if (ty - hy1) * cw >= n_tiles else 0)
                assert rows_b == min(request_rows, avail), (f, slots)
            else:                  # one fill of the slots, whole tile rows; part A keeps a fill
                assert slots > 0 and rows_b == -(-slots // cw) and pos_split >= slots, (f, slots)
    assert (n_split > 0) == (request_rows != 0)


def test_where_the_frame_is_not_split():
    # off; no rows below the rectangle; every column in the strip; a forced size on a frame of one tile row without a strip
    assert ltrace.tail_split_plan(64, 40, 30, 34, 25, 5120, 0) == (False, 40, 2560)
    assert ltrace.tail_split_plan(64, 40, 30, 34, 40, 400, 3) == (False, 40, 2560)
    assert ltrace.tail_split_plan(64, 40, 30, 34, 40, 400, -1) == (False, 40, 2560)
    assert ltrace.tail_split_plan(4, 40, 0, 4, 0, 7, 3) == (False, 40, 160)
    assert ltrace.tail_split_plan(64, 1, 0, 0, 0, 7, 1) == (False, 1, 64)
    # automatic: no slot count; a fill is more than the rows below the rectangle; part A would be less than a fill
    assert ltrace.tail_split_plan(64, 40, 30, 34, 25, 0, -1) == (False, 40, 2560)
    assert ltrace.tail_split_plan(64, 40, 30, 34, 38, 400, -1) == (False, 40, 2560)   # 7 rows needed, 2 there
    assert ltrace.tail_split_plan(64, 40, 30, 34, 10, 1300, -1) == (False, 40, 2560)  # 22 rows = 1320 tiles: 1240 left
    # ... and where it is: 400 slots over 60 columns are 7 rows
    assert ltrace.tail_split_plan(64, 40, 30, 34, 25, 400, -1) == (True, 33, 2560 - 7 * 60)
    assert ltrace.tail_split_plan(64, 40, 30, 34, 25, 400, 1 << 20) == (True, 25, 2560 - 15 * 60)
    # the flagship frame: 512 x 512 tiles, a strip of 4 columns (5 when the hole's column falls between tiles), 5120 slots
    assert ltrace.tail_split_plan(512, 512, 254, 258, 300, 5120, -1) == (True, 501, 512 * 512 - 11 * 508)
    with pytest.raises(ltrace.LtraceError):
        ltrace.tail_split_plan(0, 4, 0, 0, 0, 7, 1)
    with pytest.raises(ltrace.LtraceError):
        ltrace.tail_split_plan(8, 4, 0, 0, 5, 7, 1)
