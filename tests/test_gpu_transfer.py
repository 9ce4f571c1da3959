"""The reverberation kernel (lt_transfer.hpp) through lt_disk_transfer[_dev].  Cases, records, tables, grids, the restatement
and its bound are tests/test_transfer_host.py's (its header derives the bound): the records of test_diskmap_host -- 257 x 331
x 8, 260 x 300 x 3, 3 x 70 x 5, 1 x 1 x 1: a ragged last chunk, fewer pixels than a chunk, one pixel -- with slots that
contribute nothing in each of the rule's ways mixed in, tables with a dark stretch and a NaN delay that leave slots off both
ends, and grids of 1 x 1, 64 x 96, the cap 126 x 254 (eight key tiles in one plane) and one plane per image order of 62 x 62
(eight planes of 4096 keys at eight images: a tile each).

What would catch a wrong kernel: the restatement (a slot in a wrong key moves two keys by a whole weight, thousands of
bounds), the power-of-two records whose sums are exact in any order (an entry lost, doubled or added to a neighbour's key),
and the tiling tests (a key's bits inside a grid of several tiles against the same key in a grid of one, at another offset in
its tile and in another tile).

MEASURED on an MI355X (gfx950), the figures the tests print:
    against the restatement, largest difference in units of its bound: big 0.30, mid 0.03 (1 x 1) ... 0.28, strip 0.07 ... 0.21,
        one 0.009; the same with and without counts; the same keys hold light (27 998 of 32 768 on big's eight planes);
    the traced frame: 0.23 of the bound on 2 285 terms in 398 keys; t_ref 54.583, geometric minimum -14.28, earliest delay
        2.54; the three orders' responses start at tau >= 0, 20 and 36;
    every byte-for-byte comparison holds; the whole file runs in 2.3 s, its slowest case (the traced frame) in 0.8 s.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES
from test_transfer_host import (EXPOSURE, G_HI, G_LO, LD, T_REF, TAU_HI, TAU_LO, U, bin_ref, check, exact_case, exact_histogram, grids, make_tables,
                                restate_slots, slots_of, transfer_records)

pytestmark = pytest.mark.gpu


def setup(name):
    c = CASES[name]
    hits, n_hits = transfer_records(name)
    return c, hits, n_hits, ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a), ltrace.default_disk(r_out=c.r_out, exposure=EXPOSURE)


def transfer(hits, n_hits, met, dk, spec, grid, tables, t_ref=T_REF):
    r_min, r_max, delay, emis = tables
    return ltrace.disk_transfer(hits, n_hits, met, dk, spec.to_lt(), grid.to_lt(r_min, r_max, len(delay), t_ref), delay, emis)


def upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(a.ctypes.data), a.nbytes, 1), "hipMemcpy H2D")
    return d


# ---- 1. against the restatement ---------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1, False), (64, 96, False), (126, 254, False), (62, 62, True)]


@pytest.mark.parametrize("counts", [True, False])
@pytest.mark.parametrize("n_tau,n_bins,split", GRIDS)
@pytest.mark.parametrize("name", ["big", "mid", "strip", "one"])
def test_against_the_restatement(name, n_tau, n_bins, split, counts):
    c, hits, n_hits, met, dk = setup(name)
    spec, grid = grids(n_tau, n_bins, split)
    got = transfer(hits, n_hits if counts else None, met, dk, spec, grid, make_tables(name))
    assert got.shape == (c.m if split else 1, n_tau + 2, n_bins + 2)
    check(got, slots_of(name, counts), spec, grid, f"{name} {n_tau} x {n_bins}, split {split}, counts {counts}")
    if (n_tau, n_bins) == (126, 254) and name in ("big", "mid"):          # light on both sides of every border between two key tiles
        flat = got.ravel()
        assert flat.size == 32768 and all(flat[4096 * t - 1] > 0 and flat[4096 * t] > 0 for t in range(1, 8))
    if split and name == "big":
        assert got.size == 32768 and all(np.count_nonzero(got[j]) > 1000 for j in range(8))         # a tile per plane, each with light


# ---- 2. byte for byte ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_powers_of_two_equal_an_integer_histogram(split):
    hits, n_hits, tables, tau, exposure, t_ref = exact_case()
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(exposure=exposure)
    # keys: one tile (300; split 900); several (128 x 128 = 4 tiles; split 3 x 30 x 128 = 3 tiles); the cap (64 x 512; split 3 x 21 x 512 = 32 256)
    for n_bins, g_hi in ((8, 2.25), (126, 2.25), (510, 128.0)):
        n_tau = {8: 28, 126: 28, 510: 19}[n_bins] if split else {8: 28, 126: 126, 510: 62}[n_bins]
        spec = diskmod.Spectrum(0.25, g_hi, n_bins, split_orders=split)
        grid = diskmod.TransferGrid(8.0, 8.0 + 4.0 * n_tau, n_tau) if n_tau != 126 else diskmod.TransferGrid(8.0, 134.0, 126)
        got = transfer(hits, n_hits, met, dk, spec, grid, tables, t_ref)
        want = np.stack([exact_histogram(hits, n_hits, tau, spec, grid, j) for j in range(3)]) if split else exact_histogram(hits, n_hits, tau, spec, grid)[None]
        assert (got * (16.0 / exposure)).tobytes() == want.tobytes(), (split, n_bins)
        assert want.sum() > 1000 and want[:, 0].sum() > 0 and not np.any(np.signbit(got))
        assert got.tobytes() == diskmod.disk_transfer(hits, n_hits, exposure, spec, grid, *tables, t_ref).tobytes()


def test_a_call_repeated_and_the_dev_form():
    import hipmini
    c, hits, n_hits, met, dk = setup("strip")
    tables = make_tables("strip")
    r_min, r_max, delay, emis = tables
    d_hits, d_nh, d_delay, d_emis = upload(hits), upload(n_hits), upload(delay), upload(emis)
    for n_tau, n_bins, split in GRIDS:
        spec, grid = grids(n_tau, n_bins, split)
        for counts, d_counts in ((n_hits, d_nh.ptr), (None, 0)):
            host = transfer(hits, counts, met, dk, spec, grid, tables)
            assert transfer(hits, counts, met, dk, spec, grid, tables).tobytes() == host.tobytes()   # a second run differs in no bit
            d_out = hipmini.DeviceArray(host.shape, np.float64)
            ltrace.disk_transfer_dev(d_hits.ptr, d_counts, c.R, c.W, c.m, met, dk, spec.to_lt(), grid.to_lt(r_min, r_max, len(delay), T_REF),
                                     d_delay.ptr, d_emis.ptr, d_out.ptr)
            hipmini.device_synchronize()
            assert d_out.get().tobytes() == host.tobytes()
    c, hits, n_hits, met, dk = setup("big")
    spec, grid = grids(126, 254)
    first = transfer(hits, n_hits, met, dk, spec, grid, make_tables("big"))
    assert transfer(hits, n_hits, met, dk, spec, grid, make_tables("big")).tobytes() == first.tobytes()


def test_adjacent_ranges_match_the_spanning_grid():
    c, hits, n_hits, met, dk = setup("mid")
    tables = make_tables("mid")
    spec = diskmod.Spectrum(G_LO, G_HI, 96)
    whole = transfer(hits, n_hits, met, dk, spec, diskmod.TransferGrid(0.0, 40.0, 4), tables)
    part = transfer(hits, n_hits, met, dk, spec, diskmod.TransferGrid(0.0, 20.0, 2), tables)
    assert whole.shape == (1, 6, 98) and part.shape == (1, 4, 98)
    assert np.ascontiguousarray(part[:, :3]).tobytes() == np.ascontiguousarray(whole[:, :3]).tobytes()     # the underflow and bins 1 and 2
    assert np.count_nonzero(part[:, 1:3]) > 100
    assert np.all(np.abs(part[0, 3].astype(LD) - whole[0, 3:].astype(LD).sum(axis=0)) <= 50000 * U * part[0, 3])    # its overflow is the rest


def test_a_key_does_not_depend_on_the_tiling():
    """The header's promise.  (a) A plane of a split grid -- tile j of eight -- against the same keys in a grid of one tile: the
    records with every other slot's g made NaN, unsplit.  (b) A window of 16 delay bins cut from a grid of 64: the same
    keys at another offset in their tile and in other tiles (rows 1 ... 16 of 18 against rows 17 ... 32 of 66, 256 columns)."""
    c, hits, n_hits, met, dk = setup("big")
    tables = make_tables("big")
    split, grid = grids(30, 126, True)
    planes = transfer(hits, n_hits, met, dk, split, grid, tables)
    assert planes.shape == (8, 32, 128) and planes.size == 8 * 4096
    for j in (0, 3, 7):
        only = hits.copy()
        only[:, :, np.arange(8) != j, 2] = np.nan
        one = transfer(only, n_hits, met, dk, grids(30, 126)[0], grid, tables)
        assert one.shape == (1, 32, 128) and one[0].tobytes() == planes[j].tobytes() and np.count_nonzero(one) > 1000, j
    spec = diskmod.Spectrum(G_LO, G_HI, 254)
    whole = transfer(hits, n_hits, met, dk, spec, diskmod.TransferGrid(-16.0, 240.0, 64), tables)
    window = transfer(hits, n_hits, met, dk, spec, diskmod.TransferGrid(48.0, 112.0, 16), tables)
    assert whole.shape == (1, 66, 256) and window.shape == (1, 18, 256)
    assert np.ascontiguousarray(window[0, 1:17]).tobytes() == np.ascontiguousarray(whole[0, 17:33]).tobytes() and np.count_nonzero(window[0, 1:17]) > 3000


# ---- 3. zeros and refusals ------------------------------------------------------------------------------------------------------------------
def test_records_that_contribute_nothing_give_exact_zeros():
    c, hits, n_hits, met, dk = setup("mid")
    r_min, r_max, delay, emis = tables = make_tables("mid")
    nodes = r_min + np.arange(37) * (r_max - r_min) / 36
    changes = dict(g_nan=(2, np.nan), g_zero=(2, 0.0), g_negative=(2, -0.7), dt_nan=(3, np.nan), r_nan=(0, np.nan),
                   r_below=(0, np.nextafter(np.float32(r_min), np.float32(0))), r_above=(0, np.nextafter(np.float32(r_max), np.float32(1e9))),
                   dark_stretch=(0, 0.5 * (nodes[10] + nodes[12])), nan_delay=(0, 0.5 * (nodes[29] + nodes[31])))
    for n_tau, n_bins, split in ((64, 96, True), (126, 254, False)):
        spec, grid = grids(n_tau, n_bins, split)
        lit = transfer(hits, n_hits, met, dk, spec, grid, tables)
        assert np.count_nonzero(lit) > 5000 and np.all(lit[lit != 0] > 0) and not np.any(np.signbit(lit))   # an empty key is +0.0
        for what, (column, value) in changes.items():
            h = hits.copy()
            h[..., column] = np.float32(value)
            for counts in (n_hits, None):
                out = transfer(h, counts, met, dk, spec, grid, tables)
                assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out)), what
        for counts in (np.zeros_like(n_hits), None, n_hits):
            out = transfer(np.full_like(hits, np.nan), counts, met, dk, spec, grid, tables)
            assert np.all(out == 0.0) and not np.any(np.signbit(out))
        dark = ltrace.default_disk(r_out=c.r_out, exposure=0.0)           # every weight exactly 0: not added
        out = transfer(hits, n_hits, met, dark, spec, grid, tables)
        assert np.all(out == 0.0) and not np.any(np.signbit(out))
    # the table's ends themselves contribute: r_min and r_max as float32 compare equal to the doubles
    spec, grid = grids(64, 96)
    for end in (2.5, 17.0):
        h = hits.copy()
        h[..., 0] = np.float32(end)
        flat = (2.5, 17.0, np.array([3.0, 4.0, 5.0]), np.array([1.0, 2.0, 1.0]))
        assert transfer(h, n_hits, met, dk, spec, grid, flat, t_ref=0.0).sum() > 0


def test_refusals_in_their_order():
    c, hits, n_hits, met, dk = setup("strip")
    r_min, r_max, delay, emis = make_tables("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    tr = lambda **kw: ltrace.default_transfer(**{**dict(tau_min=TAU_LO, tau_max=TAU_HI, n_tau=8, n_r=37, r_min=r_min, r_max=r_max, t_ref=T_REF), **kw})
    sp = lambda **kw: ltrace.default_spectrum(**{**dict(g_min=G_LO, g_max=G_HI, n_bins=16), **kw})

    def call(form, hits_=hits, met_=met, disk_=dk, spec_=sp(), tr_=tr(), delay_=delay, emis_=emis, R=c.R, W=c.W, m=c.m, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full(40000, -7.0)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        fn = lib.lt_disk_transfer if form == "host" else lib.lt_disk_transfer_dev
        rc = fn(ptr(hits_), ptr(n_hits), R, W, m, ref_(met_), ref_(disk_), ref_(spec_), ref_(tr_), ptr(delay_), ptr(emis_), None if null_out else ptr(out))
        if rc != ltrace.OK:
            assert np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    nan, inf = float("nan"), float("inf")
    INV = ltrace.ERR_INVALID_ARG
    order = [(dict(hits_=None), INV, "null"), (dict(met_=None), INV, "null"), (dict(disk_=None), INV, "null"),
             (dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"), (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), INV, "bad metric"),
             (dict(R=0), INV, "empty frame"), (dict(W=-3), INV, "empty frame"), (dict(m=0), INV, "max_images"), (dict(m=9), INV, "max_images"),
             (dict(disk_=ltrace.default_disk(q=nan)), INV, "disk q"), (dict(disk_=ltrace.default_disk(exposure=-1.0)), INV, "disk q"),
             (dict(spec_="null"), INV, "null spec"), (dict(spec_=sp(g_min=0.0)), INV, "g_min"), (dict(spec_=sp(g_max=inf)), INV, "g_min"),
             (dict(spec_=sp(n_bins=0)), INV, "n_bins"), (dict(spec_=sp(n_bins=513)), INV, "n_bins"),
             (dict(tr_="null"), INV, "null transfer"), (dict(tr_=tr(tau_min=nan)), INV, "tau_min"), (dict(tr_=tr(tau_max=TAU_LO)), INV, "tau_min"),
             (dict(tr_=tr(tau_max=inf)), INV, "tau_min"), (dict(tr_=tr(n_tau=0)), INV, "n_tau"), (dict(tr_=tr(n_tau=1025)), INV, "n_tau"),
             (dict(tr_=tr(n_r=1)), INV, "n_r"), (dict(tr_=tr(n_r=65537)), INV, "n_r"), (dict(tr_=tr(r_min=0.0)), INV, "r_min"),
             (dict(tr_=tr(r_max=r_min)), INV, "r_min"), (dict(tr_=tr(r_max=inf)), INV, "r_min"), (dict(tr_=tr(t_ref=nan)), INV, "t_ref"),
             (dict(tr_=tr(t_ref=-inf)), INV, "t_ref"), (dict(delay_=None), INV, "null delay"), (dict(emis_=None), INV, "null delay"),
             (dict(spec_=sp(n_bins=510), tr_=tr(n_tau=63)), INV, "keys"), (dict(null_out=True), INV, "null out")]
    fields = [(tr(tau_min=nan, n_tau=0), "tau_min"), (tr(n_tau=0, n_r=1), "n_tau"), (tr(n_r=1, r_min=0.0), "n_r"), (tr(r_min=0.0, t_ref=nan), "r_min")]
    for form in ("host", "dev"):
        if form == "host":
            assert call(form)[0] == ltrace.OK and call(form, spec_=sp(n_bins=510), tr_=tr(n_tau=62))[0] == ltrace.OK      # 64 x 512: the cap itself
            assert call(form, tr_=tr(tau_min=-300.0, tau_max=-100.0))[0] == ltrace.OK                                    # a grid below zero
        for bad, text in fields:                                          # the struct's refusals in the header's order
            rc, msg = call(form, tr_=bad)
            assert rc == INV and text in msg, (form, text, rc, msg)
        for i, (kw, code, text) in enumerate(order):
            rc, msg = call(form, **kw)
            assert rc == code and text in msg, (form, kw, rc, msg)
            for later, _, _ in order[i + 1:]:                             # an earlier fault wins over every later one
                if set(later) & set(kw):
                    continue
                rc2, msg2 = call(form, **{**later, **kw})
                assert rc2 == code and text in msg2, (form, kw, later, rc2, msg2)
    with pytest.raises(ltrace.LtraceError):                    # the binding sizes no output for a grid beyond the cap
        transfer(hits, n_hits, met, dk, diskmod.Spectrum(G_LO, G_HI, 510), diskmod.TransferGrid(0.0, 64.0, 63), make_tables("strip"))


# ---- 4. the traced frame ----------------------------------------------------------------------------------------------------------------------
def test_the_traced_frame_through_render_sequence():
    import image_lens
    from metrics import Kerr
    from test_gpu_diskmap import SEQ
    M, a = SEQ["M"], SEQ["a"]
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"], exposure=EXPOSURE)
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
    lamp = diskmod.Lamppost(M, a, 6.0, n_r=64, n_rays=32)
    grid, spec = diskmod.TransferGrid(-8.0, 120.0, 32), diskmod.Spectrum(0.1, 1.7, 64, split_orders=True)
    out = image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk, diskmod.HotSpot(), [0.0],
                                     shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], spectrum=spec, lamppost=lamp, transfer=grid)
    hits, n_hits, tf = out["hits"], out["n_hits"], out["transfer"]
    nodes, delay, emis = out["transfer_tables"]
    t_ref = out["transfer_t_ref"]
    assert tf.shape == (3, 34, 66) and int((n_hits > 0).sum()) > 1000 and np.array_equal(out["transfer_tau_edges"], grid.edges())
    assert nodes[0] == float(diskmod.isco(M, a)) and abs(nodes[-1] - SEQ["r_out"]) < 1e-12 and np.all(emis > 0) and np.all(np.isfinite(delay))
    lt = grid.to_lt(nodes[0], SEQ["r_out"], 64, t_ref)
    assert tf.tobytes() == ltrace.disk_transfer(hits, n_hits, met, dk, spec.to_lt(), lt, delay, emis).tobytes()
    # summed over the delays it is the line of the same emissivity, from the restatement's weights binned by g alone
    slots = restate_slots(hits, n_hits, EXPOSURE, nodes[0], SEQ["r_out"], delay, emis, t_ref)
    check(tf, slots, spec, grid, "traced frame")
    on, tau, g, weight = slots
    line, n = np.zeros((3, 66), dtype=LD), np.zeros((3, 66), dtype=np.int64)
    plane = np.broadcast_to(np.arange(3), on.shape)[on]
    np.add.at(line, (plane, bin_ref(g[on], 0.1, 1.7, 64)), weight[on])
    np.add.at(n, (plane, bin_ref(g[on], 0.1, 1.7, 64)), 1)
    got = diskmod.reverberation_line(tf)
    assert got.shape == (3, 66) and np.all(np.abs(got.astype(LD) - line) <= (n + 6 + 34) * U * line) and np.count_nonzero(line) > 60
    # nothing arrives before the geometric minimum: the soonest the source lights any radius of the table, then the straight
    # way from the disk's outer edge to the camera (curvature only delays), against the direct flash
    soonest = float(delay.min()) + (SEQ["r_obs"] - SEQ["r_out"]) - t_ref
    assert all(on[..., j].any() for j in range(3))                       # every image order has hits on the table
    first = [int(np.flatnonzero(diskmod.impulse_response(tf)[j])[0]) for j in range(3)]
    edges = np.concatenate([[-np.inf], grid.edges()])                     # the lower edge of every row
    print(f"traced frame: t_ref {t_ref:.3f}, geometric minimum {soonest:.2f}; the orders' responses start in rows {first}, at tau >= {edges[first].tolist()}; "
          f"earliest delay {float(tau[on].min()):.2f}")
    assert tau[on].min() >= soonest and all(edges[k + 1] > soonest for k in first)
    assert tf[:, 0].sum() == 0.0                                          # and nothing before the flash itself by more than two bins
    assert first[2] > first[0] and first[1] >= first[0]                   # the higher orders' echoes start later
