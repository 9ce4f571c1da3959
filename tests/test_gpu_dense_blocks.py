"""Every step of a dense-track record (lt_integrate_dense: k_dense_tracks, lt_dense.hpp) held to a bound from the reference.

A record holds every accepted point, so each y_{p+1} is compared with ONE longdouble Dormand-Prince step from the device's own
float64 y_p (tests/dense_blocks.py: the replay, the units, the classes), and the controller with the reference's accept / reject
loop run in longdouble at the device's state: no new device code, no chaos.  tests/test_dense_blocks_host.py derives every K on the
CPU from the float64 oracle and the longdouble restatement alone; the device is held to 2 K.

  (a) the 8-D right-hand side (lt_rhs8_probe) per component in its unit, both metric kinds, six classes, and its bit-level rows;
  (b) every accepted step of seeded batches, class by class, cyclic momenta bit-constant;
  (c) the controller: every step size against the replay's, the clamp at max_step and min(1, factor) visible, attempts = (nfev - 2) / 6;
  (d) the start: the first step against Hairer's rule in longdouble; a one-step track;
  (e) the terminal event: order, ye against the longdouble dense output, the root's residual;
  (f) ends and edges: the attempt limit, a start inside r_zero, starts on an event radius, NaN, truncated records in both launch orders
      with a sentinel in every slot the kernel must not touch.

With LT_DENSE_BLOCKS_MEASURE=path the figures the tests print are also written there as JSON (profiles/dense_blocks_<build id>.json).
Run time on the MI355X: 6.3 s for the whole file, 42 tests; the slowest case 1.75 s (a seeded batch: 1.2 to 1.9 ms on the device
for 128 tracks and 4.7 MB of records, the rest the longdouble replay on the host); the profile's `seconds` entries hold each batch's.

MEASURED (build 5d941ec30311; profiles/dense_blocks_5d941ec30311.json): right-hand side at most 10.9 units in the
pole class (bound 42; 29.0 in the Schwarzschild kind with the floor acting), 9.2 far (16), 8.8 near the horizon (68), 4.1 on the equator
(6); every accepted step at most 1.33 units in the seeded batches (bound 4) and 5.83 in the sharp ones (bound 10); step sizes at most
0.074 (seeded) and 0.45 (sharp) of their allowance; ye 2.86 units, the root's residual 0.23 (bound 6).  Before the kernel took the
candidate's own sincos, the carried pair's drift put near-axis steps at 151 (a = 0.9), 323 (0.998) and 40 (1.0) units in p_theta.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import dense_blocks as db
import hipmini
import ltrace
from oracle import oracle

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_DENSE_BLOCKS_MEASURE")
_RECORD = {}
MP = 512
BATCHES = [(k, a, False) for k, a in db.SPINS] + [(0, 0.0, True), (1, 0.9, True)]
_IDS = [f"kind{k}_a{a}_{'sharp' if s else 'seeded'}" for k, a, s in BATCHES]


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


def metric_of(kind, a):
    return ltrace.Metric(ltrace.METRIC_KERR if kind else ltrace.METRIC_SCHWARZSCHILD, 0, db.M, float(a))


# ---- (a) the right-hand side --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", db.RHS_CLASSES)
def test_rhs8_in_its_unit(name):
    worst = np.zeros(6)
    for kind, a in db.RHS_SPINS:
        st = db.rhs_class(name, kind, a)
        got = ltrace.rhs8_probe(metric_of(kind, a), st)
        ratio = db.rhs_ratio(kind, a, st, got)[:, list(db.NONCYCLIC)]
        assert np.isfinite(got).all(), (kind, a)
        assert (got[:, [4, 7]] == 0).all() and not np.signbit(got[:, [4, 7]]).any(), "the cyclic components are +0.0"
        m = ratio.max(axis=0)
        print(f"device right-hand side, kind {kind} a = {a:5}, {name:12s}: {np.round(m, 2)} units (bound {2 * db.K_RHS8[name]})")
        worst = np.maximum(worst, m)
        assert (ratio <= 2 * db.K_RHS8[name]).all(), (kind, a, m)
    record(f"rhs8/{name}", dict(worst_units=worst.tolist(), bound=2 * db.K_RHS8[name]))


def test_rhs8_bit_level_rows():
    for kind, a in db.RHS_SPINS:
        met = metric_of(kind, a)
        rz = db.r_zero(a if kind else 0.0)
        st = db.rhs_class("far", kind, a, 130)
        st[:, 1] = np.linspace(0.3 * rz, rz, 130)
        st[-1, 1], st[-2, 1] = rz, np.nextafter(rz, 0)
        got = ltrace.rhs8_probe(met, st)
        assert (got == 0).all() and not np.signbit(got).any(), "r <= r_zero, r_zero itself included: eight zeros"
        st[:, 1] = np.nextafter(rz, np.inf)
        assert (ltrace.rhs8_probe(met, st)[:, 1:3] != 0).all()
        if kind:
            st = db.rhs_class("far", kind, a, 130)
            st[:, 2] = 0.0
            got, ref = ltrace.rhs8_probe(met, st), oracle.rhs8_n(kind, db.M, a, st)
            # every component that is non-finite in the oracle is non-finite on the device (phi', p_r', p_theta'), the cyclic ones
            # are +0.0 in both; the device's merged reciprocal makes t', r' and theta' non-finite as well, which no track can show:
            # the attempt's error norm is NaN either way (test_ends_nan_start)
            assert not np.isfinite(got[:, [3, 5, 6]]).any() and not np.isfinite(ref[:, [3, 5, 6]]).any()
            assert (got[:, [4, 7]] == 0).all() and (ref[:, [4, 7]] == 0).all()


# ---- (b) - (e): seeded batches, replayed once -----------------------------------------------------------------------------------------
_CACHE = {}


def _opts(sharp, **kw):
    o = dict(max_points=MP)
    if sharp:
        o.update(lambda_max=db.SHARP_LAMBDA_MAX, **db.SHARP_TOL)
    o.update(kw)
    return ltrace.default_dense_opts(**o)


def _batch(kind, a, sharp):
    key = (kind, a, sharp)
    if key not in _CACHE:
        s0 = db.sharp_turn_states(kind, a) if sharp else db.seeded_states(kind, a)
        kw = dict(lambda_max=db.SHARP_LAMBDA_MAX, **db.SHARP_TOL) if sharp else {}
        t0 = time.perf_counter()
        t, y, count, status, nfev = ltrace.integrate_dense(metric_of(kind, a), s0, _opts(sharp))
        t1 = time.perf_counter()
        fits = count < MP  # (room for the t_new slot; a near-critical track may orbit for longer)
        assert fits.mean() >= 0.98
        rec = tuple(x[fits] for x in (t, y, count, status, nfev))
        rp = db.replay(kind, a, *rec, k_att=2 * db.K_ATT["sharp" if sharp else "seeded"], k_err=2 * db.K_ERR, **kw)
        ev = db.event_check(kind, a, *rec[:4], **{k: v for k, v in kw.items()})
        t2 = time.perf_counter()
        _CACHE[key] = dict(s0=s0[fits], rec=rec, rp=rp, ev=ev, kw=kw, cl=db.classify(rp["blk"], rp["Y0"], rp["Y1"]),
                           seconds=dict(device_call=t1 - t0, host_replay=t2 - t1))
    return _CACHE[key]


@pytest.mark.parametrize("kind,a,sharp", BATCHES, ids=_IDS)
def test_every_accepted_step(kind, a, sharp):
    b = _batch(kind, a, sharp)
    rp, cl = b["rp"], b["cl"]
    k_att = 2 * db.K_ATT["sharp" if sharp else "seeded"]
    keep, ratio = rp["keep"], rp["ratio"][:, list(db.NONCYCLIC)]
    reg = ~rp["is_event"]
    fig = dict(steps=int(keep.sum()), left_out=int((~keep[reg]).sum()), bound=k_att, seconds=b["seconds"], classes={})
    for name, rows in cl.items():
        sel = rows & keep
        m = ratio[sel].max(axis=0) if sel.any() else np.zeros(6)
        fig["classes"][name] = dict(rows=int(sel.sum()), worst_units=m.tolist())
        print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'} {name:8s}: {int(sel.sum()):6d} steps, worst per component {np.round(m, 2)} (bound {k_att})")
    i = int(np.argmax(np.where(keep, ratio.max(axis=1), 0)))
    fig["worst_row"] = dict(y=rp["Y0"][i].tolist(), h=float(rp["h"][i]), units=ratio[i].tolist())
    print(f"    worst row: y {rp['Y0'][i].tolist()} h {rp['h'][i]!r}: {np.round(ratio[i], 2)}; {b['seconds']}")
    record(f"steps/{_IDS[BATCHES.index((kind, a, sharp))]}", fig)
    assert (~keep[reg]).mean() <= db.EXCLUDED_CAP
    assert rp["cyclic_ok"].all(), "p_t and p_phi are bit-constant along a record"
    assert rp["accept_ok"].all(), "a recorded step the longdouble loop rejects"
    # every class is populated where it exists: the sharp class in the batches built for it, the polar ones in the Kerr batches
    need = ("sharp", "axis", "equator", "turning") if sharp else ("far", "turning") + (("equator", "axis") if kind else ())
    for name in need:
        assert fig["classes"][name]["rows"] >= 16, name
    assert (ratio[keep] <= k_att).all(), fig["worst_row"]


@pytest.mark.parametrize("kind,a,sharp", BATCHES, ids=_IDS)
def test_the_controller(kind, a, sharp):
    b = _batch(kind, a, sharp)
    rp = b["rp"]
    key = "sharp" if sharp else "seeded"
    allow = rp["h_allow"] + 2 * db.K_H0 * rp["unit_h0"]
    hk = rp["h_keep"]
    d = np.abs(rp["h"] - rp["h_replay"])
    later = hk & (rp["p"] > 0)
    known = rp["attempts_known"]
    v = db.verdict(rp, 2 * db.K_ATT[key], 2 * db.K_H0)
    fig = dict(held=int(hk.sum()), rows=int(hk.size), worst_of_allowance=float((d / allow)[later].max()), clamped=int((rp["clamped"] & hk).sum()),
               after_rejection=int((rp["rejected"] & hk).sum()), capped_at_1=int((rp["capped"] & hk).sum()),
               attempts=int(rp["attempts_sum"][known].sum()), tracks_known=int(known.sum()), tracks=int(known.size), verdict=v)
    print(f"kind {kind} a = {a:5} {key}: {fig}")
    record(f"controller/{_IDS[BATCHES.index((kind, a, sharp))]}", fig)
    assert (~hk).mean() <= db.EXCLUDED_CAP
    assert (d[later] <= allow[later]).all(), "a step size that is not the reference's loop's"
    if not sharp:
        # both kinds of steps exist, and are held: clamped at max_step (the device's h is then t + 1 - t), min(1, factor) after a rejection
        assert fig["clamped"] > 1000 and fig["capped_at_1"] > 100
        c = rp["clamped"] & hk & (rp["attempts"] == 1) & ~rp["is_event"]
        assert (rp["h"][c] == (rp["t0"][c] + db.MAX_STEP) - rp["t0"][c]).all()
        assert known.all()
    else:
        assert known.mean() >= 0.9
    assert (rp["attempts_sum"] == rp["attempts_nfev"])[known].all(), "attempts summed over a track are not (nfev - 2) / 6"


@pytest.mark.parametrize("kind,a,sharp", BATCHES, ids=_IDS)
def test_the_start(kind, a, sharp):
    b = _batch(kind, a, sharp)
    rp = b["rp"]
    fi = rp["first"]
    allow = rp["h_allow"][fi] + 2 * db.K_H0 * rp["unit_h0"][fi]
    d = np.abs(rp["h"][fi] - rp["h_replay"][fi])
    ok = rp["h_keep"][fi]
    print(f"kind {kind} a = {a:5}: first step {rp['h'][fi].min():.3e} ... {rp['h'][fi].max():.3e}, worst {np.max((d / allow)[ok]):.3f} of the allowance "
          f"(2 K_H0 = {2 * db.K_H0} units of the initial step), {int(ok.sum())} of {ok.size} held")
    record(f"start/{_IDS[BATCHES.index((kind, a, sharp))]}", dict(worst_of_allowance=float(np.max((d / allow)[ok])), held=int(ok.sum())))
    assert (~ok).mean() <= db.EXCLUDED_CAP and (d[ok] <= allow[ok]).all()


def test_one_step_track():
    """lambda_max below the initial step: one clipped step, the final t equal to lambda_max bit for bit, nfev = 8."""
    for kind, a in db.SPINS:
        s0 = db.seeded_states(kind, a, 70)
        lam = 1e-3
        t, y, count, status, nfev = ltrace.integrate_dense(metric_of(kind, a), s0, ltrace.default_dense_opts(max_points=8, lambda_max=lam))
        assert (count == 2).all() and (status == 0).all() and (nfev == 8).all()
        assert (t[:, 0] == 0).all() and (t[:, 1] == lam).all()
        rec = db.oracle_records(kind, a, s0, max_points=8, lambda_max=lam)
        assert np.array_equal(rec[2], count) and np.array_equal(rec[3], status) and np.array_equal(rec[4], nfev)
        rp = db.replay(kind, a, t, y, count, status, nfev, k_att=2 * db.K_ATT["seeded"], k_err=2 * db.K_ERR, lambda_max=lam)
        assert db.verdict(rp, 2 * db.K_ATT["seeded"], 2 * db.K_H0) == dict(steps=0, sizes=0, cyclic=0, accepts=0, attempts=0)
        assert rp["attempts_known"].all() and (rp["h_replay"] == lam).all()


@pytest.mark.parametrize("kind,a,sharp", BATCHES, ids=_IDS)
def test_the_event(kind, a, sharp):
    b = _batch(kind, a, sharp)
    ev, rp = b["ev"], b["rp"]
    keep = ev["keep"]
    k = 2 * db.K_EVENT
    ratio = ev["ratio_ye"][:, list(db.NONCYCLIC)]
    root = ev["resid"] / ev["unit_root"]
    # the tracks whose final step was clipped by max_step
    clipped = ev["h"] == (ev["t_last"] + db.MAX_STEP) - ev["t_last"]
    fig = dict(events=int(keep.sum()), capture=int((ev["status"][keep] == 1).sum()), escape=int((ev["status"][keep] == 2).sum()),
               final_step_at_max_step=int((clipped & keep).sum()), ye_worst_units=ratio[keep].max(axis=0).tolist(),
               root_worst_units=float(root[keep].max()), bound=k)
    print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: {fig}")
    record(f"event/{_IDS[BATCHES.index((kind, a, sharp))]}", fig)
    assert ev["ordered"].all(), "t_last < te <= t_new"
    assert ev["cyclic_ok"].all()
    if not sharp:
        assert (~keep).mean() <= db.EXCLUDED_CAP
        assert fig["capture"] >= 16 and fig["escape"] >= 16 and fig["final_step_at_max_step"] >= 16
    else:
        assert fig["events"] >= 16
    assert (ratio[keep] <= k).all() and (root[keep] <= k).all()
    # the event step's size is the controller's (its row of the replay): held in test_the_controller; here: it is a row
    assert (rp["is_event"].sum() == ev["track"].size)


# ---- (f) ends and edges ------------------------------------------------------------------------------------------------------------
def _same_as_oracle(kind, a, s0, dev, **kw):
    rec = db.oracle_records(kind, a, s0, max_points=dev[0].shape[1], **kw)
    assert np.array_equal(rec[2], dev[2]) and np.array_equal(rec[3], dev[3]) and np.array_equal(rec[4], dev[4]), (rec[2:], dev[2:])
    return rec


def test_ends_attempt_limit():
    """max_attempts = 5: status -2 after five attempts (nfev = 2 + 6 x 5), and the points before it are those of the full record."""
    for kind, a in db.SPINS:
        b = _batch(kind, a, False)
        s0 = b["s0"][:70]
        t, y, count, status, nfev = ltrace.integrate_dense(metric_of(kind, a), s0, ltrace.default_dense_opts(max_points=16, max_attempts=5))
        assert (status == -2).all() and (nfev == 32).all()
        ft, fy, fcount = b["rec"][0][:70], b["rec"][1][:70], b["rec"][2][:70]
        rp = b["rp"]
        for i in range(70):
            m = int(count[i])
            att = rp["attempts"][rp["track"] == i]
            expect = 1 + int(np.searchsorted(np.cumsum(att), 5, side="right"))  # the accepted steps the first five attempts hold
            if rp["attempts_known"][i]:
                assert m == expect, (i, m, expect)
            assert 1 <= m <= 6
            assert np.array_equal(t[i, :m], ft[i, :m]) and np.array_equal(y[i, :m], fy[i, :m])


def test_ends_start_inside_r_zero():
    """A zero right-hand side: the step grows by 10 to max_step and walks to lambda_max with a constant state, status 0."""
    for kind, a in db.SPINS:
        aa = a if kind else 0.0
        s0 = db.seeded_states(kind, a, 3)
        s0[:, 1] = [0.5 * db.r_zero(aa), np.nextafter(db.r_zero(aa), 0), db.r_zero(aa)]
        dev = ltrace.integrate_dense(metric_of(kind, a), s0, ltrace.default_dense_opts(max_points=32, lambda_max=7.5))
        rec = _same_as_oracle(kind, a, s0, dev, lambda_max=7.5)
        t, y, count, status, nfev = dev
        assert (status == 0).all() and (count < 32).all()
        for i in range(3):
            m = count[i]
            assert np.array_equal(t[i, :m], rec[0][i, :m]) and t[i, m - 1] == 7.5
            assert (y[i, :m, 1:] == s0[i, 1:]).all()
            h = np.diff(t[i, :m])
            assert h[0] == 1e-6 and (np.abs(h[7:-1] - 1.0) < 1e-15).all()


def test_ends_start_on_an_event_radius():
    """A start exactly on r_in moving in, and exactly on r_out moving out: the event lies in the first step at te = 0."""
    for kind, a in db.SPINS:
        aa = a if kind else 0.0
        s0 = db.seeded_states(kind, a, 4)
        s0[:2, 1] = db.r_capture(aa)
        s0[:2, 5] = -np.abs(s0[:2, 5])
        s0[2:, 1] = 20.0
        s0[2:, 5] = 0.8
        o = ltrace.default_dense_opts(max_points=8, r_stop_outer=20.0)
        dev = ltrace.integrate_dense(metric_of(kind, a), s0, o)
        _same_as_oracle(kind, a, s0, dev, r_out=20.0)
        t, y, count, status, nfev = dev
        assert (count == 2).all() and status.tolist() == [1, 1, 2, 2]
        assert (t[:, 1] == 0.0).all() and np.array_equal(y[:, 1], s0) and (t[:, 2] > 0).all()


def _dev_run(kind, a, s0, sentinel=-7.25, **kw):
    """lt_integrate_dense_dev on raw device buffers filled with a sentinel beforehand -> (t, y, count, status, nfev) host arrays."""
    n = s0.shape[0]
    o = ltrace.default_dense_opts(**kw)
    mp = int(o.max_points)
    hip = hipmini.hip()
    bufs = [hipmini.DeviceArray((n, 8), np.float64), hipmini.DeviceArray((n, mp), np.float64), hipmini.DeviceArray((n, mp, 8), np.float64),
            hipmini.DeviceArray((n,), np.int32), hipmini.DeviceArray((n,), np.int8), hipmini.DeviceArray((n,), np.int32)]
    fills = [np.ascontiguousarray(s0, dtype=np.float64), np.full((n, mp), sentinel), np.full((n, mp, 8), sentinel),
             np.full(n, -99, dtype=np.int32), np.full(n, -99, dtype=np.int8), np.full(n, -99, dtype=np.int32)]
    for b, f in zip(bufs, fills):
        assert hip.hipMemcpy(C.c_void_p(b.ptr), C.c_void_p(f.ctypes.data), f.nbytes, 1) == 0  # 1 = hipMemcpyHostToDevice
    ltrace.integrate_dense_dev(metric_of(kind, a), o, bufs[0].ptr, n, *(b.ptr for b in bufs[1:]))
    hipmini.device_synchronize()
    return tuple(b.get() for b in bufs[1:])


def _untouched(t, y, count, status, sentinel=-7.25):
    """No slot outside a track's own record range changed: live points, and the t_new slot of an event record with room."""
    n, mp = t.shape
    live = np.arange(mp)[None, :] < np.minimum(count, mp)[:, None]
    t_own = live | ((np.arange(mp)[None, :] == count[:, None]) & (status > 0)[:, None])
    return (t[~t_own] == sentinel).all() and (y[~live] == sentinel).all()


def test_ends_nan_start():
    """A NaN in the start state: status -1 (the step size underflows on NaN error norms), finite bookkeeping equal to the oracle's,
    one point, and no slot outside the record written.  The same for sin theta = 0 in the Kerr kind (a non-finite right-hand side)."""
    for kind, a in db.SPINS[:2]:
        s0 = db.seeded_states(kind, a, 66)
        s0[::3, 5] = np.nan
        s0[1::3, 1] = np.nan
        if kind:
            s0[2::3, 2] = 0.0
        dev = _dev_run(kind, a, s0, max_points=8, length_binning=-1)
        t, y, count, status, nfev = dev
        rec = db.oracle_records(kind, a, s0, max_points=8)
        bad = ~np.isfinite(oracle.rhs8_n(kind, db.M, a, s0)).all(axis=1) | ~np.isfinite(s0).all(axis=1)
        assert bad.sum() >= 44
        assert (status[bad] == -1).all() and (count[bad] == 1).all()
        assert np.array_equal(rec[2], count) and np.array_equal(rec[3], status) and np.array_equal(rec[4], nfev)
        assert _untouched(t, y, count, status)
        assert (t[bad, 0] == 0).all() and np.array_equal(y[bad, 0], s0[bad], equal_nan=True)


@pytest.mark.parametrize("mp", [2, 3, 8, 9, 10, 17])
def test_ends_truncated_records_in_both_launch_orders(mp):
    """130 tracks, ragged in the last wavefront, max_points around the t-ring's length of eight: the caller-order launch (ring off)
    and the length-binned one (ring on) write the same bytes -- counts, endings, nfev, every live t and y, the last slot's final point,
    the t_new slot -- and nothing else; the first max_points - 1 points are those of the untruncated record."""
    kind, a = 1, 0.9
    s0 = db.seeded_states(kind, a, 130, seed=3)
    # short records too (2, 2, 3, 5, 7, 9, 12, 19 points): some end within max_points, where the t_new slot is written
    s0[:8, 1] = db.r_capture(a) * (1 + np.array([1e-7, 1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2]))
    s0[:8, 5] = -1.0
    full = ltrace.integrate_dense(metric_of(kind, a), s0, ltrace.default_dense_opts(max_points=MP, length_binning=-1))
    plain = _dev_run(kind, a, s0, max_points=mp, length_binning=-1)
    binned = _dev_run(kind, a, s0, max_points=mp, length_binning=1)
    for name, x, z in zip(("t", "y", "count", "status", "nfev"), plain, binned):
        assert np.array_equal(x.view(np.uint8), z.view(np.uint8)), name
    t, y, count, status, nfev = binned
    assert np.array_equal(count, full[2]) and np.array_equal(status, full[3]) and np.array_equal(nfev, full[4])
    assert (count > mp).sum() >= 100 and (count == mp).sum() + (count < mp).sum() >= 2 and count[:8].tolist() == [2, 2, 3, 5, 7, 9, 12, 19]
    for dev in (plain, binned):
        assert _untouched(dev[0], dev[1], count, status)
    for i in range(130):
        c = int(count[i])
        m = min(c, mp)
        k = m if c <= mp else mp - 1
        assert np.array_equal(t[i, :k], full[0][i, :k]) and np.array_equal(y[i, :k], full[1][i, :k]), i
        assert t[i, m - 1] == full[0][i, c - 1] and np.array_equal(y[i, m - 1], full[1][i, c - 1]), "the last slot holds the final point"
        if status[i] > 0 and c < mp:
            assert t[i, c] == full[0][i, c], "the t_new slot"
