"""One attempt of the float64 Dormand-Prince 4(5) integrator (csrc/lt_dp45.hpp) and the loop body around it, block by block,
against the same statements in longdouble and against the oracle's own attempt -- in the units of tests/dp45_blocks.py, with
the bounds tests/test_dp45_blocks_host.py derives on the CPU (K_ATT64, K_ERR64; the device forms are held to twice them),
the float32 controller's z^(-1/10) over every float32 of its domain, and what must hold in every bit: the two forms of the
attempt, the per-lane selection in advance(), advance() against the attempt probe, N attempts in one launch against N
launches of one.

Whole DP45 rays stay under the statistics of test_gpu_parity.py; this file says which operation is wrong.

The step-size controller is a member function that advance() calls and lt_dp45_controller_probe calls on any err_sq
(test_controller_against_the_reference_expressions).  It is also reached through advance(): with states at or inside r_cut,
whose right-hand side is zero, and a carried k1 that has only a dphi component the error norm is |h E1 k1 / sc| / sqrt(5)
whatever the test wants it to be, up to 6e3 (test_controller_through_advance); a non-finite err_sq with a usable candidate by
a candidate that lands within 1e-7 rad of the axis (test_decision_table).

MEASURED on the MI355X: profiles/dp45_blocks_<build id>.json (LT_DP45_BLOCKS_MEASURE=path writes it), DESIGN.md 2.1.
"""
import json
import os

import mpmath
import numpy as np
import pytest

import dp45_blocks as db
import ltrace
import step_blocks as sb
from oracle import oracle

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_DP45_BLOCKS_MEASURE")  # a path: the figures the tests print are also written there as JSON
N = db.N
_RECORD = {}
EV_RUNNING, EV_MAXRANGE, EV_INVALID, EV_CAPTURED, EV_ESCAPED = 4, 2, 0, -1, 1


def _plain(v):
    """For strict JSON: numpy scalars as Python's, a value that is not finite as a string."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, (float, np.floating)):
        return float(v) if np.isfinite(v) else str(float(v))
    if isinstance(v, np.integer):
        return int(v)
    return v


def record(key, value):
    _RECORD[key] = _plain(value)
    if MEASURE:
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, allow_nan=False)


def same_bits(x, y):
    """Elementwise: two float64 arrays have the same bit pattern (a NaN equals a NaN)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def bits32(x):
    return int(np.float32(x).view(np.uint32))


def attempt(a, st, L, h, refine, exact, checked, **kw):
    return ltrace.dp45_attempt_probe(sb.M, a, st, L, h, refine, exact=exact, checked=checked, r_obs=db.R_OBS, lambda_max=1e9, **kw)


def advance(a, st, L, h, refine, exact, r_obs=db.R_OBS, lambda_max=1e9, **kw):
    return ltrace.dp45_advance_probe(sb.M, a, st, L, h, refine, exact=exact, r_obs=r_obs, lambda_max=lambda_max, **kw)


def valid(a, out):
    """The validity test of the branch-free attempt, with the r_cut the kernels use."""
    return (out["min_r"] > sb.r_plus(a) * 1.001) & (out["max_d"] <= 0.25)


def kinds(name):
    return ("accepted", "rejected") + (("first",) if name in db.CHECKED_CLASSES else ())


ATTEMPT_KEYS = ("next", "k7", "sc", "err_sq")


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the float32 controller's power
# ---------------------------------------------------------------------------------------------------------------------------
def test_pow_minus_tenth_every_value():
    """pow_minus_tenth on every float32 of [1e-30, 1e30] against the float64 pow on the device: relative error within
    POW_TENTH_REL = 2.5e-7 (lt_dp45.hpp's `~2e-7`, and the 2.08e-7 its statements give in numpy), every result positive and
    finite.  Outside the domain it is recorded, not bounded: test_controller_through_advance and test_decision_table show
    that none of it reaches h; test_controller_against_the_reference_expressions hands the controller every such err_sq."""
    lo, hi = bits32(1e-30), bits32(1e30)
    total, worst, at, bad, first_bad = 0, 0.0, None, 0, None
    b = lo
    while b <= hi:
        e = min(hi, b + (1 << 30) - 1)
        r = ltrace.math32_probe("pow_minus_tenth", b, e)
        assert r["compared"] == e - b + 1
        total += r["compared"]
        bad += r["differing"]
        if first_bad is None:
            first_bad = r["first_differing"]
        if r["abs_sin"][0] > worst:
            worst, at = r["abs_sin"]
        b = e + 1
    z = None if at is None else float(np.uint32(at).view(np.float32))
    special = np.array([0.0, 1e-45, 1.1754944e-38, 3.4028235e38, np.inf, np.nan])
    out = ltrace.math64_probe("pow_minus_tenth_f32", special)[:, 0]
    print(f"pow_minus_tenth, {total} values in [1e-30, 1e30]: max relative error {worst:.4e} at z = {z!r}; {bad} results not positive "
          f"and finite; at 0, the smallest denormal, FLT_MIN, FLT_MAX, +inf, NaN: {out.tolist()}")
    record("pow_minus_tenth", dict(compared=total, max_rel=worst, at=z, not_positive_finite=bad, first=first_bad,
                                   special=dict(zip(("0", "denormal", "FLT_MIN", "FLT_MAX", "inf", "nan"), out.tolist()))))
    assert total == hi - lo + 1
    assert bad == 0, f"first at bits {first_bad:#x}"
    assert 0 < worst <= db.POW_TENTH_REL
    # one value and 65 values: counts, and a maximum the whole sweep contains
    one = ltrace.math32_probe("pow_minus_tenth", bits32(2.0), bits32(2.0))
    assert one["compared"] == 1 and one["differing"] == 0
    assert one["abs_sin"][0] == pytest.approx(abs(ltrace.math64_probe("pow_minus_tenth_f32", [2.0])[0, 0] / 2.0 ** -0.1 - 1.0), abs=1e-12)
    r = ltrace.math32_probe("pow_minus_tenth", bits32(3.0), bits32(3.0) + 64)
    assert r["compared"] == 65 and r["differing"] == 0 and 0 < r["abs_sin"][0] <= worst
    # the counter counts: zero and the denormals next to it give no positive finite number
    r = ltrace.math32_probe("pow_minus_tenth", 0, 64)
    assert r["compared"] == 65 and r["differing"] == 65 and r["first_differing"] == 0
    # FLT_MIN and FLT_MAX are still served; 0, a denormal, +inf and NaN are not (recorded above)
    assert np.allclose(out[2:4], special[2:4] ** -0.1, rtol=1e-6)
    assert not (np.isfinite(out[[0, 1, 4, 5]]) & (out[[0, 1, 4, 5]] > 0)).any()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the two forms of the attempt
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_attempt_forms_agree_in_every_bit(exact):
    """attempt<true> and attempt<false>: candidate, k7, (sn, cn) and err_sq equal in every bit wherever the branch-free form
    reports itself valid -- every class, every row kind, every spin."""
    n_valid = by_r = by_d = 0
    for a in sb.SPINS:
        for name in db.CLASSES:
            c = db.dp45_rows(a, name)
            if c is None:
                continue
            for kind in kinds(name):
                h = c[kind]["h"]
                chk = attempt(a, c["st"], c["L"], h, c["refine"], exact, True)
                fast = attempt(a, c["st"], c["L"], h, c["refine"], exact, False)
                assert np.isnan(chk["min_r"]).all() and np.isnan(chk["max_d"]).all()
                ok = valid(a, fast)
                for key in ATTEMPT_KEYS:
                    same = same_bits(chk[key][ok], fast[key][ok])
                    assert same.all(), (a, name, kind, key, int((~same).sum()), c["st"][ok][np.argmin(same.reshape(same.shape[0], -1).all(axis=1))])
                n_valid += int(ok.sum())
                by_r += int((~(fast["min_r"] > sb.r_plus(a) * 1.001)).sum())
                by_d += int((~(fast["max_d"] <= 0.25)).sum())
                if name not in db.CHECKED_CLASSES and kind == "accepted":
                    assert ok.mean() > 0.9, (a, name, ok.mean())
        c = db.dp45_rows(a, "mid")
        for m in (1, 65):
            for checked in (True, False):
                full = attempt(a, c["st"], c["L"], c["accepted"]["h"], c["refine"], exact, checked)
                part = attempt(a, c["st"][:m], c["L"][:m], c["accepted"]["h"][:m], c["refine"][:m], exact, checked)
                assert all(same_bits(part[k], full[k][:m]).all() for k in ATTEMPT_KEYS + ("min_r", "max_d"))
    print(f"attempt forms, exact = {exact}: {n_valid} valid rows checked == branch-free in every bit; {by_r} rows fail the radius half, "
          f"{by_d} the angle half of the validity test")
    record(f"attempt_forms_exact{int(exact)}", dict(valid=n_valid, fails_radius=by_r, fails_angle=by_d))
    assert n_valid > 35 * N and by_r > 1000 and by_d > 1000


def test_attempt_controllers_share_all_but_the_error_norm():
    """The controller's template argument reaches the error norm's five quotients and nothing else."""
    a = 0.9
    for name in ("band", "turn"):
        c = db.dp45_rows(a, name)
        x = attempt(a, c["st"], c["L"], c["rejected"]["h"], c["refine"], True, True)
        f = attempt(a, c["st"], c["L"], c["rejected"]["h"], c["refine"], False, True)
        assert all(same_bits(x[k], f[k]).all() for k in ("next", "k7", "sc"))
        assert not same_bits(x["err_sq"], f["err_sq"]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3., 4. the candidate state and the error norm in their units
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", sb.SPINS)
def test_candidate_state_in_the_unit(a):
    """The branch-free attempt where it is valid -- and the checked attempt on every kept row of `cut_graze` and `turn` --
    against ref_attempt_longdouble in the unit of dp45_blocks.py: within 2 K_ATT64 (K_ATT64: what the float64 oracle
    itself is from the longdouble attempt; the factor two as in step_blocks.py: each of the kernel's quotients comes from
    one merged reciprocal, its stage trigonometry is rotated from the base)."""
    table, over = {}, []
    for name in db.CLASSES:
        c = db.dp45_set(a, name)
        if c is None:
            continue
        for kind in ("accepted", "rejected"):
            r = c[kind]
            assert 1.0 - r["keep"].mean() <= sb.EXCLUDED_CAP
            for checked in ((False, True) if name in db.CHECKED_CLASSES else (False,)):
                out = attempt(a, c["st"], c["L"], r["h"], c["refine"], True, checked)
                sel = r["usable"] & (True if checked else valid(a, out))
                # (the branch-free form is valid on part of `cut_graze` and `turn` only -- that is what they are for -- and
                # on half of some classes' rejected rows, three times the accepted step)
                assert sel.sum() > (0.9 * N if checked or (kind == "accepted" and name not in db.CHECKED_CLASSES) else 0), (name, kind, checked, sel.sum())
                e = (np.abs(out["next"].astype(sb.LD) - r["next"]).astype(np.float64) / r["unit"])[sel]
                assert np.isfinite(e).all()
                worst = e.max(axis=0)
                table[f"{name} {kind} {'checked' if checked else 'fast'}"] = worst
                print(f"DP45 candidate, a = {a} {name:13s} {kind:8s} {'checked' if checked else 'fast':7s}: {sel.sum()} rows, max error per "
                      f"component {np.round(worst, 2)} units")
                assert worst.max() > 0
                if not worst.max() <= 2 * db.K_ATT64:
                    over.append((name, kind, checked, np.round(worst, 2).tolist()))
    record(f"candidate_a{a}", {k: v.tolist() for k, v in table.items()})
    record(f"candidate_a{a}_max", max(v.max() for v in table.values()))
    assert not over, over


@pytest.mark.parametrize("a", sb.SPINS)
def test_error_norm_in_the_unit(a):
    """sqrt(err_sq / 5) of the device against the longdouble err_norm, accepted and rejected rows, in the unit of the error
    norm (dp45_blocks.py: the estimate is a cancellation between six stage derivatives).  The exact controller within
    2 K_ERR64 units; the float32-reciprocal controller within the same plus 1.2e-7 err_norm (2^-23): one float32 rounding
    of sc and rcp_pos's 1 ulp -- the `relative error 1e-7` lt_dp45.hpp states -- on each of the five quotients of a sum of
    squares, which is sign-free."""
    worst = {True: 0.0, False: 0.0}
    over = []
    for name in db.CLASSES:
        c = db.dp45_set(a, name)
        if c is None:
            continue
        for kind in ("accepted", "rejected"):
            r = c[kind]
            for exact in (True, False):
                checked = name in db.CHECKED_CLASSES
                out = attempt(a, c["st"], c["L"], r["h"], c["refine"], exact, checked)
                sel = r["usable"] & (True if checked else valid(a, out))
                assert sel.sum() > (0.9 * N if checked or kind == "accepted" else 0), (name, kind, sel.sum())
                got = np.sqrt(out["err_sq"].astype(sb.LD) / sb.LD(5))
                d = np.abs(got - r["err"]).astype(np.float64)
                allow = 0.0 if exact else 1.2e-7 * r["err"].astype(np.float64)
                e = (np.maximum(d - allow, 0.0) / r["unit_err"])[sel]
                assert np.isfinite(e).all() and d[sel].max() > 0
                print(f"DP45 err_norm, a = {a} {name:13s} {kind:8s} {'exact' if exact else 'float32 rcp'}: {sel.sum()} rows, max error "
                      f"{e.max():.2f} units" + ("" if exact else f" beyond 1.2e-7 err_norm (raw relative {np.max(d[sel] / r['err'].astype(np.float64)[sel]):.2e})"))
                worst[exact] = max(worst[exact], e.max())
                if not e.max() <= 2 * db.K_ERR64:
                    over.append((name, kind, exact, float(e.max())))
    record(f"err_norm_a{a}", dict(exact=worst[True], float32_rcp_beyond_allowance=worst[False]))
    assert not over, over


# ---------------------------------------------------------------------------------------------------------------------------
# 5. advance() is its two attempts, selected per lane
# ---------------------------------------------------------------------------------------------------------------------------
def _redo_batch(a):
    """Rows that take the checked arithmetic in advance() -- fallback_class at the step size the oracle's sequence starts
    from (a stage inside r_cut, a large turn: unusable or rejected) and sharp_turn_rows (a large turn, accepted) -- and
    ordinary rows (`far`, `mid`, `band`), with the carried k1 and [sin, cos] handed in explicitly."""
    fst, fL, _ = sb.fallback_class(a, 896, rounded=False)
    parts = [(fst, fL, np.maximum(1.0, 0.01 * fst[:, 0]), np.zeros(896, dtype=np.uint8))]
    sst, sL, sh = db.sharp_turn_rows(a, 1024)
    parts.append((sst, sL, sh, np.zeros(1024, dtype=np.uint8)))
    for name, kind in (("far", "accepted"), ("mid", "rejected"), ("band", "accepted")):
        c = db.dp45_rows(a, name)
        parts.append((c["st"][:448], c["L"][:448], c[kind]["h"][:448], c["refine"][:448]))
    st, L, h, rf = (np.concatenate([p[i] for p in parts]) for i in range(4))
    k1 = oracle.kerr_rhs_n(st, L, sb.M, a)
    sc0 = np.stack([np.sin(st[:, 1]), np.cos(st[:, 1])], axis=1)
    return st, L, h, rf, k1, sc0


def _advance_and_its_attempts(a, exact):
    """The batch through advance() in two orders -- redo and ordinary rows alternating inside every wavefront, and every
    wavefront all-redo or all-ordinary -- and through both forms of the attempt probe."""
    st, L, h, rf, k1, sc0 = _redo_batch(a)
    n = st.shape[0]
    fast = attempt(a, st, L, h, rf, exact, False, k1=k1, sc0=sc0)
    chk = attempt(a, st, L, h, rf, exact, True, k1=k1, sc0=sc0)
    redo = ~valid(a, fast)
    assert redo.sum() > 600 and (~redo).sum() > 600, (redo.sum(), n)
    ri, oi = np.flatnonzero(redo), np.flatnonzero(~redo)
    m = min(ri.size, oi.size)
    inter = np.concatenate([np.stack([ri[:m], oi[:m]], axis=1).ravel(), ri[m:], oi[m:]])
    pad = lambda idx: np.concatenate([idx, idx[: (-idx.size) % 64]])  # (each kind padded to whole wavefronts with its own rows)
    seg = np.concatenate([pad(ri), pad(oi)])
    assert all(redo[seg[i:i + 64]].all() or not redo[seg[i:i + 64]].any() for i in range(0, seg.size, 64))
    assert all(redo[inter[i:i + 64]].any() and not redo[inter[i:i + 64]].all() for i in range(0, 2 * m - 63, 64))
    run = lambda idx: advance(a, st[idx], L[idx], h[idx], rf[idx], exact, k1=k1[idx], sc0=sc0[idx])
    out_i, out_s = run(inter), run(seg)
    back_i, back_s = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int64)
    back_i[inter] = np.arange(inter.size)
    back_s[seg] = np.arange(seg.size)  # (a padded row's last copy)
    o = {k: v[back_i] for k, v in out_i.items()}
    o_seg = {k: v[back_s] for k, v in out_s.items()}
    sel = {k: np.where(redo.reshape((n,) + (1,) * (chk[k].ndim - 1)), chk[k], fast[k]) for k in ATTEMPT_KEYS}
    return dict(st=st, L=L, h=h, rf=rf, k1=k1, sc0=sc0, redo=redo, o=o, o_seg=o_seg, sel=sel)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 1.0])
def test_advance_selects_per_lane_and_no_lane_depends_on_a_neighbour(a, exact):
    """A batch in which lanes that need the checked attempt and lanes that do not alternate inside every wavefront, and the
    same rows ordered so that a wavefront holds lanes of one kind only: the same bits per row -- state, carried k1 and
    (s0, c0), lam, step size, event, counters.  advance() accepts where the selected attempt (attempt<true> on a redo lane,
    attempt<false> elsewhere) says so and leaves every bit of a row it does not accept alone (what it accepts: the test
    below)."""
    d = _advance_and_its_attempts(a, exact)
    st, L, h, k1, sc0, redo, o, sel = (d[k] for k in ("st", "L", "h", "k1", "sc0", "redo", "o", "sel"))
    for key in ("state", "k1", "sc", "lam", "h"):
        same = same_bits(o[key], d["o_seg"][key])
        assert same.all(), (key, int((~same).sum()))
    for key in ("event", "steps", "attempts"):
        assert np.array_equal(o[key], d["o_seg"][key]), key
    assert (o["steps"] == 1).all() and (o["attempts"] == 1).all()
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(sel["next"]).all(axis=1) & (sel["next"][:, 0] > 0)
        reject = (np.sqrt(sel["err_sq"] * 0.2) > 1.0) if exact else (sel["err_sq"] > 5.0)
    accepted = o["lam"] == h
    cap = o["event"] == EV_CAPTURED  # (accepted arithmetic, but the ray ends: lam stays)
    assert ((o["lam"] == 0) | accepted).all()
    assert np.array_equal(accepted | cap, usable & ~reject)
    running = o["event"] == EV_RUNNING
    acc, rej = accepted & running, ~accepted & running
    for got, want in ((o["state"], st), (o["k1"], k1), (o["sc"], sc0)):
        assert same_bits(got[~accepted & ~cap], want[~accepted & ~cap]).all()
    assert same_bits(o["k1"][cap], k1[cap]).all() and same_bits(o["sc"][cap], sc0[cap]).all()
    assert np.isin(o["event"], (EV_RUNNING, EV_CAPTURED, EV_INVALID)).all()
    with np.errstate(invalid="ignore"):
        assert (o["h"][rej] < h[rej]).all() and (o["h"][acc] >= 0.2 * h[acc]).all() and np.isfinite(o["h"]).all() and (o["h"] > 0).all()
    counts = dict(redo_accepted=int((acc & redo).sum()), redo_rejected=int((rej & redo & usable).sum()), redo_unusable=int((redo & ~usable).sum()),
                  ordinary_accepted=int((acc & ~redo).sum()), ordinary_rejected=int((rej & ~redo).sum()), captured=int(cap.sum()))
    print(f"advance() against its attempts, a = {a}, exact = {exact}: {counts}")
    record(f"advance_selection_a{a}_exact{int(exact)}", counts)
    assert counts["redo_accepted"] > 20 and counts["redo_rejected"] > 100 and counts["redo_unusable"] > 100
    assert counts["ordinary_accepted"] > 100 and counts["ordinary_rejected"] > 100


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 1.0])
def test_advance_is_its_two_attempts_in_every_bit(a, exact):
    """What advance() accepts -- candidate, carried k1, carried (s0, c0) -- equals in every bit what the attempt probe gives
    for the same row: attempt<true> on a redo lane, attempt<false> elsewhere; and its decision and the step size it goes on
    with are, in every bit, what the controller probe makes of that attempt's err_sq (h / 4 where the candidate is unusable).

    What this test found: with attempt()'s sums written as plain multiplies and adds, 653 of 10 860 state elements of 2 172
    accepted rows differed from the probe's (a = 0.5; up to 48 ulp of the element, 1.76 units of a candidate state), 931
    elements of k1 and 99 of (s0, c0) -- on ordinary lanes as on redo lanes.  Not the selection: under -ffp-contract=fast
    which product of a sum the compiler fused depended on what else the kernel inlined (advance() inlines both forms of
    attempt() and they share products; the probe inlines one).  Every multiply-add of the stage sums, the candidate and the
    error norm is an explicit fma now, and any two kernels that inline attempt() agree."""
    d = _advance_and_its_attempts(a, exact)
    o, sel = d["o"], d["sel"]
    acc = (o["lam"] == d["h"]) & (o["event"] == EV_RUNNING)
    bad = {}
    for name, got, want in (("state", o["state"], sel["next"]), ("k1", o["k1"], sel["k7"]), ("sc", o["sc"], sel["sc"])):
        same = same_bits(got[acc], want[acc])
        with np.errstate(invalid="ignore", divide="ignore"):
            u = np.abs(got[acc] - want[acc]) / np.spacing(np.maximum(np.abs(got[acc]), np.abs(want[acc])))
        bad[name] = (int((~same).sum()), float(np.nanmax(u)))
    print(f"advance() against the attempt probe in every bit, a = {a}, exact = {exact}: {int(acc.sum())} accepted rows; differing elements "
          f"(count, max ulp) {bad}")
    record(f"advance_bits_a{a}_exact{int(exact)}", dict(accepted=int(acc.sum()), **{k: list(v) for k, v in bad.items()}))
    assert all(v[0] == 0 for v in bad.values()), bad
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(sel["next"]).all(axis=1) & (sel["next"][:, 0] > 0)
    reject, h_next = ltrace.dp45_controller_probe(sel["err_sq"], d["h"], exact=exact)
    went_on = np.isin(o["event"], (EV_RUNNING, EV_INVALID))  # (a capture leaves h alone)
    want_h = np.where(usable, h_next, 0.25 * d["h"])
    assert same_bits(o["h"][went_on], want_h[went_on]).all(), int((~same_bits(o["h"], want_h) & went_on).sum())
    assert np.array_equal((o["lam"] == d["h"]) | (o["event"] == EV_CAPTURED), usable & ~reject)
    assert (usable & reject).sum() > 100 and (usable & ~reject).sum() > 100 and (~usable).sum() > 100


# ---------------------------------------------------------------------------------------------------------------------------
# 6. / 7. the controller and the decision ladder, through advance()
# ---------------------------------------------------------------------------------------------------------------------------
E1, B1 = 71.0 / 57600.0, 35.0 / 384.0


def _inside_rows(a, n, seed):
    """States at or inside r_cut (every right-hand side of the attempt is zero), phi = 0, and carried k1 with a dphi
    component only.  With k = k1[2]: candidate phi = h B1 k, err_norm = |h E1 k| / (1e-8 + 1e-6 |h B1 k|) / sqrt(5)."""
    rng = np.random.default_rng([seed, 500, int(round(a * 1000))])
    st, L = sb._states(rng, n, 0.6 * sb.r_plus(a), 1.0005 * sb.r_plus(a), 0.3, np.pi - 0.3)
    st[:, 2] = 0.0
    return st, L


def _mp_controller(err_sq, h, exact):
    """(reject, h_next) of metrics.py:514-522, :560-564 in mpmath from err_sq; h_next as (hi, lo) float64 pairs."""
    mpmath.mp.prec = 200
    rej, hi, lo = np.empty(err_sq.size, dtype=bool), np.empty(err_sq.size), np.empty(err_sq.size)
    for i, (e2, hh) in enumerate(zip(err_sq, h)):
        e = mpmath.sqrt(mpmath.mpf(float(e2)) / 5)
        rej[i] = e > 1
        if e > 1:
            f = max(mpmath.mpf("0.2"), mpmath.mpf("0.9") * e ** mpmath.mpf("-0.2"))
        elif e < mpmath.mpf("1e-10"):
            f = mpmath.mpf(5)
        else:
            f = min(mpmath.mpf(5), mpmath.mpf("0.9") * e ** mpmath.mpf("-0.2"))
        t = mpmath.mpf(float(hh)) * f
        hi[i] = float(t)
        lo[i] = float(t - mpmath.mpf(hi[i]))
    return rej, hi, lo


@pytest.mark.parametrize("exact", [True, False])
def test_controller_against_the_reference_expressions(exact):
    """The controller alone (lt_dp45_controller_probe: the member function advance() calls) on err_sq log-uniform over
    [1e-40, 1e40], 4 096 values within 2^-30 of 5 (reject is err_sq > 5 <=> err_norm > 1), and 0, a denormal, DBL_MAX, +inf
    and NaN, against the reference's expressions (metrics.py:514-522, :560-564) in mpmath from the same err_sq.
      exact: h_next within 4 ulp of h max(0.2, 0.9 e^-0.2) / h min(5, 0.9 e^-0.2) / 5 h  (* 0.2 and the square root 0.75 ulp,
      pow_m02 2 ulp -- the bound test_gpu_step_blocks.py pins -- two products 1 ulp); reject as in mpmath except where
      |err_norm - 1| < 4 ulp.
      float32 controller: h_next within POW_TENTH_REL + 2^-23 relative; reject exactly err_sq > 5.
    Both: h_next finite and positive for every finite positive h whatever err_sq is; a NaN err_sq gives accept, h 5, as the
    reference does (tests/test_dp45_blocks_host.py); +inf gives reject, h 0.2."""
    rng = np.random.default_rng(66)
    n = 8192
    special = np.array([0.0, 5e-324, 1e-310, np.finfo(np.float64).max, np.inf, np.nan])
    err_sq = np.concatenate([np.exp(rng.uniform(np.log(1e-40), np.log(1e40), n)), 5.0 * (1.0 + rng.uniform(-2.0 ** -30, 2.0 ** -30, 4096)),
                             [5.0, np.nextafter(5.0, 6.0), np.nextafter(5.0, 4.0)], special])
    h = np.exp(rng.uniform(np.log(1e-12), np.log(1e3), err_sq.size))
    reject, h_next = ltrace.dp45_controller_probe(err_sq, h, exact=exact)
    assert np.isfinite(h_next).all() and (h_next > 0).all()
    fin = np.isfinite(err_sq)
    rej_mp, hi, lo = _mp_controller(err_sq[fin], h[fin], exact)
    _, ulps = sb.err64(h_next[fin], hi, lo)
    e = np.sqrt(err_sq[fin] / 5.0)
    if exact:
        off = np.abs(e - 1.0) < 4 * np.spacing(1.0)
        assert np.array_equal(reject[fin][~off], rej_mp[~off])
        ok = reject[fin] == rej_mp
        print(f"exact controller, {err_sq.size} err_sq in [0, DBL_MAX]: h_next max {ulps[ok].max():.3f} ulp; {int((~ok).sum())} decisions differ "
              f"from mpmath's, all within 4 ulp of the threshold ({int(off.sum())} values are)")
        record("controller_probe_exact", dict(n=int(err_sq.size), max_ulp=ulps[ok].max(), decisions_differing=int((~ok).sum()),
                                              within_4ulp_of_threshold=int(off.sum())))
        assert ulps[ok].max() <= 4.0
    else:
        assert np.array_equal(reject, err_sq > 5.0)
        ok = reject[fin] == rej_mp  # (err_sq > 5 and err_norm > 1 differ by the rounding of sqrt(err_sq / 5) only)
        assert (np.abs(e[~ok] - 1.0) < 4 * np.spacing(1.0)).all()
        rel = np.abs(h_next[fin] - hi) / hi
        print(f"float32 controller, {err_sq.size} err_sq in [0, DBL_MAX]: h_next max relative error {rel[ok].max():.3e}; {int((~ok).sum())} "
              f"decisions differ from err_norm > 1, all within 4 ulp of it")
        record("controller_probe_float32", dict(n=int(err_sq.size), max_rel=rel[ok].max(), decisions_differing=int((~ok).sum())))
        assert rel[ok].max() <= db.POW_TENTH_REL + 2.0 ** -23
    k = err_sq.size - special.size
    assert not reject[k:k + 3].any() and (h_next[k:k + 3] == 5.0 * h[k:k + 3]).all()        # 0 and the denormals: tiny
    assert reject[k + 3] and h_next[k + 3] == 0.2 * h[k + 3]                                 # DBL_MAX
    assert reject[k + 4] and h_next[k + 4] == 0.2 * h[k + 4]                                 # +inf
    assert not reject[k + 5] and h_next[k + 5] == 5.0 * h[k + 5]                             # NaN: accept, h 5
    assert not reject[k - 3] and not reject[k - 1]                                           # 5 itself is not rejected
    assert exact or reject[k - 2]        # (the exact controller's sqrt(err_sq / 5) is 1 one ulp above 5: inside the 4 ulp)
    part = ltrace.dp45_controller_probe(err_sq[:65], h[:65], exact=exact)
    assert np.array_equal(part[0], reject[:65]) and same_bits(part[1], h_next[:65]).all()


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 1.0])
def test_controller_through_advance(a, exact):
    """The step-size controller on error norms from 1e-14 to 6e3 -- `tiny`, both clamps, growth, shrinking, and 2 048 values
    around the reject threshold -- against the reference's expressions evaluated in mpmath from the err_sq the attempt
    itself hands the controller.
      exact: h_next within 4 ulp of h max(0.2, 0.9 e^-0.2) / h min(5, 0.9 e^-0.2) / 5 h  (* 0.2 and the square root
      0.75 ulp of e, a fifth of which reaches e^-0.2; pow_m02 2 ulp, the bound test_gpu_step_blocks.py pins; two products
      1 ulp); reject as in mpmath except where |err_norm - 1| < 4 ulp.  Written in the float64 constants the kernel and
      the reference use (0.2, 0.9 as float64) the difference to the decimal constants is 0.06 ulp.
      float32 controller: h_next within POW_TENTH_REL + 2^-23 relative (the power, its float32 argument and its product
      with 0.9 in float64), reject exactly err_sq > 5.
    Either: h_next positive and finite, the candidate carried on accept, the state untouched on reject."""
    n = 6144
    st, L = _inside_rows(a, n, 1)
    rng = np.random.default_rng(77)
    h = np.exp(rng.uniform(np.log(1e-3), np.log(10.0), n))
    # err_norm wanted -> k: q = sqrt(5) err; k = q 1e-8 / (h (E1 - q 1e-6 B1)), q below E1 / (1e-6 B1) = 1.35e4
    want = np.concatenate([np.exp(rng.uniform(np.log(1e-14), np.log(6e3), n - 2048 - 4)), 1.0 + rng.uniform(-2.0 ** -30, 2.0 ** -30, 2048),
                           [0.0, 1e-10, (0.9 / 5.0) ** 5, (0.9 / 0.2) ** 5]])
    q = np.sqrt(5.0) * want
    k1 = np.zeros((n, 5))
    k1[:, 2] = q * 1e-8 / (h * (E1 - q * 1e-6 * B1)) * rng.choice([-1.0, 1.0], n)
    rf = np.zeros(n, dtype=np.uint8)
    att = attempt(a, st, L, h, rf, exact, True, k1=k1)
    assert (att["next"][:, [0, 1, 3, 4]] == st[:, [0, 1, 3, 4]]).all() and (att["k7"] == 0).all()
    err_sq = att["err_sq"]
    e_dev = np.sqrt(err_sq / 5.0)
    assert np.allclose(e_dev, want, rtol=1e-9 if exact else 1e-6, atol=1e-300)  # (the construction gives the error norm it was asked for)
    out = advance(a, st, L, h, rf, exact, k1=k1)
    assert (out["event"] == EV_RUNNING).all() and (out["steps"] == 1).all()
    rej_mp, hi, lo = _mp_controller(err_sq, h, exact)
    got_rej = out["lam"] == 0
    assert ((out["lam"] == h) | got_rej).all()
    _, ulps = sb.err64(out["h"], hi, lo)
    if exact:
        off = np.abs(e_dev - 1.0) < 4 * np.spacing(1.0)
        assert np.array_equal(got_rej[~off], rej_mp[~off])
        ok = got_rej == rej_mp
        print(f"exact controller through advance(), a = {a}: {n} error norms, h_next max {ulps[ok].max():.3f} ulp; {int((~ok).sum())} decisions "
              f"differ from mpmath's, all within 4 ulp of the threshold ({int(off.sum())} values are)")
        record(f"controller_exact_a{a}", dict(n=n, max_ulp=ulps[ok].max(), decisions_differing=int((~ok).sum()), within_4ulp_of_threshold=int(off.sum())))
        assert ulps[ok].max() <= 4.0
    else:
        assert np.array_equal(got_rej, err_sq > 5.0)
        ok = got_rej == rej_mp  # (err_sq > 5 and err_norm > 1 can differ by the rounding of sqrt(err_sq / 5) only)
        assert (np.abs(e_dev[~ok] - 1.0) < 4 * np.spacing(1.0)).all()
        rel = np.abs(out["h"] - hi) / hi
        print(f"float32 controller through advance(), a = {a}: {n} error norms, h_next max relative error {rel[ok].max():.3e}")
        record(f"controller_float32_a{a}", dict(n=n, max_rel=rel[ok].max()))
        assert rel[ok].max() <= db.POW_TENTH_REL + 2.0 ** -23
    assert np.isfinite(out["h"]).all() and (out["h"] > 0).all()
    acc = ~got_rej
    assert same_bits(out["state"][acc], att["next"][acc]).all() and same_bits(out["state"][got_rej], st[got_rej]).all()
    assert (out["k1"][acc] == 0).all() and same_bits(out["k1"][got_rej], k1[got_rej]).all()
    # the branches were all there
    assert (out["h"][want < 1e-10] == 5.0 * h[want < 1e-10]).all() and (want < 1e-10).sum() > 100
    assert (out["h"][want > 2000.0] == 0.2 * h[want > 2000.0]).all() and (want > 2000.0).sum() > 50
    grown = (want > 1e-9) & (want < 1e-4)
    assert (out["h"][grown] == 5.0 * h[grown]).all() and grown.sum() > 500


def _axis_row(a):
    """A carried k1 whose dtheta component puts the candidate 1e-7 rad from the axis (found with the oracle alone, by the
    secant rule on that component): k7's dp_theta is ~1e21 there and err_sq ~1e50, +inf as a float32."""
    st = np.array([[12.0, 0.05, 0.0, -0.9, 0.2]])
    L = np.array([0.3])
    h = 0.01
    k1 = oracle.kerr_rhs_n(st, L, sb.M, a)
    f = lambda x: oracle.dp45_attempt(st, L, h, sb.M, a, r_obs=db.R_OBS, lambda_max=1e9, k1=np.concatenate([k1[0, :1], [x], k1[0, 2:]])[None, :],
                                      axis_refine=1)["next"][0, 1] - 1e-7
    x0, x1 = k1[0, 1], -0.05 / (h * B1)
    for _ in range(60):
        f0, f1 = f(x0), f(x1)
        if f1 == f0 or abs(f1) < 1e-12:
            break
        x0, x1 = x1, x1 - f1 * (x1 - x0) / (f1 - f0)
    k1[0, 1] = x1
    return st, L, h, k1


TABLE_R_OBS, TABLE_LAM_MAX = 50.0, 5000.0


def decision_rows(a):
    """The rows of test_decision_table and what the oracle makes of them (no GPU): dict(label, st, L, h, k1, custom (k1 is
    not the right-hand side at the state), lam, steps, refine, oracle)."""
    rp = sb.r_plus(a)
    r_cap = rp * 1.01
    inside = np.array([0.9 * rp, 1.1, 0.0, 0.3, -0.4])
    far = np.array([30.0, 1.2, 0.5, -0.9, 3.0])
    rows = []  # (label, state, L, h, k1 or None, lam, steps, refine)
    nan_k1 = np.array([0.0, np.nan, 0.0, 0.0, 0.0])
    inf_k1 = np.array([0.0, 0.0, 0.0, np.inf, 0.0])
    rows.append(("k1 NaN", far, 2.0, 1.0, nan_k1, 0.0, 0, 0))
    rows.append(("k1 inf", far, 2.0, 1.0, inf_k1, 0.0, 0, 0))
    rows.append(("overshoot", np.array([3.0 * rp, 1.2, 0.0, -2.0, 40.0]), 2.0, 1e6, None, 0.0, 0, 0))
    rows.append(("r <= 0", inside, 2.0, 1.0, np.array([-100.0, 0.0, 0.0, 0.0, 0.0]), 0.0, 7, 0))
    rows.append(("k1 NaN, h small", far, 2.0, 3e-12, nan_k1, 0.0, 0, 0))
    rows.append(("r <= 0, h small", inside, 2.0, 3.9e-12, np.array([-1e14, 0.0, 0.0, 0.0, 0.0]), 0.0, 0, 0))
    rows.append(("reject below h_min", inside, 2.0, 1.5e-12, np.array([0.0, 0.0, 1e9, 0.0, 0.0]), 0.0, 0, 0))
    rows.append(("zero rhs", inside, 2.0, 0.7, np.zeros(5), 3.0, 11, 0))
    rows.append(("r_prev == r_capture", np.array([r_cap, 1.2, 0.0, -1.0, 0.5]), 1.0, 1e-3, None, 0.0, 0, 0))
    rows.append(("lam == lambda_max", far, 2.0, 1.0, None, TABLE_LAM_MAX, 5, 0))
    rows.append(("lam one ulp below", far, 2.0, 1.0, None, np.nextafter(TABLE_LAM_MAX, 0.0), 5, 0))
    rows.append(("h > remaining", far, 2.0, 1.0, None, TABLE_LAM_MAX - 0.3, 5, 0))
    rows.append(("steps 199 999", far, 2.0, 1.0, None, 0.0, 199999, 0))
    rows.append(("steps 200 000", far, 2.0, 1.0, None, 0.0, 200000, 0))
    ax_st, ax_L, ax_h, ax_k1 = _axis_row(a)
    rows.append(("axis: err_sq > 1.7e39", ax_st[0], ax_L[0], ax_h, ax_k1[0], 0.0, 0, 1))
    # capture and escape crossings: states a step away from the terminal radii, the step size the oracle accepts
    rng = np.random.default_rng([9, int(round(a * 1000))])
    m = 96
    cs = np.zeros((2 * m, 5))
    cs[:m, 0] = r_cap * (1.0 + np.exp(rng.uniform(np.log(1e-7), np.log(1e-2), m)))
    cs[m:, 0] = 2.0 * TABLE_R_OBS - np.exp(rng.uniform(np.log(1e-3), np.log(0.5), m))
    cs[:, 1] = rng.uniform(0.5, np.pi - 0.5, 2 * m)
    cs[:, 2] = rng.uniform(-3.0, 3.0, 2 * m)
    cs[:m, 3], cs[m:, 3] = -rng.uniform(0.5, 3.0, m), rng.uniform(0.7, 1.0, m)
    cs[:, 4] = rng.uniform(-3.0, 3.0, 2 * m)
    cL = rng.uniform(-3.0, 3.0, 2 * m)
    ch = np.maximum(1.0, 0.01 * cs[:, 0])
    for _ in range(200):
        o = oracle.dp45_attempt(cs, cL, ch, sb.M, a, r_obs=TABLE_R_OBS, lambda_max=TABLE_LAM_MAX)
        if (o["decision"] == 2).all():
            break
        ch = np.where(o["decision"] == 2, ch, o["h_next"])
    for i in range(2 * m):
        rows.append(("capture" if i < m else "escape", cs[i], cL[i], ch[i], None, 1.0, 3, 0))
    st = np.array([r[1] for r in rows])
    L = np.array([r[2] for r in rows], dtype=np.float64)
    k1 = oracle.kerr_rhs_n(st, L, sb.M, a)
    for i, r in enumerate(rows):
        if r[4] is not None:
            k1[i] = r[4]
    t = dict(label=[r[0] for r in rows], st=st, L=L, h=np.array([r[3] for r in rows], dtype=np.float64), k1=k1,
             custom=np.array([r[4] is not None for r in rows]), lam=np.array([r[5] for r in rows], dtype=np.float64),
             steps=np.array([r[6] for r in rows], dtype=np.uint32), refine=np.array([r[7] for r in rows], dtype=np.uint8))
    t["oracle"] = oracle.dp45_attempt(st, L, t["h"], sb.M, a, r_obs=TABLE_R_OBS, lambda_max=TABLE_LAM_MAX, k1=k1, lam=t["lam"], axis_refine=t["refine"])
    return t


def check_decision_rows(t):
    """What the oracle says about each row is what the row is there for.  -> (index by label, captures, escapes)"""
    orc, label = t["oracle"], t["label"]
    by = {lb: i for i, lb in enumerate(label)}
    assert [int(orc["decision"][by[lb]]) for lb in ("k1 NaN", "k1 inf", "overshoot", "r <= 0")] == [0, 0, 0, 0]
    assert [int(orc["event"][by[lb]]) for lb in ("k1 NaN", "k1 inf", "overshoot", "r <= 0")] == [4, 4, 4, 4]
    assert [int(orc["event"][by[lb]]) for lb in ("k1 NaN, h small", "r <= 0, h small", "reject below h_min")] == [0, 0, 0]
    assert orc["decision"][by["reject below h_min"]] == 1 and orc["decision"][by["zero rhs"]] == 2 and orc["err_norm"][by["zero rhs"]] == 0
    assert orc["event"][by["r_prev == r_capture"]] == EV_RUNNING and orc["decision"][by["r_prev == r_capture"]] == 2
    assert orc["event"][by["lam == lambda_max"]] == EV_MAXRANGE and orc["decision"][by["lam == lambda_max"]] == -1
    assert orc["decision"][by["lam one ulp below"]] == 2 and orc["decision"][by["h > remaining"]] == 2
    i = by["axis: err_sq > 1.7e39"]
    assert orc["decision"][i] == 1 and orc["err_norm"][i] ** 2 * 5 > 1.7e39 and 0 < orc["next"][i, 1] < 2e-7
    cap, esc = np.array([lb == "capture" for lb in label]), np.array([lb == "escape" for lb in label])
    assert (orc["decision"][cap | esc] == 2).all()
    n_cap, n_esc = int((orc["event"][cap] == EV_CAPTURED).sum()), int((orc["event"][esc] == EV_ESCAPED).sum())
    assert n_cap >= 10 and n_esc >= 10 and (orc["event"][cap] == EV_RUNNING).sum() >= 10, (n_cap, n_esc)
    return by, n_cap, n_esc


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 1.0])
def test_decision_table(a, exact):
    """The ladder of metrics.py:454-564, one attempt per row, against the oracle's own attempt (oracle.dp45_attempt) field
    by field: event and attempt count equal; the state within 3 K_ATT64 units (2 K_ATT64 for the device and K_ATT64 for the
    oracle, each against longdouble) where it is a candidate, and in every bit where it must be untouched; h equal in every
    bit where the factor is 0.25, 0.2, 5 or the clamp to the remaining range, and elsewhere within the controller's
    tolerance of test_controller_through_advance (4 ulp, and one for the oracle's own pow / POW_TENTH_REL + 2^-23) plus a
    fifth of the relative distance the two error norms may have: 3 K_ERR64 units (2 K_ERR64 the device's, K_ERR64 the
    oracle's), or 16 roundings where the error norm is one product over one scale (a carried k1 at zero right-hand side);
    for the float32 controller another fifth of the 1.2e-7 of its quotients.

    The device forms err_sq before it tests the candidate, the reference after; and the reference tests the accepted state
    a second time.  Rows `k1 NaN` and `k1 inf` have a candidate AND an error norm that are not finite: both orders must turn
    them away by the first test, h / 4, and the small-h twins must end the ray."""
    t = decision_rows(a)
    by, n_cap, n_esc = check_decision_rows(t)
    label, st, L, h, k1, lam, steps, rf, orc = (t[k] for k in ("label", "st", "L", "h", "k1", "lam", "steps", "refine", "oracle"))
    n = st.shape[0]
    lam_max = TABLE_LAM_MAX
    sc0 = np.stack([np.sin(st[:, 1]), np.cos(st[:, 1])], axis=1)
    dev = advance(a, st, L, h, rf, exact, r_obs=TABLE_R_OBS, lambda_max=lam_max, k1=k1, sc0=sc0, lam=lam, steps=steps)
    capped = by["steps 200 000"]  # (the oracle's attempt has no counter: metrics.py:454 ends the loop)
    want_event = orc["event"].copy()
    want_event[capped] = EV_MAXRANGE

    # event and counters
    assert np.array_equal(dev["event"], want_event), [(label[i], int(dev["event"][i]), int(want_event[i])) for i in np.flatnonzero(dev["event"] != want_event)]
    attempted = (orc["decision"] >= 0) & (np.arange(n) != capped)
    assert np.array_equal(dev["steps"], steps.astype(np.int64) + attempted) and (dev["attempts"] == 1).all()
    # the step size
    hc = np.where(lam < lam_max, np.minimum(h, lam_max - lam), h)
    went_on = want_event == EV_RUNNING
    factor_exact = (orc["h_next"] == 0.2 * hc) | (orc["h_next"] == 5.0 * hc)
    exact_h = (orc["decision"] <= 0) | ((orc["decision"] == 2) & ~went_on) | factor_exact
    exact_h[capped] = True
    want_h = orc["h_next"].copy()
    want_h[capped] = h[capped]  # (a row that ends at the attempt cap or at lam >= lambda_max leaves before the clamp)
    bad = exact_h & ~same_bits(dev["h"], want_h)
    assert not bad.any(), [(label[i], dev["h"][i], want_h[i]) for i in np.flatnonzero(bad)]
    idx = np.flatnonzero(~exact_h)
    assert idx.size >= 20
    delta = np.full(idx.size, 16 * sb.U64)
    nat = ~t["custom"][idx]
    err_ld, unit_err = db.err_unit(a, st[idx][nat], L[idx][nat], hc[idx][nat], rf[idx][nat])
    delta[nat] = 3 * db.K_ERR64 * unit_err / err_ld.astype(np.float64)
    tol = (5 * 2.0 ** -52 if exact else db.POW_TENTH_REL + 2.0 ** -23 + 0.2 * 1.2e-7) + 0.2 * delta
    rel = np.abs(dev["h"] - want_h)[idx] / want_h[idx]
    print(f"decision table, a = {a}, exact = {exact}: {n} rows ({n_cap} captures, {n_esc} escapes); h_next against the oracle's where it is "
          f"a computed factor ({idx.size} rows): max relative difference {rel.max():.3e}, {np.max(rel / tol):.3f} of what is allowed")
    record(f"decision_table_a{a}_exact{int(exact)}", dict(rows=n, captures=n_cap, escapes=n_esc, h_rel_max=rel.max(), h_of_allowed=np.max(rel / tol)))
    assert (rel <= tol).all(), [(label[i], r, x) for i, r, x in zip(idx, rel, tol) if r > x]
    # lam
    moved = went_on & (orc["decision"] == 2)
    assert np.array_equal(dev["lam"][moved], (lam + hc)[moved]) and same_bits(dev["lam"][~moved], lam[~moved]).all()
    assert dev["lam"][by["lam one ulp below"]] == lam_max and dev["lam"][by["h > remaining"]] == lam_max
    # the state: untouched in every bit unless the oracle moved it
    still = (orc["decision"] != 2) | (np.arange(n) == capped)
    assert same_bits(dev["state"][still], st[still]).all() and same_bits(dev["k1"][still], k1[still]).all() and same_bits(dev["sc"][still], sc0[still]).all()
    z = by["zero rhs"]
    assert same_bits(dev["state"][z], st[z]).all() and dev["h"][z] == 5.0 * 0.7 and (dev["k1"][z] == 0).all() and dev["steps"][z] == 12
    # ... and where it moved: the candidate (or the point on the chord to it) within 3 K_ATT64 units of the oracle's
    mv = np.flatnonzero(~still & (np.arange(n) != z))
    _, unit, _ = sb.step_unit(a, st[mv], L[mv], hc[mv], lambda s, l, x: (oracle.dp45_attempt(s, l, x, sb.M, a, r_obs=TABLE_R_OBS, lambda_max=1e9)["next"],
                                                                      np.full((np.asarray(s).shape[0], 1), 1e3)), u=sb.U64)
    # the interpolated state y + frac (next - y), frac = (target - r) / (r_next - r): an error d in r_next moves frac by
    # frac d / |r_next - r|, the state by that times |next_i - y_i|; the chord itself adds an ulp of the state
    dy = np.abs(orc["next"][mv] - st[mv])
    ev = ~went_on[mv]
    allow = np.where(ev[:, None], unit + unit[:, :1] * dy / np.maximum(dy[:, :1], 1e-300) + sb.U64 * np.abs(orc["state"][mv]), unit)
    e = np.abs(dev["state"][mv] - orc["state"][mv]) / allow
    print(f"    moved rows: {mv.size}, max difference to the oracle's state {e.max():.2f} units")
    record(f"decision_table_state_a{a}_exact{int(exact)}", e.max())
    assert e.max() <= 3 * db.K_ATT64
    # an event leaves k1, (s0, c0) and lam as they were
    evr = mv[ev]
    assert same_bits(dev["k1"][evr], k1[evr]).all() and same_bits(dev["sc"][evr], sc0[evr]).all() and same_bits(dev["lam"][evr], lam[evr]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 8. what a ray carries from step to step
# ---------------------------------------------------------------------------------------------------------------------------
def _rays(a):
    """256 rays from a camera at r = 50 on the equator: a fan across the shadow's edge (alpha_crit ~ 0.1), every image-plane
    direction, a quarter of them flagged axis-refine."""
    rng = np.random.default_rng([21, int(round(a * 1000))])
    alpha = np.concatenate([rng.uniform(0.02, 0.3, 160), rng.uniform(0.095, 0.115, 96)])
    theta = rng.uniform(-np.pi, np.pi, 256)
    theta[:32] = np.pi / 2 + rng.uniform(-0.02, 0.02, 32)  # (towards the axis)
    st, L = np.zeros((256, 5)), np.zeros(256)
    for i in range(256):
        ok, s, _, pp = oracle.kerr_ic(sb.M, a, 50.0, alpha[i], theta[i], np.pi / 2)
        assert ok
        st[i], L[i] = s, pp
    refine = np.zeros(256, dtype=np.uint8)
    refine[:64] = 1
    return st, L, refine


_CHAINS = {}


def carried_chain(a, exact):
    """The rays of _rays(a) through 400 launches of one attempt each, chained on the host; computed once per case.
    -> dict(st, L, refine, h0, chain {1, 16, 400: the state after that many}, accepted (n,), base (n,5) the state k1 and
    (s0, c0) belong to: an event interpolates the state and leaves them alone)."""
    if (a, exact) in _CHAINS:
        return _CHAINS[(a, exact)]
    st, L, refine = _rays(a)
    n = st.shape[0]
    h0 = np.full(n, 1.0)  # max(1, 0.01 r_obs), metrics.py:449
    cur = dict(state=st.copy(), k1=None, sc=None, lam=np.zeros(n), h=h0.copy(), steps=np.zeros(n, dtype=np.int32),
               event=np.full(n, EV_RUNNING, dtype=np.int32))
    accepted = np.zeros(n, dtype=np.int64)
    base = st.copy()
    chain = {}
    for it in range(1, 401):
        o = advance(a, cur["state"], L, cur["h"], refine, exact, r_obs=50.0, lambda_max=5000.0, k1=cur["k1"], sc0=cur["sc"],
                    lam=cur["lam"], steps=cur["steps"])
        live = cur["event"] == EV_RUNNING
        accepted += live & (o["lam"] > cur["lam"])
        nxt = {}
        for key in ("state", "k1", "sc", "lam", "h", "steps", "event"):
            prev = o[key] if cur[key] is None else cur[key]
            nxt[key] = np.where(live.reshape((n,) + (1,) * (o[key].ndim - 1)), o[key], prev)
        cur = nxt
        on = live & (cur["event"] == EV_RUNNING)
        base[on] = cur["state"][on]
        if it in (1, 16, 400):
            chain[it] = {k: v.copy() for k, v in cur.items()}
    _CHAINS[(a, exact)] = dict(st=st, L=L, refine=refine, h0=h0, chain=chain, accepted=accepted, base=base)
    return _CHAINS[(a, exact)]


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 0.998, 1.0])
def test_carried_values_over_a_ray(a, exact):
    """N attempts in one launch leave, in every bit, what N launches of one attempt chained on the host leave (N = 1, 16,
    400).  After 400 attempts the carried (s0, c0) is within
    3 2^-53 (accepted steps + 1) of sincos(theta) (mpmath) at the state it belongs to, the last one the ray was running in:
    3 u is the project's bound for one sincos_shift (test_gpu_step_blocks.py); s0^2 + c0^2 within the same of 1.  (The
    carried k1 against the right-hand side at that state: the test below.)"""
    c = carried_chain(a, exact)
    st, L, refine, h0, chain, accepted, base = (c[k] for k in ("st", "L", "refine", "h0", "chain", "accepted", "base"))
    n = st.shape[0]
    for n_att in (1, 16, 400):
        o = advance(a, st, L, h0, refine, exact, r_obs=50.0, lambda_max=5000.0, n_attempts=n_att)
        want = chain[n_att]
        for key in ("state", "k1", "sc", "lam", "h"):
            same = same_bits(o[key], want[key])
            assert same.all(), (n_att, key, int((~same).sum()))
        assert np.array_equal(o["event"], want["event"]) and np.array_equal(o["steps"], want["steps"])
        assert np.isin(o["event"], (EV_RUNNING, EV_CAPTURED, EV_ESCAPED)).all()
        assert (o["attempts"] == o["steps"]).all() and (o["attempts"][o["event"] == EV_RUNNING] == n_att).all()
    ended = o["event"] != EV_RUNNING
    hi, lo = sb.mp_sincos(base[:, 1])
    err, _ = sb.err64(o["sc"], hi, lo)
    bound = 3 * sb.U64 * (accepted + 1)
    drift = err.max(axis=1) / bound
    norm = np.abs(o["sc"][:, 0] ** 2 + o["sc"][:, 1] ** 2 - 1.0) / bound
    print(f"carried values, a = {a}, exact = {exact}: after 400 attempts {int(ended.sum())} of {n} rays ended ({int((o['event'] == EV_CAPTURED).sum())} "
          f"captured), {int(accepted.min())} ... {int(accepted.max())} accepted steps; (s0, c0) drift at most {drift.max():.3f} of 3 u per step "
          f"({err.max() / sb.U64:.2f} u), |s0^2 + c0^2 - 1| {norm.max():.3f} of it")
    record(f"carried_a{a}_exact{int(exact)}", dict(ended=int(ended.sum()), accepted_max=int(accepted.max()), drift_of_bound=drift.max(),
                                                   drift_u=err.max() / sb.U64, norm_of_bound=norm.max()))
    assert accepted.max() >= 50 and np.median(accepted) >= 20 and (o["event"] == EV_CAPTURED).sum() >= 10 and (o["event"] == EV_ESCAPED).sum() >= 10
    assert drift.max() <= 1.0 and norm.max() <= 1.0


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("a", [0.5, 0.998, 1.0])
def test_carried_k1_is_the_right_hand_side_at_the_carried_state(a, exact):
    """After 400 attempts the carried k1 lies within 2 K_REF 2^-53 S of ref_rhs_longdouble at the state it belongs to
    (the rays and the chain of the test above).  Measured: 9.4 units (dp_theta), bound 26.

    What this test found: with the candidate's (sn, cn) rotated from the step's base like a stage's, dphi and dp_theta of
    the carried k1 reached 706 and 1 062 units at a = 0.5 and 26 192 at a = 1, on the 39 % of rays that cross the equator
    (23 011 units at theta = pi/2 - 1.0e-4 after 101 accepted steps) or pass the axis (1 668 at theta = 1.8e-3).  The
    carried pair was inside its bound -- 8.6 to 12.8 u after 28 to 381 accepted steps -- but that is an ABSOLUTE error,
    and 1e-15 absolute on a cosine of 1e-4 is 1e5 units of S, which takes sin and cos as good to their own relative
    precision.  attempt() now takes the candidate's (sn, cn) from its angle (one sincos in place of one rotation per
    attempt; the six stages still rotate): the carried pair is a fresh sincos, 0.7 u from mpmath's, on every step."""
    c = carried_chain(a, exact)
    k1, base, L = c["chain"][400]["k1"], c["base"], c["L"]
    S = sb.scales(a, base, L)
    with np.errstate(invalid="ignore", divide="ignore"):
        ek = np.abs(k1.astype(sb.LD) - sb.ref_rhs_longdouble(a, base, L)).astype(np.float64) / (sb.U64 * S)
    worst = np.nanmax(ek, axis=0)
    print(f"carried k1, a = {a}, exact = {exact}: per component {np.round(worst, 2)} 2^-53 S")
    record(f"carried_k1_a{a}_exact{int(exact)}", worst.tolist())
    assert worst.max() <= 2 * sb.K_REF, worst
