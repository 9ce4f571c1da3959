"""Where the bounds of tests/test_gpu_dp45_blocks.py come from, on the CPU, from the oracle and longdouble alone
(tests/dp45_blocks.py states the units, the classes, the step sizes and the exclusions).

One attempt of the float64 oracle's DP45 loop (oracle.dp45_attempt: the function its tracer runs) against the same statements
in longdouble, on the accepted and the rejected row of every class at every spin:

    K_ATT64 = 5   candidate state, in its unit (measured 4.69: accepted row of `cut_graze` at a = 0.5)
    K_ERR64 = 33  error norm, in its unit (measured 32.34: rejected row of `turn` at a = 0.5)

Each is asserted from both sides: the measured maximum lies in (K - 1, K].  No class leaves out more than 2 % of its states.
The oracle's accept / reject decisions are the longdouble's wherever the longdouble error norm is farther from 1 than
K_ERR64 units.  The reference's min / max on a NaN, which the oracle's decision and the kernels' clamps are held to.  The
statements of pow_minus_tenth emulated in numpy, one float32 in 16 of [1e-30, 1e30] and every one within 2^12 of a power of
two (every float32 takes minutes in numpy; the GPU test sweeps them all): POW_TENTH_REL.
"""
import math

import numpy as np

import dp45_blocks as db
import step_blocks as sb
from oracle import oracle

COMPONENTS = ("r", "theta", "phi", "p_r", "p_theta")


def test_oracle_attempt_against_longdouble_in_the_units():
    worst_att, worst_err, at_att, at_err = 0.0, 0.0, None, None
    disagree = checked = 0
    for a in sb.SPINS:
        for name in db.CLASSES:
            c = db.dp45_set(a, name)
            if c is None:
                assert (name == "near" and a > 0.9) or (name in db.CHECKED_CLASSES and a > 0.9)
                continue
            for kind in ("accepted", "rejected"):
                r = c[kind]
                keep = r["keep"]
                left_out = 1.0 - keep.mean()
                assert left_out <= sb.EXCLUDED_CAP, (a, name, kind, left_out)  # (decided before any compared value is read)
                o = db.oracle_attempt(a, c["st"], c["L"], r["h"], c["refine"])
                assert (o["decision"] == 2).all() or kind == "rejected"
                usable = keep & (o["decision"] != 0)
                assert usable.sum() > 0.9 * db.N
                e = (np.abs(o["next"].astype(sb.LD) - r["next"]).astype(np.float64) / r["unit"])[usable]
                ee = (np.abs(o["err_norm"].astype(sb.LD) - r["err"]).astype(np.float64) / r["unit_err"])[usable]
                assert np.isfinite(e).all() and np.isfinite(ee).all() and e.max() > 0 and ee.max() > 0
                print(f"float64 oracle attempt, a = {a}, {name:13s} {kind:8s}: left out {100 * left_out:.2f} %, median h {np.median(r['h']):.3g}, "
                      f"median err_norm {float(np.median(r['err'])):.3g}; max error per component {np.round(e.max(axis=0), 2)} units, err_norm {ee.max():.2f} units")
                if e.max() > worst_att:
                    i = np.unravel_index(np.argmax(e), e.shape)
                    worst_att, at_att = e.max(), (a, name, kind, COMPONENTS[i[1]], c["st"][usable][i[0]].tolist(), float(c["L"][usable][i[0]]))
                if ee.max() > worst_err:
                    i = int(np.argmax(ee))
                    worst_err, at_err = ee.max(), (a, name, kind, c["st"][usable][i].tolist(), float(c["L"][usable][i]))
                # decisions: the oracle's is the longdouble's wherever the longdouble error norm is clear of the threshold
                clear = usable & (np.abs(r["err"].astype(np.float64) - 1.0) > db.K_ERR64 * r["unit_err"])
                want = np.where(r["err"].astype(np.float64) > 1.0, 1, 2)
                disagree += int((o["decision"][clear] != want[clear]).sum())
                checked += int(clear.sum())
                assert clear.sum() > 0.95 * usable.sum()
    print(f"K_att64: measured {worst_att:.2f} -> {math.ceil(worst_att)} at {at_att}")
    print(f"K_err64: measured {worst_err:.2f} -> {math.ceil(worst_err)} at {at_err}")
    print(f"decisions: {checked} rows clear of the threshold, {disagree} differ")
    assert db.K_ATT64 - 1 < worst_att <= db.K_ATT64
    assert db.K_ERR64 - 1 < worst_err <= db.K_ERR64
    assert checked > 50000 and disagree == 0


def test_classes_hold_what_they_are_for():
    """Both row kinds exist on both sides of the threshold; `cut_graze` and `turn` fail the branch-free attempt's validity
    test on part of their rows, the other classes on almost none (from the oracle's stage radii and the longdouble angles)."""
    accepted = rejected = 0
    for a in sb.SPINS[:3]:
        for name in db.CLASSES:
            c = db.dp45_set(a, name)
            for kind in ("accepted", "rejected") + (("first",) if name in db.CHECKED_CLASSES else ()):
                r = c[kind]
                o = db.oracle_attempt(a, c["st"], c["L"], r["h"], c["refine"])
                inside = (o["stage_r"] <= sb.r_cut(a)).any(axis=1)
                if kind == "first":
                    assert np.array_equal(r["h"], np.maximum(1.0, 0.01 * c["st"][:, 0]))
                    assert name != "cut_graze" or inside.sum() > 0.9 * db.N, (a, inside.sum())
                    continue
                accepted += int((o["decision"] == 2).sum())
                rejected += int((o["decision"] == 1).sum())
                turned = np.abs(r["next"][:, 1].astype(np.float64) - c["st"][:, 1]) > 0.25
                if name == "turn" and kind == "rejected":
                    assert turned.sum() > 500, (a, turned.sum())
                if name in ("far", "mid", "far_large"):
                    assert not inside.any()
    assert accepted > 10 * db.N and rejected > 10 * db.N


def test_h_comes_from_the_oracle_alone():
    """The accepted row's h is accepted by the oracle and is max(1, 0.01 r) times the oracle's own factors."""
    a, name = 0.9, "band"
    st, L, rf = db.dp45_class(name, a)
    refine = np.full(db.N, rf, dtype=np.uint8)
    h = db.accepted_h(a, st, L, refine)
    assert (db.oracle_attempt(a, st, L, h, refine)["decision"] == 2).all()
    h0 = np.maximum(1.0, 0.01 * st[:, 0])
    o = db.oracle_attempt(a, st, L, h0, refine)
    first = o["decision"] == 2
    assert first.any() and (~first).any() and np.array_equal(h[first], h0[first]) and (h[~first] < h0[~first]).all()
    assert np.array_equal(db.dp45_set(a, name)["accepted"]["h"], h) and np.array_equal(db.dp45_set(a, name)["rejected"]["h"], 3.0 * h)


def test_nan_semantics_of_the_controllers_clamps():
    """The truth: the reference's expressions (metrics.py:518, :564) are plain Python min / max on floats, and those return
    their FIRST argument unless the second compares beyond it.  The oracle's decision is held to that (its rmin / rmax
    return the NaN); the kernels' fmax / fmin are, in tests/test_gpu_dp45_blocks.py."""
    nan = float("nan")
    assert max(0.2, nan) == 0.2 and min(5.0, nan) == 5.0
    assert max(0.2, 0.9 * nan ** (-0.2)) == 0.2 and min(5.0, 0.9 * nan ** (-0.2)) == 5.0
    assert not (nan > 1.0) and not (nan < 1e-10)  # metrics.py:516, :561: a NaN error norm is accepted and not `tiny`
    for f32 in (False, True):
        e = np.array([nan, np.inf, 0.0, 1e-11, 0.5, 1.0, np.nextafter(1.0, 2.0), 2.0, 1e300 if not f32 else 1e30])
        h = np.full(e.size, 0.75)
        dec, hn = oracle.dp45_decide(e, h, f32=f32)
        want_dec, want_h = [], []
        for x in e.astype(np.float32 if f32 else np.float64).astype(np.float64):
            x = float(x)
            if x > 1.0:
                want_dec.append(1)
                want_h.append(0.75 * max(0.2, 0.9 * x ** (-0.2)))
            else:
                want_dec.append(2)
                want_h.append(0.75 * 5.0 if x < 1e-10 else 0.75 * min(5.0, 0.9 * (x ** (-0.2) if x > 0 else math.inf)))
        assert dec.tolist() == want_dec
        assert np.allclose(hn, want_h, rtol=1e-6 if f32 else 1e-15, atol=0) and np.isfinite(hn).all() and (hn > 0).all()
        t = np.float32 if f32 else np.float64
        assert dec[0] == 2 and hn[0] == 0.75 * 5.0 and dec[1] == 1 and hn[1] == t(0.75) * t(0.2)


def _sweep_bits():
    lo, hi = int(np.float32(1e-30).view(np.uint32)), int(np.float32(1e30).view(np.uint32))
    step = 16 << 24
    for b in range(lo, hi + 1, step):
        yield np.arange(b, min(hi + 1, b + step), 16, dtype=np.uint32)
    e = np.arange((lo >> 23) + 1, (hi >> 23) + 1, dtype=np.int64) << 23
    near = (e[:, None] + np.arange(-(1 << 12), (1 << 12) + 1)[None, :]).ravel()
    yield near[(near >= lo) & (near <= hi)].astype(np.uint32)


def test_pow_minus_tenth_statements_emulated():
    worst, at, count = 0.0, None, 0
    for bits in _sweep_bits():
        z = bits.view(np.float32)
        y = db.pow_minus_tenth_emulated(z)
        assert np.isfinite(y).all() and (y > 0).all()
        want = z.astype(np.float64) ** -0.1
        rel = np.abs(y.astype(np.float64) - want) / want
        i = int(np.argmax(rel))
        if rel[i] > worst:
            worst, at = float(rel[i]), float(z[i])
        count += z.size
    print(f"pow_minus_tenth emulated, {count} arguments in [1e-30, 1e30]: max relative error {worst:.3e} at z = {at!r}")
    assert count > 1.0e8
    assert 1.5e-7 < worst <= db.POW_TENTH_REL
    # outside the domain: what advance() must keep out of h (lt_dp45.hpp)
    out = db.pow_minus_tenth_emulated(np.array([0.0, 1e-45, np.inf, np.nan], dtype=np.float32))
    assert np.isnan(out).all()
    edge = db.pow_minus_tenth_emulated(np.array([1.1754944e-38, 3.4028235e38], dtype=np.float32)).astype(np.float64)
    assert np.allclose(edge, np.array([1.1754944e-38, 3.4028235e38]) ** -0.1, rtol=1e-6)


def test_longdouble_attempt_restates_the_reference():
    """ref_attempt_longdouble against an independent float64 restatement of metrics.py:464-514 on the oracle's right-hand
    side: the two agree to float64 rounding (a slip in a coefficient or a stage shows as 1e-3 and more)."""
    a = 0.9
    c = db.dp45_set(a, "mid")
    st, L, h = c["st"][:200], c["L"][:200], c["accepted"]["h"][:200]
    rhs = lambda y: oracle.kerr_rhs_n(y, L, sb.M, a)
    k1 = rhs(st)
    hh = h[:, None]
    k2 = rhs(st + hh * (1 / 5) * k1)
    k3 = rhs(st + hh * (3 / 40 * k1 + 9 / 40 * k2))
    k4 = rhs(st + hh * (44 / 45 * k1 - 56 / 15 * k2 + 32 / 9 * k3))
    k5 = rhs(st + hh * (19372 / 6561 * k1 - 25360 / 2187 * k2 + 64448 / 6561 * k3 - 212 / 729 * k4))
    k6 = rhs(st + hh * (9017 / 3168 * k1 - 355 / 33 * k2 + 46732 / 5247 * k3 + 49 / 176 * k4 - 5103 / 18656 * k5))
    nxt = st + hh * (35 / 384 * k1 + 500 / 1113 * k3 + 125 / 192 * k4 - 2187 / 6784 * k5 + 11 / 84 * k6)
    k7 = rhs(nxt)
    e = hh * (71 / 57600 * k1 - 71 / 16695 * k3 + 71 / 1920 * k4 - 17253 / 339200 * k5 + 22 / 525 * k6 - 1 / 40 * k7)
    err = np.sqrt(((e / (1e-8 + 1e-6 * np.maximum(np.abs(st), np.abs(nxt)))) ** 2).sum(axis=1) / 5)
    got = db.ref_attempt_longdouble(a, st, L, h, c["refine"][:200])
    assert np.abs(got[0].astype(np.float64) - nxt).max() < 1e-12 and np.abs(got[1].astype(np.float64) - k7).max() < 1e-12
    assert np.allclose(got[2].astype(np.float64), err, rtol=1e-4, atol=1e-9)
    o = db.oracle_attempt(a, st, L, h, c["refine"][:200])
    assert np.array_equal(o["next"], nxt) or np.abs(o["next"] - nxt).max() < 1e-13
