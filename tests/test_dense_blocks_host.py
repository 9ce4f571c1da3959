"""The units and bounds of tests/dense_blocks.py, derived on the CPU from the reference's restatements alone: every K the GPU tests
of the dense-trajectory path hold the device to (tests/test_gpu_dense_blocks.py), the exclusion caps, the replay of the oracle's own
records (every step, every decision, every attempt), and the replay's negative controls."""
import numpy as np
import pytest

import dense_blocks as db
from oracle import oracle

_CACHE = {}


def _batch(kind, a, sharp=False):
    """The oracle's records of one seeded batch and their replay, computed once and not changed afterwards."""
    key = (kind, a, sharp)
    if key not in _CACHE:
        if sharp:
            kw = dict(lambda_max=db.SHARP_LAMBDA_MAX, **db.SHARP_TOL)
            s0 = db.sharp_turn_states(kind, a)
        else:
            kw = {}
            s0 = db.seeded_states(kind, a)
        rec = db.oracle_records(kind, a, s0, **kw)
        rp = db.replay(kind, a, *rec, k_att=db.K_ATT["sharp" if sharp else "seeded"], k_err=db.K_ERR, **kw)
        Y0 = rp["Y0"]
        f0 = oracle.rhs8_n(kind, db.M, a, Y0)
        att = oracle.dense_attempt(kind, db.M, a, Y0, f0, rp["h"], **({k: kw[k] for k in ("rtol", "atol")} if sharp else {}))
        _CACHE[key] = dict(rec=rec, rp=rp, f0=f0, att=att, kw=kw, s0=s0)
    return _CACHE[key]


BATCHES = [(k, a, False) for k, a in db.SPINS] + [(0, 0.0, True), (1, 0.9, True)]


def test_restated_blocks_are_the_oracles_loop():
    """The exported blocks ARE what lto_integrate_dense runs: a record's next point, bit for bit, from oracle.dense_attempt at the
    record's own (y_p, h_p); its first step from oracle.dense_initial_step; its event point from oracle.dense_event."""
    b = _batch(1, 0.9)
    rp, att, rec = b["rp"], b["att"], b["rec"]
    reg = ~rp["is_event"]
    assert np.array_equal(att["y_new"][reg], rp["Y1"][reg])
    fi = rp["first"]
    h0 = oracle.dense_initial_step(1, db.M, 0.9, rp["Y0"][fi], b["f0"][fi])
    assert np.array_equal(h0, rp["h"][fi])  # (no first attempt of this batch is rejected; the clamp at max_step is not reached)
    t, y, count, status = rec[:4]
    for i in (0, 5, 77):
        c = count[i]
        row = np.flatnonzero((rp["track"] == i) & rp["is_event"])[0]
        radius = db.r_capture(0.9) if status[i] == 1 else 2 * y[i, 0, 1]
        te, ye = oracle.dense_event(y[i, c - 2], t[i, c - 2], rp["h"][row], att["Q"][row], radius, t[i, c])
        assert te == t[i, c - 1] and np.array_equal(ye, y[i, c - 1])


@pytest.mark.parametrize("name", db.RHS_CLASSES)
def test_k_of_the_right_hand_side(name):
    worst, where = 0.0, None
    for kind, a in db.RHS_SPINS:
        st = db.rhs_class(name, kind, a)
        got = oracle.rhs8_n(kind, db.M, a, st)
        ratio = db.rhs_ratio(kind, a, st, got)
        keep = np.isfinite(got).all(axis=1)
        assert (~keep).mean() <= db.EXCLUDED_CAP
        assert (got[:, [4, 7]] == 0).all() and not np.signbit(got[:, [4, 7]]).any()
        ratio = ratio[:, list(db.NONCYCLIC)]
        m = np.max(ratio[keep], axis=0)
        print(f"float64 right-hand side, kind {kind} a = {a:5}, {name:12s}: {np.round(m, 2)} units")
        if np.nanmax(m) > worst:
            i = int(np.nanargmax(np.nan_to_num(ratio).max(axis=1)))
            worst, where = float(np.nanmax(m)), (kind, a, st[i].tolist())
    print(f"{name}: worst {worst:.3f} units at {where}")
    assert int(np.ceil(worst)) == db.K_RHS8[name], worst


def test_edge_rows_of_the_right_hand_side():
    """Zero at and inside 1.001 r_plus, r = r_zero itself included; sin theta = 0 in the Kerr kind: the restatement is non-finite
    where the oracle is."""
    for kind, a in db.RHS_SPINS:
        st = db.rhs_class("far", kind, a, 64)
        rz = db.r_zero(a if kind else 0.0)
        st[:, 1] = np.linspace(0.3 * rz, rz, 64)
        st[-1, 1] = rz
        st[-2, 1] = np.nextafter(rz, 0)
        assert (oracle.rhs8_n(kind, db.M, a, st) == 0).all() and (db.rhs8_ld(kind, a, st) == 0).all()
        st[:, 1] = np.nextafter(rz, np.inf)
        assert (oracle.rhs8_n(kind, db.M, a, st)[:, 1:3] != 0).any()
        if kind:
            st = db.rhs_class("far", kind, a, 64)
            st[:, 2] = 0.0
            got, ref = oracle.rhs8_n(kind, db.M, a, st), db.rhs8_ld(kind, a, st).astype(np.float64)
            assert (np.isfinite(got) == np.isfinite(ref)).all() and not np.isfinite(got[:, [3, 5, 6]]).any()


def test_k_of_one_attempt_and_every_step_of_the_oracles_records():
    worst = dict(seeded=0.0, sharp=0.0)
    for kind, a, sharp in BATCHES:
        b = _batch(kind, a, sharp)
        rp = b["rp"]
        keep, ratio = rp["keep"], rp["ratio"]
        reg = ~rp["is_event"]
        assert (~keep[reg]).mean() <= db.EXCLUDED_CAP, (kind, a, sharp)
        cl = db.classify(rp["blk"], rp["Y0"], rp["Y1"])
        m = np.max(ratio[keep][:, list(db.NONCYCLIC)], axis=0)
        print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: {int(keep.sum())} steps, {int((~keep[reg]).sum())} left out, "
              f"worst per component {np.round(m, 2)}; per class "
              + ", ".join(f"{c} {int((v & keep).sum())}: {np.nanmax(ratio[v & keep]) if (v & keep).any() else 0:.2f}" for c, v in cl.items()))
        key = "sharp" if sharp else "seeded"
        if np.nanmax(m) > worst[key]:
            i = int(np.argmax(np.where(keep, np.nan_to_num(ratio).max(axis=1), 0)))
            worst[key] = float(np.nanmax(m))
            print(f"    worst row: y {rp['Y0'][i].tolist()} h {rp['h'][i]!r}")
        assert rp["cyclic_ok"].all()
        if sharp:
            assert (cl["sharp"] & keep).sum() >= 16
    for key in worst:
        assert int(np.ceil(worst[key])) == db.K_ATT[key], worst


def test_k_of_the_error_norm():
    worst = 0.0
    for kind, a, sharp in BATCHES:
        b = _batch(kind, a, sharp)
        blk, att = b["rp"]["blk"], b["att"]
        keep = blk["keep"]
        e = np.abs(att["err"].astype(db.LD) - blk["err"]).astype(np.float64) / blk["unit_err"]
        i = int(np.argmax(np.where(keep, e, 0)))
        print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: error norm {e[keep].max():.2f} units (y {b['rp']['Y0'][i].tolist()} h {b['rp']['h'][i]!r}); "
              f"nearest accepted err to 1: {np.min(np.abs(att['err'][keep] - 1)):.1e}")
        worst = max(worst, float(e[keep].max()))
    assert int(np.ceil(worst)) == db.K_ERR, worst


def test_k_of_the_initial_step():
    worst = 0.0
    for kind, a, sharp in BATCHES:
        b = _batch(kind, a, sharp)
        rp = b["rp"]
        fi = rp["first"]
        kw = {k: v for k, v in b["kw"].items()}
        h0 = oracle.dense_initial_step(kind, db.M, a, rp["Y0"][fi], b["f0"][fi], **kw)
        e = np.abs(h0.astype(db.LD) - rp["h0"]).astype(np.float64) / rp["unit_h0"][fi]
        print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: initial step {h0.min():.3e} ... {h0.max():.3e}, {e.max():.2f} units")
        worst = max(worst, float(e.max()))
    assert int(np.ceil(worst)) == db.K_H0, worst


def test_k_of_the_event():
    worst, kinds = 0.0, set()
    for kind, a, sharp in BATCHES:
        b = _batch(kind, a, sharp)
        ev = db.event_check(kind, a, *b["rec"][:4], **{k: v for k, v in b["kw"].items() if k != "max_step"})
        keep = ev["keep"]
        assert ev["ordered"].all() and ev["cyclic_ok"].all()
        if not sharp:
            assert (~keep).mean() <= db.EXCLUDED_CAP
        if keep.any():
            ye, root = np.nanmax(ev["ratio_ye"][keep]), np.max((ev["resid"] / ev["unit_root"])[keep])
            print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: {int(keep.sum())} events, ye {ye:.2f} units, root residual {root:.2f} units")
            worst = max(worst, float(ye), float(root))
            kinds |= set(ev["status"][keep].tolist())
    assert kinds == {1, 2}
    assert int(np.ceil(worst)) == db.K_EVENT, worst


def test_every_decision_and_attempt_of_the_oracles_records_is_reproduced():
    n_rej = n_clamp = 0
    for kind, a, sharp in BATCHES:
        b = _batch(kind, a, sharp)
        rp = b["rp"]
        v = db.verdict(rp, db.K_ATT["sharp" if sharp else "seeded"], db.K_H0)
        d = (np.abs(rp["h"] - rp["h_replay"]) / (rp["h_allow"] + db.K_H0 * rp["unit_h0"]))[rp["h_keep"]]
        known = rp["attempts_known"]
        print(f"kind {kind} a = {a:5} {'sharp ' if sharp else 'seeded'}: {v}; step sizes {int(rp['h_keep'].sum())} of {rp['h_keep'].size} held, worst "
              f"{d.max():.3f} of the allowance; {int(rp['rejected'].sum())} steps after a rejection, {int(rp['clamped'].sum())} clamped at max_step; "
              f"attempts {int(rp['attempts_sum'].sum())} on {int(known.sum())} of {known.size} tracks")
        assert v == dict(steps=0, sizes=0, cyclic=0, accepts=0, attempts=0), v
        assert (~rp["h_keep"]).mean() <= db.EXCLUDED_CAP
        # (the cap is on decisions; a track counts once every one of its decisions does: all 128 of a seeded batch do, and a
        # sharp batch -- seven steps a track at a loose tolerance -- may lose a track to one decision near 1)
        assert known.all() if not sharp else known.mean() >= 0.9
        n_rej += int(rp["rejected"].sum())
        n_clamp += int(rp["clamped"].sum())
    assert n_rej > 1000 and n_clamp > 10000


# ---- negative controls: the replay fails when it should ----------------------------------------------------------------------------
def _replayed(rec):
    return db.replay(1, 0.9, *rec, k_att=db.K_ATT["seeded"], k_err=db.K_ERR)


def _small():
    b = _batch(1, 0.9)
    return [x[:4].copy() for x in b["rec"]], b["rp"]


def test_control_one_element_moved_by_three_bounds_is_flagged():
    rec, rp = _small()
    row = np.flatnonzero((rp["track"] == 2) & (rp["p"] == 40))[0]
    for c in db.NONCYCLIC:
        moved = [x.copy() for x in rec]
        moved[1][2, 41, c] += 3.0 * db.K_ATT["seeded"] * rp["blk"]["unit"][row, c]
        v = db.verdict(_replayed(moved), db.K_ATT["seeded"], db.K_H0)
        assert v["steps"] >= 1, (c, v)
    assert db.verdict(_replayed(rec), db.K_ATT["seeded"], db.K_H0)["steps"] == 0


def test_control_one_point_dropped_is_flagged():
    rec, _ = _small()
    t, y, count = rec[0], rec[1], rec[2]
    c = count[1]
    t[1, 30:c] = t[1, 31:c + 1]  # (the t_new slot moves along)
    y[1, 30:c - 1] = y[1, 31:c]
    count[1] = c - 1
    v = db.verdict(_replayed(rec), db.K_ATT["seeded"], db.K_H0)
    assert v["steps"] >= 1 and (v["sizes"] >= 1 or v["attempts"] >= 1), v


def test_control_one_step_size_scaled_is_flagged():
    rec, rp = _small()
    # a step the controller chose (not clamped at max_step): the replay's size is then the controller's own
    rows = np.flatnonzero((rp["track"] == 3) & ~rp["clamped"] & (rp["p"] > 5) & ~rp["is_event"] & rp["h_keep"])
    p = int(rp["p"][rows[0]])
    t = rec[0]
    c = rec[2][3]
    shift = 0.01 * (t[3, p + 1] - t[3, p])
    t[3, p + 1:c + 1] -= shift
    out = _replayed(rec)
    row = np.flatnonzero((out["track"] == 3) & (out["p"] == p))[0]
    assert out["h_keep"][row] and abs(out["h"][row] - out["h_replay"][row]) > out["h_allow"][row]
    v = db.verdict(out, db.K_ATT["seeded"], db.K_H0)
    assert v["sizes"] >= 1 and v["steps"] >= 1, v
