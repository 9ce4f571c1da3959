"""The time a stored hit carries, block by block on the device: the rates and the step rule in their units
(lt_time_rates_probe, lt_step_time_probe) against longdouble; one iteration of the timed lane against its parts, the carried
lane, the two-term sum and the production kernels against the probe (lt_disk_timed_advance_probe), as bit identities between
device outputs and numpy replays of add / subtract sequences.  tests/hit_blocks.py states the units, the classes and the
bound on the sum; tests/test_hit_blocks_host.py derives every K on the CPU.  A device block is held to 2 K.

With LT_HIT_BLOCKS_MEASURE=path the figures the tests print are also written there as JSON (profiles/hit_blocks_<build id>.json).
"""
import os

import numpy as np
import pytest

import disk_blocks as dk
import dp45_blocks as db
import hit_blocks as hb
import ltrace
import ray_ends as re_

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_HIT_BLOCKS_MEASURE")
_RECORD = {}
KERR = ltrace.METRIC_KERR
INTEGRATORS = {"rk4_f32": (ltrace.INTEGRATOR_RK4, 32, False), "rk4_f64": (ltrace.INTEGRATOR_RK4, 64, False),
               "dp45_exact": (ltrace.INTEGRATOR_DP45_EXACT, 64, True)}
COLS = [0, 1, 3, 4]  # (r, theta, p_r, p_theta) of a state (r, theta, phi, p_r, p_theta)
MAX_IMAGES = 2
CARRY = ("lam", "h", "steps", "k1", "sc", "t_hi", "t_lo", "rate", "have", "n")
SHARED = ("event", "steps", "iters", "state", "lam", "h", "k1", "sc", "t_hi", "t_lo", "rate", "have", "n", "img", "tim", "trace")


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


def same(x, y):
    if x is None or y is None:
        return x is None and y is None
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def metric_of(M, a):
    return ltrace.Metric(KERR, 0, M, a)


# ---- 1. the rates and the step rule in their units ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_rates_in_their_units(precision):
    worst, per_class = np.zeros(3), {}
    for spin, name, c in hb.rate_classes():
        unit, keep = hb.rate_units(c["M"], c["a"], c["L"], c["y"], precision)
        ref = hb.rates_ld(c["M"], c["a"], c["L"], c["y"])
        got = ltrace.time_rates_probe(metric_of(c["M"], c["a"]), c["L"], c["y"], precision)
        e = (np.abs(got.astype(hb.LD) - ref).astype(np.float64) / unit)[keep]
        rel = np.max(np.abs(got[keep, 0] / ref[keep, 0].astype(np.float64) - 1))
        print(f"float{precision} rates, a = {spin:6}, {name:8s}: {np.round(e.max(axis=0), 2)} units (t', r', theta'); t' relative {rel:.1e}")
        per_class[f"{spin}/{name}"] = e.max(axis=0).tolist() + [float(rel)]
        assert e.max() <= 2 * hb.k_rate(precision), (spin, name, e.max(axis=0))
        worst = np.maximum(worst, e.max(axis=0))
    print(f"float{precision} rates: {np.round(worst, 2)} units (bound {2 * hb.k_rate(precision)})")
    record(f"rates_f{precision}", dict(worst=worst.tolist(), per_class=per_class))


@pytest.mark.parametrize("precision", [64, 32])
def test_step_rule_in_its_unit(precision):
    worst, per_class = 0.0, {}
    for spin, name, c in hb.step_classes(precision):
        ref, keep = c["ref"], c["ref"]["keep"]
        got = ltrace.step_time_probe(metric_of(c["M"], c["a"]), c["L"], c["y0"], c["y1"], c["h"], c["tau"], precision)
        e = (np.abs(got.astype(hb.LD) - ref["dt"]).astype(np.float64) / ref["unit"])[keep]
        by_tau = [float(e[(np.arange(keep.size) % 4 == k)[keep]].max()) for k in range(4)]
        rel = np.max(np.abs(got[keep] / ref["dt"][keep].astype(np.float64) - 1))
        print(f"float{precision} step rule, a = {spin:6}, {name:22s}: {e.max():.2f} units (tau {hb.TAUS}: {np.round(by_tau, 2)}); relative {rel:.1e}")
        per_class[f"{spin}/{name}"] = by_tau + [float(rel)]
        i = np.nonzero(keep)[0][int(np.argmax(e))]
        assert e.max() <= 2 * hb.k_dt(precision), (spin, name, e.max(), int(i), c["y0"][i].tolist(), c["y1"][i].tolist(), float(c["L"][i]),
                                                   float(c["h"][i]), float(c["tau"][i]), got[i], float(ref["dt"][i]))
        worst = max(worst, float(e.max()))
    print(f"float{precision} step rule: {worst:.2f} units (bound {2 * hb.k_dt(precision)})")
    record(f"step_rule_f{precision}", dict(worst=worst, per_class=per_class))


@pytest.mark.parametrize("precision", [64, 32])
def test_step_rule_edge_rows(precision):
    """h = 0: the rule is (tau h) / 6 (...), an exact 0 on finite states, as disk.step_time's.  On a NaN state the reference
    says 0 (it tests h first) and the device's unguarded function NaN (0 x NaN); the contract is the lane's, which never calls
    the rule with h = 0 (it adds an exact 0: test_one_iteration_against_its_parts) -- pinned here so that a change shows.
    NaN in any input: NaN out."""
    c = hb.step_class("crossing", "ordinary", 0.9, precision)
    met = metric_of(c["M"], c["a"])
    n = 64
    y0, y1, L, h, tau = c["y0"][:n].copy(), c["y1"][:n].copy(), c["L"][:n], c["h"][:n], c["tau"][:n]
    zero = ltrace.step_time_probe(met, L, y0, y1, 0.0, tau, precision)
    assert (zero == 0.0).all() and not np.signbit(zero).any()
    k = np.arange(n)
    y0[k[k % 2 == 0], (k[k % 2 == 0] // 2) % 4] = np.nan
    y1[k[k % 2 == 1], (k[k % 2 == 1] // 2) % 4] = np.nan
    assert np.isnan(ltrace.step_time_probe(met, L, y0, y1, h, tau, precision)).all()
    assert np.isnan(ltrace.step_time_probe(met, L, y0, y1, 0.0, tau, precision)).all()
    assert np.isnan(ltrace.step_time_probe(met, L, c["y0"][:n], c["y1"][:n], np.nan, tau, precision)).all()
    assert np.isnan(ltrace.step_time_probe(met, L, c["y0"][:n], c["y1"][:n], h, np.nan, precision)).all()
    assert np.isnan(ltrace.time_rates_probe(met, L, y0, precision)).any(axis=1)[k % 2 == 0].all()


# ---- 2. one iteration against its parts ---------------------------------------------------------------------------------------------------
def iteration_rows(kind):
    """-> (label, dict(M, a, st (n,5), L, lam, h (RK4: h_retry; DP45: the step size), refine, r_in, r_out, r_obs)) per set of rows."""
    integ, precision, dp45 = INTEGRATORS[kind]
    for a in dk.SPINS:
        for name in dk.ADVANCE_CLASSES:
            c = dk.crossing_class(name, a, precision)
            if c is None:
                continue
            h = dk.accepted_dp45_h(c) if dp45 else 0.0
            yield f"{name}/{a}", dict(M=c["M"], a=c["a"], st=c["y0"], L=c["L"], lam=0.0, h=h, refine=0, r_in=c["r_in_arg"], r_out=c["r_out"],
                                     r_obs=c["r_obs"])
    if dp45:
        c = dk.dp45_capture_class()
        yield "dp45_capture", dict(M=c["M"], a=c["a"], st=c["y0"], L=c["L"], lam=0.0, h=c["h"], refine=0, r_in=0.0, r_out=c["r_out"], r_obs=c["r_obs"])
        for a in (0.9, 0.998):
            for name in ("mid", "band"):
                r = db.dp45_rows(a, name)
                for rows in ("accepted", "rejected"):
                    yield f"dp45_{rows}/{name}/{a}", dict(M=1.0, a=a, st=r["st"], L=r["L"], lam=0.0, h=r[rows]["h"], refine=r["refine"], r_in=0.0,
                                                          r_out=20.0, r_obs=db.R_OBS)
    else:
        for a in re_.RK4_SPINS:  # the decision table: retries, the range end, the shorter last step, chords, failures
            t = re_.rk4_table(a, f32=precision == 32, variants=4)
            yield f"rk4_table/{a}", dict(M=1.0, a=a, st=t["st"], L=t["L"], lam=t["lam"], h=0.0, refine=t["refine"], r_in=0.0, r_out=20.0,
                                         r_obs=re_.RK4_R_OBS)


def lane_inputs(met, rows, precision):
    """A lane in mid-ray: an elapsed time with both words set, a hit count of 0, 1 or 2 (2: the slots are full), and the rates
    either carried (odd rows: the device's own at the state) or not yet set."""
    n = rows["st"].shape[0]
    k = np.arange(n)
    t_hi = dk.as_t(137.0 + 0.37 * (k % 11), precision)
    t_lo = dk.as_t(t_hi * dk.u_of(precision) * 0.3 * ((k % 5) - 2), precision)
    have = k % 2 == 1
    rate = ltrace.time_rates_probe(met, rows["L"], rows["st"][:, COLS], precision)
    return dict(t_hi=t_hi, t_lo=t_lo, have=have, rate=np.where(have[:, None], rate, 0.0), n=(k % 3).astype(np.int32))


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_one_iteration_against_its_parts(kind):
    integ, precision, dp45 = INTEGRATORS[kind]
    T = hb.dtype_of(precision)
    count = dict(rows=0, moved=0, still=0, hits=0, stored=0, full=0, terminal_hits=0)
    for label, r in iteration_rows(kind):
        met = metric_of(r["M"], r["a"])
        geo = dict(r_in=r["r_in"], r_out=r["r_out"], r_obs=r["r_obs"], lambda_max=dk.LAMBDA_MAX, h_max=1.0)
        args = (met, r["st"], r["L"], integ, precision)
        base = dict(lam=r["lam"], h=r["h"], refine=r["refine"])
        A = ltrace.disk_advance_probe(*args, act=True, **base, **geo)
        A0 = ltrace.disk_advance_probe(*args, act=False, **base, **geo)
        lane = lane_inputs(met, r, precision)
        run = lambda **kw: ltrace.disk_timed_advance_probe(*args, **base, **geo, **lane, max_images=MAX_IMAGES, iters=1, trace=True, **kw)
        P = run()
        n = r["st"].shape[0]
        lam_in = np.broadcast_to(dk.as_t(r["lam"], precision), (n,))
        # the integrator's side: every bit of disk_advance's; the event is the integrator's own (a thin disk's hit ends no ray)
        for key in ("state", "lam", "h", "steps"):
            assert same(P[key], A[key]), (kind, label, key)
        assert same(P["event"], A0["event"]), (kind, label)
        assert (P["iters"] == 1).all()
        hit = A["is_hit"]
        assert same(P["n"], lane["n"] + hit), (kind, label)
        # the time added: the rule on (y0, y1, h, 1) where lambda moved, an exact 0 where it did not
        moved = P["lam"] != lam_in
        h_cnt, dt = P["trace"][0, :, 4], P["trace"][0, :, 5]
        assert same(P["trace"][0, :, :4], P["state"][:, COLS]) and same(P["trace"][0, :, 6], P["n"])
        assert (h_cnt[~moved] == 0).all() and (dt[~moved] == 0).all() and not np.signbit(dt[~moved]).any(), (kind, label)
        assert same(h_cnt[hit & moved], A["on_h"][hit & moved]), (kind, label)  # (a hit on a step that ended the ray: lambda stays)
        still_lam0 = moved & (lam_in == 0)
        assert same(h_cnt[still_lam0], P["lam"][still_lam0]), (kind, label)  # (0 + h is h)
        rule = ltrace.step_time_probe(met, r["L"], r["st"][:, COLS], P["state"][:, COLS], h_cnt, 1.0, precision)
        assert same(dt[moved], rule[moved]), (kind, label, np.nonzero(moved & (dt != rule))[0][:8])
        hi, lo = hb.two_sum_replay(dt[None, :], T, lane["t_hi"], lane["t_lo"])
        assert same(P["t_hi"], hi) and same(P["t_lo"], lo), (kind, label)
        assert same(P["t_hi"][~moved], lane["t_hi"][~moved]) and same(P["t_lo"][~moved], lane["t_lo"][~moved])
        # the rates it hands on: those of the state it leaves, whatever came in
        assert P["have"].all()
        assert same(P["rate"], ltrace.time_rates_probe(met, r["L"], P["state"][:, COLS], precision)), (kind, label)
        # the records: slot n of a hit below max_images, and nothing else
        slot = lane["n"]
        stored = hit & (slot < MAX_IMAGES)
        part = ltrace.step_time_probe(met, r["L"], r["st"][:, COLS], A["on_y1"][:, COLS], A["on_h"], A["on_tau"], precision)
        with np.errstate(invalid="ignore"):
            want_t = (lane["t_hi"].astype(T) + (lane["t_lo"].astype(T) + part.astype(T))).astype(np.float64)
        for j in range(MAX_IMAGES):
            here = stored & (slot == j)
            assert same(P["img"][j, here, 0], A["hit"][here, 0]) and same(P["img"][j, here, 1], A["hit"][here, 2]), (kind, label, j)
            assert same(P["tim"][j, here], want_t[here]), (kind, label, j, np.nonzero(here & (P["tim"][j] != want_t))[0][:8])
            assert not np.isnan(P["tim"][j, here]).any()
            assert np.isnan(P["img"][j, ~here]).all() and np.isnan(P["tim"][j, ~here]).all(), (kind, label, j)
        assert np.isnan(P["mom"]).all()
        # act = 0 stores nothing, counts nothing and changes no other output
        Q = run(act=False)
        assert np.isnan(Q["img"]).all() and np.isnan(Q["tim"]).all() and same(Q["n"], lane["n"])
        for key in SHARED:
            if key not in ("img", "tim", "n", "trace"):
                assert same(Q[key], P[key]), (kind, label, key)
        assert same(Q["trace"][..., :6], P["trace"][..., :6])
        # the polarized lane: the same bits, and the hit's own momenta
        R = run(pol=True)
        for key in SHARED:
            assert same(R[key], P[key]), (kind, label, key)
        for j in range(MAX_IMAGES):
            here = stored & (slot == j)
            assert same(R["mom"][j, here], A["hit"][here][:, 3:]) and np.isnan(R["mom"][j, ~here]).all(), (kind, label, j)
        ended = np.isin(A0["event"], (ltrace.EV_CAPTURED, ltrace.EV_ESCAPED))
        count = {k: v + int(x) for (k, v), x in zip(count.items(), (n, moved.sum(), (~moved).sum(), hit.sum(), stored.sum(),
                                                                   (hit & ~stored).sum(), (stored & ended).sum()))}
    print(f"{kind}: {count}")
    record(f"iteration_{kind}", count)
    assert count["moved"] > 5000 and count["still"] >= 100 and count["stored"] > 2000 and count["full"] > 1000 and count["terminal_hits"] >= 10


# ---- the chains: every ray of a fan from the camera to its end ----------------------------------------------------------------------------
THETA_OBS = 1.4
_CHAIN = {}


def chain_fan(r_obs, r_out=20.0):
    """256 rays: 8 screen angles x (24 alphas over the disk's image and 8 impact parameters 4 ... 8 around the critical curve)."""
    ang = 0.2 + np.arange(8) * (2 * np.pi / 8)
    amax = 1.3 * np.arctan(r_out / r_obs)
    one = np.concatenate([np.linspace(0.05 * amax, amax, 24), np.arctan(np.linspace(4.0, 8.0, 8) / r_obs)])
    return np.tile(one, 8), np.repeat(ang, one.size)


def lam_max(r_obs):
    return max(5000.0, 6.0 * r_obs)


def chain_start(kind, a, r_obs):
    integ, precision, dp45 = INTEGRATORS[kind]
    al, th = chain_fan(r_obs)
    rec = ltrace.ic_probe(KERR, 1.0, a, r_obs, THETA_OBS, al, th, precision=precision)[:al.size]
    assert (rec[:, 3].astype(int) & ltrace.FLAG_OK).all() and not (rec[:, 3].astype(int) & ltrace.FLAG_REFINE).any()
    st = np.stack([np.full(al.size, r_obs), np.full(al.size, float(dk.as_t(THETA_OBS, precision))), np.zeros(al.size), rec[:, 0], rec[:, 1]], axis=1)
    h0 = max(1.0, 0.01 * r_obs) if dp45 else 0.0  # Dp45::start's first step size; RK4: nothing to retry
    return al, th, rec, st, h0


def chain(kind, a, r_obs=50.0, pol=False, iters=1 << 18, trace=False):
    """Every ray of the fan from its camera record to its end in ONE launch -- computed once, never changed."""
    key = (kind, a, r_obs, pol, iters, trace)
    if key not in _CHAIN:
        integ, precision, dp45 = INTEGRATORS[kind]
        al, th, rec, st, h0 = chain_start(kind, a, r_obs)
        out = ltrace.disk_timed_advance_probe(metric_of(1.0, a), st, rec[:, 2], integ, precision, pol=pol, h=h0, max_images=MAX_IMAGES, iters=iters,
                                              trace=trace, r_obs=r_obs, lambda_max=lam_max(r_obs))
        _CHAIN[key] = dict(al=al, th=th, rec=rec, st=st, h0=h0, out=out)
    return _CHAIN[key]


# ---- 3. the carried lane ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_the_carried_sum_is_the_two_sum_of_the_traced_terms(kind):
    _, precision, _ = INTEGRATORS[kind]
    o = chain(kind, 0.9, iters=400, trace=True)["out"]
    hi, lo = hb.two_sum_replay(o["trace"][:, :, 5], hb.dtype_of(precision))
    assert same(o["t_hi"], hi) and same(o["t_lo"], lo)
    assert (o["t_lo"] != 0).mean() > 0.9 and (o["iters"] > 10).all()
    counted = (o["trace"][:, :, 4] > 0).sum(axis=0)
    print(f"{kind}: {int(o['iters'].min())} ... {int(o['iters'].max())} iterations, {int(counted.min())} ... {int(counted.max())} of them counted")


@pytest.mark.parametrize("kind", list(INTEGRATORS))
@pytest.mark.parametrize("n_iters", [1, 16, 400])
def test_n_iterations_in_one_launch_equal_n_launches_of_one(kind, n_iters):
    integ, precision, dp45 = INTEGRATORS[kind]
    c = chain(kind, 0.9, pol=True, iters=n_iters, trace=True)
    one, rec, n = c["out"], c["rec"], c["st"].shape[0]
    met = metric_of(1.0, 0.9)
    cur = dict(state=c["st"], lam=np.zeros(n), h=np.full(n, c["h0"]), steps=np.zeros(n, dtype=np.uint32), k1=None, sc=None, t_hi=np.zeros(n),
               t_lo=np.zeros(n), rate=np.zeros((n, 3)), have=np.zeros(n, dtype=bool), n=np.zeros(n, dtype=np.int32))
    acc = dict(event=np.full(n, ltrace.EV_RUNNING, dtype=np.int32), iters=np.zeros(n, dtype=np.int32), img=np.full((MAX_IMAGES, n, 2), np.nan),
               tim=np.full((MAX_IMAGES, n), np.nan), mom=np.full((MAX_IMAGES, n, 2), np.nan), trace=np.full((n_iters, n, 7), np.nan))
    for it in range(n_iters):
        alive = acc["event"] == ltrace.EV_RUNNING
        if not alive.any():
            break
        o = ltrace.disk_timed_advance_probe(met, cur["state"], rec[:, 2], integ, precision, pol=True, max_images=MAX_IMAGES, iters=1, trace=True,
                                            r_obs=50.0, lambda_max=lam_max(50.0), **{k: cur[k] for k in CARRY})
        for k in ("state",) + CARRY:  # a row whose ray has ended stays as it ended
            if cur[k] is None:
                cur[k] = o[k].copy()
            else:
                cur[k] = np.where(alive.reshape((n,) + (1,) * (np.ndim(o[k]) - 1)), o[k], cur[k])
        acc["event"] = np.where(alive, o["event"], acc["event"])
        acc["iters"] += alive
        acc["trace"][it, alive] = o["trace"][0, alive]
        for k in ("img", "tim", "mom"):
            new = ~np.isnan(o[k]) & alive.reshape((1, n) + (1,) * (o[k].ndim - 2))
            assert np.isnan(acc[k][new]).all()  # a slot is written once
            acc[k] = np.where(new, o[k], acc[k])
    for k in ("state",) + CARRY:
        assert same(one[k], cur[k]), (kind, n_iters, k)
    for k in acc:
        assert same(one[k], acc[k]), (kind, n_iters, k)


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_a_timed_lane_does_not_depend_on_its_wavefront(kind):
    """The same row alone, as lane 37 among 63 lanes that are no candidates, and among 63 hit candidates: every bit equal."""
    integ, precision, dp45 = INTEGRATORS[kind]
    c = dk.crossing_class("ordinary", 0.9, precision)
    met = metric_of(c["M"], c["a"])
    hs = dk.accepted_dp45_h(c) if dp45 else np.zeros(dk.N)
    lane = lane_inputs(met, dict(st=c["y0"], L=c["L"]), precision)

    def run(rows):
        return ltrace.disk_timed_advance_probe(met, c["y0"][rows], c["L"][rows], integ, precision, pol=True, h=hs[rows], max_images=MAX_IMAGES,
                                               iters=1, trace=True, r_in=c["r_in_arg"], r_out=c["r_out"], r_obs=c["r_obs"],
                                               lambda_max=dk.LAMBDA_MAX, **{k: v[rows] for k, v in lane.items()})
    everything = run(np.arange(dk.N))
    hit_rows = np.nonzero(everything["n"] > lane["n"])[0]
    miss_rows = np.nonzero(everything["n"] == lane["n"])[0]
    assert hit_rows.size > 70 and miss_rows.size > 70
    keys = SHARED + ("mom",)
    for row in (int(hit_rows[3]), int(hit_rows[-1]), int(miss_rows[0])):
        alone = run(np.array([row]))
        for others in (miss_rows[miss_rows != row][:63], hit_rows[hit_rows != row][:63]):
            got = run(np.insert(others, 37, row))
            for k in keys:
                ax = 0 if got[k].shape[0] == 64 else 1
                assert same(np.take(got[k], [37], axis=ax), alone[k]), (kind, row, k)
                assert same(np.take(everything[k], [row], axis=ax), alone[k]), (kind, row, k)


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_the_polarized_lane_is_the_timed_lane(kind):
    a, b = chain(kind, 0.9, pol=False)["out"], chain(kind, 0.9, pol=True)["out"]
    for k in SHARED:
        assert same(a[k], b[k]), (kind, k)
    assert same(np.isnan(b["mom"][..., 0]), np.isnan(b["img"][..., 0])) and np.isnan(a["mom"]).all()


# ---- 4. the sum's quality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.9, 0.998])
def test_stored_float32_times_are_within_the_sums_bound(a):
    """Rays from r_obs = 600: >= 500 counted steps before the first hit (tests/test_hit_blocks_host.py shows on the oracle's
    rays that the plain float32 sum misses the bound there)."""
    r_obs = 600.0
    c = chain("rk4_f32", a, r_obs=r_obs, iters=2500, trace=True)
    o, rec = c["out"], c["rec"]
    met = metric_of(1.0, a)
    tr = o["trace"]
    n_after = np.nan_to_num(tr[:, :, 6], nan=1e9)
    rays = worst = missed = 0
    ratio = []
    for j in range(MAX_IMAGES):
        rows = np.nonzero(~np.isnan(o["tim"][j]))[0]
        k = np.argmax(n_after[:, rows] >= j + 1, axis=0)        # the iteration that stored slot j
        assert (k >= hb.MIN_SUM_STEPS).all()
        y0 = tr[k - 1, rows, :4]
        st = np.stack([y0[:, 0], y0[:, 1], np.zeros(rows.size), y0[:, 2], y0[:, 3]], axis=1)
        # (h: the length the lane counted, handed over as the step to take -- the base rule's, or the halved one after a retry;
        # 0, the base rule again, where the hit's step ended the ray and counted nothing)
        A = ltrace.disk_advance_probe(met, st, rec[rows, 2], ltrace.INTEGRATOR_RK4, 32, h=tr[k, rows, 4], r_obs=r_obs, lambda_max=lam_max(r_obs))
        ok = A["is_hit"] & ((A["on_h"] == tr[k, rows, 4]) | (tr[k, rows, 4] == 0))
        assert ok.all(), (a, j, np.nonzero(~ok)[0][:8])          # every stored time is held
        part = ltrace.step_time_probe(met, rec[rows, 2], y0, A["on_y1"][:, COLS], A["on_h"], A["on_tau"], 32)
        terms = np.where(np.arange(tr.shape[0])[:, None] < k[None, :], tr[:, rows, 5], np.nan)
        assert (np.nan_to_num(terms, nan=0.0) > 0).sum(axis=0).min() >= hb.MIN_SUM_STEPS
        hi, lo = hb.two_sum_replay(terms, np.float32)
        replay = (hi + (lo + part.astype(np.float32))).astype(np.float64)
        assert same(o["tim"][j, rows][ok], replay[ok])           # the stored time is that read of the carried sum
        exact = np.nansum(terms.astype(hb.LD), axis=0) + part.astype(hb.LD)
        bound = hb.sum_bound(terms, part, 32)
        e2 = np.abs(o["tim"][j, rows].astype(hb.LD) - exact).astype(np.float64)[ok]
        plain = (hb.plain_sum_replay(terms, np.float32) + part.astype(np.float32)).astype(np.float64)
        e1 = np.abs(plain.astype(hb.LD) - exact).astype(np.float64)[ok]
        assert (e2 <= bound[ok]).all(), (a, j, np.max(e2 / bound[ok]))
        rays, missed, worst = rays + int(ok.sum()), missed + int((e1 > bound[ok]).sum()), max(worst, float(np.max(e2 / bound[ok])))
        ratio.append(np.median(e1 / bound[ok]))
    print(f"a = {a}: {rays} stored float32 times within {worst:.2f} of the bound; the plain sum of the same terms misses it on {missed} "
          f"(median {np.round(ratio, 2)} of the bound per slot)")
    record(f"sum_a{a}", dict(times=rays, worst=worst, plain_missed=missed))
    assert rays >= 100 and missed >= rays / 2  # (at least 100 of the 256 rays have to reach the disk for this to say anything)


# ---- 5. the product runs the probe's arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a", [0.9, 0.998])
@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_the_timed_kernels_store_what_the_probe_stores(kind, a):
    integ, precision, dp45 = INTEGRATORS[kind]
    c = chain(kind, a, pol=True)
    o, n = c["out"], c["al"].size
    assert (o["event"] != ltrace.EV_RUNNING).all()
    disk, field = ltrace.default_disk(), ltrace.default_bfield(b_r=0.3, b_phi=0.8, b_z=0.5)
    args = (1.0, a, 50.0, c["al"], c["th"], THETA_OBS, lam_max(50.0), disk)
    kw = dict(max_images=MAX_IMAGES, integrator=integ, precision=precision)
    prod = ltrace.trace_batch_kerr_disk_hits(*args, **kw)
    polp = ltrace.trace_batch_kerr_disk_pol(*args, field, **kw)
    assert same(prod["n_hits"], o["n"]) and same(polp["n_hits"], o["n"]) and same(polp["hits"], prod["hits"])
    stored = 0
    for j in range(MAX_IMAGES):
        assert same(prod["hits"][:, j, 0], o["img"][j, :, 0]), (kind, a, j)                                   # r: every bit
        assert same(prod["hits"][:, j, 3], o["tim"][j]), (kind, a, j, np.nonzero(prod["hits"][:, j, 3] != o["tim"][j])[0][:8])  # the time: every bit
        here = ~np.isnan(o["tim"][j])
        phi = o["img"][j, here, 1]
        d = dk.circle_distance(prod["hits"][here, j, 1], np.mod(phi, 2 * np.pi))
        assert (d <= 2 * dk.K_WRAP * dk.U64 * (np.abs(phi) + 2 * np.pi)).all()
        hitrec = np.stack([o["img"][j, here, 0], o["mom"][j, here, 0], o["mom"][j, here, 1]], axis=1)
        want = ltrace.polarization_probe(metric_of(1.0, a), 50.0, THETA_OBS, c["rec"][here, 2], hitrec, c["rec"][here, :2], field)
        assert same(polp["pol"][here, j], want), (kind, a, j, np.nonzero((polp["pol"][here, j] != want).any(axis=1))[0][:8])
        assert np.isnan(polp["pol"][~here, j]).all()
        stored += int(here.sum())
    print(f"{kind}, a = {a}: {stored} stored hits of {n} rays equal the production kernels' in r, time and (q, u, sin zeta, mu)")
    record(f"product_{kind}_a{a}", dict(stored=stored))
    assert stored >= 100  # (at least 100 stored hits among the 256 rays)


# ---- 6. the polarization rule where it is hardest -------------------------------------------------------------------------------------------
def pol_probe(c, rows=slice(None), field=None):
    b = c["field"] if field is None else field
    return ltrace.polarization_probe(metric_of(c["M"], c["a"]), c["r_obs"], c["theta_obs"], c["L"][rows], c["hit"][rows], c["cam"][rows],
                                     ltrace.default_bfield(b_r=float(b[0]), b_phi=float(b[1]), b_z=float(b[2])))


@pytest.mark.parametrize("name", list(hb.POL_CLASSES))
def test_polarization_rule_per_class(name):
    """The existing rule of tests/test_gpu_polarization.py -- the device within 4 x numpy-float64's own error against longdouble
    on the same records -- with that error measured per class on the CPU and written down (hit_blocks.POL_F64_ERR)."""
    c = hb.pol_class(name)
    got = pol_probe(c)
    assert np.isfinite(got).all()
    e = float(np.max(np.abs(got.astype(hb.LD) - hb.pol_reference(c, hb.LD))))
    print(f"{name:10s}: device against longdouble {e:.2e}; numpy float64 {hb.POL_F64_ERR[name]:.2e}, bound {4 * hb.POL_F64_ERR[name]:.2e}")
    record(f"pol_{name}", dict(device=e, float64=hb.POL_F64_ERR[name]))
    assert e <= 4 * hb.POL_F64_ERR[name]


def test_polarization_with_the_field_almost_along_the_photon():
    """sin zeta from 1e-3 down to 1e-9: (q, u) lose digits as 1 / sin zeta, so the error is held in |d(q, u)| sin zeta, to 4 x what
    numpy's float64 is off from longdouble in the same measure on the same rows (one call per row: a call has one field)."""
    c = hb.pol_class("a998")
    n = hb.POL_PARALLEL_ROWS
    delta = 10.0 ** -np.linspace(3.0, 9.0, n)
    b, _ = hb.tilted_fields(c, np.arange(n), delta)
    dev = np.stack([pol_probe(c, slice(i, i + 1), b[i])[0] for i in range(n)])
    f64 = np.stack([hb.pol_reference(c, np.float64, slice(i, i + 1), b[i])[0] for i in range(n)])
    ld = np.stack([hb.pol_reference(c, hb.LD, slice(i, i + 1), b[i])[0] for i in range(n)])
    assert np.isfinite(dev).all()
    sz = ld[:, 2].astype(np.float64)
    assert (sz < 2e-3).all() and (sz > 2e-10).all()
    e_dev = float(np.max(np.abs(dev[:, :2].astype(hb.LD) - ld[:, :2]).astype(np.float64) * sz[:, None]))
    e_f64 = float(np.max(np.abs(f64[:, :2].astype(hb.LD) - ld[:, :2]).astype(np.float64) * sz[:, None]))
    e_sz = float(np.max(np.abs(dev[:, 2] - sz) / sz))
    print(f"field within 1e-3 ... 1e-9 of the photon: |d(q, u)| sin zeta device {e_dev:.2e}, numpy float64 {e_f64:.2e}; sin zeta relative {e_sz:.2e}")
    record("pol_parallel", dict(device=e_dev, float64=e_f64, sin_zeta_rel=e_sz))
    assert e_dev <= 4 * e_f64


def test_polarization_switch_rows():
    """sin^2 zeta a factor 4 either side of 1e-24: dark rows are exact zeros, lit rows have q^2 + u^2 = 1 to 4 u; no NaN.  (No
    row sits ON the value -- a float64 field cannot be placed there to better than the rounding of its cross product --, so
    `<` against `<=` cannot be observed.)"""
    c = hb.pol_class("a998")
    n = 64
    for delta, lit in ((2e-12, True), (5e-13, False)):
        b, _ = hb.tilted_fields(c, np.arange(n), np.full(n, delta))
        dev = np.stack([pol_probe(c, slice(i, i + 1), b[i])[0] for i in range(n)])
        assert not np.isnan(dev).any()
        if lit:
            assert (np.abs(dev[:, 0] ** 2 + dev[:, 1] ** 2 - 1.0) <= 4 * hb.U64).all() and (dev[:, 2] > 0).all()
        else:
            assert (dev[:, :3] == 0).all() and not np.signbit(dev[:, :3]).any()
        assert (dev[:, 3] > 0).all()
