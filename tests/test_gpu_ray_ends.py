"""A ray's two ends on the device -- the prologue's records (lt_ic_probe), the Schwarzschild integrator
(lt_schw_trace_probe), the epilogue's extraction (lt_extract_probe) -- and the fixed-step RK4 loop body
(lt_rk4_advance_probe), each by the function the production kernels call, against the same statements in longdouble and
against the oracle's own functions, in the units of tests/ray_ends.py.  Every bound is a constant that
tests/test_ray_ends_host.py derives on the CPU from the oracle and longdouble alone; the device is held to twice it.

Whole production rays are held to their replay through these probes, bit for bit, by test_gpu_ray_replay.py (against the
reference they stay under the statistics of test_gpu_parity.py); this file says which operation is wrong.

MEASURED on the MI355X: profiles/ray_ends_<build id>.json (LT_RAY_ENDS_MEASURE=path writes it), DESIGN.md 2.1.
"""
import json
import os

import numpy as np
import pytest

import ltrace
import ray_ends as re
from oracle import oracle

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_RAY_ENDS_MEASURE")  # a path: the figures the tests print are also written there as JSON
LD = re.LD
KERR, SCHW = ltrace.METRIC_KERR, ltrace.METRIC_SCHWARZSCHILD
_RECORD = {}


def record(key, value):
    def plain(v):
        if isinstance(v, dict):
            return {k: plain(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [plain(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return float(v) if np.isfinite(v) else str(float(v))
        if isinstance(v, np.integer):
            return int(v)
        return v
    _RECORD[key] = plain(value)
    print(f"{key}: {_RECORD[key]}")
    if MEASURE:
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, allow_nan=False)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. initial records
# ---------------------------------------------------------------------------------------------------------------------------
def fixture_records(golden_dir):
    """F2 (tests/golden/kerr_ic.npz, the reference's own initial conditions) -> (inputs, ok, [p_r, p_theta, p_phi] of the
    reference, the device's float64 records)."""
    g = np.load(os.path.join(golden_dir, "kerr_ic.npz"), allow_pickle=False)
    inp, exp = g["inputs"], g["outputs"]
    rec = np.empty((inp.shape[0], 4))
    for key in np.unique(inp[:, [0, 1, 2, 5]], axis=0):
        rows = np.nonzero((inp[:, [0, 1, 2, 5]] == key).all(axis=1))[0]
        rec[rows] = ltrace.ic_probe(KERR, key[0], key[1], key[2], key[3], inp[rows, 3], inp[rows, 4])[:rows.size]
    return inp, exp[:, 0] == 1.0, exp[:, [4, 5, 7]], rec


def test_kerr_record_against_the_reference_fixture(golden_dir):
    """F2 against the float64 record at the tolerance test_oracle_golden.py holds the oracle to on that file (rtol 1e-13,
    atol 1e-13), `ok` equal.  84 of the 1008 rows are rays whose Theta = Q - cos^2 (L^2 / sin^2 - a^2) cancels completely (in
    longdouble below 1e-3 u S_Theta): the reference's p_theta there, 0 ... 9.5e-7, is the square root of its own rounding, and
    only the reference's operations on the reference's sines give it.  (With sines within an ulp of them and products fused
    into the sums, these rows were off by up to 4.1e-7.)"""
    inp, ok, want, rec = fixture_records(golden_dir)
    assert np.array_equal((rec[:, 3].astype(int) & ltrace.FLAG_OK) != 0, ok)
    miss = ok[:, None] & (np.abs(rec[:, :3] - want) > 1e-13 + 1e-13 * np.abs(want))
    record("ic_fixture_F2", dict(rows=int(inp.shape[0]), ok=int(ok.sum()), rows_missing=int(miss.any(axis=1).sum()),
                                 missing_per_component=miss.sum(axis=0).tolist(),
                                 worst_abs=float(np.abs(rec[:, :3] - want)[miss].max()) if miss.any() else 0.0))
    np.testing.assert_allclose(rec[ok, :3], want[ok], rtol=1e-13, atol=1e-13)


def test_kerr_record_against_the_reference_fixture_in_units(golden_dir):
    """F2 again, every row: `ok`, p_r and p_phi at the oracle's tolerance, and Theta = p_theta^2 with the sign of p_theta
    against the longdouble statements within 2 K_IC units -- the rows of complete cancellation included."""
    inp, ok, want, rec = fixture_records(golden_dir)
    assert np.array_equal((rec[:, 3].astype(int) & ltrace.FLAG_OK) != 0, ok) and ok.sum() > 0.5 * ok.size
    np.testing.assert_allclose(rec[ok][:, [0, 2]], want[ok][:, [0, 2]], rtol=1e-13, atol=1e-13)
    worst = 0.0
    for i in np.nonzero(ok)[0]:
        Mq, a, r_obs, al, th, th_obs = inp[i]
        assert Mq == re.M
        ref = re.ic_longdouble(a, r_obs, th_obs, inp[i:i + 1, 3], inp[i:i + 1, 4])
        worst = max(worst, float(re.ic_errors(ref, rec[i:i + 1, 0], rec[i:i + 1, 1], rec[i:i + 1, 2]).max()))
        assert np.signbit(rec[i, 1]) == bool(ref["negative"][0])
    record("ic_fixture_F2_units", dict(worst=worst, bound=2 * re.K_IC))
    assert worst <= 2 * re.K_IC


def test_kerr_record_against_longdouble():
    """The float64 record against the statements of metrics.py:148-218 in longdouble, p_phi, Theta and p_r^2 within 2 K_IC
    units, the sign of p_theta exact (a zero's included); the float32 record is the float64 record rounded, in every bit."""
    alpha, theta = re.ic_rows()
    refine = (np.arange(alpha.size) % 3 == 0)
    worst = np.zeros(3)
    for a in re.SPINS:
        for r_obs, th_obs in re.ic_observers(a):
            ref = re.ic_longdouble(a, r_obs, th_obs, alpha, theta)
            rec = ltrace.ic_probe(KERR, re.M, a, r_obs, th_obs, alpha, theta, refine)
            n = alpha.size
            assert rec.shape[0] == (n + 63) // 64 * 64 and (rec[n:] == [0, 0, 0, ltrace.FLAG_PAD]).all()
            assert np.array_equal(rec[:n, 3], ltrace.FLAG_OK + ltrace.FLAG_REFINE * refine)
            e = re.ic_errors(ref, rec[:n, 0], rec[:n, 1], rec[:n, 2])
            worst = np.maximum(worst, e.max(axis=0))
            assert np.array_equal(np.signbit(rec[:n, 1]), ref["negative"]) and (rec[:n, 0] <= 0).all()
            r32 = ltrace.ic_probe(KERR, re.M, a, r_obs, th_obs, alpha, theta, refine, precision=32)
            assert re.same_bits(r32, rec.astype(np.float32)).all()
    record("ic_kerr_units", dict(p_phi=worst[0], Theta=worst[1], p_r2=worst[2], bound=2 * re.K_IC))
    assert worst.max() <= 2 * re.K_IC


def test_kerr_record_of_an_observer_inside_the_horizon():
    alpha, theta = re.ic_rows(n=32)
    for a, r_obs in ((0.0, 2.0), (0.9, 1.2), (1.0, 1.0), (-0.7, 1.5)):
        for precision in (64, 32):
            rec = ltrace.ic_probe(KERR, re.M, a, r_obs, 1.0, alpha, theta, np.ones(alpha.size), precision=precision)
            assert (rec[:alpha.size] == [0, 0, 0, ltrace.FLAG_REFINE]).all() and not np.signbit(rec[:alpha.size, :3]).any()


def test_schwarzschild_record_against_longdouble():
    alpha = np.unique(np.concatenate([re.ic_rows()[0], [np.nextafter(np.pi / 2, 0), np.nextafter(np.pi / 2, 4)]]))
    worst = 0.0
    for r_obs in (2.5, 6.0, 8.0, 12.0, 50.0, 300.0):
        w0sq, S = re.schw_w0_longdouble(r_obs, alpha)
        rec = ltrace.ic_probe(SCHW, re.M, 0.0, r_obs, np.pi / 2, alpha)[:alpha.size]
        ok = rec[:, 3] == ltrace.FLAG_OK
        assert ((rec[:, 3] == 0) | ok).all() and (rec[:, 1:3] == 0).all() and (rec[~ok, 0] == 0).all()
        unit = re.U64 * S.astype(np.float64)
        clear = np.abs(w0sq.astype(np.float64)) > 4 * re.K_W0 * unit
        assert np.array_equal(ok[clear], (w0sq > 0)[clear])
        assert np.array_equal(ok[clear], oracle.schw_ic(re.M, r_obs, alpha)[1][clear]) and clear.mean() > 0.98
        worst = max(worst, float((np.abs(rec[:, 0].astype(LD) ** 2 - np.maximum(w0sq, 0)).astype(np.float64) / unit)[ok].max()))
        r32 = ltrace.ic_probe(SCHW, re.M, 0.0, r_obs, np.pi / 2, alpha, precision=32)
        assert re.same_bits(r32[:alpha.size], rec.astype(np.float32)).all()
    record("ic_schw_w0sq_units", dict(worst=worst, bound=2 * re.K_W0))
    assert worst <= 2 * re.K_W0
    for r_obs, al in ((50.0, [0.0, -0.0]), (2.0, [0.5, 2.0]), (1.5, [0.5, 2.0])):   # b == 0; r_obs <= R_S
        assert (ltrace.ic_probe(SCHW, re.M, 0.0, r_obs, np.pi / 2, al)[:2] == 0).all()


def test_exact_sincos_against_mpmath():
    """sincos_f64_exact, the prologue's: both results within half an ulp + 2^-16 ulp of the true value (its double-double
    evaluation is good to 2^-70 of the result) -- on angles of a few radians, next to multiples of pi / 2 (the float64 nearest,
    its neighbours, 1e-9 ... 1e-3 away), small angles, and the angles of the fixture F2."""
    rng = np.random.default_rng([0, 71])
    k = np.arange(-6, 7) * (np.pi / 2)
    near = np.concatenate([re.ulps(k, j) for j in (-2, -1, 0, 1, 2)] + [k + s * e for s in (-1, 1) for e in (1e-9, 1e-6, 1e-3)])
    x = np.concatenate([rng.uniform(-7.0, 7.0, 3000), np.exp(rng.uniform(np.log(1e-9), np.log(3.2), 1000)), near, [0.0, 1.2, 2.0, 0.7, 3.0]])
    got = ltrace.math64_probe("sincos_exact", x)
    hi, lo = re.sb.mp_sincos(x)
    err, ulp = re.sb.err64(got, hi, lo)
    exact_zero = hi == 0.0      # sin(0)
    assert (got[exact_zero] == 0.0).all()
    worst = float(ulp[~exact_zero].max())
    record("sincos_f64_exact", dict(n=int(x.size), worst_ulps=worst, not_correctly_rounded=int((ulp[~exact_zero] > 0.5).sum())))
    assert worst <= 0.5 + 2.0 ** -16


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the Schwarzschild integrator
# ---------------------------------------------------------------------------------------------------------------------------
def device_schw_step(u, w, phi_max, h_max, precision=64):
    p = ltrace.schw_trace_probe(re.M, re.SCHW_R_OBS, u, w, phi_max=phi_max, h_max=h_max, precision=precision)
    assert (p["steps"] == 1).all()
    return p["u"], p["w"], p["event"]


@pytest.mark.parametrize("precision", [64, 32])
def test_schwarzschild_step_against_longdouble(precision):
    """One step -- h = 0.05, 0.01 and a last, shorter step -- of schw_trace, whose association is not the reference's
    (h * (1/6), k1 + 2 (k2 + k3) + k4, fmas), against the reference's statements in longdouble: within 2 K units."""
    K = re.K_SCHW64 if precision == 64 else re.K_SCHW32
    e = re.schw_step_errors(lambda u, w, pm, hm: device_schw_step(u, w, pm, hm, precision), precision == 32)
    record(f"schw_step_float{precision}_units", dict({k: [x, y] for k, (x, y) in e.items()}, bound=2 * K))
    assert max(max(v) for v in e.values()) <= 2 * K


def test_schwarzschild_chords_against_longdouble():
    u, w, _ = re.schw_chord_rows()
    p = ltrace.schw_trace_probe(re.M, re.SCHW_R_OBS, u, w, phi_max=0.05, h_max=0.05)
    assert (p["steps"] == 1).all() and (p["full_steps"] == 0).all()
    ew, ep = re.schw_chord_errors(p["u"], p["w"], p["phi_last"], p["event"])
    record("schw_chord_units", dict(w=ew, phi=ep, bound=2 * re.K_CHORD))
    assert max(ew, ep) <= 2 * re.K_CHORD


def test_schwarzschild_event_table():
    """Each row of the event table against the oracle's loop: the event, the evaluations, u in every bit where the ray ended
    on a threshold, and the rest within 3 K of the step's and the chord's units -- device against ORACLE: K for the oracle's
    own distance from longdouble and the 2 K the device is allowed (the rule wherever this file compares the two directly)."""
    rows = re.schw_event_rows()
    u, w = np.array([r[1] for r in rows]), np.array([r[2] for r in rows])
    o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, u, w, phi_max=0.05, h_max=0.05)
    p = ltrace.schw_trace_probe(re.M, re.SCHW_R_OBS, u, w, phi_max=0.05, h_max=0.05)
    got = {r[0]: int(e) for r, e in zip(rows, p["event"])}
    assert got == {r[0]: int(e) for r, e in zip(rows, o["status"])}, got
    assert np.array_equal(4 * p["steps"], o["evals"])
    ended = o["status"] != 2
    assert np.array_equal(p["u"][ended], o["u"][ended]) and (p["full_steps"] == ~ended).all()
    _, _, unit_u, unit_w = re.schw_unit(u, w, 0.05, re.U64)
    assert (np.abs(p["u"] - o["u"]) <= 3 * re.K_SCHW64 * unit_u).all()
    for i in np.nonzero(ended)[0]:
        _, _, cw, cphi = re.schw_chord_units(u[i:i + 1], w[i:i + 1], 0.05, o["u"][i], re.U64)
        assert abs(p["w"][i] - o["w"][i]) <= 3 * re.K_CHORD * cw[0] and abs(p["phi_last"][i] - o["phi"][i]) <= 3 * re.K_CHORD * cphi[0], rows[i]
    assert (np.abs(p["w"] - o["w"])[~ended] <= 3 * re.K_SCHW64 * unit_w[~ended]).all() and (p["phi_last"][~ended] == 0).all()
    landed = [i for i, r in enumerate(rows) if r[0] in ("lands_on_u_capture", "lands_on_u_escape")]
    assert (p["phi_last"][landed] == 0.05).all()


@pytest.mark.parametrize("phi_max,h_max", [(6.3, 0.1), (3.2, 0.05), (3.0, 0.07)])
@pytest.mark.parametrize("precision", [64, 32])
def test_schwarzschild_range_end_from_the_photon_sphere(phi_max, h_max, precision):
    """An orbit that survives the whole range (u = 1 / 3M moved by an ulp; the perturbation grows by e^phi, 5e2 over 6.3 rad):
    the steps -- the reference's own count for the range, its last, rounding-sized step included --, the evaluations the
    epilogue reports for them, and phi_f as the epilogue rebuilds it equal the oracle's."""
    u0 = np.array([np.nextafter(1.0 / 3.0, 0.0), np.nextafter(1.0 / 3.0, 1.0), 1.0 / 3.0])
    o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, u0, 0.0, phi_max=phi_max, h_max=h_max)
    p = ltrace.schw_trace_probe(re.M, re.SCHW_R_OBS, u0, 0.0, phi_max=phi_max, h_max=h_max, precision=precision)
    want = re.STEP_COUNTS[(phi_max, h_max)]
    assert (o["status"] == 2).all() and (o["evals"] == 4 * want).all()
    assert (p["event"] == 2).all() and (p["steps"] == want).all() and p["n_full"] + (p["h_last"] > 0) == want
    phi_f = p["full_steps"] * h_max + p["phi_last"]
    tol = 1e-12 if precision == 64 else re.U32 * h_max   # (phi_last is the float32 of the last step's h)
    assert np.abs(phi_f - o["phi"]).max() <= tol and np.abs(phi_f - phi_max).max() <= tol
    fin0 = np.stack([p["u"], p["w"], p["phi_last"], p["full_steps"].astype(np.float64)], axis=1)
    fin1 = np.stack([np.zeros(3), np.zeros(3), p["event"].astype(np.float64), p["steps"].astype(np.float64)], axis=1)
    x = ltrace.extract_probe(SCHW, re.M, 0.0, fin0, fin1, precision=precision, h_schw=h_max)
    assert np.array_equal(x["evals"], o["evals"])
    if precision == 64:
        assert np.abs(p["u"] - o["u"]).max() <= 1e-12 and np.abs(p["w"] - o["w"]).max() <= 1e-12


@pytest.mark.parametrize("phi_max,h_max", [(3.2, 0.05), (3.0, 0.07)])
def test_schwarzschild_rays_that_reach_the_range_end(phi_max, h_max):
    """Whole float64 rays under a range short enough that many end at it (lt_trace_batch_schw against the oracle's tracer):
    status, winding and evaluations equal, final_alpha within 1e-10 -- the range-end rays' included, whose angle is taken at
    phi_f = phi_max (one-step errors of 1e-16 grow by at most e^phi_max < 600)."""
    alphas = np.linspace(0.02, 0.6, 1200)
    n = alphas.size
    fa, w, st, ev = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int8), np.empty(n, dtype=np.uint32)
    ltrace.trace_batch_schw(re.M, re.SCHW_R_OBS, alphas, fa, w, phi_max=phi_max, h_max=h_max, precision=64, out_status=st, out_rhs_evals=ev)
    ofa, ow, ost, oev = oracle.trace_batch_schw(re.M, re.SCHW_R_OBS, alphas, phi_max=phi_max, h_max=h_max)
    at_end = oev == 4 * re.STEP_COUNTS[(phi_max, h_max)]
    assert at_end.sum() > 100 and (~at_end).sum() > 100
    assert np.array_equal(st, ost) and np.array_equal(w, ow) and np.array_equal(ev, oev)
    assert np.array_equal(np.isnan(fa), np.isnan(ofa))
    d = np.abs(fa - ofa)[~np.isnan(ofa)]
    record(f"schw_range_end_rays_{phi_max}_{h_max}", dict(at_range_end=int(at_end.sum()), worst_fa=d.max()))
    assert d.max() <= 1e-10


# ---------------------------------------------------------------------------------------------------------------------------
# 3. extraction
# ---------------------------------------------------------------------------------------------------------------------------
def device_half_orbits(phi):
    """half_orbits(phi) through the Kerr epilogue: a captured record keeps its count whatever phi is."""
    rec = np.zeros((len(phi), 6))
    rec[:, 0], rec[:, 1], rec[:, 2] = 1.5, 1.0, phi
    x = ltrace.extract_probe(KERR, re.M, 0.9, *re.kerr_fin(rec, ltrace.EV_CAPTURED))
    assert (x["status"] == -1).all()
    return x["winding"]


def test_half_orbits_equal_floor_division():
    v = re.half_orbit_values()
    assert np.array_equal(device_half_orbits(v), re.python_half_orbits(v))
    assert np.array_equal(device_half_orbits(np.array([1e15, -1e15, 3e300, np.inf, -np.inf, np.nan])), np.zeros(6, dtype=np.int64))


def kerr_table(a):
    """-> (names, records (n,6), events)"""
    rc11 = (re.r_plus(abs(a)) * 1.01) * 1.1
    good = [100.0, 1.2, 2.5, 0.9, 3.0, 2.0]
    rows = []
    for ev in (-1, 1, 2):
        rows.append((f"event_{ev}", good, ev))
        rows.append((f"event_{ev}_wound", [100.0, 1.2, -17.0, 0.9, 3.0, 2.0], ev))
        for k in (-1, 0, 1):
            rows.append((f"event_{ev}_r_at_1.1_r_capture_{k:+d}ulp", [float(re.ulps(rc11, k))] + good[1:], ev))
    for j, name in ((0, "r"), (1, "theta"), (2, "phi")):
        for bad in (np.nan, np.inf, -np.inf):
            if name == "r" and bad == -np.inf:
                continue  # (r = -inf is "captured" with the half orbits of phi on both sides; it is in the r rows below)
            rec = list(good)
            rec[j] = bad
            rows.append((f"{name}_{bad}", rec, 1))
    rows += [("r_-inf", [-np.inf] + good[1:], 1), ("r_negative", [-3.0] + good[1:], 2), ("r_zero", [0.0] + good[1:], 1),
             ("theta_0", [100.0, 0.0, 2.5, 0.9, 3.0, 0.0], 1), ("theta_pi", [100.0, np.pi, 2.5, 0.9, 3.0, 0.0], 1),
             ("theta_0_with_L", [100.0, 0.0, 2.5, 0.9, 3.0, 2.0], 1), ("theta_negative", [100.0, -0.3, 2.5, 0.9, 3.0, 2.0], 1),
             ("momenta_0", [100.0, 1.2, 2.5, 0.0, 0.0, 0.0], 1), ("momenta_inf", [100.0, 1.2, 2.5, np.inf, 3.0, 2.0], 1),
             ("p_theta_nan", [100.0, 1.2, 2.5, 0.9, np.nan, 2.0], 2), ("range_end_inside", [3.0, 1.2, 40.0, 0.0, 1.0, 5.0], 2),
             # padding records (event 3): all zeros, and the observer's state as the integrate kernels store it
             ("pad_zeros", [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], 3), ("pad_observer", [50.0, np.pi / 2, 0.0, 0.0, 0.0, 0.0], 3)]
    return [r[0] for r in rows], np.array([r[1] for r in rows], dtype=np.float64), np.array([r[2] for r in rows])


@pytest.mark.parametrize("a", [0.0, 0.9, 1.0, -0.7])
def test_kerr_status_table(a):
    """status, n_half and the presence of an angle, field by field against the oracle's kerr_extract_angle: each event code,
    r at 1.1 r_capture and its neighbours, a NaN or an infinity in each coordinate, the poles (the sin^2 floor), no momentum at
    all (escaped with a NaN angle where nothing drags the frame), a range-end ray (through the escape branch).  An invalid ray
    (the tracer returns before the extraction) has status 0 and no count.  A padding record (event 3) is nothing special to
    the extraction -- the epilogues read the rows below n only --: it is extracted like a range-end record of the same state,
    captured (-1, no count) for the zeros, status 1 for the observer's state, as the oracle does with an event that is not -1."""
    names, rec, ev = kerr_table(a)
    ofa, onh, ost = oracle.kerr_extract(rec[:, :5], rec[:, 5], ev, re.M, a)
    x = ltrace.extract_probe(KERR, re.M, a, *re.kerr_fin(rec, ev))
    got = {n: (int(s), int(w), bool(np.isnan(f))) for n, s, w, f in zip(names, x["status"], x["winding"], x["fa"])}
    want = {n: (int(s), int(w), bool(np.isnan(f)) or s != 1) for n, s, w, f in zip(names, ost, onh, ofa)}
    assert got == want
    assert {-1, 0, 1} <= set(int(s) for s in ost) and want["momenta_0"] == (1, 0, a == 0.0)
    assert want["pad_zeros"] == (-1, 0, True) and want["pad_observer"][:2] == (1, 0)
    both = ~np.isnan(x["fa"])
    assert np.abs(x["fa"][both] - ofa[both]).max() <= 1e-9
    inv = ltrace.extract_probe(KERR, re.M, a, *re.kerr_fin(rec, ltrace.EV_INVALID))
    assert (inv["status"] == 0).all() and (inv["winding"] == 0).all() and np.isnan(inv["fa"]).all()


def test_schwarzschild_status_table():
    """The Schwarzschild tail against the oracle's: each event code, r_f = 1 / u_f at 1.1 R_S and its neighbours, windings."""
    u11 = 1.0 / (2.0 * re.M * 1.1)
    rows = [(ev, u, w, phi) for ev in (-1, 1, 2) for u in (0.01, 0.3, 0.49, float(re.ulps(u11, -2)), float(re.ulps(u11, -1)), u11,
                                                                  float(re.ulps(u11, 1)), float(re.ulps(u11, 2)))
            for w, phi in ((-0.05, 2.0), (0.05, -11.0), (0.0, 0.0), (-0.2, 50.0))]
    ev, u, w, phi = (np.array(c) for c in zip(*rows))
    ofa, onh, ost = oracle.schw_extract(re.M, ev, phi, u, w)
    x = ltrace.extract_probe(SCHW, re.M, 0.0, *re.schw_fin(u, w, phi, ev))
    assert np.array_equal(x["status"], ost) and np.array_equal(x["winding"], onh) and {-1, 1} == set(int(s) for s in ost)
    assert np.array_equal(np.isnan(x["fa"]), np.isnan(ofa) | (ost != 1))
    both = ~np.isnan(x["fa"])
    assert both.sum() > 20 and np.abs(x["fa"][both] - ofa[both]).max() <= 1e-12
    inv = ltrace.extract_probe(SCHW, re.M, 0.0, *re.schw_fin(u, w, phi, ltrace.EV_INVALID))
    assert (inv["status"] == 0).all() and (inv["winding"] == 0).all() and np.isnan(inv["fa"]).all()
    # a NaN or an infinity in u, w or phi; a padding record (event 3: like a range-end record of the same state); u = 0
    bad = [(e, uu, ww, pp) for e in (1, 2, 3, -1) for uu, ww, pp in ((np.nan, -0.05, 2.0), (np.inf, -0.05, 2.0), (0.01, np.nan, 2.0),
                                                                 (0.01, np.inf, 2.0), (0.01, -np.inf, 2.0), (0.0, -0.05, 2.0), (0.0, 0.0, 0.0),
                                                                 (0.01, -0.05, np.nan), (0.01, -0.05, np.inf), (0.01, -0.05, -np.inf))]
    bev, bu, bw, bphi = (np.array(c) for c in zip(*bad))
    with np.errstate(all="ignore"):
        bfa, bnh, bst = oracle.schw_extract(re.M, np.where(bev == 3, 2, bev), bphi, bu, bw)
    y = ltrace.extract_probe(SCHW, re.M, 0.0, *re.schw_fin(bu, bw, bphi, bev))
    assert np.array_equal(y["status"], bst) and np.array_equal(np.isnan(y["fa"]), np.isnan(bfa) | (bst != 1))
    fin = np.isfinite(bphi)     # (the count of a phi that is not finite: 0 on the device, undefined in the reference)
    assert np.array_equal(y["winding"][fin], bnh[fin]) and (y["winding"][~fin] == 0).all()
    both = ~np.isnan(y["fa"])
    assert np.abs(y["fa"][both] - bfa[both]).max() <= 1e-12 if both.any() else True
    # phi_f = full steps * h + phi_last, in float64
    f0, f1 = re.schw_fin(u, w, 0.013, ev)
    f0[:, 3] = 777.0
    y = ltrace.extract_probe(SCHW, re.M, 0.0, f0, f1, h_schw=0.05)
    assert np.array_equal(y["winding"], re.python_half_orbits(np.full(u.size, 777.0 * 0.05 + 0.013)))


def test_kerr_final_angle_against_longdouble():
    """final_alpha of kerr_extract -- one reciprocal for four quotients, sincos_f64, a reciprocal of |v| -- against the
    reference's statements in longdouble on exits through r_escape: within 2 K_EXT units."""
    def dev(a, rec):
        x = ltrace.extract_probe(KERR, re.M, a, *re.kerr_fin(rec, ltrace.EV_ESCAPED))
        assert np.array_equal(x["winding"], re.python_half_orbits(rec[:, 2]))
        return x["fa"], x["status"]
    worst, at = re.kerr_fa_errors(dev)
    record("kerr_final_alpha_units", dict(worst=worst, at=at, bound=2 * re.K_EXT))
    assert worst <= 2 * re.K_EXT


def test_schwarzschild_final_angle_against_longdouble():
    def dev(rec):
        x = ltrace.extract_probe(SCHW, re.M, 0.0, *re.schw_fin(rec[:, 0], rec[:, 1], rec[:, 2], ltrace.EV_ESCAPED))
        return x["fa"], x["status"]
    worst, at = re.schw_fa_errors(dev)
    record("schw_final_alpha_units", dict(worst=worst, at=at, bound=2 * re.K_EXT_SCHW))
    assert worst <= 2 * re.K_EXT_SCHW


def test_float32_records_extract_as_their_rounded_values():
    """Precision 32 on a record is precision 64 on the float32-rounded record, in every bit of every output.  (With the
    products of vx, vy, vz left to the compiler to fuse, the two instantiations of the epilogue fused different ones: 75 of 1092
    Kerr angles within 1e-3 rad of the +-x axis differed by up to 3e-5 of the angle -- acos near +-1 turns one ulp of the
    cosine into 1e-10 rad.)"""
    failures = []
    for a in (0.9, -0.7):
        names, rec, ev = kerr_table(a)
        rec = np.concatenate([rec, re.kerr_exit_rows(a, 50.0, n=512)])
        ev = np.concatenate([ev, np.ones(512, dtype=ev.dtype)])
        f0, f1 = re.kerr_fin(rec, ev, steps=np.arange(rec.shape[0]) * 7)
        x32 = ltrace.extract_probe(KERR, re.M, a, f0, f1, precision=32)
        with np.errstate(over="ignore"):
            x64 = ltrace.extract_probe(KERR, re.M, a, f0.astype(np.float32), f1.astype(np.float32), precision=64)
        for k in ("status", "winding", "evals"):
            assert np.array_equal(x32[k], x64[k]), k
        differ = ~re.same_bits(x32["fa"], x64["fa"])
        record(f"extract_float32_vs_rounded_a{a}", dict(rows=int(differ.size), differ=int(differ.sum()),
                                                        worst_ulps=float((np.abs(x32["fa"] - x64["fa"]) / np.spacing(x64["fa"]))[differ].max()) if differ.any() else 0.0))
        failures.append(int(differ.sum()))
    rec = re.schw_exit_rows(n=512)
    f0, f1 = re.schw_fin(rec[:, 0], rec[:, 1], rec[:, 2], 1, steps=np.arange(512))
    f0[:, 3] = np.arange(512) % 40
    x32 = ltrace.extract_probe(SCHW, re.M, 0.0, f0, f1, precision=32, h_schw=0.05)
    x64 = ltrace.extract_probe(SCHW, re.M, 0.0, f0.astype(np.float32), f1.astype(np.float32), precision=64, h_schw=0.05)
    for k in ("status", "winding", "evals"):
        assert np.array_equal(x32[k], x64[k]), k
    assert re.same_bits(x32["fa"], x64["fa"]).all()
    assert failures == [0, 0]


def test_evaluation_counts():
    """evals = fixed + steps * per step: 4 per RK4 step, 1 + 6 per DP45 attempt, 4 per Schwarzschild step."""
    steps = np.array([0, 1, 2, 999, 12345, 2 ** 24 - 1, 2 ** 24])
    rec = np.tile([100.0, 1.2, 2.5, 0.9, 3.0, 2.0], (steps.size, 1))
    for precision in (64, 32):
        for integ, fixed, per in (("rk4", 0, 4), ("dp45", 1, 6), ("dp45_exact", 1, 6)):
            x = ltrace.extract_probe(KERR, re.M, 0.9, *re.kerr_fin(rec, 1, steps=steps), precision=precision, integrator=integ)
            assert np.array_equal(x["evals"], fixed + per * steps), (precision, integ)
        x = ltrace.extract_probe(SCHW, re.M, 0.0, *re.schw_fin(np.full(steps.size, 0.01), -0.05, 2.0, 1, steps=steps), precision=precision)
        assert np.array_equal(x["evals"], 4 * steps)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the fixed-step RK4 loop body
# ---------------------------------------------------------------------------------------------------------------------------
def rk4_probe(a, st, L, refine, lam, precision, n_iters=1, h_retry=None, steps=None):
    return ltrace.rk4_advance_probe(re.M, a, st, L, refine, lam=lam, h_retry=h_retry, steps=steps, precision=precision, n_iters=n_iters,
                                    r_obs=re.RK4_R_OBS, lambda_max=re.RK4_LAMBDA_MAX)


def rk4_reference_iteration(a, t, precision):
    """The device up to the next boundary of a reference iteration: single attempts until the row has ended or has no
    halved step left to retry (h_retry == 0)."""
    n = len(t["names"])
    cur = dict(state=t["st"].copy(), lam=t["lam"].copy(), h_retry=np.zeros(n), steps=np.zeros(n, dtype=np.int32), event=np.full(n, 4))
    todo = np.ones(n, dtype=bool)
    for _ in range(10):
        i = np.nonzero(todo)[0]
        p = rk4_probe(a, cur["state"][i], t["L"][i], t["refine"][i], cur["lam"][i], precision, h_retry=cur["h_retry"][i], steps=cur["steps"][i])
        for k in ("state", "lam", "h_retry", "steps", "event"):
            cur[k][i] = p[k]
        todo[i] = (p["event"] == 4) & (p["h_retry"] > 0)
        if not todo.any():
            break
    assert not todo.any()
    return cur


@pytest.mark.parametrize("a", re.RK4_SPINS)
def test_rk4_decision_table_float64(a):
    """kerr_rk4_advance against the oracle's iteration (lto_rk4_iteration), row by row at the reference's iteration boundaries:
    the event, the attempts (the halvings down to h_floor included), lam -- hence every h -- equal; against longdouble, the
    state of a row that goes on within 2 K_STEP64 units and the state of a row that ends on a chord within 2 K_RK4_CHORD of
    the chord's unit -- the redo lanes included: only rows with a stage within 1e-3 r_cut of r_cut are left out."""
    t = re.rk4_table(a)
    o = re.rk4_oracle(a, t, oracle)
    d = rk4_reference_iteration(a, t, 64)
    got = {n: (int(e), int(s)) for n, e, s in zip(t["names"], d["event"], d["steps"])}
    assert got == {n: (int(e), int(s)) for n, e, s in zip(t["names"], o["event"], o["attempts"])}
    on = o["event"] == 4
    assert np.array_equal(d["lam"][on], o["lam"][on])
    bad = (o["event"] == 0) | (o["event"] == 2)
    assert re.same_bits(d["state"][bad], t["st"][bad]).all()
    rows, err, keep, chord = re.rk4_state_errors(a, t, o, d["state"], re.U64, oracle)
    kept = [t["names"][r] for r, k in zip(rows, keep) if k]
    assert sum(n.startswith("redo_radius") for n in kept) >= 6 and sum(n.startswith("redo_angle") for n in kept) == 6
    record(f"rk4_table_float64_a{a}", dict(rows=len(t["names"]), compared=int(keep.sum()), accepted_units=err[~chord & keep].max(),
                                           accepted_bound=2 * re.sb.K_STEP64, chord_units=err[chord & keep].max(), chord_bound=2 * re.K_RK4_CHORD))
    assert err[~chord & keep].max() <= 2 * re.sb.K_STEP64 and err[chord & keep].max() <= 2 * re.K_RK4_CHORD


@pytest.mark.parametrize("a", re.RK4_SPINS)
def test_rk4_decision_table_float32(a):
    """The float32 loop body -- the production path -- on the float32 table (every row 16 times, theta, p_theta and L varied),
    restricted to the rows whose reference decision is stable under 2 K_FALLBACK float32 units of every attempt's candidate
    (ray_ends.rk4_f32_stable; test_ray_ends_host.py: no class loses more than 2 %): event and attempts equal the float64
    oracle's, lam is the float32 of its lam (every h the float32 of the reference's), a row that ends without a step keeps its
    state in every bit; state in the float32 unit against the float64 step: 2 K_STEP where the step is the ordinary one,
    2 K_FALLBACK in the classes that reach the checked step or r_cut (redo, capture chords, the start beside r_capture, steps
    below zero)."""
    t = re.rk4_table(a, f32=True, variants=16)
    o = re.rk4_oracle(a, t, oracle)
    stable = re.rk4_f32_stable(a, t, o, oracle)
    d = rk4_reference_iteration(a, t, 32)
    assert np.array_equal(d["event"][stable], o["event"][stable]) and np.array_equal(d["steps"][stable], o["attempts"][stable])
    on = stable & (o["event"] == 4)
    assert np.array_equal(d["lam"][on], o["lam"][on].astype(np.float32).astype(np.float64))
    bad = stable & ((o["event"] == 0) | (o["event"] == 2))
    assert re.same_bits(d["state"][bad], t["st"][bad]).all()
    rows, err, keep, chord = re.rk4_state_errors(a, t, o, d["state"], re.U32, oracle)
    keep &= stable[rows]
    cls = np.array([re.rk4_class(t["names"][r]) for r in rows])
    hard = np.isin(cls, ("redo_radius", "redo_angle", "capture_chord", "steps_below_zero", "starts"))
    bound = np.where(hard, 2 * re.sb.K_FALLBACK, 2 * re.sb.K_STEP)
    worst = {c: float(err[keep & (cls == c)].max()) for c in re.RK4_CLASSES if (keep & (cls == c)).any()}
    record(f"rk4_table_float32_a{a}", dict(rows=len(t["names"]), stable=int(stable.sum()), compared=int(keep.sum()), worst_units=worst,
                                           bounds=[2 * re.sb.K_STEP, 2 * re.sb.K_FALLBACK]))
    assert keep.sum() > 0.6 * rows.size and (err[keep].max(axis=1) <= bound[keep]).all()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n_iters", [1, 16, 400])
def test_rk4_iterations_in_one_launch_equal_single_launches(precision, n_iters):
    """N iterations in one launch against N launches of one, every bit of every output: table rows and plain lanes mixed."""
    a = 0.9
    t = re.rk4_table(a)
    ps, pL = re.rk4_plain_rows(a, 128 - len(t["names"]) % 64)
    st, L = np.concatenate([t["st"], ps]), np.concatenate([t["L"], pL])
    rf, lam = np.concatenate([t["refine"], np.zeros(len(pL), dtype=np.uint8)]), np.concatenate([t["lam"], np.zeros(len(pL))])
    one = rk4_probe(a, st, L, rf, lam, precision, n_iters=n_iters)
    cur = dict(state=st.copy(), lam=lam.copy(), h_retry=np.zeros(len(L)), steps=np.zeros(len(L), dtype=np.int32), event=np.full(len(L), 4),
               iters=np.zeros(len(L), dtype=np.int32))
    for _ in range(n_iters):
        i = np.nonzero(cur["event"] == 4)[0]
        if i.size == 0:
            break
        p = rk4_probe(a, cur["state"][i], L[i], rf[i], cur["lam"][i], precision, h_retry=cur["h_retry"][i], steps=cur["steps"][i])
        for k in ("state", "lam", "h_retry", "steps", "event"):
            cur[k][i] = p[k]
        cur["iters"][i] += 1
    for k in ("event", "steps", "iters"):
        assert np.array_equal(one[k], cur[k]), k
    for k in ("state", "lam", "h_retry"):
        assert re.same_bits(one[k], cur[k]).all(), k
    assert (one["event"] == 4).sum() > 8 and (one["event"] != 4).sum() > 8


@pytest.mark.parametrize("precision", [64, 32])
def test_rk4_special_rows_do_not_depend_on_their_neighbours(precision):
    """Every table row alone among 63 plain far-field lanes against all table rows mixed in the same wavefronts, three
    iterations, every bit: `advance` promises that nobody's numbers depend on a neighbour."""
    a = 0.9
    t = re.rk4_table(a)
    n = len(t["names"])
    ps, pL = re.rk4_plain_rows(a, 63)
    mixed = rk4_probe(a, t["st"], t["L"], t["refine"], t["lam"], precision, n_iters=3)
    st = np.concatenate([np.concatenate([t["st"][i:i + 1], ps]) for i in range(n)])
    L = np.concatenate([np.concatenate([t["L"][i:i + 1], pL]) for i in range(n)])
    rf = np.concatenate([np.concatenate([t["refine"][i:i + 1], np.zeros(63, dtype=np.uint8)]) for i in range(n)])
    lam = np.concatenate([np.concatenate([t["lam"][i:i + 1], np.zeros(63)]) for i in range(n)])
    alone = rk4_probe(a, st, L, rf, lam, precision, n_iters=3)
    for k in ("event", "steps", "iters"):
        assert np.array_equal(alone[k][::64], mixed[k]), k
    for k in ("state", "lam", "h_retry"):
        assert re.same_bits(alone[k][::64], mixed[k]).all(), k
    plain = np.ones(64 * n, dtype=bool)
    plain[::64] = False
    for k in ("state", "lam"):   # and the plain lanes are the same next to every special row
        got = alone[k][plain].reshape(n, 63, -1)
        assert re.same_bits(got, np.broadcast_to(got[:1], got.shape)).all(), k
