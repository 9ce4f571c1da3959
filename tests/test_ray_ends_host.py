"""Where the bounds of tests/test_gpu_ray_ends.py come from, on the CPU, from the oracle and longdouble alone
(tests/ray_ends.py states the units, the classes and the tables).

Each K is the float64 oracle's worst error against the same statements in longdouble, in the unit of its block, rounded up
to an integer and asserted from both sides -- the measured maximum lies in (K - 1, K]:

    K_IC = 9        Kerr initial record: p_phi, Theta = p_theta^2, p_r^2 (measured 5.26, 8.22, 3.19: Theta at a = 0.998 seen from
                    the equator at 3 r_plus, alpha = 3e-6)
    K_W0 = 8        Schwarzschild w0^2 (measured 7.96 at r_obs = 2.5, where f0 = 1 - R_S / r_obs = 0.2 carries five roundings of its own)
    K_SCHW64 = 2    one Schwarzschild step, float64 (measured 1.04, w of the shorter last step; 0.89 at h = 0.05)
    K_SCHW32 = 1    one Schwarzschild step, the reference's statements with every operation rounded to float32 (measured 0.75)
    K_CHORD = 1     the chord's w and phi at a capture / escape, float64 (measured 0.48, 0.49)
    K_EXT = 2       final_alpha of the Kerr extraction (measured 1.18);  K_EXT_SCHW = 1  of the Schwarzschild tail (measured 0.92)
    K_RK4_CHORD = 2 the state an RK4 iteration ends in on a capture / escape chord, in the chord's unit (measured 1.78, a = 0)

What needs no reference is checked here too: the reference's step count in Python float64 against the oracle's loop and against
the host's step plan of the library (no device needed for it), and the statements of half_orbits against Python's own `//`.
"""
import math

import numpy as np

import ltrace
import ray_ends as re
from oracle import oracle

LD = re.LD


def _k(name, measured, K, at=None):
    print(f"{name}: measured {measured:.3f} -> {math.ceil(measured)}" + (f" at {at}" if at is not None else ""))
    assert K - 1 < measured <= K, (name, measured, K)


# ---------------------------------------------------------------------------------------------------------------------------
# step counts and half orbits: no reference needed
# ---------------------------------------------------------------------------------------------------------------------------
def test_reference_step_count_three_ways():
    """The steps of the reference's loop `while phi < phi_max: h = min(h_max, phi_max - phi); phi += h` for each (phi_max, h_max)
    of the table: the loop in Python float64, the oracle's loop on an orbit that never ends (u = w = 0), and the host's step
    plan n_full + (h_last > 0) of the library, with the last step's h equal in all three."""
    for (phi_max, h_max), want in re.STEP_COUNTS.items():
        steps, h_last = re.ref_step_plan(phi_max, h_max)
        o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, [0.0], [0.0], phi_max=phi_max, h_max=h_max)
        p = ltrace.schw_trace_probe(re.M, re.SCHW_R_OBS, np.zeros(0), np.zeros(0), phi_max=phi_max, h_max=h_max)
        got = p["n_full"] + (p["h_last"] > 0)
        print(f"phi_max {phi_max:.6g}, h_max {h_max}: reference {steps} steps (last h {h_last:.3g}), oracle {int(o['evals'][0]) // 4}, "
              f"host plan {p['n_full']} + {int(p['h_last'] > 0)} (h_last {p['h_last']:.3g})")
        assert steps == want and o["status"][0] == 2 and int(o["evals"][0]) == 4 * want
        assert got == want
        assert p["h_last"] == (h_last if h_last < h_max else 0.0)
        assert o["phi"][0] == (phi_max if steps > 1 or h_last < h_max else h_max)


def test_half_orbits_statements_equal_floor_division():
    """The statements of half_orbits (q from one multiplication, corrected by the sign and size of the exact residual rounded
    once) against Python's abs(phi) // pi on k pi and its neighbours, 1e5 values over 315 decades, zeros, a denormal and
    negative values; |phi| >= 1e15, infinities and NaN give 0."""
    v = re.half_orbit_values()
    got, want = re.half_orbits_restated(v), re.python_half_orbits(v)
    corrected = int((np.floor(np.abs(v) * re.INV_PI).astype(np.int64) != want).sum())
    print(f"{v.size} values, largest count {want.max()}, candidate corrected on {corrected}")
    assert v.size > 130000 and want.max() > 2 ** 47 and corrected > 1000
    assert np.array_equal(got, want)
    assert np.array_equal(re.half_orbits_restated([1e15, -1e15, 3e300, np.inf, -np.inf, np.nan]), np.zeros(6, dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------------------------
# initial records
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_kerr_initial_record_against_longdouble():
    alpha, theta = re.ic_rows()
    worst, at, signs = np.zeros(3), [None] * 3, 0
    for a in re.SPINS:
        for r_obs, th_obs in re.ic_observers(a):
            ref = re.ic_longdouble(a, r_obs, th_obs, alpha, theta)
            rec = np.array([np.concatenate([[ok], st[3:5], [pp]]) for ok, st, _, pp in
                            (oracle.kerr_ic(re.M, a, r_obs, al, th, th_obs) for al, th in zip(alpha, theta))])
            assert ref["ok"] and (rec[:, 0] == 1).all()
            e = re.ic_errors(ref, rec[:, 1], rec[:, 2], rec[:, 3])
            assert np.isfinite(e).all()
            assert np.array_equal(np.signbit(rec[:, 2]), ref["negative"])
            signs += int(ref["negative"].sum())
            for j in range(3):
                if e[:, j].max() > worst[j]:
                    i = int(np.argmax(e[:, j]))
                    worst[j], at[j] = e[:, j].max(), (a, r_obs, th_obs, alpha[i], theta[i])
    print(f"oracle initial record, worst error in units: p_phi {worst[0]:.2f} at {at[0]}, Theta {worst[1]:.2f} at {at[1]}, "
          f"p_r^2 {worst[2]:.2f} at {at[2]}; {signs} negative p_theta")
    _k("K_ic", worst.max(), re.K_IC)
    # the observer at or inside the horizon: not OK
    for a, r_obs in ((0.0, 2.0), (0.9, 1.2), (1.0, 1.0), (-0.7, 1.5)):
        assert not re.ic_longdouble(a, r_obs, 1.0, alpha[:1], theta[:1])["ok"]
        assert not oracle.kerr_ic(re.M, a, r_obs, 1.0, 0.5, 1.0)[0]


def test_oracle_schwarzschild_w0_against_longdouble():
    alpha = np.unique(np.concatenate([re.ic_rows()[0], [np.nextafter(np.pi / 2, 0), np.nextafter(np.pi / 2, 4)]]))
    worst, at = 0.0, None
    for r_obs in (2.5, 6.0, 8.0, 12.0, 50.0, 300.0):
        w0sq, S = re.schw_w0_longdouble(r_obs, alpha)
        w0, ok = oracle.schw_ic(re.M, r_obs, alpha)
        unit = re.U64 * S.astype(np.float64)
        clear = np.abs(w0sq.astype(np.float64)) > 2 * re.K_W0 * unit
        assert np.array_equal(ok[clear], (w0sq > 0)[clear]) and clear.mean() > 0.98
        e = (np.abs(w0.astype(LD) ** 2 - np.maximum(w0sq, 0)).astype(np.float64) / unit)[ok]
        if e.max() > worst:
            worst, at = e.max(), (r_obs, alpha[ok][int(np.argmax(e))])
    _k("K_w0", worst, re.K_W0, at)
    assert not oracle.schw_ic(re.M, 50.0, [0.0, -0.0])[1].any()                        # b == 0
    assert not oracle.schw_ic(re.M, 2.0, [0.5])[1].any() and not oracle.schw_ic(re.M, 1.5, [0.5])[1].any()   # r_obs <= R_S


# ---------------------------------------------------------------------------------------------------------------------------
# the Schwarzschild integrator
# ---------------------------------------------------------------------------------------------------------------------------
def oracle_schw_step(u, w, phi_max, h_max, f32=False):
    o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, u, w, phi_max=phi_max, h_max=h_max, f32=f32)
    return o["u"].astype(np.float64), o["w"].astype(np.float64), o["status"]


def test_oracle_schwarzschild_step_against_longdouble():
    for f32, K, label in ((False, re.K_SCHW64, "K_schw64"), (True, re.K_SCHW32, "K_schw32")):
        e = re.schw_step_errors(lambda u, w, pm, hm: oracle_schw_step(u, w, pm, hm, f32=f32), f32)
        print(label, {k: (round(float(x), 3), round(float(y), 3)) for k, (x, y) in e.items()})
        _k(label, max(max(v) for v in e.values()), K)


def test_oracle_schwarzschild_chord_against_longdouble():
    u, w, _ = re.schw_chord_rows()
    o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, u, w, phi_max=0.05, h_max=0.05)
    ew, ep = re.schw_chord_errors(o["u"], o["w"], o["phi"], o["status"])
    print(f"chord: w {ew:.3f}, phi {ep:.3f} units")
    _k("K_chord", max(ew, ep), re.K_CHORD)


def test_schwarzschild_event_table_of_the_oracle():
    """What the table's rows are for, by the oracle: landing on a threshold ends the ray with the whole step used, an ulp
    short of it does not; a start on a threshold does not end it, an ulp inside does."""
    want = dict(lands_on_u_capture=-1, lands_an_ulp_below_u_capture=2, lands_an_ulp_above_u_capture=-1, starts_on_u_capture_inward=2,
                starts_on_u_capture_outward=2, starts_an_ulp_below_u_capture=-1, starts_on_u_escape_outward=2,
                starts_on_u_escape_inward=2, starts_an_ulp_above_u_escape=1, lands_on_u_escape=1, lands_an_ulp_above_u_escape=2,
                capture_chord=-1, capture_chord_late=-1, escape_chord=1, escape_chord_early=1, no_event=2,
                at_rest_on_the_photon_sphere=2)
    rows = re.schw_event_rows()
    o = oracle.schw_orbit(re.M, re.SCHW_R_OBS, [r[1] for r in rows], [r[2] for r in rows], phi_max=0.05, h_max=0.05)
    assert {r[0]: int(s) for r, s in zip(rows, o["status"])} == want
    byname = {r[0]: i for i, r in enumerate(rows)}
    for name in ("lands_on_u_capture", "lands_on_u_escape"):
        assert o["phi"][byname[name]] == 0.05  # frac == 1


# ---------------------------------------------------------------------------------------------------------------------------
# extraction
# ---------------------------------------------------------------------------------------------------------------------------
def test_oracle_kerr_final_angle_against_longdouble():
    worst, at = re.kerr_fa_errors(lambda a, rec: oracle.kerr_extract(rec[:, :5], rec[:, 5], 1, re.M, a)[::2])
    _k("K_ext", worst, re.K_EXT, at)


def test_oracle_schwarzschild_final_angle_against_longdouble():
    worst, at = re.schw_fa_errors(lambda rec: oracle.schw_extract(re.M, 1, rec[:, 2], rec[:, 0], rec[:, 1])[::2])
    _k("K_ext_schw", worst, re.K_EXT_SCHW, at)


# ---------------------------------------------------------------------------------------------------------------------------
# the RK4 loop body
# ---------------------------------------------------------------------------------------------------------------------------
def test_rk4_decision_table_holds_what_it_is_for():
    """By the oracle's own iteration (the function its tracer runs): every outcome occurs -- goes on, captured, escaped, out
    of range, invalid after the halvings down to h_floor --, each cap of the step-size rule is taken on the inside of its
    radius only, a start on r_capture / r_escape does not end the ray and an ulp inside does."""
    for a in re.RK4_SPINS:
        t = re.rk4_table(a)
        o = oracle.rk4_iteration(t["st"], t["L"], t["lam"], re.M, a, r_obs=re.RK4_R_OBS, lambda_max=re.RK4_LAMBDA_MAX, axis_refine=t["refine"])
        got = {n: (int(e), int(k), float(h)) for n, e, k, h in zip(t["names"], o["event"], o["attempts"], o["h"])}
        assert {4, -1, 1, 2, 0} == set(e for e, _, _ in got.values())
        for mult, caps in ((4.0, (0.25, 0.20)), (2.0, (0.10, 0.08)), (1.2, (0.05, 0.03))):
            outer = {4.0: (1.0, 0.5), 2.0: (0.25, 0.20), 1.2: (0.10, 0.08)}[mult]
            for rf in (0, 1):
                assert got[f"cap_{mult}_-1ulp_refine{rf}"][2] == caps[rf]
                assert got[f"cap_{mult}_+0ulp_refine{rf}"][2] == outer[rf] and got[f"cap_{mult}_+1ulp_refine{rf}"][2] == outer[rf]
        assert got["lam_at_lambda_max_refine0"][:2] == (2, 0) and got["lam_an_ulp_below_lambda_max_refine0"][:2] == (4, 1)
        assert got["lam_within_a_base_step_refine1"][2] == 0.3 or abs(got["lam_within_a_base_step_refine1"][2] - 0.3) < 1e-12
        assert got["starts_on_r_capture_inward"][0] == 4 and got["starts_just_above_r_capture_inward"][0] == -1
        assert got["starts_on_r_escape_outward"][0] == 4 and got["starts_just_below_r_escape_outward"][0] == 1
        assert got["p_r_inf_refine0"][:2] == (0, 7) and got["p_r_inf_refine1"][:2] == (0, 7) and got["p_r_inf_near_refine0"][:2] == (0, 4)
        assert max(k for _, k, _ in got.values()) == 7 and any(e == -1 and k > 1 for e, k, _ in got.values())


def test_oracle_rk4_iteration_state_against_longdouble():
    """The state the oracle's iteration leaves each table row in, against longdouble: the accepted candidate within K_STEP64
    units of step_blocks.py, the chord within K_RK4_CHORD of its own unit (the step's, the sensitivity to frac, the
    interpolation's rounding).  Only rows with a stage within 1e-3 r_cut of r_cut are left out: every redo-by-angle row and at
    least six of the nine redo-by-radius rows of a spin are compared."""
    worst_on, worst_chord, at = 0.0, 0.0, None
    for a in re.RK4_SPINS:
        t = re.rk4_table(a)
        o = re.rk4_oracle(a, t, oracle)
        rows, err, keep, chord = re.rk4_state_errors(a, t, o, o["state"], re.U64, oracle)
        kept = [t["names"][r] for r, k in zip(rows, keep) if k]
        assert sum(n.startswith("redo_radius") for n in kept) >= 6 and sum(n.startswith("redo_angle") for n in kept) == 6
        assert (chord & keep).sum() >= 15 and (~chord & keep).sum() >= 40
        worst_on = max(worst_on, err[~chord & keep].max())
        if err[chord & keep].max() > worst_chord:
            i = np.unravel_index(np.argmax(np.where((chord & keep)[:, None], err, 0)), err.shape)
            worst_chord, at = err[chord & keep].max(), (a, t["names"][rows[i[0]]], int(i[1]))
    print(f"oracle RK4 iteration: accepted states {worst_on:.2f} units (K_STEP64 = {re.sb.K_STEP64})")
    assert worst_on <= re.sb.K_STEP64
    _k("K_rk4_chord", worst_chord, re.K_RK4_CHORD, at)


def test_rk4_float32_table_keeps_its_classes():
    """The float32 table's rows are chosen from the reference alone (rk4_f32_stable); no class loses more than 2 % of them."""
    for a in re.RK4_SPINS:
        t = re.rk4_table(a, f32=True, variants=16)
        o = re.rk4_oracle(a, t, oracle)
        stable = re.rk4_f32_stable(a, t, o, oracle)
        cls = np.array([re.rk4_class(n) for n in t["names"]])
        lost = {c: float((~stable[cls == c]).mean()) for c in re.RK4_CLASSES}
        print(f"a = {a}: {len(cls)} rows, lost per class {lost}")
        assert all((cls == c).sum() >= 32 for c in re.RK4_CLASSES) and max(lost.values()) <= 0.02
        assert {4, -1, 1, 2, 0} == set(o["event"][stable].tolist()) and o["attempts"][stable].max() == 7
