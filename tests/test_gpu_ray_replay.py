"""Every production ray equals its replay through the pinned loop body, in every bit.

The production integrate kernels -- the tile loop, the far-field streak, the ghost-lane phase with the packed lone-wave
step, the queue schedule -- are compared with each other elsewhere (test_gpu_parity.py, test_gpu_eq_streak.py,
test_gpu_unit_streak.py, test_gpu_ghost_lanes.py), and with the reference only in the median and at the 99th percentile.
The probes (lt_ic_probe, lt_rk4_advance_probe, lt_dp45_advance_probe, lt_schw_trace_probe, lt_extract_probe) are held to
float64 or longdouble operation by operation (test_gpu_step_blocks.py, test_gpu_dp45_blocks.py, test_gpu_ray_ends.py).  This
file joins the two: each ray of each case of tests/ray_replay.py is run by the batch twins and by lt_render in every
configuration the case admits, and status, winding, steps and the bits of final_alpha must be the replay's on EVERY ray.
No tolerance, no ray left out.  Along the float32 rays of three cases the pinned one-step bound of tests/step_blocks.py is
then held on the states the rays really visit.

What shows that a variant ran: the fixed-quadrant streak by its counter (eq_iters); a retried step by a ray with more steps
than the oracle's ray has iterations; the ghost-lane phase of either schedule by wavefronts of far_observer in which two
rays of different length both run past the schedule's threshold (ray_replay.ghost_phase_waves) -- in every other case the
longest ray takes 383 steps and that phase is never entered.  The streak's unit-step form is switched on and off
(lt_set_unit_streak) and both settings must equal the replay, but the library has no counter that says it was taken.

MEASURED on the MI355X (build 8574001eb171; profiles/ray_replay_8574001eb171.json, LT_RAY_REPLAY_MEASURE=path writes it;
DESIGN.md 2.1):
    every comparison equal: 13 505 Kerr rays per configuration (2.77e6 float32 RK4 steps, longest ray 1 874) and 3 261
      Schwarzschild rays in the batch twins, 12 224 + 3 200 pixels per frame configuration
    wide, float32: 10 476 (direct) / 10 812 (queue) fixed-quadrant iterations, 0 with the switch off
    near_axis: 40 rays retry a halved step (the oracle's own rays: the same 40), 126 refine rays
    far_observer: 18 of 18 batch wavefronts and 15 of 18 frame tiles end lanes inside the ghost-lane phase (both schedules,
      both precisions)
    step bound, sampled states / outside the domain / largest share of the bound:
      wide 12 443 / 287 / 0.065    near_axis 5 936 / 61 / 0.071    critical_curve 12 244 / 533 (4.4 %) / 0.068
    one state below the step classes' radii (a = 1, r = 1.075, p_r = -327, h = 0.05): the float32 step is 441
      units in p_r from longdouble, the reference's float32 arithmetic 43; no bound is stated there and none is held
    wall time of the file: 0.6 s from its first test to its last, 1.2 s with collection (47 tests; the slowest, the first
    call of the library, 0.27 s)
"""
import functools
import json
import os
import time

import numpy as np
import pytest

import ltrace
import ray_replay as rr
import step_blocks as sb

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_RAY_REPLAY_MEASURE")  # a path: the figures the tests print are also written there as JSON
T0 = None      # set when the file's first test starts (the file is imported long before, at collection)
_RECORD = {}

KERR_CONFIGS = [(32, "rk4"), (64, "rk4"), (64, "dp45_exact")]
# when a wavefront turns long (lt_api.hip, read once per process): iterations in the direct schedule, a lane's steps in the queue
LONG = {"direct": int(os.environ.get("LT_D_LONG", "384")), "queue": int(os.environ.get("LT_Q_LONG", "600"))}
SCHEDULES = ("direct", "queue")
COUNTERS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid")
ROW_BLOCK = 8


def stops_at_a_device_error(test):
    """A HIP error in a test of this file ends the session: nothing more is started on a device that may have faulted.
    Every other error of the library is an ordinary failure of the test."""
    @functools.wraps(test)
    def run(*args, **kw):
        global T0
        T0 = T0 or time.time()
        try:
            return test(*args, **kw)
        except ltrace.LtraceError as e:
            if e.code != ltrace.ERR_HIP:
                raise
            pytest.exit(f"HIP error, no further GPU work: {e}", returncode=3)
    return run


def record(key, value):
    _RECORD[key] = value
    _RECORD["wall_seconds_so_far"] = round(time.time() - (T0 or time.time()), 2)
    print(f"{key}: {value}")
    if MEASURE:
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, allow_nan=False)


def counters_of(rep):
    st = np.asarray(rep["status"])
    return dict(rays=int(st.size), steps=int(np.asarray(rep["steps"]).sum()), rhs_evals=int(np.asarray(rep["rhs_evals"]).astype(np.int64).sum()),
                escaped=int((st == 1).sum()), captured=int((st == -1).sum()), invalid=int((st == 0).sum()))


# ---------------------------------------------------------------------------------------------------------------------------
# a. production equals replay: the batch twins
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,integrator", KERR_CONFIGS, ids=[f"{i}_float{p}" for p, i in KERR_CONFIGS])
@pytest.mark.parametrize("name", rr.KERR_CASES)
@stops_at_a_device_error
def test_kerr_batch_equals_replay(name, precision, integrator):
    case = rr.CASES[name]
    al, th, rf = rr.rays(case)
    n = al.size
    rep = rr.replay_kerr(case, precision, integrator)
    for sched in SCHEDULES:
        fa, w, st, ev = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int8), np.empty(n, dtype=np.uint32)
        ltrace.trace_batch_kerr(rr.M, case.a, case.r_obs, al, th, case.theta_obs, rr.lambda_max(case), rf, fa, w, integrator=integrator,
                                precision=precision, schedule=sched, out_status=st, out_rhs_evals=ev)
        msg = rr.explain(case, dict(fa=fa, winding=w, status=st, rhs_evals=ev), rep, count="rhs_evals")
        assert msg is None, f"{sched}: {msg}"
    c = counters_of(rep)
    record(f"batch_{name}_{integrator}_float{precision}", dict(c, longest=int(rep["steps"].max())))
    if case.cut is None:   # a case proves something only if its rays end both ways
        assert c["escaped"] > 0 and c["captured"] > 0
    if name == "far_observer" and integrator == "rk4":
        # c. the ghost-lane phase ran in both schedules: a batch call's wavefronts are 64 consecutive rays
        waves = rep["steps"][:n // 64 * 64].reshape(-1, 64)
        ghost = {s: int(rr.ghost_phase_waves(waves, LONG[s]).sum()) for s in SCHEDULES}
        record(f"batch_{name}_float{precision}_ghost_phase_waves", dict(ghost, waves=int(waves.shape[0])))
        assert min(ghost.values()) > 0


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("name", rr.SCHW_CASES)
@stops_at_a_device_error
def test_schwarzschild_batch_equals_replay(name, precision):
    case = rr.CASES[name]
    al = rr.rays(case)[0]
    n = al.size
    rep = rr.replay_schw(case, precision)
    fa, w, st, ev = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int8), np.empty(n, dtype=np.uint32)
    ltrace.trace_batch_schw(rr.M, case.r_obs, al, fa, w, precision=precision, out_status=st, out_rhs_evals=ev)
    msg = rr.explain(case, dict(fa=fa, winding=w, status=st, rhs_evals=ev), rep, count="rhs_evals")
    assert msg is None, msg
    c = counters_of(rep)
    record(f"batch_{name}_float{precision}", c)
    assert c["escaped"] > 0 and c["captured"] > 0 and c["invalid"] > 0   # (alpha = 0 on the axis pixel: no impact parameter)


# ---------------------------------------------------------------------------------------------------------------------------
# b. the frame path
# ---------------------------------------------------------------------------------------------------------------------------
def render_parts(case, n_parts, **opts):
    """The case's frame through lt_render in n_parts row-block partitions -> (full-frame fa, winding, status, steps (H, W),
    the parts' counters summed, eq_iters summed)."""
    cam, met = rr.camera(case), rr.metric(case)
    out = {k: None for k in ("fa", "winding", "status", "steps")}
    total, eq = dict.fromkeys(COUNTERS, 0), 0
    for part in range(n_parts):
        o = ltrace.default_opts(row_block=ROW_BLOCK, n_parts=n_parts, part=part, **opts)
        assert o.tb_symmetry == 0   # (it substitutes rays)
        r = ltrace.render(cam, met, o, want=tuple(out))
        rows = ltrace.global_rows(case.H, ROW_BLOCK, n_parts, part)
        for k in out:
            if out[k] is None:
                out[k] = np.zeros((case.H, case.W), dtype=r[k].dtype)
            assert r[k].shape == (rows.size, case.W)
            out[k][rows] = r[k]
        for k in COUNTERS:
            total[k] += r["stats"][k]
        eq += r["stats"]["eq_iters"]
    return out, total, eq


def check_frame(case, rep, tag, **opts):
    n = case.W * case.H
    want = {k: np.asarray(v)[:n] for k, v in rep.items() if k in ("fa", "winding", "status", "steps", "rhs_evals")}
    want["winding"] = np.clip(want["winding"], 0, 65535)   # (the frame's winding is a uint16, saturated)
    eq_total = 0
    for n_parts in (1, 3):
        got, total, eq = render_parts(case, n_parts, **opts)
        msg = rr.explain(case, {k: v.ravel() for k, v in got.items()}, want, count="steps")
        assert msg is None, f"{tag}, {n_parts} part(s): {msg}"
        assert total == counters_of(want), (tag, n_parts)
        eq_total += eq
    return eq_total


@pytest.mark.parametrize("name", [n for n in rr.FRAME_CASES if n in rr.KERR_CASES])
@stops_at_a_device_error
def test_kerr_frames_equal_replay(name):
    """lt_render of the case's camera: both schedules, one and three row-block partitions; float32 RK4 with the streak
    switches on and off, float64 RK4, float64 DP45 (exact controller).  Every pixel and the six counters."""
    case = rr.CASES[name]
    eq_seen = {}
    try:
        for sched in SCHEDULES:
            rep = rr.replay_kerr(case, 32, "rk4")
            for eq, unit in ((True, True), (True, False), (False, True), (False, False)):
                ltrace.set_eq_streak(eq)
                ltrace.set_unit_streak(unit)
                seen = check_frame(case, rep, f"rk4 float32 {sched} eq_streak={eq} unit_streak={unit}", integrator="rk4", precision=32,
                                   schedule=sched)
                eq_seen[(sched, eq, unit)] = seen
                assert eq or seen == 0
            ltrace.set_eq_streak(True)
            ltrace.set_unit_streak(True)
            check_frame(case, rr.replay_kerr(case, 64, "rk4"), f"rk4 float64 {sched}", integrator="rk4", precision=64, schedule=sched)
            check_frame(case, rr.replay_kerr(case, 64, "dp45_exact"), f"dp45_exact float64 {sched}", integrator="dp45_exact", precision=64,
                        schedule=sched)
    finally:
        ltrace.set_eq_streak(True)
        ltrace.set_unit_streak(True)
    record(f"frame_{name}_eq_iters", {f"{s}_eq{int(e)}_unit{int(u)}": v for (s, e, u), v in eq_seen.items()})
    if name == "far_observer":   # c. the ghost-lane phase ran: the frame path's wavefronts are 8 x 8 tiles
        for precision in (32, 64):
            waves = rr.frame_waves(case, rr.replay_kerr(case, precision, "rk4")["steps"])
            ghost = {s: int(rr.ghost_phase_waves(waves, LONG[s]).sum()) for s in SCHEDULES}
            record(f"frame_{name}_float{precision}_ghost_phase_tiles", dict(ghost, tiles=int(waves.shape[0])))
            assert min(ghost.values()) > 0
    if name == "wide":   # c. the variant ran: a replay test that never meets a streak proves nothing
        assert eq_seen[("direct", True, True)] > 0 and eq_seen[("queue", True, True)] > 0 and eq_seen[("direct", True, False)] > 0


@pytest.mark.parametrize("name", rr.SCHW_CASES)
@stops_at_a_device_error
def test_schwarzschild_frames_equal_replay(name):
    case = rr.CASES[name]
    for precision in (32, 64):
        check_frame(case, rr.replay_schw(case, precision), f"schwarzschild float{precision}", precision=precision)


# ---------------------------------------------------------------------------------------------------------------------------
# c. the variant ran
# ---------------------------------------------------------------------------------------------------------------------------
@stops_at_a_device_error
def test_near_axis_rays_retry_and_refine():
    """A ray of near_axis takes more RK4 steps than the oracle's ray of the same pixel takes ITERATIONS: a step was halved and
    retried (the oracle itself retried on that ray); refine lanes are in the set."""
    case = rr.CASES["near_axis"]
    o = rr.oracle_rays(case)
    rep = rr.replay_kerr(case, 64, "rk4")
    retried = (rep["steps"] > o["iters"]) & (o["attempts"] > o["iters"])
    record("near_axis_retries", dict(rays_with_a_retry=int(retried.sum()), refine_rays=int(rr.rays(case)[2].sum()),
                                     oracle_rays_with_a_retry=int((o["attempts"] > o["iters"]).sum())))
    assert retried.any() and rr.rays(case)[2].any()
    rep32 = rr.replay_kerr(case, 32, "rk4")
    assert (rep32["steps"] > o["iters"]).any()


# ---------------------------------------------------------------------------------------------------------------------------
# d. the pinned step bound on visited states
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.BOUND_CASES)
@stops_at_a_device_error
def test_step_bound_on_visited_states(name):
    """From the state a float32 ray holds after every 32nd iteration, one more iteration in float32 and one in float64
    (lt_rk4_advance_probe): the difference in the unit A + h u S of tests/step_blocks.py stays within 2 K_STEP, and within
    2 K_FALLBACK (fallback_unit) where the branch-free step is not valid and the lane takes the checked one -- the bounds and
    exclusions of test_gpu_step_blocks.py and of test_gpu_ray_ends.py's float32 decision table, nothing new.  Outside the
    bound's domain (ray_replay.step_domain: no ordinary accepted step, a stage at r_cut, stiff, a radius below the step
    classes'; or the float32 iteration decides otherwise than the float64 one) a state is counted, printed and left out: at most 5 % of the case's samples."""
    case = rr.CASES[name]
    s = rr.replay_states(case, 32, rr.SAMPLE_EVERY)
    m = s["ray"].size
    assert m > 1000 and (s["h_retry"] == 0).all()
    d = rr.step_domain(case, s["state"], s["L"], s["refine"], s["lam"])
    kw = dict(lam=s["lam"], steps=s["steps"], n_iters=1)
    p32 = rr._rk4_probe(case, 32, s["state"], s["L"], s["refine"], **kw)
    p64 = rr._rk4_probe(case, 64, s["state"], s["L"], s["refine"], **kw)
    # both precisions made the oracle's decision: an accepted step of the oracle's size
    lam32 = (s["lam"].astype(np.float32) + d["h"].astype(np.float32)).astype(np.float64)
    same = ((p32["event"] == 4) & (p32["h_retry"] == 0) & (p32["lam"] == lam32) &
            (p64["event"] == 4) & (p64["h_retry"] == 0) & (p64["lam"] == s["lam"] + d["h"]))
    fast = ltrace.kerr_step_probe(rr.M, case.a, s["state"], s["L"], d["h"], refine=s["refine"], precision=32, form="fast")
    valid = sb.fast_step_valid(case.a, fast)
    checked = d["ordinary"] & ~valid
    unit, keep = d["unit"].copy(), d["keep"].copy()
    if checked.any():
        i = np.nonzero(checked)[0]
        with np.errstate(all="ignore"):
            _, unit[i], keep[i] = sb.fallback_unit(case.a, s["state"][i], s["L"][i], d["h"][i], rr.ref_step(case.a))
    # (`same` is no part of the host's cap test, which has no device: a state on which the two precisions decide differently
    # counts as outside here, under the same cap)
    inside = d["ordinary"] & keep & d["covered"] & same & np.isfinite(unit).all(axis=1)
    outside = int((~inside).sum())
    bound = np.where(checked, 2 * sb.K_FALLBACK, 2 * sb.K_STEP)
    with np.errstate(all="ignore"):
        e = np.abs(p32["state"] - p64["state"]) / unit
    share = (e.max(axis=1) / bound)[inside]
    worst = int(np.nonzero(inside)[0][np.argmax(share)])
    record(f"step_bound_{name}", dict(rays=int(np.unique(s["ray"]).size), iterations=int(s["iterations"]), sampled_states=int(m),
                                      out_of_domain=outside, not_ordinary=int((~d["ordinary"]).sum()), excluded_by_unit=int((~keep).sum()),
                                      below_the_classes_radii=int((~d["covered"]).sum()),
                                      decided_differently=int((d["ordinary"] & ~same).sum()), checked_step=int((checked & inside).sum()),
                                      largest_share_of_bound=float(share.max()),
                                      largest_share_checked=float(share[checked[inside]].max()) if (checked & inside).any() else 0.0,
                                      worst_state=s["state"][worst].tolist(), worst_L=float(s["L"][worst]), worst_h=float(d["h"][worst]),
                                      worst_units=e[worst].tolist()))
    assert outside <= rr.DOMAIN_CAP * m, (outside, m)
    assert np.isfinite(share).all() and share.max() <= 1.0


def test_wall_time():
    """(last in the file) The file's wall time from the start of its first test, printed and recorded."""
    record("wall_seconds", round(time.time() - (T0 or time.time()), 2))
