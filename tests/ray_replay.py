"""What tests/test_gpu_ray_replay.py and tests/test_ray_replay_host.py share: small sets of real camera rays, their replay
through the probes of the pinned loop body, and the comparison that holds a production ray to its replay.

THE CHAIN.  The production integrate kernels (tile loop, far-field streak, ghost-lane phase with its packed lone-wave
step, queue schedule; the streak's unit-step form is switched on and off, but no counter says that it ran) are held to
each other byte for byte by test_gpu_parity.py, test_gpu_eq_streak.py,
test_gpu_unit_streak.py and test_gpu_ghost_lanes.py; one step, one attempt, one loop iteration and a ray's two ends are
held to float64 or longdouble on synthetic states through the probe kernels (test_gpu_step_blocks.py,
test_gpu_dp45_blocks.py, test_gpu_ray_ends.py).  Here a whole production ray is replayed through those probes:
    lt_ic_probe -> lt_rk4_advance_probe / lt_dp45_advance_probe / lt_schw_trace_probe -> lt_extract_probe
and must equal the production result in every bit, ray by ray.  There is no tolerance and no ray is left out.

THE CASES are cameras (lt_pixel_angles: axis-refine columns occur as in a frame), each a few thousand rays.  A case's ray
set is the frame's pixels in row-major order followed by its first `rem` pixels again, so that a batch call is a whole
number of wavefronts plus a ragged remainder and still contains every pixel; the `ragged` cases are the first n rays of
`wide`.  lambda_max is the frame path's (metrics.py:1132).

THE STEP BOUND ON VISITED STATES (step_domain): a state a float32 ray visits at a reference-iteration boundary is inside the
domain of the one-step bound of tests/step_blocks.py where the float64 oracle's iteration from it (lto_rk4_iteration)
accepts one ordinary step -- no retry, no chord, range not exhausted --, step_blocks.step_unit keeps it (no float64 stage
radius within 1.002 r_cut, not stiff) and its radius is one the step classes cover at the case's spin
(step_blocks.step_r_min: K_STEP was derived down to 1.05 r_plus, and to 1.3 r_plus at a > 0.9, where `near` is no class;
below that no one-step bound is stated, and this file states none).  Nothing else is a domain; at most DOMAIN_CAP of a case's
samples may lie outside it.
"""
import functools
from collections import namedtuple

import numpy as np

import ray_ends as re
import step_blocks as sb
from oracle import oracle

M = re.M
KERR, SCHW = 1, 0                       # ltrace.METRIC_KERR, ltrace.METRIC_SCHWARZSCHILD
DOMAIN_CAP = 0.05
MAX_ITERS = 1 << 22                     # above any ray's length: lambda_max / h_floor is 6e5 attempts
SAMPLE_EVERY = 32

Case = namedtuple("Case", "name kind W H vfov a r_obs theta_obs psi_x rem cut")


def _case(name, kind, W, H, vfov_deg=40.0, a=0.0, r_obs=50.0, theta_obs=np.pi / 2, psi_x=0.0, rem=0, cut=None):
    return Case(name, kind, W, H, float(np.radians(vfov_deg)), a, r_obs, theta_obs, psi_x, rem, cut)


_WIDE = dict(kind=KERR, W=72, H=40, a=0.9)
CASES = {c.name: c for c in (
    _case("wide", rem=37, **_WIDE),
    _case("near_axis", KERR, 40, 40, a=0.998, theta_obs=0.005, rem=63),      # refine lanes, retried steps
    # aimed 0.09 rad to the side, at the prograde edge of the shadow: looking straight at the hole, two thirds of the rays are
    # captured and 6.3 % of the states the oracle's rays visit lie outside the step bound's domain (step_domain; 4.4 % here)
    _case("critical_curve", KERR, 64, 48, vfov_deg=8.0, a=1.0, psi_x=-0.09, rem=1),
    _case("retrograde", KERR, 48, 40, a=-0.7, theta_obs=1.0, rem=29),
    _case("close", KERR, 40, 40, a=0.3, r_obs=12.0, rem=5),
    # every RK4 ray runs 900 steps and more (1 800 on the refine columns): the only rays long enough for the ghost-lane
    # phase of either schedule and the lone-wave step (ghost_phase_waves); the other cases' longest ray takes 383
    _case("far_observer", KERR, 48, 24, vfov_deg=5.0, a=0.9, r_obs=300.0, rem=17),
    _case("schw_r12", SCHW, 40, 40, r_obs=12.0, rem=11),
    _case("schw_r50", SCHW, 40, 40, r_obs=50.0, rem=50),
    _case("ragged_1", cut=1, **_WIDE), _case("ragged_63", cut=63, **_WIDE), _case("ragged_65", cut=65, **_WIDE),
    _case("ragged_1000", cut=1000, **_WIDE))}
KERR_CASES = [n for n, c in CASES.items() if c.kind == KERR]
SCHW_CASES = [n for n, c in CASES.items() if c.kind == SCHW]
FRAME_CASES = [n for n, c in CASES.items() if c.cut is None]
BOUND_CASES = ["wide", "near_axis", "critical_curve"]


def hfov(case):
    return float(2.0 * np.arctan(np.tan(case.vfov / 2.0) * case.W / case.H))


def lambda_max(case):
    return max(5000.0, 6.0 * case.r_obs)


def ray_index(case):
    """The pixel (row-major) of every ray of the case's set."""
    n = case.W * case.H
    return np.arange(case.cut) if case.cut is not None else np.concatenate([np.arange(n), np.arange(case.rem)])


def camera(case):
    import ltrace
    return ltrace.Camera(case.W, case.H, hfov(case), case.vfov, 0.0, case.psi_x, case.r_obs, case.theta_obs)


def metric(case):
    import ltrace
    return ltrace.Metric(case.kind, 0, M, case.a)


@functools.lru_cache(maxsize=None)
def _pixels(name, source):
    case = CASES[name]
    if source == "device":
        import ltrace
        al, th, cols = ltrace.pixel_angles(camera(case))
    else:
        al, th, cols = oracle.pixel_angles(case.H, case.W, hfov(case), case.vfov, psi=(0.0, case.psi_x))
    refine = np.broadcast_to(cols.astype(np.uint8), (case.H, case.W))
    return al.astype(np.float64).ravel(), th.ravel().copy(), refine.ravel().copy()


def rays(case, source="device"):
    """-> (alpha, theta float64, refine uint8), each (n,): the case's rays from the device's lt_pixel_angles, or
    (source="oracle") from the oracle's on the host."""
    i = ray_index(case)
    return tuple(x[i] for x in _pixels(case.name, source))


# ---------------------------------------------------------------------------------------------------------------------------
# the replay
# ---------------------------------------------------------------------------------------------------------------------------
def _kerr_start(case, precision):
    """-> (ok (n,) bool, state (n,5), L (n,), refine (n,)) from lt_ic_probe, the state as ray_start sets it."""
    import ltrace
    al, th, rf = rays(case)
    n = al.size
    rec = ltrace.ic_probe(KERR, M, case.a, case.r_obs, case.theta_obs, al, th, rf, precision=precision)
    assert rec.shape[0] == (n + 63) // 64 * 64 and (rec[n:, 3] == ltrace.FLAG_PAD).all()
    rec = rec[:n]
    flags = rec[:, 3].astype(int)
    assert np.array_equal((flags & ltrace.FLAG_REFINE) != 0, rf != 0) and not (flags & ltrace.FLAG_PAD).any()
    st = np.zeros((n, 5))
    st[:, 0], st[:, 1], st[:, 3], st[:, 4] = case.r_obs, case.theta_obs, rec[:, 0], rec[:, 1]
    return (flags & ltrace.FLAG_OK) != 0, st, rec[:, 2].copy(), rf


def _rk4_probe(case, precision, st, L, rf, **kw):
    import ltrace
    return ltrace.rk4_advance_probe(M, case.a, st, L, rf, precision=precision, r_obs=case.r_obs, lambda_max=lambda_max(case), **kw)


@functools.lru_cache(maxsize=None)
def _replay_kerr(name, precision, integrator):
    import ltrace
    case = CASES[name]
    ok, st, L, rf = _kerr_start(case, precision)
    n = ok.size
    event, steps = np.full(n, ltrace.EV_INVALID), np.zeros(n, dtype=np.int64)
    i = np.nonzero(ok)[0]
    if i.size:
        if integrator == "rk4":
            p = _rk4_probe(case, precision, st[i], L[i], rf[i], n_iters=MAX_ITERS)
        else:
            assert integrator == "dp45_exact" and precision == 64
            p = ltrace.dp45_advance_probe(M, case.a, st[i], L[i], max(1.0, 0.01 * case.r_obs), refine=rf[i], exact=True,
                                          n_attempts=MAX_ITERS, r_obs=case.r_obs, lambda_max=lambda_max(case))
        assert (p["event"] != ltrace.EV_RUNNING).all()
        st[i], event[i], steps[i] = p["state"], p["event"], p["steps"]
    fin = np.concatenate([st, L[:, None]], axis=1)
    x = ltrace.extract_probe(KERR, M, case.a, *re.kerr_fin(fin, event, steps=steps), precision=precision, integrator=integrator)
    return dict(fa=x["fa"], winding=x["winding"], status=x["status"], steps=steps, rhs_evals=x["evals"], event=event, state=st)


def replay_kerr(case, precision, integrator="rk4"):
    """The case's rays from the prologue's records through the advance probe to their end and through the epilogue.
    -> dict(fa, winding, status, steps, rhs_evals, event, state); computed once per (case, precision, integrator)."""
    return _replay_kerr(case.name, precision, integrator)


@functools.lru_cache(maxsize=None)
def _replay_schw(name, precision, phi_max, h_max):
    import ltrace
    case = CASES[name]
    al = rays(case)[0]
    n = al.size
    rec = ltrace.ic_probe(SCHW, M, 0.0, case.r_obs, np.pi / 2, al, precision=precision)[:n]
    ok = (rec[:, 3].astype(int) & ltrace.FLAG_OK) != 0
    u, w, phi_last = np.full(n, 1.0 / case.r_obs), rec[:, 0].copy(), np.zeros(n)
    event, steps, full = np.full(n, ltrace.EV_INVALID), np.zeros(n, dtype=np.int64), np.zeros(n)
    i = np.nonzero(ok)[0]
    if i.size:
        p = ltrace.schw_trace_probe(M, case.r_obs, u[i], w[i], phi_max=phi_max, h_max=h_max, precision=precision)
        u[i], w[i], phi_last[i], event[i], steps[i], full[i] = p["u"], p["w"], p["phi_last"], p["event"], p["steps"], p["full_steps"]
    fin0 = np.stack([u, w, phi_last, full], axis=1)
    fin1 = np.stack([np.zeros(n), np.zeros(n), event.astype(np.float64), steps.astype(np.float64)], axis=1)
    x = ltrace.extract_probe(SCHW, M, 0.0, fin0, fin1, precision=precision, h_schw=h_max)
    return dict(fa=x["fa"], winding=x["winding"], status=x["status"], steps=steps, rhs_evals=x["evals"], event=event)


def replay_schw(case, precision, phi_max=50.0, h_max=0.05):
    """The same through lt_schw_trace_probe from the observer's own start (u = 1 / r_obs, w from the prologue's record)."""
    return _replay_schw(case.name, precision, phi_max, h_max)


def replay_states(case, precision, every=SAMPLE_EVERY):
    """The RK4 replay in calls of `every` iterations -> dict(ray, state (m,5), L, refine, lam, h_retry, steps): what the rows
    that are still running hold after each call, kept only where the row stands at a reference-iteration boundary
    (h_retry == 0); and `iterations`, every iteration made."""
    import ltrace
    ok, st, L, rf = _kerr_start(case, precision)
    idx = np.nonzero(ok)[0]
    cur = dict(state=st[idx], lam=np.zeros(idx.size), h_retry=np.zeros(idx.size), steps=np.zeros(idx.size, dtype=np.int64))
    out = {k: [] for k in ("ray", "state", "lam", "h_retry", "steps")}
    iterations = 0
    for _ in range(MAX_ITERS // every):
        if idx.size == 0:
            break
        p = _rk4_probe(case, precision, cur["state"], L[idx], rf[idx], lam=cur["lam"], h_retry=cur["h_retry"], steps=cur["steps"],
                       n_iters=every)
        iterations += int(p["iters"].sum())
        run = p["event"] == ltrace.EV_RUNNING
        at = run & (p["h_retry"] == 0)
        out["ray"].append(idx[at])
        for k in ("state", "lam", "h_retry", "steps"):
            out[k].append(p[k][at])
        idx = idx[run]
        cur = {k: p[k][run] for k in ("state", "lam", "h_retry", "steps")}
    assert idx.size == 0
    res = {k: np.concatenate(v) for k, v in out.items()}
    res["L"], res["refine"], res["iterations"] = L[res["ray"]], rf[res["ray"]], iterations
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------------
def same_bits(x, y):
    """Elementwise: two float arrays of one type have the same bit pattern (a NaN equals a NaN)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    assert x.dtype == y.dtype and x.dtype.kind == "f" and x.shape == y.shape
    ui = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    return (x.view(ui) == y.view(ui)) | (np.isnan(x) & np.isnan(y))


def differing(got, want, count="steps"):
    """-> (n,) bool: the rays on which a production result `got` departs from the replay `want` in status, winding, the
    count (`steps` or `rhs_evals`) or a bit of fa.  fa is compared in got's type: a frame's float32 against the replay's
    angle rounded to float32, a batch call's float64 as it is.  A result's fa must be a NaN wherever the ray did not escape."""
    fa = np.asarray(got["fa"])
    bad = ~same_bits(fa, np.asarray(want["fa"]).astype(fa.dtype))
    bad |= ~np.isnan(fa) & (np.asarray(got["status"]) != 1)
    for k in ("status", "winding", count):
        bad |= np.asarray(got[k]).astype(np.int64) != np.asarray(want[k]).astype(np.int64)
    return bad


def explain(case, got, want, count="steps", index=None, source="device"):
    """None if `got` equals `want` on every ray; else a message with the number of differing rays and the first one's
    (alpha, theta, refine), its step count and both sides.  index: the ray of each entry (default: the case's own order);
    source: where the quoted angles come from (rays)."""
    bad = differing(got, want, count)
    if not bad.any():
        return None
    al, th, rf = rays(case, source)
    j = int(np.argmax(bad))
    i = j if index is None else int(np.asarray(index)[j])
    fa = np.asarray(got["fa"])
    side = lambda r, k, dt=None: np.asarray(r[k]).astype(dt or np.asarray(r[k]).dtype)[j]  # noqa: E731
    fmt = lambda r, dt: (f"fa={float(side(r, 'fa', dt))!r} (bits {side(r, 'fa', dt).tobytes()[::-1].hex()}) status={int(side(r, 'status'))} "  # noqa: E731
                         f"winding={int(side(r, 'winding'))} {count}={int(side(r, count))}")
    return (f"{case.name}: {int(bad.sum())} of {bad.size} rays differ; first: entry {j}, ray {i}, alpha={float(al[i])!r}, theta={float(th[i])!r}, "
            f"refine={int(rf[i])}, steps={int(np.asarray(want['steps'])[j])}\n  production: {fmt(got, fa.dtype)}\n  replay:     {fmt(want, fa.dtype)}")


def ghost_phase_waves(steps, long_steps):
    """steps (w, 64): the step counts of the rays that share a wavefront -> (w,) bool: the wavefront entered the ghost-lane
    phase and lanes ended INSIDE it.  A lane takes at most one step per iteration its wave issues, so a ray of more than
    long_steps steps was still running when the wave turned long (direct schedule: LT_D_LONG iterations; queue schedule:
    a lane past LT_Q_LONG steps, the queue drained); where two such rays of one wave differ in length, the shorter one
    ended in that phase -- stored by its real lane -- and its lane went on as a ghost of a lane still running."""
    s = np.asarray(steps).reshape(-1, 64)
    shortest_long = np.where(s > long_steps, s, np.iinfo(np.int64).max).min(axis=1)
    return (s.max(axis=1) > long_steps) & (shortest_long < s.max(axis=1))


def frame_waves(case, x):
    """(H * W,) row-major -> (tiles, 64): the frame path's wavefronts, 8 x 8 pixel tiles."""
    assert case.H % 8 == 0 and case.W % 8 == 0
    return np.asarray(x)[:case.H * case.W].reshape(case.H // 8, 8, case.W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


# ---------------------------------------------------------------------------------------------------------------------------
# the one-step bound's domain, and the oracle's own rays (host)
# ---------------------------------------------------------------------------------------------------------------------------
def ref_step(a):
    return lambda st, L, h: oracle.rk4_step_kerr(st, L, h, M, a)


def step_domain(case, state, L, refine, lam):
    """For states (m,5) at reference-iteration boundaries -> dict(h, ordinary, y1, unit, keep, inside): the float64 oracle's
    iteration from each (its step size h; `ordinary`: it accepts the first attempt and the ray goes on), the float64 step of
    that size with its unit and exclusions exactly as test_gpu_step_blocks.py takes them (step_blocks.step_unit), `covered`:
    the radius is inside the step classes' range at this spin, and inside = ordinary & keep & covered."""
    state = np.asarray(state, dtype=np.float64).reshape(-1, 5)
    if state.shape[0] == 0:
        z = np.zeros(0, dtype=bool)
        return dict(h=np.zeros(0), ordinary=z, y1=state, unit=state, keep=z, covered=z, inside=z)
    o = oracle.rk4_iteration(state, L, lam, M, case.a, r_obs=case.r_obs, lambda_max=lambda_max(case), axis_refine=refine)
    ordinary = (o["event"] == 4) & (o["attempts"] == 1)
    h = np.where(ordinary, o["h"], 1.0)
    with np.errstate(all="ignore"):
        y1, unit, keep = sb.step_unit(case.a, state, L, h, ref_step(case.a))
    keep = keep & np.isfinite(unit).all(axis=1)
    covered = state[:, 0] >= sb.step_r_min(case.a)
    return dict(h=h, ordinary=ordinary, y1=y1, unit=unit, keep=keep, covered=covered, inside=ordinary & keep & covered)


@functools.lru_cache(maxsize=None)
def _oracle_rays(name, every):
    case = CASES[name]
    al, th, rf = rays(case, "oracle")
    n = al.size
    st, L, ok = np.zeros((n, 5)), np.zeros(n), np.zeros(n, dtype=bool)
    for i in range(n):
        ok[i], st[i], _, L[i] = oracle.kerr_ic(M, case.a, case.r_obs, al[i], th[i], case.theta_obs)
    iters, attempts, event = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    idx, lam = np.nonzero(ok)[0], np.zeros(int(ok.sum()))
    cur = st[idx]
    samples = {k: [] for k in ("ray", "state", "lam")}
    it = 0
    while idx.size:
        o = oracle.rk4_iteration(cur, L[idx], lam, M, case.a, r_obs=case.r_obs, lambda_max=lambda_max(case), axis_refine=rf[idx])
        it += 1
        run = o["event"] == 4
        iters[idx] += 1
        attempts[idx] += o["attempts"]
        event[idx[~run]] = o["event"][~run]
        idx, cur, lam = idx[run], o["state"][run], o["lam"][run]
        if it % every == 0:
            samples["ray"].append(idx.copy()); samples["state"].append(cur.copy()); samples["lam"].append(lam.copy())
        assert it < MAX_ITERS
    s = {k: (np.concatenate(v) if v else np.zeros((0, 5) if k == "state" else 0, dtype=np.int64 if k == "ray" else float))
         for k, v in samples.items()}
    s["L"], s["refine"] = L[s["ray"]], rf[s["ray"]]
    return dict(ok=ok, iters=iters, attempts=attempts, event=event, samples=s)


def oracle_rays(case, every=SAMPLE_EVERY):
    """The case's rays through the float64 oracle's own iteration (lto_rk4_iteration) on the host, from the oracle's pixel
    angles and records -> dict(ok, iters (reference iterations), attempts (RK4 steps: iterations plus retries), event, and
    samples: ray, state, lam, L, refine of the rays still running after every `every`-th iteration)."""
    return _oracle_rays(case.name, every)
