"""What tests/test_dp45_blocks_host.py and tests/test_gpu_dp45_blocks.py share: one attempt of the Dormand-Prince 4(5)
integrator (metrics.py:454-564) in longdouble, the state classes with the step sizes the oracle's own controller settles
on, and the units the candidate state and the error norm of a float64 attempt are stated in.  Built on tests/step_blocks.py
(the scales S, the longdouble right-hand side, the classes, the mpmath helpers).

STEP SIZES come from the oracle alone (oracle.dp45_attempt, the function its tracer runs): from max(1, 0.01 r) the oracle's own
reject factors are applied until the oracle accepts.  That h is a state's ACCEPTED row; 3 h is its REJECTED row (what the
oracle decides there is not asked: the row exists so that the arithmetic is also pinned at an error norm above the
threshold).  `cut_graze` and `turn` have a third row, FIRST: max(1, 0.01 r) itself, where the oracle's sequence starts.  Nearly
every `cut_graze` state has a stage at or inside r_cut there, where the reference's right-hand side jumps to zero: a third
of those rows has a stage radius within 1e-3 of r_cut, so no first-order unit describes them and no class range brings that
under the cap.  They are used for what holds in every bit (the two forms of the attempt, the selection in advance()), not in
the unit.

THE UNIT OF THE CANDIDATE STATE is step_blocks.step_unit with u = 2^-53 and the oracle's DP45 attempt in place of its RK4
step: A_i + h u S_i(y0).  Exclusions as there, from the oracle alone: a stage radius (the state's own included) within
1.002 r_cut, or a stiff step; `cut_graze` takes fallback_unit's ambiguity exclusion instead.  At most EXCLUDED_CAP = 2 % of
a class.

THE UNIT OF THE ERROR NORM.  err_norm = sqrt(sum_i (e_i / sc_i)^2 / 5) with e_i = h sum_s E_s k_s,i is a cancellation between
six stage derivatives, so a relative tolerance says nothing.  Its unit is the first-order propagation, through the longdouble
err_norm, of one float64 rounding
    of each input:               sum_j |err(y0 + 2^-52 |y0_j| e_j) - err(y0)| / 2          (the form of A_i)
    of each stage derivative:    sum_i |q_i| / (5 err) * h sum_s |E_s| 2^-53 S_i(y0) / sc_i,  q_i = e_i / sc_i
    of the result:               2^-53 err.
The second line is the direct effect of a perturbation 2^-53 S_i -- the scale a right-hand side's rounding is stated in,
K_REF of them per evaluation -- of k_s,i on e_i; what the same perturbation does through the later stages is smaller by a
factor h |df/dy| and of the form the first line already holds.

THE BOUNDS, measured by tests/test_dp45_blocks_host.py from the float64 oracle and the longdouble attempt alone and rounded up
to an integer (each asserted there from both sides):
    K_ATT64 = 5   candidate state, accepted and rejected rows (measured 4.69 in p_r: accepted row of `cut_graze` at
                  a = 0.5, state r 1.9050393513396648, theta 1.6891860154293075, phi -4.2243707553964835,
                  p_r -0.9833288358717089, p_theta 6.685045397459971, L 7.802339868369078; at most 4.1 in every other class,
                  all but `near`, `band` and `cut_graze` within 2.9)
    K_ERR64 = 33  error norm (measured 32.34: rejected row of `turn` at a = 0.5, state r 4.842539722348375,
                  theta 0.5081869200473397, phi 0.5829632479458491, p_r 1.470965971679866, p_theta -59.378509564844904,
                  L 3.714408398507109; accepted rows at most 27.4)
A float64 GPU attempt is held to twice these, for the reason of step_blocks.py: merged reciprocals and rotated stage
trigonometry where the reference has a division and a sincos.

POW_TENTH_REL = 2.5e-7: the float32 controller's z^(-1/10) on [1e-30, 1e30] (lt_dp45.hpp states ~2e-7; the emulation of its
statements in the host test reaches 2.1e-7).
"""
import numpy as np

import step_blocks as sb
from oracle import oracle

LD = sb.LD
N = 1501  # states per class: no multiple of 64
R_OBS = 1000.0  # the probes' observer radius: no state of a class is near r_escape = 2 r_obs
K_ATT64 = 5
K_ERR64 = 33
POW_TENTH_REL = 2.5e-7
CLASSES = sb.STEP_CLASSES + ("far_large", "cut_graze", "turn")
CHECKED_CLASSES = ("cut_graze", "turn")  # where the branch-free attempt is not valid: a stage inside r_cut, a large turn

# the reference's coefficients: float64 quotients (metrics.py:335-362), the same values in the oracle and in the kernels
_A = ((1.0 / 5.0,), (3.0 / 40.0, 9.0 / 40.0), (44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0),
      (19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0),
      (9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0))
_B = (35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0)
_E = (71.0 / 57600.0, 0.0, -71.0 / 16695.0, 71.0 / 1920.0, -17253.0 / 339200.0, 22.0 / 525.0, -1.0 / 40.0)


def tolerances(refine):
    refine = np.asarray(refine).astype(bool)
    return np.where(refine, 1e-10, 1e-8), np.where(refine, 1e-8, 1e-6)  # metrics.py:431-432


def ref_attempt_longdouble(a, states, L, h, refine, parts=False):
    """The statements of metrics.py:464-514 on step_blocks.ref_rhs_longdouble: -> (next (n,5), k7 (n,5), err_norm (n,)),
    longdouble.  Every input of the first right-hand side is a float64.  parts=True: also q (n,5) = e_i / sc_i and sc (n,5)."""
    y = np.asarray(states, dtype=np.float64).astype(LD)
    n = y.shape[0]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)).astype(LD)[:, None]
    atol, rtol = (t.astype(LD)[:, None] for t in tolerances(np.broadcast_to(np.asarray(refine), (n,))))
    k = [sb.ref_rhs_longdouble(a, y, L)]
    for row in _A:
        acc = LD(row[0]) * k[0]
        for c, ks in zip(row[1:], k[1:]):
            acc = acc + LD(c) * ks
        k.append(sb.ref_rhs_longdouble(a, y + h * acc, L))
    acc = LD(_B[0]) * k[0]
    for c, ks in zip(_B[2:], k[2:]):
        acc = acc + LD(c) * ks
    nxt = y + h * acc
    k.append(sb.ref_rhs_longdouble(a, nxt, L))
    acc = LD(_E[0]) * k[0]
    for c, ks in zip(_E[2:], k[2:]):
        acc = acc + LD(c) * ks
    sc = atol + rtol * np.maximum(np.abs(y), np.abs(nxt))
    q = h * acc / sc
    err = np.sqrt((q * q).sum(axis=1) / LD(5))
    return (nxt, k[6], err, q, sc) if parts else (nxt, k[6], err)


def dp45_class(name, a, n=N, seed=0):
    """-> (states (n,5), L (n,), refine) at float64 precision (nothing rounded to float32); None if the class does not exist
    at this spin.  The step classes of step_blocks.py, and: far_large r 100 ... 600; cut_graze: fallback_class's first half
    (just outside r_cut and falling); turn: its second half (a polar momentum of 20 ... 60)."""
    if name in sb.STEP_CLASSES:
        c = sb.step_class(name, a, n, seed, rounded=False)
        return None if c is None else (c[0], c[1], c[3])
    if name == "far_large":
        rng = np.random.default_rng([seed, 400, int(round(a * 1000))])
        st, L = sb._states(rng, n, 100.0, 600.0, 0.35, np.pi - 0.35)
        return st, L, 0
    if a > 0.9:  # (as step_blocks' users of fallback_class: not at a = 0.998)
        return None
    st, L, _ = sb.fallback_class(a, 2 * n, seed, rounded=False)
    if name == "cut_graze":
        return st[:n], L[:n], 0
    if name == "turn":
        return st[n:], L[n:], 0
    raise KeyError(name)


def oracle_attempt(a, st, L, h, refine, **kw):
    return oracle.dp45_attempt(st, L, h, sb.M, a, r_obs=R_OBS, lambda_max=1e9, axis_refine=refine, **kw)


def accepted_h(a, st, L, refine):
    """The step size the oracle's controller settles on from max(1, 0.01 r): its own reject / unusable-candidate factors
    applied until it accepts."""
    h = np.maximum(1.0, 0.01 * st[:, 0])
    for _ in range(200):
        o = oracle_attempt(a, st, L, h, refine)
        acc = o["decision"] == 2
        if acc.all():
            return h
        assert (o["event"][~acc] == 4).all()
        h = np.where(acc, h, o["h_next"])
    raise AssertionError("the oracle accepts no step size")


def _ref_step(a, refine):
    def f(st, L, h):
        o = oracle_attempt(a, st, L, h, refine)
        return o["next"], np.concatenate([np.asarray(st)[:, :1], o["stage_r"]], axis=1)
    return f


def err_unit(a, st, L, h, refine):
    """The unit of the error norm (module docstring) -> (err_norm longdouble (n,), unit float64 (n,))."""
    _, _, err, q, sc = ref_attempt_longdouble(a, st, L, h, refine, parts=True)
    unit = sb.U64 * err
    for j in range(5):
        pert = np.array(st, dtype=np.float64)
        pert[:, j] += 2.0 * sb.U64 * np.abs(pert[:, j])
        unit = unit + np.abs(ref_attempt_longdouble(a, pert, L, h, refine)[2] - err) / 2
    hS = (np.asarray(h, dtype=np.float64)[:, None] * sb.scales(a, st, L)).astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        direct = (np.abs(q) * hS * LD(sum(abs(e) for e in _E) * sb.U64) / sc).sum(axis=1) / (5 * err)
    unit = unit + np.where(err > 0, direct, 0)
    return err, unit.astype(np.float64)


_ROWS, _SETS = {}, {}


def dp45_rows(a, name):
    """A class at one spin with its step sizes, from the oracle alone (cheap): st, L, refine (n,), and per row kind
    (`accepted`, `rejected`; `first` for CHECKED_CLASSES) dict(h).  None if the class does not exist."""
    key = (a, name)
    if key not in _ROWS:
        c = dp45_class(name, a)
        if c is None:
            _ROWS[key] = None
            return None
        st, L, rf = c
        refine = np.full(st.shape[0], rf, dtype=np.uint8)
        h_acc = accepted_h(a, st, L, refine)
        rows = dict(accepted=dict(h=h_acc), rejected=dict(h=3.0 * h_acc))
        if name in CHECKED_CLASSES:
            rows["first"] = dict(h=np.maximum(1.0, 0.01 * st[:, 0]))
        _ROWS[key] = dict(st=st, L=L, refine=refine, **rows)
    return _ROWS[key]


def dp45_set(a, name):
    """dp45_rows, with everything a comparison in the units needs, computed once and not changed afterwards: the accepted
    and the rejected row carry h, the longdouble attempt (next, k7, err), the units (unit (n,5) of a state, unit_err (n,)),
    keep (n,) and usable (n,) = keep and the oracle's candidate usable.  None if the class does not exist."""
    key = (a, name)
    if key not in _SETS:
        c = dp45_rows(a, name)
        if c is None:
            _SETS[key] = None
            return None
        st, L, refine = c["st"], c["L"], c["refine"]
        rows = {k: v for k, v in c.items() if k == "first"}
        for kind in ("accepted", "rejected"):
            h = c[kind]["h"]
            unit_fn = sb.fallback_unit if name == "cut_graze" else sb.step_unit
            _, unit, keep = unit_fn(a, st, L, h, _ref_step(a, refine), u=sb.U64)
            nxt, k7, err = ref_attempt_longdouble(a, st, L, h, refine)
            keep = keep & np.isfinite(nxt.astype(np.float64)).all(axis=1)
            _, unit_err = err_unit(a, st, L, h, refine)
            # (a row whose candidate the oracle finds unusable -- non-finite or r <= 0 -- has no error norm)
            usable = keep & (oracle_attempt(a, st, L, h, refine)["decision"] != 0)
            rows[kind] = dict(h=h, next=nxt, k7=k7, err=err, unit=unit, unit_err=unit_err, keep=keep, usable=usable)
        _SETS[key] = dict(st=st, L=L, refine=refine, **rows)
    return _SETS[key]


def sharp_turn_rows(a, n, seed=0):
    """States whose attempt the oracle ACCEPTS although a stage turns by more than 0.25 rad (about one in six of them):
    r 3 ... 5, a polar momentum of 60 ... 200, the oracle's accepted h.  The only accepted attempts that take the checked
    arithmetic in advance(): a stage at or inside r_cut is always rejected.  -> (states, L, h)"""
    rng = np.random.default_rng([seed, 600, int(round(a * 1000))])
    st, L = sb._states(rng, n, 3.0, 5.0, 0.5, np.pi - 0.5)
    st[:, 4] = rng.choice([-1.0, 1.0], n) * rng.uniform(60.0, 200.0, n)
    return st, L, accepted_h(a, st, L, np.zeros(n, dtype=np.uint8))


def pow_minus_tenth_emulated(z):
    """The statements of pow_minus_tenth (lt_dp45.hpp) on an array of float32, the fused multiply-add as a float64 product
    and sum rounded once to float32 (the product of two float32 is exact in float64; the sum's double rounding differs from
    the fma in a vanishing share of cases: a cross-check, the GPU test measures the kernel's own)."""
    f = np.float32
    z = np.asarray(z, dtype=f)
    with np.errstate(all="ignore"):
        v = f(1171454846.0) - f(0.1) * z.view(np.uint32).astype(f)
        y = np.where(np.isfinite(v) & (v >= 0) & (v < 2.0 ** 32), v, 0).astype(np.uint32).view(f)
        for _ in range(3):
            y2 = y * y
            y4 = y2 * y2
            y5 = y4 * y
            y10 = y5 * y5
            t = (-(z.astype(np.float64)) * y10.astype(np.float64) + 1.0).astype(f)
            t = f(0.1) * t
            y = (y.astype(np.float64) * t.astype(np.float64) + y.astype(np.float64)).astype(f)
    return y
