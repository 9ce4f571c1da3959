"""What tests/test_dense_blocks_host.py and tests/test_gpu_dense_blocks.py share: the dense-trajectory integrator
(geodesic_tracer.py:22-71: solve_ivp RK45 on metrics.py:763-790 / :946-1029; oracle/lt_oracle_dense.c; lt_dense.hpp
k_dense_tracks) restated block by block in longdouble, vectorised over rows, the units its float64 errors are stated in,
and the REPLAY of a record.

THE REPLAY.  A record holds every accepted point (t_p, y_p), so y_{p+1} is ONE Dormand-Prince step from y_p with
h_p = t_{p+1} - t_p.  The longdouble step started from the record's own float64 y_p bounds y_{p+1} per component: no chaos, no
probe of the integrator.  The controller is pinned the same way: the trial size of step p + 1 is h_p times the reference's
factor on the longdouble error norm of step p; the reference's accept / reject loop is run from there in longdouble at the
record's y_{p+1}; the record's h_{p+1} must be the loop's, and the loop's attempts, summed over a track, (nfev - 2) / 6.

THE UNIT OF THE RIGHT-HAND SIDE.  u = 2^-53.  tests/step_blocks.py's scales with E = -p_t a variable: from
    s2 = sin^2 theta (floored at 1e-15 in the Schwarzschild class only), ra = r^2 + a^2, Sigma = ra - a^2 s2, Delta = ra - 2 M r,
    P = E ra - a L, D = L - a E s2, q = P / Delta,
    k_Delta = (ra + 2 M r) / Delta, k_P = (|E| ra + |a L|) / |P|, k_q = 1 + k_Delta + k_P     (the cancellations in Delta, P)
    S_F   = Delta p_r^2 (1 + k_Delta) + p_theta^2 + L^2 / s2 + 2 |a E L| + a^2 E^2 s2 + |P q| k_q     (holds the one in D^2 / s2)
    S_dt  = (|a| (|L| + |a E| s2) + ra |q| k_q) / Sigma
    S_dr  = |Delta p_r / Sigma| (1 + k_Delta)
    S_dth = |p_theta / Sigma|
    S_dph = (|a q| k_q + |L| / s2 + |a E|) / Sigma
    S_dpr = [ |r - M| (2 q^2 k_q + p_r^2) + r (2 |E q| k_q + S_F / Sigma) ] / Sigma
    S_dpth = |sin theta cos theta| (a^2 E^2 + a^2 S_F / Sigma + (L / s2)^2) / Sigma
the sum of the magnitudes of the terms each output is formed from; the cyclic rows (p_t, p_phi) have no unit: they are +0.0.
One term more, for what no float64 sincos with a two-word reduction can give: next to a multiple k of pi / 2 the reduced angle
is off by up to REDUCTION |k| = 1.4e-26 |k| -- an absolute error of the small one of sin and cos, not an ulp of it (derived and
pinned for M<double>::sincos in tests/test_gpu_step_blocks.py).  At theta = fl(pi / 2), where cos theta = 6.1e-17 is all of
p_theta', that is 5e5 u |p_theta'| and 3.5e-27 in absolute terms.  S_dpth takes REDUCTION |k| / u times (|sin| + |cos|) times
its bracket, and the terms in 1 / s2 of S_dph, S_dpr and S_dpth the same as a relative error 2 REDUCTION |k| / |sin| of s2.

ONE STEP.  The unit of component i of an attempt of size h from y0 is A_i + h u sum_s |b_s| S_i(Y_s) over the stage states Y_s,
    A_i = sum_j |y1_i(y0 + 2^-52 |y0_j| e_j) - y1_i(y0)| / 2 + u |y1_i|,  j over r, theta, p_r, p_theta
(t and phi enter no right-hand side; p_t and p_phi are carried bit for bit): the first-order propagation, through the longdouble
step, of one float64 rounding of each input, plus the rounding of the result.  The perturbed copies are stacked into the same
arrays: the cost is width, not calls.  THE ERROR NORM, a cancellation between seven stage derivatives, has a unit of its own as
in tests/dp45_blocks.py: u err + sum_j |err(y0 + ...) - err| / 2 + sum_i |q_i| h sum_s |E_s| T_s,i / (8 err sc_i), where
T_s,i = u S_i(Y_s) + sum_j |k_s,i(y0 + ...) - k_s,i(y0)| / 2 is the error of stage derivative s: its evaluation, and one rounding of
each input of its own stage state (seven independent roundings, on which the norm's cancellation between the stages does not act:
next to the axis, where d f / d theta is of the order 1 / sin^2, they are all of the norm's error).
THE INITIAL STEP: u h + sum_j |h(y0 + ...) - h| / 2 + 0.2 h (direct effect of u S on the norm that binds, d1 or d2).
THE EVENT: the dense output at te has the step's unit with |p_s(x)| for |b_s|; the event time's residual is held to Brent's stated
tolerance 4 eps (1 + |te|) times |r'(te)| plus that unit.

LEFT OUT (at most EXCLUDED_CAP of a class): a point or stage at or inside 1.001 r_plus (the right-hand side jumps to zero), a
non-finite value, and a decision whose longdouble error norm lies within k units of 1 together with the step after it (whose
`rejected` flag is then unknown); k = K_ERR for the float64 oracle, 2 K_ERR for the device.

THE BOUNDS, measured by tests/test_dense_blocks_host.py from the float64 oracle's blocks and the longdouble restatement alone and
rounded up to an integer (each asserted there from both sides); worst rows are printed by that test and stand in DESIGN.md 10:
    K_RHS8, K_ATT, K_ERR, K_H0, K_EVENT  (below)
The device is held to TWICE each: its form adds the merged reciprocal, fused multiply-adds, its own sincos and the stage rotation.
"""
import numpy as np

from oracle import oracle

LD = np.longdouble
M = 1.0
U = 2.0 ** -53
EPS = 2.0 ** -52
EXCLUDED_CAP = 0.02
REDUCTION = 1.4e-26  # per multiple of pi / 2: the absolute error of a two-word argument reduction (see the module docstring)
SPINS = ((0, 0.0), (1, 0.9), (1, 0.998), (1, 1.0))  # (kind, a) of the replayed batches
RHS_SPINS = ((0, 0.0), (1, 0.0), (1, 0.5), (1, 0.9), (1, 0.998), (1, 1.0))
RTOL, ATOL, MAX_STEP, LAMBDA_MAX = 1e-8, 1e-10, 1.0, 1000.0
R_OBS = 50.0
N_TRACKS = 128
NONCYCLIC = (0, 1, 2, 3, 5, 6)
PERTURBED = (1, 2, 5, 6)

K_RHS8 = dict(far=8, near_horizon=34, pole=21, equator=3, energy=9, off_shell=7)
K_ATT = dict(seeded=2, sharp=5)
K_ERR = 5
K_H0 = 3
K_EVENT = 3

_A = ((1.0 / 5,), (3.0 / 40, 9.0 / 40), (44.0 / 45, -56.0 / 15, 32.0 / 9),
      (19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729),
      (9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656))
_B = (35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84)
_E = (-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40)
_P = ((1, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432),
      (0, 0, 0, 0),
      (0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799),
      (0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072),
      (0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632),
      (0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844),
      (0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423))


def r_plus(a):
    return M + np.sqrt(M * M - a * a)


def r_zero(a):
    """The float64 threshold both the oracle and the device compare r with."""
    return 1.001 * r_plus(a)


def r_capture(a):
    return 1.01 * r_plus(a)


# ---- the right-hand side -----------------------------------------------------------------------------------------------------------
def rhs8_ld(kind, a, Y):
    """The reference's own expressions (metrics.py:763-790 kind 0, :946-1029 kind 1; oracle/lt_oracle_dense.c) in longdouble:
    Y (n, 8) -> (n, 8).  Zero at and inside 1.001 r_plus."""
    Y = np.asarray(Y, dtype=LD)
    r, th, p_t, p_r, p_th, p_phi = Y[:, 1], Y[:, 2], Y[:, 4], Y[:, 5], Y[:, 6], Y[:, 7]
    o = np.zeros(Y.shape, dtype=LD)
    sn, cs = np.sin(th), np.cos(th)
    r2 = r * r
    with np.errstate(all="ignore"):
        if kind == 0:
            R_S = LD(2.0 * M)
            f = 1 - R_S / r
            s2 = np.maximum(sn * sn, LD(1e-15))
            o[:, 0] = -p_t / f
            o[:, 1] = f * p_r
            o[:, 2] = p_th / r2
            o[:, 3] = p_phi / (r2 * s2)
            o[:, 5] = (-(R_S / (2 * r2)) * (p_t * p_t / (f * f)) - (R_S / (2 * r2)) * (p_r * p_r)
                       + (p_th * p_th + p_phi * p_phi / s2) / (r2 * r))
            o[:, 6] = cs * (p_phi * p_phi) / (r2 * s2 * sn)
            inside = Y[:, 1].astype(np.float64) <= 2.0 * M * 1.001
        else:
            al, Mq = LD(a), LD(M)
            a2, s2 = al * al, sn * sn
            Sigma = r2 + a2 * (cs * cs)
            Delta = r2 - 2 * Mq * r + a2
            A = (r2 + a2) * (r2 + a2) - a2 * Delta * s2
            SD = Sigma * Delta
            g_tt, g_tp, g_rr, g_thth = -A / SD, -2 * Mq * al * r / SD, Delta / Sigma, 1 / Sigma
            g_pp = (Delta - a2 * s2) / (SD * s2)
            o[:, 0] = g_tt * p_t + g_tp * p_phi
            o[:, 1] = g_rr * p_r
            o[:, 2] = g_thth * p_th
            o[:, 3] = g_tp * p_t + g_pp * p_phi
            dS, dD = 2 * r, 2 * r - 2 * Mq
            dA = 4 * r * (r2 + a2) - a2 * dD * s2
            SD2, S2 = SD * SD, Sigma * Sigma
            mix = dS * Delta + Sigma * dD
            d_tt = -(dA * Sigma * Delta - A * mix) / SD2
            d_tp = -(2 * Mq * al * (SD - r * mix)) / SD2
            d_rr = (dD * Sigma - Delta * dS) / S2
            d_thth = -dS / S2
            den = SD * s2
            d_pp = (dD * Sigma * Delta * s2 - (Delta - a2 * s2) * mix * s2) / (den * den)
            o[:, 5] = -LD(0.5) * (d_tt * (p_t * p_t) + 2 * d_tp * p_t * p_phi + d_rr * (p_r * p_r) + d_thth * (p_th * p_th)
                                  + d_pp * (p_phi * p_phi))
            dSt = -2 * a2 * sn * cs
            dAt = -a2 * Delta * 2 * sn * cs
            h_tt = -(dAt * Sigma * Delta - A * dSt * Delta) / SD2
            h_tp = 2 * Mq * al * r * dSt / (S2 * Delta)
            h_rr = -Delta * dSt / S2
            h_thth = -dSt / S2
            num = Delta - a2 * s2
            dnum = -a2 * 2 * sn * cs
            dden = dSt * Delta * s2 + Sigma * Delta * 2 * sn * cs
            h_pp = (dnum * den - num * dden) / (den * den)
            o[:, 6] = -LD(0.5) * (h_tt * (p_t * p_t) + 2 * h_tp * p_t * p_phi + h_rr * (p_r * p_r) + h_thth * (p_th * p_th)
                                  + h_pp * (p_phi * p_phi))
            inside = Y[:, 1].astype(np.float64) <= r_zero(a)
    o[inside] = 0
    o[:, 4] = 0
    o[:, 7] = 0
    return o


def scales8(kind, a, Y):
    """S (n, 8) of the module docstring, longdouble arithmetic, float64 out; the cyclic columns are 0."""
    Y = np.asarray(Y, dtype=LD)
    r, th, E, pr, pth, L = Y[:, 1], Y[:, 2], -Y[:, 4], Y[:, 5], Y[:, 6], Y[:, 7]
    al, Mq = LD(a if kind else 0.0), LD(M)
    sn, cs = np.sin(th), np.cos(th)
    s2 = np.maximum(sn * sn, LD(1e-15)) if kind == 0 else sn * sn
    S = np.zeros(Y.shape, dtype=LD)
    with np.errstate(all="ignore"):
        ra = r * r + al * al
        Sigma = ra - al * al * s2
        Delta = ra - 2 * Mq * r
        P = E * ra - al * L
        q = P / Delta
        kD = (ra + 2 * Mq * r) / Delta
        kP = (np.abs(E) * ra + np.abs(al * L)) / np.abs(P)
        kq = 1 + kD + kP
        SF = (Delta * pr * pr * (1 + kD) + pth * pth + L * L / s2 + 2 * np.abs(al * E * L) + al * al * E * E * s2
              + np.abs(P * q) * kq)
        S[:, 0] = (np.abs(al) * (np.abs(L) + np.abs(al * E) * s2) + ra * np.abs(q) * kq) / Sigma
        S[:, 1] = np.abs(Delta * pr / Sigma) * (1 + kD)
        S[:, 2] = np.abs(pth / Sigma)
        S[:, 3] = (np.abs(al * q) * kq + np.abs(L) / s2 + np.abs(al * E)) / Sigma
        S[:, 5] = (np.abs(r - Mq) * (2 * q * q * kq + pr * pr) + r * (2 * np.abs(E * q) * kq + SF / Sigma)) / Sigma
        G = (al * al * E * E + al * al * SF / Sigma + (L / s2) ** 2) / Sigma
        S[:, 6] = np.abs(sn * cs) * G
        # the argument reduction of a float64 sincos (REDUCTION): an ABSOLUTE error of sin and cos, in units of u
        red = LD(REDUCTION / U) * np.abs(np.rint(th * (2 / LD(np.pi))))
        red_s2 = 2 * red / np.abs(sn)  # ... as a relative error of sin^2
        S[:, 3] += red_s2 * np.abs(L) / s2 / Sigma
        S[:, 5] += r * (red_s2 * L * L / s2) / (Sigma * Sigma)
        S[:, 6] += red * (np.abs(sn) + np.abs(cs)) * G + 2 * red_s2 * np.abs(sn * cs) * (L / s2) ** 2 / Sigma
    return S.astype(np.float64)


# ---- one attempt ---------------------------------------------------------------------------------------------------------------------
def attempt_ld(kind, a, Y, h, rtol=RTOL, atol=ATOL, F=None):
    """One Dormand-Prince attempt of size h (n,) from Y (n, 8), everything in longdouble (F = rhs8_ld(Y) unless given)
    -> dict(y_new, f_new, err, q (n, 8) = e_i / sc_i, sc, K (7 x (n, 8)), stages (7 x (n, 8): Y, the five stage states, y_new))."""
    Y = np.asarray(Y, dtype=LD)
    n = Y.shape[0]
    hh = np.broadcast_to(np.asarray(h, dtype=LD), (n,))[:, None]
    K = [rhs8_ld(kind, a, Y) if F is None else np.asarray(F, dtype=LD)]
    stages = [Y]
    with np.errstate(all="ignore"):
        for row in _A:
            acc = K[0] * LD(row[0])
            for c, ks in zip(row[1:], K[1:]):
                acc = acc + ks * LD(c)
            stages.append(Y + acc * hh)
            K.append(rhs8_ld(kind, a, stages[-1]))
        acc = K[0] * LD(_B[0])
        for c, ks in zip(_B[2:], K[2:]):
            acc = acc + ks * LD(c)
        y_new = Y + hh * acc
        stages.append(y_new)
        K.append(rhs8_ld(kind, a, y_new))
        acc = K[0] * LD(_E[0])
        for c, ks in zip(_E[2:], K[2:]):
            acc = acc + ks * LD(c)
        sc = LD(atol) + np.maximum(np.abs(Y), np.abs(y_new)) * LD(rtol)
        q = acc * hh / sc
        err = rms(q)
    return dict(y_new=y_new, f_new=K[6], err=err, q=q, sc=sc, K=K, stages=stages)


def rms(x):
    """The RMS norm over the 8 components, longdouble."""
    x = np.asarray(x, dtype=LD)
    return np.sqrt((x * x).sum(axis=1)) / np.sqrt(LD(8))


def factor_accept(err, rejected):
    """The controller's factor after an accepted attempt: min(10, 0.9 err^-1/5), 10 at err = 0, at most 1 after a rejection."""
    err = np.asarray(err, dtype=LD)
    with np.errstate(all="ignore"):
        f = np.where(err == 0, LD(10), np.minimum(LD(10), LD(0.9) * err ** LD(-0.2)))
    return np.where(np.asarray(rejected, dtype=bool), np.minimum(LD(1), f), f)


def factor_reject(err):
    """... after a rejected one: max(0.2, 0.9 err^-1/5); a NaN norm shrinks by 0.2."""
    err = np.asarray(err, dtype=LD)
    with np.errstate(all="ignore"):
        f = np.maximum(LD(0.2), LD(0.9) * err ** LD(-0.2))
    return np.where(np.isnan(err), LD(0.2), f)


def dense_Q(K):
    """Q = K^T P: list of 4 (n, 8) longdouble arrays."""
    return [sum(K[s] * LD(_P[s][j]) for s in (0, 2, 3, 4, 5, 6)) for j in range(4)]


def dense_weights(x):
    """p_s(x) = sum_j P[s][j] x^(j+1): (7, n) longdouble, the weight of stage derivative s in the dense output at x."""
    x = np.asarray(x, dtype=LD)
    return np.stack([sum(LD(_P[s][j]) * x ** (j + 1) for j in range(4)) for s in range(7)])


def dense_eval(Y, h, Q, x):
    """y(t_old + x h) = Y + h (Q0 x + Q1 x^2 + Q2 x^3 + Q3 x^4), x (n,)."""
    x = np.asarray(x, dtype=LD)[:, None]
    hh = np.broadcast_to(np.asarray(h, dtype=LD), (Y.shape[0],))[:, None]
    return Y + hh * (((Q[3] * x + Q[2]) * x + Q[1]) * x + Q[0]) * x


def _stack_perturbed(Y64):
    """(5 n, 8): the rows, then the rows with r, theta, p_r, p_theta moved by one float64 rounding each."""
    Y64 = np.asarray(Y64, dtype=np.float64)
    out = [Y64]
    for j in PERTURBED:
        p = Y64.copy()
        p[:, j] += EPS * np.abs(p[:, j])
        out.append(p)
    return np.concatenate(out)


def step_blocks(kind, a, Y64, h, rtol=RTOL, atol=ATOL, x=None):
    """The longdouble attempt of size h from the float64 rows Y64 with everything a comparison needs, computed once:
    dict(y_new, f_new, err, unit (n, 8), unit_err (n,), keep (n,), stages, K, and with x (n,): ye, unit_ye (n, 8), dr (n,) = r'(x))."""
    Y64 = np.ascontiguousarray(Y64, dtype=np.float64)
    n = Y64.shape[0]
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,))
    o = attempt_ld(kind, a, _stack_perturbed(Y64), np.tile(h, 5), rtol, atol)
    y_all, e_all = o["y_new"], o["err"]
    y1, err = y_all[:n], e_all[:n]
    K = [k[:n] for k in o["K"]]
    stages = [s[:n] for s in o["stages"]]
    S = [scales8(kind, a, s) for s in stages]
    hS_b = h[:, None] * U * sum(abs(b) * s for b, s in zip(_B, S[:6]))
    # a stage derivative's error: u S of its evaluation, plus what one float64 rounding of each input of ITS stage state does
    # (the seven roundings are independent, so the error norm's cancellation between the stages does not act on them)
    with np.errstate(all="ignore"):
        T = [U * S[s] + sum(np.abs(o["K"][s][j * n:(j + 1) * n] - K[s]).astype(np.float64) for j in range(1, 5)) / 2 for s in range(7)]
    hS_e = h[:, None] * sum(abs(e) * ts for e, ts in zip(_E, T))
    with np.errstate(all="ignore"):
        A = U * np.abs(y1).astype(np.float64)
        Ae = U * err.astype(np.float64)
        for j in range(1, 5):
            A = A + np.abs(y_all[j * n:(j + 1) * n] - y1).astype(np.float64) / 2
            Ae = Ae + np.abs(e_all[j * n:(j + 1) * n] - err).astype(np.float64) / 2
        q, sc = o["q"][:n], o["sc"][:n]
        direct = ((np.abs(q) / sc).astype(np.float64) * hS_e).sum(axis=1) / (8 * err.astype(np.float64))
        unit_err = Ae + np.where(err > 0, direct, 0.0)
        unit = A + hS_b
    rz = r_zero(a if kind else 0.0)
    stage_r = np.stack([s[:, 1].astype(np.float64) for s in stages], axis=1)
    finite = np.isfinite(y1.astype(np.float64)).all(axis=1) & np.isfinite(unit).all(axis=1) & np.isfinite(unit_err)
    keep = finite & ~(stage_r <= rz).any(axis=1)
    out = dict(y_new=y1, f_new=K[6], err=err, unit=unit, unit_err=unit_err, keep=keep, stages=stages, K=K, h=h)
    if x is not None:
        x = np.asarray(x, dtype=LD)
        Q_all = dense_Q(o["K"])
        ye_all = dense_eval(np.asarray(_stack_perturbed(Y64), dtype=LD), np.tile(h, 5), Q_all, np.tile(x, 5))
        ye = ye_all[:n]
        w = np.abs(dense_weights(x)).astype(np.float64)  # (7, n)
        with np.errstate(all="ignore"):
            Ay = U * np.abs(ye).astype(np.float64)
            for j in range(1, 5):
                Ay = Ay + np.abs(ye_all[j * n:(j + 1) * n] - ye).astype(np.float64) / 2
            out["unit_ye"] = Ay + h[:, None] * U * sum(w[s][:, None] * S[s] for s in range(7))
        Q = [qq[:n] for qq in Q_all]
        out["ye"] = ye
        out["dr"] = (((4 * Q[3][:, 1] * x + 3 * Q[2][:, 1]) * x + 2 * Q[1][:, 1]) * x + Q[0][:, 1]).astype(np.float64)
    return out


# ---- the initial step ----------------------------------------------------------------------------------------------------------------
def initial_step_ld(kind, a, Y64, lambda_max=LAMBDA_MAX, rtol=RTOL, atol=ATOL, max_step=MAX_STEP):
    """Hairer's rule (solve_ivp's select_initial_step, error-estimator order 4) in longdouble -> (h_abs (n,), unit (n,) float64)."""
    Y64 = np.ascontiguousarray(Y64, dtype=np.float64)
    n = Y64.shape[0]
    Y = _stack_perturbed(Y64).astype(LD)
    with np.errstate(all="ignore"):
        f = rhs8_ld(kind, a, Y)
        sc = LD(atol) + np.abs(Y) * LD(rtol)
        d0, d1 = rms(Y / sc), rms(f / sc)
        h0 = np.where((d0 < 1e-5) | (d1 < 1e-5), LD(1e-6), LD(0.01) * d0 / d1)
        h0 = np.minimum(h0, LD(lambda_max))
        y1 = Y + h0[:, None] * f
        f1 = rhs8_ld(kind, a, y1)
        w = (f1 - f) / sc
        R = rms(w)
        d2 = R / h0
        dm = np.maximum(d1, d2)
        h1 = np.where((d1 <= 1e-15) & (d2 <= 1e-15), np.maximum(LD(1e-6), h0 * LD(1e-3)), (LD(0.01) / dm) ** LD(0.2))
        h = np.minimum(np.minimum(100 * h0, h1), LD(min(lambda_max, max_step)))
        hb = h[:n]
        unit = U * hb.astype(np.float64)
        for j in range(1, 5):
            unit = unit + np.abs(h[j * n:(j + 1) * n] - hb).astype(np.float64) / 2
        # the direct effect of one unit u S of each right-hand side on the norm that binds
        S0 = scales8(kind, a, Y[:n]) * U
        S1 = scales8(kind, a, y1[:n]) * U
        scn = sc[:n].astype(np.float64)
        via_d2 = (np.abs(w[:n]).astype(np.float64) * (S0 + S1) / scn).sum(axis=1) / (8 * (R[:n] ** 2).astype(np.float64))
        v1 = (f[:n] / sc[:n])
        via_d1 = (np.abs(v1).astype(np.float64) * S0 / scn).sum(axis=1) / (8 * (d1[:n] ** 2).astype(np.float64))
        binds = (h1[:n] <= 100 * h0[:n]) & (h1[:n] < LD(min(lambda_max, max_step)))
        direct = np.where(d2[:n] >= d1[:n], via_d2, via_d1)
        unit = unit + np.where(binds, 0.2 * hb.astype(np.float64) * direct, 0.0)
    return hb, unit


# ---- the accept / reject loop ------------------------------------------------------------------------------------------------------
def accept_loop(kind, a, Y64, t, h_trial, k_err, lambda_max=LAMBDA_MAX, rtol=RTOL, atol=ATOL, max_step=MAX_STEP, max_iter=40,
                known=None):
    """The reference's loop for one step from the float64 rows (t, Y64) with trial size h_trial (longdouble), the attempts in
    longdouble, the arithmetic on t in float64 as the reference states it: clamp to [10 ulp(t), max_step], t_new = t + h_abs
    clipped at lambda_max, h = t_new - t, attempt, accept below 1 or shrink.
    -> dict(h (n,) float64 accepted size, t_new, attempts (n,), rejected (n,), near (n,): some decision's error norm within k_err
    units of 1, rel (n,): the relative allowance of h that 2... k_err units of every error norm in the chain give, ok (n,))."""
    Y64 = np.ascontiguousarray(Y64, dtype=np.float64)
    n = Y64.shape[0]
    t = np.broadcast_to(np.asarray(t, dtype=np.float64), (n,))
    min_step = 10 * np.abs(np.nextafter(t, np.inf) - t)
    h_abs = np.asarray(h_trial, dtype=LD).copy()
    h_abs = np.where(h_abs > max_step, LD(max_step), np.where(h_abs < min_step, min_step.astype(LD), h_abs))
    clamped = np.asarray(h_trial, dtype=LD) > max_step
    h_out, tn_out = np.zeros(n), np.zeros(n)
    attempts = np.zeros(n, dtype=np.int64)
    near, ok = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    rel = np.zeros(n)
    err_acc = np.zeros(n, dtype=LD)
    active = np.arange(n)
    for it in range(max_iter):
        if active.size == 0:
            break
        ha = h_abs[active].astype(np.float64)  # (the reference's h_abs is a float64: the trial size rounded once)
        tn = t[active] + ha
        tn = np.where(tn - lambda_max > 0, lambda_max, tn)
        hh = tn - t[active]
        if known is not None and it == 0 and (same := hh == known["h"]).any():
            # (the attempt at the record's own size is already there: nearly every first trial)
            err, unit_err, keep = known["err"].copy(), known["unit_err"].copy(), known["keep"].copy()
            if not same.all():
                b2 = step_blocks(kind, a, Y64[~same], hh[~same], rtol, atol)
                err[~same], unit_err[~same], keep[~same] = b2["err"], b2["unit_err"], b2["keep"]
            blk = dict(err=err, unit_err=unit_err, keep=keep)
        else:
            blk = step_blocks(kind, a, Y64[active], hh, rtol, atol)
        err = blk["err"]
        attempts[active] += 1
        e64 = err.astype(np.float64)
        with np.errstate(all="ignore"):
            near[active] |= ~(np.abs(e64 - 1.0) > k_err * blk["unit_err"])
            rel[active] += 0.2 * k_err * blk["unit_err"] / e64
        ok[active] &= blk["keep"]
        acc = (err < 1)
        done = active[acc]
        h_out[done], tn_out[done], err_acc[done] = hh[acc], tn[acc], err[acc]
        rej = active[~acc]
        h_abs[rej] = np.abs(hh[~acc]).astype(LD) * factor_reject(err[~acc])
        under = h_abs[rej] < min_step[rej]
        ok[rej[under]] = False
        active = rej[~under]
    ok[active] = False
    return dict(h=h_out, t_new=tn_out, attempts=attempts, rejected=attempts > 1, near=near, rel=rel, ok=ok, err=err_acc,
                clamped=clamped)


# ---- records ---------------------------------------------------------------------------------------------------------------------------
def seeded_states(kind, a, n=N_TRACKS, seed=0, r_obs=R_OBS):
    """n starts of a camera at r_obs: alpha in [0, 0.35], any position angle (metrics.initial_conditions)."""
    import metrics
    rng = np.random.default_rng([seed, 700 + kind, int(round(a * 1000))])
    met = metrics.Kerr(M, a) if kind else metrics.Schwarzschild(M)
    al, ps = rng.uniform(0.0, 0.35, n), rng.uniform(0, 2 * np.pi, n)
    return np.array([met.initial_conditions(r_obs, x, p) if kind else met.initial_conditions(r_obs, x) for x, p in zip(al, ps)])


def sharp_turn_states(kind, a, n=64, seed=0):
    """Starts with a large p_theta / Sigma (off shell: the right-hand side is defined for any state), so that accepted steps have
    stage angles more than 0.25 rad from the step's base -- the device's full-sincos fallback.  Integrated at SHARP_TOL."""
    rng = np.random.default_rng([seed, 800 + kind, int(round(a * 1000))])
    s = np.zeros((n, 8))
    s[:, 1] = rng.uniform(6.0, 12.0, n)
    s[:, 2] = rng.uniform(0.6, np.pi - 0.6, n)
    s[:, 4] = -1.0
    s[:, 5] = rng.uniform(-0.5, 0.5, n)
    s[:, 6] = rng.choice([-1.0, 1.0], n) * rng.uniform(40.0, 120.0, n)
    s[:, 7] = rng.uniform(-4.0, 4.0, n)
    return s


SHARP_TOL = dict(rtol=1e-3, atol=1e-5)
SHARP_LAMBDA_MAX = 4.0


def oracle_records(kind, a, s0, max_points=512, lambda_max=LAMBDA_MAX, rtol=RTOL, atol=ATOL, max_step=MAX_STEP, r_out=None):
    """The oracle's records in the device's layout: t (n, mp), y (n, mp, 8), count, status, nfev; the slot past an event record
    holds the t_new of the step that contains the event (oracle.dense_last_t_new)."""
    s0 = np.asarray(s0, dtype=np.float64).reshape(-1, 8)
    n = s0.shape[0]
    t, y = np.full((n, max_points), np.nan), np.full((n, max_points, 8), np.nan)
    count, status, nfev = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int8), np.zeros(n, dtype=np.int32)
    aa = a if kind else 0.0
    for i in range(n):
        ro = 2 * s0[i, 1] if r_out is None else r_out
        ot, oy, st, nf, full = oracle.integrate_dense(kind, M, aa, s0[i], lambda_max, r_capture(aa), ro, rtol, atol, max_step, max_points,
                                                      with_count=True)
        m = len(ot)
        t[i, :m], y[i, :m], count[i], status[i], nfev[i] = ot, oy.T, full, st, nf
        if st > 0 and full < max_points:
            t[i, m] = oracle.dense_last_t_new()
    return t, y, count, status, nfev


def replay(kind, a, t, y, count, status, nfev, k_att, k_err, lambda_max=LAMBDA_MAX, rtol=RTOL, atol=ATOL, max_step=MAX_STEP,
           t_new_slot=True):
    """Replays untruncated records (module docstring).  Rows are the accepted steps p -> p + 1 of every track, the step that holds
    the terminal event included when t_new_slot (its end time stands in the slot past the record; its end STATE is not recorded).
    -> dict over rows: track, p, ratio (rows, 8) = |y_{p+1} - longdouble step| / unit (NaN where there is no unit or no state),
    keep, cyclic_ok, h, h_replay, h_allow, h_keep, attempts, and per track: attempts_sum, attempts_known, start_* of the first step."""
    aa = a if kind else 0.0
    n, mp = t.shape
    count = np.asarray(count, dtype=np.int64)
    assert (count <= mp).all(), "replay needs untruncated records"
    ev = np.asarray(status) > 0
    n_reg = np.where(ev, count - 1, count)  # regular points 0 .. n_reg - 1
    has_tnew = ev & (count < mp) & bool(t_new_slot)
    n_steps = n_reg - 1 + has_tnew
    trk = np.repeat(np.arange(n), n_steps)
    p = np.concatenate([np.arange(k) for k in n_steps]) if n_steps.sum() else np.zeros(0, dtype=np.int64)
    is_ev = p == (n_reg - 1)[trk]  # the step that holds the event: its end is t_new, no state
    t0, Y0 = t[trk, p], y[trk, p]
    t1 = np.where(is_ev, t[trk, np.minimum(p + 2, mp - 1)], t[trk, np.minimum(p + 1, mp - 1)])
    h = t1 - t0
    blk = step_blocks(kind, aa, Y0, h, rtol, atol)
    Y1 = y[trk, np.minimum(p + 1, mp - 1)]
    with np.errstate(all="ignore"):
        ratio = np.abs(Y1.astype(LD) - blk["y_new"]).astype(np.float64) / blk["unit"]
    ratio[:, [4, 7]] = np.nan
    ratio[is_ev] = np.nan
    cyclic_ok = is_ev | ((Y1[:, 4].view(np.int64) == Y0[:, 4].view(np.int64)) & (Y1[:, 7].view(np.int64) == Y0[:, 7].view(np.int64)))
    keep = blk["keep"] & ~is_ev
    err = blk["err"]
    e64 = err.astype(np.float64)
    with np.errstate(all="ignore"):
        near_acc = ~(np.abs(e64 - 1.0) > k_err * blk["unit_err"])
        rel_acc = 0.2 * k_err * blk["unit_err"] / e64
    accept_ok = (err < 1) | near_acc | ~blk["keep"]  # the record's own step is one the longdouble loop accepts

    # the first step of every track: the initial step through the loop
    first = np.flatnonzero(p == 0)
    h0, unit_h0 = initial_step_ld(kind, aa, Y0[first], lambda_max, rtol, atol, max_step)
    nrow = trk.size
    rejected = np.zeros(nrow, dtype=bool)
    res = dict(h=np.zeros(nrow), attempts=np.zeros(nrow, dtype=np.int64), near=np.zeros(nrow, dtype=bool), rel=np.zeros(nrow),
               ok=np.zeros(nrow, dtype=bool), clamped=np.zeros(nrow, dtype=bool))

    def run(rows, trial):
        o = accept_loop(kind, aa, Y0[rows], t0[rows], trial, k_err, lambda_max, rtol, atol, max_step,
                        known=dict(h=h[rows], err=err[rows], unit_err=blk["unit_err"][rows], keep=blk["keep"][rows]))
        for key in res:
            res[key][rows] = o[key]
        changed = rejected[rows] != o["rejected"]
        rejected[rows] = o["rejected"]
        return rows[changed]

    err = blk["err"]
    run(first, h0)
    later = np.flatnonzero(p > 0)
    todo = later
    for _ in range(64):  # the trial of step p needs step p - 1's `rejected` flag: iterate on the rows whose flag changed
        if todo.size == 0:
            break
        prev = todo - 1  # (rows of a track are consecutive)
        trial = np.abs(h[prev]).astype(LD) * factor_accept(err[prev], rejected[prev])
        changed = run(todo, trial)
        nxt = changed + 1
        nxt = nxt[(nxt < nrow)]
        todo = nxt[p[nxt] > 0]
    assert todo.size == 0, "the replay of the rejected flags did not settle"
    prev_near = np.zeros(nrow, dtype=bool)
    prev_rel = np.zeros(nrow)
    prev_near[later] = near_acc[later - 1] | res["near"][later - 1] | ~blk["keep"][later - 1]
    prev_rel[later] = rel_acc[later - 1]
    h_keep = res["ok"] & ~res["near"] & ~prev_near & blk["keep"]
    with np.errstate(all="ignore"):
        rel = np.where(res["clamped"] & (res["attempts"] == 1), 0.0, res["rel"] + prev_rel)
        h_allow = np.abs(res["h"]) * rel + 4 * np.spacing(np.abs(t1))
    capped = np.zeros(nrow, dtype=bool)  # min(1, factor) acted: the step before was accepted after a rejection with a factor above 1
    with np.errstate(all="ignore"):
        capped[later] = rejected[later - 1] & (LD(0.9) * err[later - 1] ** LD(-0.2) > 1)
    unit_first = np.zeros(nrow)
    unit_first[first] = unit_h0
    known = np.ones(n, dtype=bool)
    np.logical_and.at(known, trk, h_keep)
    known &= (n_steps == n_reg - 1 + ev) & (np.asarray(status) >= 0)  # every attempt of the track belongs to a row
    att_sum = np.zeros(n, dtype=np.int64)
    np.add.at(att_sum, trk, res["attempts"])
    return dict(track=trk, p=p, is_event=is_ev, ratio=ratio, keep=keep, cyclic_ok=cyclic_ok, accept_ok=accept_ok, h=h,
                h_replay=res["h"], h_allow=h_allow, h_keep=h_keep, attempts=res["attempts"], rejected=rejected,
                clamped=res["clamped"], capped=capped, near=near_acc | res["near"], attempts_sum=att_sum, attempts_known=known,
                attempts_nfev=(np.asarray(nfev, dtype=np.int64) - 2) // 6, first=first, h0=h0, unit_h0=unit_first, blk=blk,
                Y0=Y0, Y1=Y1, t0=t0, n_steps=n_steps)


STEP_CLASSES = ("far", "turning", "equator", "axis", "sharp")


def classify(blk, Y0, Y1):
    """-> dict(name -> (rows,) bool) of STEP_CLASSES from the longdouble stages of each step: far (r > 20 throughout), turning
    point (p_r changes sign), equator crossing, within 0.3 rad of the axis, a stage more than 0.25 rad from the step's base."""
    st = np.stack([s.astype(np.float64) for s in blk["stages"]], axis=1)  # (rows, 7, 8)
    th = st[:, :, 2]
    dist = np.abs(np.mod(th + np.pi / 2, np.pi) - np.pi / 2)  # distance from the nearest pole (theta = k pi)
    return dict(far=(st[:, :, 1] > 20.0).all(axis=1),
                turning=(st[:, 0, 5] * st[:, 6, 5] < 0),
                equator=(np.cos(st[:, 0, 2]) * np.cos(st[:, 6, 2]) < 0),
                axis=(dist < 0.3).any(axis=1),
                sharp=(np.abs(th - th[:, :1]) > 0.25).any(axis=1))


def event_check(kind, a, t, y, count, status, lambda_max=LAMBDA_MAX, rtol=RTOL, atol=ATOL, r_out=None):
    """The terminal event of every event record with room for its t_new slot: inputs are the last regular point, the stored t_new,
    te and ye.  -> dict(track, ordered (t_last < te <= t_new), ratio_ye (m, 8), resid = |r_dense(te) - radius|, unit_root, keep)."""
    aa = a if kind else 0.0
    n, mp = t.shape
    count = np.asarray(count, dtype=np.int64)
    rows = np.flatnonzero((np.asarray(status) > 0) & (count < mp) & (count >= 2))
    c = count[rows]
    t_last, Y_last = t[rows, c - 2], y[rows, c - 2]
    te, ye, t_new = t[rows, c - 1], y[rows, c - 1], t[rows, c]
    h = t_new - t_last
    x = (te.astype(LD) - t_last.astype(LD)) / h.astype(LD)
    blk = step_blocks(kind, aa, Y_last, h, rtol, atol, x=x)
    ro = 2 * y[rows, 0, 1] if r_out is None else np.full(rows.size, r_out)
    radius = np.where(np.asarray(status)[rows] == 1, r_capture(aa), ro)
    with np.errstate(all="ignore"):
        ratio = np.abs(ye.astype(LD) - blk["ye"]).astype(np.float64) / blk["unit_ye"]
        ratio[:, [4, 7]] = np.nan
        resid = np.abs(blk["ye"][:, 1] - radius.astype(LD)).astype(np.float64)
        unit_root = 4 * EPS * (1 + np.abs(te)) * np.abs(blk["dr"]) + blk["unit_ye"][:, 1]
    cyc = (ye[:, 4].view(np.int64) == Y_last[:, 4].view(np.int64)) & (ye[:, 7].view(np.int64) == Y_last[:, 7].view(np.int64))
    return dict(track=rows, ordered=(t_last < te) & (te <= t_new), ratio_ye=ratio, resid=resid, unit_root=unit_root,
                keep=blk["keep"], status=np.asarray(status)[rows], cyclic_ok=cyc, h=h, t_last=t_last, te=te, radius=radius)


# ---- right-hand-side classes ---------------------------------------------------------------------------------------------------------
RHS_CLASSES = ("far", "near_horizon", "pole", "equator", "energy", "off_shell")


def rhs_class(name, kind, a, n=257, seed=0):
    """States (n, 8) of one class (n is no multiple of 64).  On shell means nothing to a right-hand side: momenta are drawn
    independently except where the class says otherwise."""
    rng = np.random.default_rng([seed, 900 + RHS_CLASSES.index(name), kind, int(round(a * 1000))])
    rp = r_plus(a if kind else 0.0)
    s = np.zeros((n, 8))
    s[:, 0] = rng.uniform(0, 100, n)
    s[:, 1] = np.exp(rng.uniform(np.log(3.0), np.log(60.0), n))
    s[:, 2] = rng.uniform(0.3, np.pi - 0.3, n)
    s[:, 3] = rng.uniform(-6, 6, n)
    s[:, 4] = -1.0
    s[:, 5] = rng.uniform(-1.5, 1.5, n)
    s[:, 6] = rng.uniform(-8, 8, n)
    s[:, 7] = rng.uniform(0.0, 8.0, n)
    if name == "far":
        s[:, 1] = np.exp(rng.uniform(np.log(100.0), np.log(600.0), n))
    elif name == "near_horizon":
        s[:, 1] = rng.uniform(1.002 * rp, 1.2 * rp, n)
    elif name == "pole":
        d = np.exp(rng.uniform(np.log(1e-8), np.log(1e-3), n))
        s[:, 2] = np.where(rng.random(n) < 0.5, d, np.pi - d)
        s[:, 7] *= np.sin(s[:, 2])  # (a ray this close to the axis has |L| <~ b sin theta)
    elif name == "equator":
        s[:, 2] = np.pi / 2
    elif name == "energy":
        s[:, 4] = -rng.uniform(0.3, 3.0, n)
        s[:, 7] = -rng.uniform(0.5, 8.0, n)
    elif name == "off_shell":
        s[:, 5] = rng.uniform(-20, 20, n)
        s[:, 6] = rng.uniform(-60, 60, n)
    else:
        raise KeyError(name)
    return s


def rhs_ratio(kind, a, states, got):
    """|got - longdouble| / (u S) per component (n, 8); NaN in the cyclic columns (held bit for bit instead)."""
    ref = rhs8_ld(kind, a, states)
    S = scales8(kind, a, states)
    with np.errstate(all="ignore"):
        ratio = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).astype(np.float64) / (U * S)
    ratio[:, [4, 7]] = np.nan
    return ratio


def verdict(rp, k_att, k_h0):
    """What a replay holds against a record: the number of kept steps outside k_att units, of kept step sizes outside their allowance
    (the first step's includes k_h0 units of the initial step), of cyclic momenta that moved, of recorded steps the longdouble loop
    does not accept, and of tracks with nothing left out whose attempts do not sum to (nfev - 2) / 6."""
    with np.errstate(invalid="ignore"):
        steps = int((np.nan_to_num(rp["ratio"], nan=0.0, posinf=np.inf).max(axis=1) > k_att)[rp["keep"]].sum())
        allow = rp["h_allow"] + k_h0 * rp["unit_h0"]
        sizes = int((np.abs(rp["h"] - rp["h_replay"]) > allow)[rp["h_keep"]].sum())
    known = rp["attempts_known"]
    return dict(steps=steps, sizes=sizes, cyclic=int((~rp["cyclic_ok"]).sum()), accepts=int((~rp["accept_ok"]).sum()),
                attempts=int((rp["attempts_sum"] != rp["attempts_nfev"])[known].sum()))
