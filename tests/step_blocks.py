"""What tests/test_step_blocks_host.py and tests/test_gpu_step_blocks.py share: the unit float32 errors of the Kerr
right-hand side and of one RK4 step are stated in, the state classes, and the bounds that follow from the reference's
own float32 arithmetic.

THE UNIT.  u = 2^-24.  For a state (r, theta, p_r, p_theta) and the ray's constant L, from the reference's quantities
(metrics.py:221-303), computed in longdouble:
    s2 = max(sin^2 theta, 1e-15), ra = r^2 + a^2, Sigma = ra - a^2 s2, Delta = ra - 2 M r, P = ra - a L, q = P / Delta,
    k_Delta = (ra + 2 M r) / Delta            (the cancellation in Delta)
    k_P = (ra + |a L|) / |P|,   k_q = 1 + k_Delta + k_P
    S_F   = Delta p_r^2 (1 + k_Delta) + p_theta^2 + L^2 / s2 + 2 |a L| + a^2 s2 + |P q| k_q
    S_dr  = |Delta p_r / Sigma| (1 + k_Delta)
    S_dth = |p_theta / Sigma|
    S_dph = (|a q| k_q + |L| / s2 + |a|) / Sigma
    S_dpr = [ |r - M| (2 q^2 k_q + p_r^2) + r (2 |q| k_q + S_F / Sigma) ] / Sigma
    S_dpth = |sin theta cos theta| (a^2 + a^2 S_F / Sigma + (L / s2)^2) / Sigma
-- the sum of the magnitudes of the terms each output is formed from, the two cancellations in its inputs counted.  An
error of a right-hand side is stated as a multiple of u S.

ONE STEP.  The unit of component i of a step of size h from y0 is A_i + h u S_i(y0), where
    A_i = sum_j |y1_i(y0 + 2^-23 |y0_j| e_j) - y1_i(y0)| / 2 + u |y1_i|
from the float64 step of the reference: first-order propagation of one float32 rounding of each input, plus the rounding
of the result.  (phi has no right-hand side of its own scale: it takes S_dph.)  A state is left out where a float64 stage
radius is <= 1.002 r_cut (the reference's right-hand side jumps to zero at r_cut) or where A_i > 2^10 u (|y1_i| + h S_i)
for some i (the step is stiff: a first-order model says nothing) -- decided from the float64 step alone; at most 2 % of a
class.

THE BOUNDS are the reference's own float32 arithmetic (oracle/liblt_oracle_f32.so: every operation of the same statements
rounded to float32), measured by tests/test_step_blocks_host.py on the classes below and rounded up to an integer:
    K_REF  = 13   right-hand side, every class but `near` (measured 12.01; the reference's formula loses digits of its own
                  in `near`: 25 at a = 0.5, 176 at a = 0.998 -- the kernel's form does not, and is held to 2 K_REF there too)
    K_STEP = 4    one step (measured 3.74, `near` at a = 0.9; 0.5 ... 0.9 in `far`, `mid` and the equatorial band: half an
                  ulp of the result)
    K_FALLBACK = 26   one step from a state that fails the branch-free step's validity test (fallback_class: a stage at
                  or inside r_cut, or a stage angle offset beyond 0.25 rad; measured 25.92, dp_r just outside r_cut at a = 0.5)
    K_STEP64 = 27  one step of the float64 oracle against the same step in longdouble, in the unit with 2^-53 for u
                  (measured 26.2 at ONE state of `pole_approach`, a = 0.9, whose step crosses the polar axis: theta
                  0.073 -> -0.007, p_theta -4.8 -> -141; a perturbation of 2^-52 sees none of that curvature, one of 2^-23
                  does.  Every other state of every class: at most 4.3, all but 0.5 % within 1.)  A float64 GPU step is
                  held to 2 K_STEP where the float64 oracle itself is within K_STEP of the longdouble step, and to
                  2 K_STEP64 elsewhere.
The GPU forms are held to twice these: what the kernel's form adds over the reference's is three roundings where a
division has one (each of its quotients comes from one merged reciprocal).
"""
import numpy as np
from mpmath import libmp

M = 1.0
U32 = 2.0 ** -24
U64 = 2.0 ** -53
SPINS = (0.0, 0.5, 0.9, 0.998)
K_REF = 13
K_STEP = 4
K_FALLBACK = 26
K_STEP64 = 27
EXCLUDED_CAP = 0.02
LD = np.longdouble


def r_plus(a):
    return M + np.sqrt(M * M - a * a)


def r_cut(a):
    return 1.001 * r_plus(a)


def f32(x):
    """Rounded to float32, held in float64: what either side of a comparison is given."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def scales(a, states, L, floor_added=False):
    """S (n,5) for [dr, dtheta, dphi, dp_r, dp_theta], longdouble arithmetic, returned as float64.
    floor_added: s2 = sin^2 + 1e-15 (how the float32 kernel applies the floor) in place of the max."""
    st = np.asarray(states, dtype=LD)
    r, th, pr, pth = st[:, 0], st[:, 1], st[:, 3], st[:, 4]
    L = np.asarray(L, dtype=LD)
    a = LD(a)
    Mq = LD(M)
    sn, cs = np.sin(th), np.cos(th)
    s2 = sn * sn + LD(1e-15) if floor_added else np.maximum(sn * sn, LD(1e-15))
    ra = r * r + a * a
    Sigma = ra - a * a * s2
    Delta = ra - 2 * Mq * r
    P = ra - a * L
    q = P / Delta
    kD = (ra + 2 * Mq * r) / Delta
    kP = (ra + np.abs(a * L)) / np.abs(P)
    kq = 1 + kD + kP
    SF = Delta * pr * pr * (1 + kD) + pth * pth + L * L / s2 + 2 * np.abs(a * L) + a * a * s2 + np.abs(P * q) * kq
    S = np.empty(st.shape, dtype=LD)
    S[:, 0] = np.abs(Delta * pr / Sigma) * (1 + kD)
    S[:, 1] = np.abs(pth / Sigma)
    S[:, 2] = (np.abs(a * q) * kq + np.abs(L) / s2 + np.abs(a)) / Sigma
    S[:, 3] = (np.abs(r - Mq) * (2 * q * q * kq + pr * pr) + r * (2 * np.abs(q) * kq + SF / Sigma)) / Sigma
    S[:, 4] = np.abs(sn * cs) * (a * a + a * a * SF / Sigma + (L / s2) ** 2) / Sigma
    return S.astype(np.float64)


def ref_rhs_longdouble(a, states, L):
    """The statements of the reference's right-hand side (metrics.py:221-303, p_t = -1; oracle/lt_oracle.c kerr_rhs) in
    longdouble: the yardstick of the FLOAT64 right-hand sides, whose errors are of the size of the float64 oracle's own
    (K_REF 2^-53 S, and more in the `near` class).  tests/test_step_blocks_host.py holds it to the oracle."""
    st = np.asarray(states, dtype=LD)
    r, th, p_r, p_th = st[:, 0], st[:, 1], st[:, 3], st[:, 4]
    p_phi, p_t, a, Mq = np.asarray(L, dtype=LD), LD(-1), LD(a), LD(M)
    sn, cs = np.sin(th), np.cos(th)
    s2 = np.maximum(sn * sn, LD(1e-15))
    Sigma = r * r + a * a * cs * cs
    Delta = r * r - 2 * Mq * r + a * a
    A = (r * r + a * a) ** 2 - a * a * Delta * s2
    SD = Sigma * Delta
    out = np.zeros(st.shape, dtype=LD)
    out[:, 0] = Delta / Sigma * p_r
    out[:, 1] = p_th / Sigma
    out[:, 2] = -2 * Mq * a * r / SD * p_t + (Delta - a * a * s2) / (SD * s2) * p_phi
    dS, dD = 2 * r, 2 * r - 2 * Mq
    dA = 4 * r * (r * r + a * a) - a * a * dD * s2
    mix = dS * Delta + Sigma * dD
    g_tt = -(dA * SD - A * mix) / SD ** 2
    g_tp = -(2 * Mq * a * (SD - r * mix)) / SD ** 2
    g_rr = (dD * Sigma - Delta * dS) / Sigma ** 2
    g_thth = -dS / Sigma ** 2
    den = SD * s2
    g_pp = (dD * den - (Delta - a * a * s2) * mix * s2) / den ** 2
    out[:, 3] = -(g_tt * p_t * p_t + 2 * g_tp * p_t * p_phi + g_rr * p_r * p_r + g_thth * p_th * p_th + g_pp * p_phi * p_phi) / 2
    dSt = -2 * a * a * sn * cs
    dAt = -a * a * Delta * 2 * sn * cs
    h_tt = -(dAt * SD - A * dSt * Delta) / SD ** 2
    h_tp = 2 * Mq * a * r * dSt / (Sigma ** 2 * Delta)
    h_rr = -Delta * dSt / Sigma ** 2
    h_thth = -dSt / Sigma ** 2
    num = Delta - a * a * s2
    dden = dSt * Delta * s2 + SD * 2 * sn * cs
    h_pp = (-a * a * 2 * sn * cs * den - num * dden) / den ** 2
    out[:, 4] = -(h_tt * p_t * p_t + 2 * h_tp * p_t * p_phi + h_rr * p_r * p_r + h_thth * p_th * p_th + h_pp * p_phi * p_phi) / 2
    out[r <= LD(r_plus(float(a))) * LD(1.001)] = 0
    return out


def ref_step_longdouble(a, states, L, h):
    """The reference's RK4 step (metrics.py:306-323) on ref_rhs_longdouble: the yardstick of the FLOAT64 steps.  (The
    float64 oracle's own step is up to 26 units of A + h 2^-53 S from it: `pole_approach` at a = 0.9.)"""
    y = np.asarray(states, dtype=LD)
    h = np.broadcast_to(np.asarray(h, dtype=LD), (y.shape[0],))[:, None]
    k1 = ref_rhs_longdouble(a, y, L)
    k2 = ref_rhs_longdouble(a, y + LD(0.5) * h * k1, L)
    k3 = ref_rhs_longdouble(a, y + LD(0.5) * h * k2, L)
    k4 = ref_rhs_longdouble(a, y + h * k3, L)
    return y + (h / LD(6)) * (k1 + 2 * k2 + 2 * k3 + k4)


def _states(rng, n, r_lo, r_hi, th_lo, th_hi, log_theta=False, mirror=False):
    st = np.zeros((n, 5))
    st[:, 0] = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), n))
    th = np.exp(rng.uniform(np.log(th_lo), np.log(th_hi), n)) if log_theta else rng.uniform(th_lo, th_hi, n)
    if mirror:
        th = np.where(rng.random(n) < 0.5, th, np.pi - th)
    st[:, 1] = th
    st[:, 2] = rng.uniform(-6.0, 6.0, n)
    st[:, 3] = rng.uniform(-1.5, 1.5, n)
    st[:, 4] = rng.uniform(-8.0, 8.0, n)
    return st, rng.uniform(-8.0, 8.0, n)


RHS_CLASSES = ("far", "mid", "near", "pole", "equator", "edge")


def rhs_class(name, a, n, seed=0):
    """-> (states (n,5), L (n,)), float32 values.  On- and off-shell: p_r, p_theta and L are independent."""
    rng = np.random.default_rng([seed, RHS_CLASSES.index(name), int(round(a * 1000))])
    rp = r_plus(a)
    if name == "far":
        st, L = _states(rng, n, 20.0, 600.0, 0.05, np.pi - 0.05)
    elif name == "mid":
        st, L = _states(rng, n, 3.0, 20.0, 0.05, np.pi - 0.05)
    elif name == "near":
        st, L = _states(rng, n, 1.002 * rp, 1.2 * rp, 0.05, np.pi - 0.05)
    elif name == "pole":
        st, L = _states(rng, n, 3.0, 600.0, 1e-3, 3e-2, log_theta=True, mirror=True)
    elif name == "equator":
        st, L = _states(rng, n, 3.0, 600.0, 1.5, 1.64)
    else:
        # theta = 0 and theta = pi exactly.  Float32 has no pi: its nearest value lies 8.7e-8 beyond it, where sin^2 =
        # 7.6e-15 is of the size of the 1e-15 floor, which the float32 kernel ADDS where the reference takes the larger
        # (M<float>::sin2_floor).  The two differ there by 1e-15 / s2 of every L / s2 term -- by design, and without
        # effect on a ray: a geodesic that comes within 1e-7 rad of the axis has |L| < 1e-7 r.  So the theta = pi rows
        # carry L = 0, the only value a ray has on the axis; the theta = 0 rows (s2 is the floor itself on either side)
        # carry any L.
        st, L = _states(rng, n, 3.0, 600.0, 0.0, 0.0)
        st[n // 2:, 1] = np.float32(np.pi)
        L[n // 2:] = 0.0
    return f32(st), f32(L)


def inside_cut_class(a, n, seed=0):
    """States at or inside r_cut, where the reference's right-hand side is zero."""
    rng = np.random.default_rng([seed, 99, int(round(a * 1000))])
    st, L = _states(rng, n, 0.5 * r_plus(a), 1.0009 * r_plus(a), 0.05, np.pi - 0.05)
    return f32(st), f32(L)


STEP_CLASSES = ("far", "mid", "band", "near", "pole_approach")
BAND_R = (1.3, 4.0)      # radial range of `band`, in r_plus
NEAR_R = (1.05, 1.2)     # ... and of `near`, which exists up to NEAR_MAX_SPIN only
NEAR_MAX_SPIN = 0.9


def step_r_min(a):
    """The smallest radius the step classes cover at spin a, hence the smallest at which K_STEP was derived: the inner edge
    of `near`, or of `band` at the spins `near` does not exist at.  Below it no bound for one float32 step is stated
    anywhere: nothing here says that the kernel's step is sound there, nor that it is not."""
    return (NEAR_R[0] if abs(a) <= NEAR_MAX_SPIN else BAND_R[0]) * r_plus(a)


def fast_step_valid(a, out):
    """The validity test of the branch-free step on lt_kerr_step_probe's report `out` (min_r, max_d), with the r_cut the
    float32 kernels use: a lane for which it fails takes the checked step."""
    with np.errstate(invalid="ignore"):
        return (out["min_r"] > float(np.float32(r_plus(a) * 1.001))) & (out["max_d"] <= 0.25)


def step_class(name, a, n, seed=0, rounded=True):
    """-> (states (n,5), L (n,), h, refine) with h as the tracer's step-size rule gives it (metrics.py:597-611); None if
    the class does not exist at this spin.  Momenta of the size a ray from a camera at r ~ 50 has.  rounded=False: the
    values as drawn, at float64 precision (tests/dp45_blocks.py), not rounded to float32."""
    rng = np.random.default_rng([seed, 200 + (STEP_CLASSES + ("eq_band",)).index(name), int(round(a * 1000))])
    rp = r_plus(a)
    th = (0.35, np.pi - 0.35)
    if name == "far":
        (st, L), h, refine = _states(rng, n, 20.0, 600.0, *th), 1.0, 0
    elif name == "mid":
        (st, L), h, refine = _states(rng, n, 4.2 * rp, 20.0, *th), 1.0, 0
    elif name == "band":
        (st, L), h, refine = _states(rng, n, BAND_R[0] * rp, BAND_R[1] * rp, *th), 0.1, 0
    elif name == "near":
        if a > NEAR_MAX_SPIN:
            return None
        (st, L), h, refine = _states(rng, n, NEAR_R[0] * rp, NEAR_R[1] * rp, *th), 0.05, 0
    elif name == "pole_approach":
        (st, L), h, refine = _states(rng, n, 5.0, 50.0, 0.05, 0.3), 0.5, 1
        L *= np.sin(st[:, 1])  # (a ray this close to the axis has |L| <~ b sin theta)
    elif name == "eq_band":  # the polar angle strictly inside the fixed-quadrant band of the float32 streak
        (st, L), h, refine = _states(rng, n, 8.2 * rp, 600.0, 0.81, 2.33), 1.0, 0
    else:
        raise KeyError(name)
    return (f32(st), f32(L), h, refine) if rounded else (st, L, h, refine)


def step_unit(a, states, L, h, ref_step, u=U32):
    """-> (y1 (n,5) the float64 step, unit (n,5), keep (n,) bool) from the float64 step `ref_step(states, L, h) -> (y1,
    stage radii)` alone."""
    y1, unit, stage_r, stiff = _step_parts(a, states, L, h, ref_step, u)
    crossing = (stage_r <= 1.002 * r_cut(a)).any(axis=1)
    return y1, unit, ~(crossing | stiff)


def _step_parts(a, states, L, h, ref_step, u):
    st = np.asarray(states, dtype=np.float64)
    y1, stage_r = ref_step(st, L, h)
    A = u * np.abs(y1)
    for j in range(5):
        pert = st.copy()
        pert[:, j] += 2.0 * u * np.abs(st[:, j])
        A += np.abs(ref_step(pert, L, h)[0] - y1) / 2.0
    hS = np.broadcast_to(np.asarray(h, dtype=np.float64), (st.shape[0],))[:, None] * scales(a, st, L)
    stiff = (A > 2.0 ** 10 * u * (np.abs(y1) + hS)).any(axis=1)
    return y1, A + u * hS, stage_r, stiff


def fallback_class(a, n, seed=0, rounded=True):
    """States whose step fails the branch-free step's validity test.  First half: just outside r_cut and falling, so that
    later stages are evaluated at or inside it (h = 0.05); second half: a polar momentum that turns the stage angles by
    more than 0.25 rad (h = 0.5).  -> (states, L, h (n,))"""
    rng = np.random.default_rng([seed, 300, int(round(a * 1000))])
    rp, m = r_plus(a), n // 2
    st, L = _states(rng, n, 1.003 * rp, 1.03 * rp, 0.35, np.pi - 0.35)
    st[:m, 3] = -rng.uniform(0.5, 3.0, m)
    st[m:, 0] = rng.uniform(4.0, 8.0, n - m)
    st[m:, 1] = rng.uniform(0.5, np.pi - 0.5, n - m)
    st[m:, 4] = rng.choice([-1.0, 1.0], n - m) * rng.uniform(20.0, 60.0, n - m)
    h = np.where(np.arange(n) < m, 0.05, 0.5)
    return (f32(st), f32(L), h) if rounded else (st, L, h)


def fallback_unit(a, states, L, h, ref_step, u=U32):
    """step_unit for fallback_class: a stage inside r_cut is what the class is about, so a state is left out only where a
    float64 stage radius lies within 1e-3 r_cut of r_cut (either side may then see the jump in another stage), or is stiff."""
    y1, unit, stage_r, stiff = _step_parts(a, states, L, h, ref_step, u)
    ambiguous = (np.abs(stage_r / r_cut(a) - 1.0) < 1e-3).any(axis=1)
    return y1, unit, ~(ambiguous | stiff)


# ---- float64 truths from mpmath (160 bits) as unevaluated sums hi + lo of two float64 ---------------------------------------
_PREC = 160


def _split(t):
    hi = libmp.to_float(t, rnd=libmp.round_nearest)
    return hi, libmp.to_float(libmp.mpf_sub(t, libmp.from_float(hi), _PREC), rnd=libmp.round_nearest)


def mp_sincos(x):
    """-> (hi (n,2), lo (n,2)) with hi + lo = [sin x, cos x] to ~1e-32 relative."""
    x = np.asarray(x, dtype=np.float64).ravel()
    hi, lo = np.empty((x.size, 2)), np.empty((x.size, 2))
    for i, v in enumerate(x):
        c, s = libmp.mpf_cos_sin(libmp.from_float(float(v)), _PREC)
        hi[i, 0], lo[i, 0] = _split(s)
        hi[i, 1], lo[i, 1] = _split(c)
    return hi, lo


def mp_rcp(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    hi, lo = np.empty(x.size), np.empty(x.size)
    for i, v in enumerate(x):
        hi[i], lo[i] = _split(libmp.mpf_div(libmp.fone, libmp.from_float(float(v)), _PREC))
    return hi, lo


def mp_pow_m02(x):
    x = np.asarray(x, dtype=np.float64).ravel()
    hi, lo = np.empty(x.size), np.empty(x.size)
    e = libmp.mpf_div(libmp.from_int(-1), libmp.from_int(5), _PREC + 20)
    for i, v in enumerate(x):
        hi[i], lo[i] = _split(libmp.mpf_pow(libmp.from_float(float(v)), e, _PREC))
    return hi, lo


def err64(got, hi, lo):
    """|got - (hi + lo)|: absolute (n...) and in ulps of the true value (float64 ulp of hi).  got - hi is exact wherever
    the two are within a factor 2 (Sterbenz); a NaN or an infinity in `got` comes out as inf."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)
    e = np.where(np.isfinite(e), e, np.inf)
    return e, e / np.spacing(np.abs(hi))
