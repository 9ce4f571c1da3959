"""What tests/test_ray_ends_host.py and tests/test_gpu_ray_ends.py share: a ray's two ends -- the prologue's records, the
Schwarzschild integrator, the epilogue's extraction -- and the fixed-step RK4 loop body around the step, each against the
reference's statements in longdouble and against the oracle's own functions, in stated units.  

u = 2^-53 (float64) or 2^-24 (float32).  An error is a multiple of a UNIT built as in step_blocks.py: the sum S of the
magnitudes of the terms a quantity is formed from, times u, plus -- where a quantity is a function of rounded inputs -- the
first-order propagation A of one rounding of each input through the longdouble function.

INITIAL RECORDS (metrics.py:148-218), compared as p_phi, Theta = p_theta^2 and p_r^2, a clamped radicand counting as 0:
    rho = r sin(alpha) sqrt(Sigma / Delta),  alpha_s = -rho sin(theta),  beta_s = -rho cos(theta),  L = -alpha_s sin(th_obs)
    S_pphi  = |L|
    S_Theta = beta_s^2 + cos^2 alpha_s^2 + cos^2 L^2 / s2 + 2 a^2 cos^2
    S_pr2   = (1 + k_Delta) (|g_tt| + 2 |g_tphi L| + g_thth S_Theta + |g_phiphi| L^2) / g_rr,  k_Delta = (r^2 + a^2 + 2 M r) / Delta
  Schwarzschild (metrics.py:57-65):  w0^2 = 1 / b^2 - u^2 + 2 M u^3,  S_w0sq = 1 / b^2 + u^2 + 2 M u^3.

SCHWARZSCHILD STEP (metrics.py:74-88) of size h from (u, w): unit_i = A_i + h u S_i with S_u = |w|, S_w = |u| + 3 M u^2 and
    A_i = sum_j |y1_i(y0 + 2 u |y0_j| e_j) - y1_i(y0)| / 2 + u |y1_i|.
  A chord (metrics.py:90-111) from (u, w) to the candidate (un, wn), frac = (target - u) / (un - u):
    unit_wc  = unit_w + |wn - w| frac unit_u / |un - u| + u (|w| + |wn - w|),   unit_phi = h frac unit_u / |un - u| + u h.

FINAL ANGLE (metrics.py:363-416) as a function of the record x = (r, theta, phi, p_r, p_theta, p_phi):
    unit_fa = sum_j |fa(x + 2 u |x_j| e_j) - fa(x)| / 2  +  u S_c / |sin fa|  +  u |fa|
    S_c = (|sin th cos ph dr| + |r cos th cos ph dth| + |r sin th sin ph| S_dphi) / |v| + |cos fa|,
    S_dphi = |2 M a r / (Sigma Delta)| + |(Delta - a^2 s2) p_phi / (Sigma Delta s2)|.

THE BOUNDS are the float64 oracle's own worst error against longdouble in these units (float32: the oracle's float32 build,
every operation of the same statements rounded to float32), measured by tests/test_ray_ends_host.py on the classes below and
rounded up to an integer; the GPU is held to twice each (tests/test_gpu_ray_ends.py), and to 3 K where it is compared with
the oracle itself (K for the oracle's own distance from longdouble).  Measured values: DESIGN.md 2.1.

RK4 LOOP BODY: a row that goes on is held in step_blocks.py's step unit; a row that ends on a chord (metrics.py:628-647) from
y to the candidate n, frac = (target - r) / (n_r - r), in  unit_i + |n_i - y_i| frac unit_r / |n_r - r| + u (|y_i| + |n_i - y_i|).
"""
import math
from fractions import Fraction

import numpy as np

import step_blocks as sb

M = 1.0
LD = np.longdouble
U64 = 2.0 ** -53
U32 = 2.0 ** -24
SPINS = (0.0, 0.5, 0.9, 0.998, 1.0, -0.7)
N = 2048  # rows per class

# measured by tests/test_ray_ends_host.py (the oracle against longdouble), rounded up
K_IC = 9          # Kerr initial record: p_phi, Theta, p_r^2
K_W0 = 8          # Schwarzschild w0^2
K_SCHW64 = 2      # one Schwarzschild step, float64
K_SCHW32 = 1      # one Schwarzschild step, the reference's statements in float32
K_CHORD = 1       # the chord's w and phi, float64
K_EXT = 2         # final_alpha, float64
K_EXT_SCHW = 1    # final_alpha of the Schwarzschild tail, float64
K_RK4_CHORD = 2   # the RK4 chord's state, float64, in the chord's unit


def r_plus(a):
    return M + np.sqrt(M * M - a * a)


def same_bits(x, y):
    """Elementwise: two float64 arrays have the same bit pattern (a NaN equals a NaN)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def ulps(x, k):
    """x moved by k units in the last place (k may be negative)."""
    x = np.asarray(x, dtype=np.float64)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.inf if k > 0 else -np.inf)
    return x


# ---------------------------------------------------------------------------------------------------------------------------
# initial records
# ---------------------------------------------------------------------------------------------------------------------------
IC_R_OBS = ("3r+", 8.0, 12.0, 50.0, 300.0)
IC_THETA_OBS = (np.pi / 2, 1.0, 0.05, np.pi - 0.05)


def ic_rows(n=256, seed=0):
    """-> (alpha (m,), theta (m,)): alpha log-uniform in [1e-6, pi] and near pi, pi / 2 and pi / 2 +- 1e-9 (where p_r^2
    cancels to 0), pi itself; screen angles uniform in (-pi, pi], and at and one ulp beside +-pi / 2 and 0 (where the sign
    of p_theta switches: cos(theta) > 0 decides it), crossed with a few alphas."""
    rng = np.random.default_rng([seed, 11])
    al = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(np.pi), n)), np.pi - np.exp(rng.uniform(np.log(1e-6), 0.0, n // 4)),
                         [np.pi / 2, np.pi / 2 - 1e-9, np.pi / 2 + 1e-9, np.pi, 1e-6]])
    th = rng.uniform(-np.pi, np.pi, al.size)
    special = np.array([s * ulps(b, k) for b in (np.pi / 2, 0.0) for s in (1.0, -1.0) for k in (-1, 0, 1)] + [np.pi, -np.pi])
    sal = np.array([0.3, np.pi / 2, 2.5, np.pi / 2 - 1e-9])
    return np.concatenate([al, np.repeat(sal, special.size)]), np.concatenate([th, np.tile(special, sal.size)])


def ic_longdouble(a, r_obs, theta_obs, alpha, theta):
    """The statements of metrics.py:148-218 in longdouble.  -> dict(ok, p_phi, Theta, p_r2 (clamped at 0), negative (the
    sign of p_theta is -1), S_pphi, S_Theta, S_pr2); None for the values where the observer is not outside the horizon."""
    r, a, Mq, th = LD(r_obs), LD(a), LD(M), LD(theta_obs)
    sn, cs = np.sin(th), np.cos(th)
    s2 = max(sn * sn, LD(1e-15))
    Sigma = r * r + a * a * cs * cs
    Delta = r * r - 2 * Mq * r + a * a
    if not (Delta > 0 and Sigma > 0):
        return dict(ok=False)
    al, ts = np.asarray(alpha, dtype=LD), np.asarray(theta, dtype=LD)
    rho = r * np.sin(al) * np.sqrt(Sigma) / np.sqrt(Delta)
    a_s, b_s = -rho * np.sin(ts), -rho * np.cos(ts)
    L = -a_s * sn
    Q = b_s * b_s + cs * cs * (a_s * a_s - a * a)
    Theta = Q - cs * cs * (L * L / s2 - a * a)
    S_Theta = b_s * b_s + cs * cs * a_s * a_s + cs * cs * L * L / s2 + 2 * a * a * cs * cs
    Theta = np.maximum(Theta, 0)
    SD = Sigma * Delta
    g_tt = -((r * r + a * a) ** 2 - a * a * Delta * s2) / SD
    g_tp = -2 * Mq * a * r / SD
    g_rr, g_thth = Delta / Sigma, 1 / Sigma
    g_pp = (Delta - a * a * s2) / (SD * s2)
    other = g_tt - 2 * g_tp * L + g_thth * Theta + g_pp * L * L
    kD = (r * r + a * a + 2 * Mq * r) / Delta
    S_pr2 = (1 + kD) * (abs(g_tt) + 2 * np.abs(g_tp * L) + g_thth * S_Theta + abs(g_pp) * L * L) / g_rr
    return dict(ok=True, p_phi=L, Theta=Theta, p_r2=np.maximum(-other / g_rr, 0), negative=np.cos(ts) > 0,
                S_pphi=np.abs(L), S_Theta=S_Theta, S_pr2=S_pr2)


def ic_errors(ref, p_r, p_theta, p_phi, u=U64):
    """Errors of a record (float64 arrays) against ic_longdouble's, in units -> (n,3) for p_phi, Theta, p_r^2.  (S > 0
    wherever alpha > 0: the smallest normal stands in for S = 0.)"""
    tiny = LD(np.finfo(np.float64).tiny)
    e = np.empty((np.size(p_r), 3))
    e[:, 0] = (np.abs(np.asarray(p_phi, dtype=LD) - ref["p_phi"]) / (u * np.maximum(ref["S_pphi"], tiny))).astype(np.float64)
    e[:, 1] = (np.abs(np.asarray(p_theta, dtype=LD) ** 2 - ref["Theta"]) / (u * np.maximum(ref["S_Theta"], tiny))).astype(np.float64)
    e[:, 2] = (np.abs(np.asarray(p_r, dtype=LD) ** 2 - ref["p_r2"]) / (u * np.maximum(ref["S_pr2"], tiny))).astype(np.float64)
    return e


def ic_observers(a):
    return [(3.0 * r_plus(abs(a)) if r == "3r+" else r, t) for r in IC_R_OBS for t in IC_THETA_OBS]


def schw_w0_longdouble(r_obs, alpha):
    """metrics.py:57-65 in longdouble -> (w0^2 unclamped, S)."""
    r, Mq = LD(r_obs), LD(M)
    f0 = 1 - 2 * Mq / r
    b = r * np.sin(np.asarray(alpha, dtype=LD)) / np.sqrt(f0)
    u = 1 / r
    with np.errstate(divide="ignore"):
        return 1 / (b * b) - u * u + 2 * Mq * u ** 3, 1 / (b * b) + u * u + 2 * Mq * u ** 3


# ---------------------------------------------------------------------------------------------------------------------------
# the Schwarzschild integrator
# ---------------------------------------------------------------------------------------------------------------------------
SCHW_R_OBS = 50.0
U_CAPTURE = 1.0 / (2.0 * M * 1.01)
U_ESCAPE = 1.0 / (2.0 * SCHW_R_OBS)
H_PARTIAL = 0.05 - 7.0e-3       # a last, shorter step: phi_max = H_PARTIAL < h_max = 0.05
SCHW_STEPS = (("h05", 0.05, 0.05), ("h01", 0.01, 0.01), ("partial", H_PARTIAL, 0.05))   # name, phi_max, h_max: one step each

# (phi_max, h_max) -> the steps the reference's loop takes (the table of the step-count issue, and a few more)
STEP_COUNTS = {(50.0, 0.05): 1001, (50.0, 0.01): 5001, (6.3, 0.1): 64, (30.0, 0.1): 300, (40.0, 0.02): 2000,
               (12.5, 0.05): 250, (20.0, 0.03): 667, (10.0, 0.3): 34, (8 * np.pi, 0.05): 503,
               (3.2, 0.05): 65, (0.05, 0.05): 1, (0.043, 0.05): 1, (1.0, 0.1): 11, (3.0, 0.07): 43, (100.0, 0.05): 2001}


def ref_step_plan(phi_max, h_max):
    """The reference's loop (metrics.py:68-73) in Python float64 -> (steps, the last step's h)."""
    phi, steps, h = 0.0, 0, 0.0
    while phi < phi_max:
        h = h_max
        remaining = phi_max - phi
        if remaining < h:
            h = remaining
        if h <= 0.0:
            break
        phi = phi + h
        steps += 1
    return steps, h


def schw_rows(n=N, seed=0, f32=False):
    """(u, w): u log-uniform from u_escape = 1 / (2 r_obs) up to u_capture, |w| from 0 up to 0.3 (a tenth of the rows w = 0
    exactly)."""
    rng = np.random.default_rng([seed, 21])
    u = np.exp(rng.uniform(np.log(U_ESCAPE), np.log(U_CAPTURE), n))
    w = rng.uniform(-0.3, 0.3, n)
    w[::10] = 0.0
    return (sb.f32(u), sb.f32(w)) if f32 else (u, w)


def schw_step_ld(u, w, h):
    """The reference's step (metrics.py:74-88, its association) in longdouble -> (un, wn)."""
    u, w, h, Mq = np.asarray(u, dtype=LD), np.asarray(w, dtype=LD), LD(h), LD(M)

    def f(uu, ww):
        return ww, -uu + 3 * Mq * uu * uu
    k1u, k1w = f(u, w)
    k2u, k2w = f(u + LD(0.5) * h * k1u, w + LD(0.5) * h * k1w)
    k3u, k3w = f(u + LD(0.5) * h * k2u, w + LD(0.5) * h * k2w)
    k4u, k4w = f(u + h * k3u, w + h * k3w)
    return u + (h / 6) * (k1u + 2 * k2u + 2 * k3u + k4u), w + (h / 6) * (k1w + 2 * k2w + 2 * k3w + k4w)


def schw_unit(u, w, h, eps):
    """-> (un, wn longdouble, unit_u, unit_w float64) of one step of size h."""
    u, w = np.asarray(u, dtype=np.float64), np.asarray(w, dtype=np.float64)
    un, wn = schw_step_ld(u, w, h)
    A = [eps * np.abs(un), eps * np.abs(wn)]
    for du, dw in ((2 * eps * np.abs(u), 0.0), (0.0, 2 * eps * np.abs(w))):
        pu, pw = schw_step_ld(u.astype(LD) + du, w.astype(LD) + dw, h)
        A[0] = A[0] + np.abs(pu - un) / 2
        A[1] = A[1] + np.abs(pw - wn) / 2
    S_u, S_w = np.abs(w), np.abs(u) + 3 * M * u * u
    return un, wn, (A[0] + h * eps * S_u).astype(np.float64), (A[1] + h * eps * S_w).astype(np.float64)


def schw_chord_units(u, w, h, target, eps):
    """The chord to `target` of the step of size h from (u, w) -> (wc, phi_used longdouble, unit_wc, unit_phi)."""
    un, wn, unit_u, unit_w = schw_unit(u, w, h, eps)
    frac = (LD(target) - u) / (un - u)
    amp = (frac / np.abs(un - u)).astype(np.float64) * unit_u
    dw = np.abs(wn - w).astype(np.float64)
    return w + frac * (wn - w), frac * LD(h), unit_w + dw * amp + eps * (np.abs(w) + dw), h * amp + eps * h


def schw_landing(u, target, h, w_start=0.1):
    """w (float64) for which the step of size h from (u, w) lands on `target`: Newton on the longdouble step (d un / d w = h
    to first order).  h ulp(w) / 2 is a hundredth of an ulp of the landing point, so the float64 step -- the reference's
    association or the kernel's -- rounds to `target` itself."""
    w = LD(w_start)
    for _ in range(8):
        w = w - (schw_step_ld(u, w, h)[0] - LD(target)) / LD(h)
    return float(w)


def schw_event_rows():
    """The event table, float64, r_obs = 50, h = 0.05 -> list of (name, u, w).  (denom == 0 and a clamped frac cannot be
    reached: a capture needs u < u_capture <= un and an escape u > u_escape >= un, so un - u has the sign and at least the
    size of target - u, and 0 < frac <= 1 before the clamp; frac == 1 is the row that lands on the target.)"""
    h, uc, ue = 0.05, U_CAPTURE, U_ESCAPE
    u_in, u_out = uc - 0.004, ue + 0.002
    return [("lands_on_u_capture", u_in, schw_landing(u_in, uc, h)),
            ("lands_an_ulp_below_u_capture", u_in, schw_landing(u_in, float(ulps(uc, -1)), h)),
            ("lands_an_ulp_above_u_capture", u_in, schw_landing(u_in, float(ulps(uc, 1)), h)),
            ("starts_on_u_capture_inward", uc, 0.2), ("starts_on_u_capture_outward", uc, -0.2),
            ("starts_an_ulp_below_u_capture", float(ulps(uc, -1)), 0.2),
            ("starts_on_u_escape_outward", ue, -0.05), ("starts_on_u_escape_inward", ue, 0.05),
            ("starts_an_ulp_above_u_escape", float(ulps(ue, 1)), -0.05),
            ("lands_on_u_escape", u_out, schw_landing(u_out, ue, h, -0.04)),
            ("lands_an_ulp_above_u_escape", u_out, schw_landing(u_out, float(ulps(ue, 1)), h, -0.04)),
            ("capture_chord", uc - 0.005, 0.25), ("capture_chord_late", uc - 0.0123, 0.25),
            ("escape_chord", ue + 0.001, -0.05), ("escape_chord_early", ue + 1e-6, -0.05),
            ("no_event", 0.1, 0.01), ("at_rest_on_the_photon_sphere", 1.0 / (3.0 * M), 0.0)]


# ---------------------------------------------------------------------------------------------------------------------------
# extraction
# ---------------------------------------------------------------------------------------------------------------------------
PI, INV_PI = 3.141592653589793, 0.3183098861837907


def half_orbit_values(seed=0):
    """The values half_orbits is held to Python's own abs(phi) // pi on."""
    rng = np.random.default_rng([seed, 31])
    ks = np.concatenate([np.arange(1, 4097), 2 ** np.arange(13, 49)]).astype(np.float64)
    kpi = ks * math.pi
    kpi = kpi[kpi < 1e15]
    near = np.concatenate([ulps(kpi, k) for k in range(-4, 5)])
    rand = np.exp(rng.uniform(np.log(1e-300), np.log(1e15), 100000))
    rand = rand[rand < 1e15]
    special = np.array([0.0, -0.0, 5e-324, 2.2e-308, -1.0, -math.pi, -7.5, -3e14, float(ulps(1e15, -1))])
    return np.concatenate([near, -near[::7], rand, special])


def python_half_orbits(phi):
    return np.array([int(abs(float(p)) // math.pi) for p in phi], dtype=np.int64)


def half_orbits_restated(phi):
    """The device's statements (csrc/lt_kernels.hpp, half_orbits): q = floor(|phi| INV_PI), r = fma(-q, PI, |phi|) -- the exact
    residual (rational arithmetic) rounded once --, q - 1 if r < 0, q + 1 if r >= PI; 0 unless |phi| < 1e15."""
    out = np.zeros(len(phi), dtype=np.int64)
    fpi = Fraction(PI)
    for i, p in enumerate(phi):
        a = abs(float(p))
        if not a < 1e15:
            continue
        q = math.floor(a * INV_PI)
        r = float(Fraction(a) - q * fpi)
        out[i] = q - 1 if r < 0.0 else (q + 1 if r >= PI else q)
    return out


def kerr_fa_longdouble(a, rec):
    """metrics.py:377-416 in longdouble on records (n,6) [r, theta, phi, p_r, p_theta, p_phi], p_t = -1.
    -> (fa, S_c): the angle and the scale of its cosine's terms."""
    x = np.asarray(rec, dtype=LD)
    r, th, ph, pr, pth, L = (x[:, j] for j in range(6))
    a, Mq = LD(a), LD(M)
    sn, cs, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    s2 = np.maximum(sn * sn, LD(1e-15))
    Sigma = r * r + a * a * cs * cs
    Delta = r * r - 2 * Mq * r + a * a
    dr = Delta / Sigma * pr
    dth = pth / Sigma
    t1, t2 = 2 * Mq * a * r / (Sigma * Delta), (Delta - a * a * s2) / (Sigma * Delta * s2) * L
    dph = t1 + t2
    vx = sn * cp * dr + r * cs * cp * dth - r * sn * sp * dph
    vy = sn * sp * dr + r * cs * sp * dth + r * sn * cp * dph
    vz = cs * dr - r * sn * dth
    vm = np.sqrt(vx * vx + vy * vy + vz * vz)
    c = np.clip(-vx / vm, -1, 1)
    S_c = (np.abs(sn * cp * dr) + np.abs(r * cs * cp * dth) + np.abs(r * sn * sp) * (np.abs(t1) + np.abs(t2))) / vm + np.abs(c)
    return np.arccos(c), S_c


def fa_unit(fa_fn, rec, eps):
    """-> (fa longdouble, unit float64) of an angle function fa_fn(rec) -> (fa, S_c) on records (n,k)."""
    rec = np.asarray(rec, dtype=np.float64)
    fa, S_c = fa_fn(rec)
    A = np.zeros(rec.shape[0], dtype=LD)
    for j in range(rec.shape[1]):
        p = rec.astype(LD)
        p[:, j] += 2 * eps * np.abs(rec[:, j])
        A += np.abs(fa_fn(p)[0] - fa) / 2
    return fa, (A + eps * S_c / np.abs(np.sin(fa)) + eps * np.abs(fa)).astype(np.float64)


EXT_R_OBS = (12.0, 50.0, 300.0)


def kerr_exit_rows(a, r_obs, n=N, seed=0):
    """Records (n,6) of rays leaving through r_escape = 2 r_obs: exit directions from 1e-6 off the -x axis (fa -> 0) to 1e-6
    off +x (fa -> pi), log-spaced towards both ends; theta_f across the sphere and, for an eighth of the rows, 1e-3 ... 1e-1
    from a pole; windings 0 ... 6 pi of either sense.  The momenta are the ones whose exit velocity is that direction with
    |v| ~ 1 (computed in float64: they are inputs)."""
    rng = np.random.default_rng([seed, 41, 2000 + int(round(a * 1000)), int(r_obs)])
    r = np.full(n, 2.0 * r_obs)
    th = rng.uniform(0.2, np.pi - 0.2, n)
    pole = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1), n))
    th[::8] = np.where(rng.random(n) < 0.5, pole, np.pi - pole)[::8]
    ph = rng.uniform(-6 * np.pi, 6 * np.pi, n)
    kind = rng.integers(0, 3, n)
    small = np.exp(rng.uniform(np.log(1e-6), np.log(1.0), n))
    fa = np.where(kind == 0, small, np.where(kind == 1, np.pi - small, rng.uniform(0.0, np.pi, n)))
    az = rng.uniform(0, 2 * np.pi, n)
    speed = rng.uniform(0.8, 1.2, n)
    v = speed * np.array([-np.cos(fa), np.sin(fa) * np.cos(az), np.sin(fa) * np.sin(az)])
    sn, cs, sp, cp = np.sin(th), np.cos(th), np.sin(ph), np.cos(ph)
    dr = v[0] * sn * cp + v[1] * sn * sp + v[2] * cs
    dth = (v[0] * cs * cp + v[1] * cs * sp - v[2] * sn) / r
    dph = (-v[0] * sp + v[1] * cp) / (r * sn)
    s2 = np.maximum(sn * sn, 1e-15)
    Sigma, Delta = r * r + a * a * cs * cs, r * r - 2 * M * r + a * a
    L = (dph - 2 * M * a * r / (Sigma * Delta)) * (Sigma * Delta * s2) / (Delta - a * a * s2)
    return np.stack([r, th, ph, dr * Sigma / Delta, dth * Sigma, L], axis=1)


def kerr_fin(rec, event, steps=0):
    """Records (n,6) -> (fin0, fin1) in the integrate kernels' layout (store_fin)."""
    rec = np.asarray(rec, dtype=np.float64)
    n = rec.shape[0]
    fin1 = np.stack([rec[:, 4], rec[:, 5], np.broadcast_to(np.asarray(event, dtype=np.float64), (n,)),
                     np.broadcast_to(np.asarray(steps, dtype=np.float64), (n,))], axis=1)
    return np.ascontiguousarray(rec[:, :4]), np.ascontiguousarray(fin1)


def schw_fin(u, w, phi, event, steps=0):
    """(u, w, phi_f) -> (fin0, fin1) with phi_f handed over as phi_last (no full steps), so that any float64 phi passes."""
    u = np.asarray(u, dtype=np.float64)
    n = u.size
    z = np.zeros(n)
    b = lambda v: np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))  # noqa: E731
    return np.stack([u, b(w), b(phi), z], axis=1), np.stack([z, z, b(event), b(steps)], axis=1)


def schw_fa_longdouble(rec):
    """metrics.py:137-145 in longdouble on (n,3) [u, w, phi] -> (fa, S_c).  cos(heading) = x / hypot(x, y) with
    x = dr cos - r sin, y = dr sin + r cos: S_c is the magnitude of x's two terms over the hypotenuse, plus |cos|."""
    x = np.asarray(rec, dtype=LD)
    u, w, ph = x[:, 0], x[:, 1], x[:, 2]
    r = 1 / u
    d = -w / (u * u)
    sp, cp = np.sin(ph), np.cos(ph)
    hx, hy = d * cp - r * sp, d * sp + r * cp
    hyp = np.sqrt(hx * hx + hy * hy)
    c = np.clip(-hx / hyp, -1, 1)
    return np.arccos(c), (np.abs(d * cp) + np.abs(r * sp)) / hyp + np.abs(c)


def schw_exit_rows(n=N, seed=0):
    """(n,3) [u, w, phi]: u at u_escape of r_obs in {12, 50, 300}, headings across the plane and towards both axes, windings
    0 ... 6 pi of either sense."""
    rng = np.random.default_rng([seed, 51])
    u = 1.0 / (2.0 * rng.choice(EXT_R_OBS, n))
    ph = rng.uniform(-6 * np.pi, 6 * np.pi, n)
    kind = rng.integers(0, 3, n)
    small = np.exp(rng.uniform(np.log(1e-6), np.log(1.0), n))
    psi = np.where(kind == 0, small, np.where(kind == 1, np.pi - small, rng.uniform(0.0, np.pi, n))) * rng.choice([-1.0, 1.0], n)
    # the direction of motion makes the angle psi with the outward radial direction: dr/dphi = r / tan(psi)
    w = -(u * u) * (1.0 / u) / np.tan(psi)
    return np.stack([u, w, ph], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------
# errors in units of a function under test (the oracle's on the CPU, the device's on the GPU), on the classes above
# ---------------------------------------------------------------------------------------------------------------------------
def schw_step_errors(step, f32):
    """Errors in units of a one-step function step(u, w, phi_max, h_max) -> (un, wn, event) on every class; rows whose
    longdouble candidate lies within 8 units of an event threshold are left out (at most 2 %)."""
    eps = U32 if f32 else U64
    out = {}
    for name, phi_max, h_max in SCHW_STEPS:
        u, w = schw_rows(f32=f32)
        h = float(np.float32(phi_max)) if f32 else phi_max
        un, wn, unit_u, unit_w = schw_unit(u, w, h, eps)
        unf = un.astype(np.float64)
        uc, ue = (float(np.float32(U_CAPTURE)), float(np.float32(U_ESCAPE))) if f32 else (U_CAPTURE, U_ESCAPE)
        keep = (np.abs(unf - uc) > 8 * unit_u) & (np.abs(unf - ue) > 8 * unit_u) & (u < uc) & (u > ue)
        plain = keep & (unf < uc) & (unf > ue)
        assert keep.mean() >= 0.98 and plain.mean() > 0.9
        gu, gw, ev = step(u, w, phi_max, h_max)
        assert np.array_equal(ev[keep] == 2, plain[keep])
        eu = (np.abs(gu.astype(LD) - un).astype(np.float64) / unit_u)[plain]
        ew = (np.abs(gw.astype(LD) - wn).astype(np.float64) / unit_w)[plain]
        out[name] = (eu.max(), ew.max())
    return out


def schw_chord_rows():
    """Rows whose step of 0.05 crosses u_capture (first half) or u_escape -> (u, w, target)."""
    rng = np.random.default_rng([0, 22])
    n = N // 2
    wc, we = rng.uniform(0.05, 0.3, n), -rng.uniform(0.005, 0.05, n)
    uc = U_CAPTURE - 0.05 * wc * rng.uniform(0.02, 0.9, n)
    ue = U_ESCAPE - 0.05 * we * rng.uniform(0.02, 0.9, n)
    return np.concatenate([uc, ue]), np.concatenate([wc, we]), np.concatenate([np.full(n, U_CAPTURE), np.full(n, U_ESCAPE)])


def schw_chord_errors(got_u, got_w, got_phi, got_ev):
    u, w, target = schw_chord_rows()
    wc, phi, unit_w, unit_phi = (np.empty(u.size, dtype=LD), np.empty(u.size, dtype=LD), np.empty(u.size), np.empty(u.size))
    for t in (U_CAPTURE, U_ESCAPE):
        m = target == t
        wc[m], phi[m], unit_w[m], unit_phi[m] = schw_chord_units(u[m], w[m], 0.05, t, U64)
    assert np.array_equal(got_ev, np.where(target == U_CAPTURE, -1, 1)) and np.array_equal(got_u, target)
    return (np.abs(got_w.astype(LD) - wc).astype(np.float64) / unit_w).max(), (np.abs(got_phi.astype(LD) - phi).astype(np.float64) / unit_phi).max()


def kerr_fa_errors(extract):
    """extract(a, rec (n,6)) -> (fa, status): errors in units over every exit class, and where the worst is."""
    worst, at = 0.0, None
    for a in SPINS:
        for r_obs in EXT_R_OBS:
            rec = kerr_exit_rows(a, r_obs)
            fa, unit = fa_unit(lambda x: kerr_fa_longdouble(a, x), rec, U64)
            got, status = extract(a, rec)
            assert (status == 1).all() and np.isfinite(got).all()
            e = np.abs(got.astype(LD) - fa).astype(np.float64) / unit
            if e.max() > worst:
                i = int(np.argmax(e))
                worst, at = e.max(), (a, r_obs, float(fa[i]), rec[i].tolist())
            assert float(fa.min()) < 3e-6 and float(fa.max()) > np.pi - 3e-6
    return worst, at


def schw_fa_errors(extract):
    rec = schw_exit_rows()
    fa, unit = fa_unit(schw_fa_longdouble, rec, U64)
    got, status = extract(rec)
    assert (status == 1).all() and np.isfinite(got).all()
    e = np.abs(got.astype(LD) - fa).astype(np.float64) / unit
    i = int(np.argmax(e))
    return e.max(), (float(fa[i]), rec[i].tolist())


# ---------------------------------------------------------------------------------------------------------------------------
# the fixed-step RK4 loop body: the decision table
# ---------------------------------------------------------------------------------------------------------------------------
RK4_R_OBS = 50.0
RK4_LAMBDA_MAX = 5000.0
RK4_SPINS = (0.0, 0.9, 0.998, -0.7)


RK4_CLASSES = ("capture_chord", "cap", "lam", "starts", "escape_chord", "p_", "steps_below_zero", "redo_radius", "redo_angle", "plain")


def rk4_class(name):
    return next(c for c in RK4_CLASSES if name.startswith(c))


def rk4_table(a, f32=False, variants=1, seed=0):
    """The rows of the decision table at spin a -> dict(names, st (n,5), L, refine, lam).  (A step cannot cross both radii,
    and denom == 0 cannot be reached: a capture needs r_prev > r_capture >= r_next, an escape r_prev < r_escape <= r_next,
    which exclude each other and r_next == r_prev.)
    variants > 1: every row that many times, the first as stated and the others with theta in [0.9, 2.2], p_theta scaled by
    0.3 ... 1.5 and L in [-4, 4] drawn at random (`name#v`).
    f32: the values a float32 record can hold -- everything rounded to float32; radii beside a threshold 2^-18 of it away
    where the float64 table is an ulp away (the kernel's thresholds are the float32 of the reference's, so an input nearer
    than a float32 ulp is on one side for the one and on the other for the other); for the same reason no row starts ON
    r_capture or r_escape and no capture chord starts within 1e-5 r_capture of it."""
    rc, resc = r_plus(abs(a)) * 1.01, RK4_R_OBS * 2.0
    rng = np.random.default_rng([seed, 61, 2000 + int(round(a * 1000)), int(f32)])
    names, st, L, refine, lam = [], [], [], [], []

    def row(name, r, p_r, rf=0, lm=0.0, p_th=1.5, ell=2.0, th=1.2):
        for v in range(variants):
            names.append(name if variants == 1 else f"{name}#{v}")
            if v:
                th, p_th, ell = rng.uniform(0.9, 2.2), p_th * rng.uniform(0.3, 1.5), rng.uniform(-4.0, 4.0)
            st.append([r, th, 0.3, p_r, p_th]); L.append(ell); refine.append(rf); lam.append(lm)

    def beside(x, k):
        return x * (1.0 + k * 2.0 ** -18) if f32 else float(ulps(x, k))
    for mult in (4.0, 2.0, 1.2):                      # each cap of kerr_rk4_h, on and just beside its radius
        for k in ((-1, 1) if f32 else (-1, 0, 1)):
            for rf in (0, 1):
                row(f"cap_{mult}_{k:+d}ulp_refine{rf}", beside(rc * mult, k), -0.4, rf)
    below = float(np.nextafter(np.float32(RK4_LAMBDA_MAX), np.float32(0))) if f32 else float(ulps(RK4_LAMBDA_MAX, -1))
    for rf in (0, 1):                                 # the range end
        row(f"lam_at_lambda_max_refine{rf}", 30.0, -0.9, rf, RK4_LAMBDA_MAX)
        row(f"lam_an_ulp_below_lambda_max_refine{rf}", 30.0, -0.9, rf, below)
        row(f"lam_within_a_base_step_refine{rf}", 30.0, -0.9, rf, RK4_LAMBDA_MAX - 0.3)
        row(f"lam_within_a_base_step_near_refine{rf}", 1.5 * rc, -0.2, rf, RK4_LAMBDA_MAX - 0.04)
    if not f32:
        row("starts_on_r_capture_inward", rc, -2.0)   # the strict compares act on inputs
        row("starts_on_r_escape_outward", resc, 0.9)
    row("starts_just_above_r_capture_inward", beside(rc, 1), -2.0)
    row("starts_just_below_r_escape_outward", beside(resc, -1), 0.9)
    for eps in ((1e-5, 1e-4, 3e-3, 2e-2) if f32 else (1e-9, 1e-4, 3e-3, 2e-2)):   # chords
        for p_r in (-1.0, -6.0):
            row(f"capture_chord_{eps}_{p_r}", rc * (1.0 + eps), p_r)
    for eps in (1e-12, 1e-6, 1e-3, 8e-3):
        row(f"escape_chord_{eps}", resc * (1.0 - eps), 0.9)
        row(f"escape_chord_{eps}_refine", resc * (1.0 - eps), 0.9, 1)
    for rf in (0, 1):                                 # h, h / 2, ... down to h_floor, then invalid
        row(f"p_r_inf_refine{rf}", 30.0, np.inf, rf)
        row(f"p_theta_nan_refine{rf}", 30.0, -0.9, rf, p_th=np.nan)
        row(f"p_r_inf_near_refine{rf}", 1.5 * rc, -np.inf, rf)
        for p_r in (-12.0, -40.0, -300.0, -1e4, -1e8):
            row(f"steps_below_zero_{p_r}_refine{rf}", 8.0, p_r, rf)
    for p_r in (-0.5, -2.0, -8.0):                    # redo lanes: a stage at or inside r_cut
        for f in (1.0031, 1.012, 1.03):
            row(f"redo_radius_{f}_{p_r}", f * r_plus(abs(a)), p_r)
    for p_th in (25.0, -40.0, 60.0):                  # redo lanes: a stage angle offset beyond 0.25 rad
        for r in (4.5, 7.0):
            row(f"redo_angle_{r}_{p_th}", r, -0.5, p_th=p_th, th=1.4)
    row("plain_far", 40.0, -0.9)
    row("plain_far_refine", 40.0, -0.9, 1)
    t = dict(names=names, st=np.array(st), L=np.array(L), refine=np.array(refine, dtype=np.uint8), lam=np.array(lam))
    if f32:
        with np.errstate(over="ignore"):
            t["st"], t["L"], t["lam"] = sb.f32(t["st"]), sb.f32(t["L"]), sb.f32(t["lam"])
    return t


def rk4_oracle(a, t, oracle):
    return oracle.rk4_iteration(t["st"], t["L"], t["lam"], M, a, r_obs=RK4_R_OBS, lambda_max=RK4_LAMBDA_MAX, axis_refine=t["refine"])


def rk4_step_units(a, t, o, eps, oracle):
    """For the rows that the reference's iteration o leaves running or ends on a chord: the accepted step of size o["h"] in
    longdouble and its unit -> (rows, candidate (m,5) longdouble, unit (m,5), keep (m,)); keep is false only where a float64
    stage radius lies within 1e-3 r_cut of r_cut (either side may see the right-hand side's jump in another stage) or the step
    is stiff (step_blocks.fallback_unit): the rows whose stages sit INSIDE r_cut stay."""
    rows = np.nonzero(np.isin(o["event"], (4, -1, 1)))[0]
    st, L, h = t["st"][rows], t["L"][rows], o["h"][rows]
    _, unit, keep = sb.fallback_unit(a, st, L, h, lambda s, l, hh: oracle.rk4_step_kerr(s, l, hh, M, a), u=eps)
    return rows, sb.ref_step_longdouble(a, st, L, h), unit, keep


def rk4_state_errors(a, t, o, got_state, eps, oracle):
    """Errors in units of the states `got_state` (n,5) a function under test leaves the table's rows in, against longdouble:
    the candidate on rows that go on, the chord (metrics.py:628-647) on rows that end on one, whose unit is
        unit_i + |n_i - y_i| frac unit_r / |n_r - r| + eps (|y_i| + |n_i - y_i|),   frac = (target - r) / (n_r - r).
    -> (rows, err (m,5), keep, chord (m,) bool)"""
    rows, cand, unit, keep = rk4_step_units(a, t, o, eps, oracle)
    y = t["st"][rows].astype(LD)
    ev = o["event"][rows]
    chord = ev != 4
    target = np.where(ev == -1, LD(r_plus(abs(a)) * 1.01), LD(2 * RK4_R_OBS))
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.clip((target - y[:, 0]) / (cand[:, 0] - y[:, 0]), 0, 1)
        d = np.abs(cand - y).astype(np.float64)
        amp = (frac / np.abs(cand[:, 0] - y[:, 0])).astype(np.float64) * unit[:, 0]
        cunit = unit + d * amp[:, None] + eps * (np.abs(t["st"][rows]) + d)
        want = np.where(chord[:, None], y + frac[:, None] * (cand - y), cand)
        u = np.where(chord[:, None], cunit, unit)
        err = np.abs(np.asarray(got_state, dtype=np.float64)[rows].astype(LD) - want).astype(np.float64) / u
    return rows, err, keep & np.isfinite(u).all(axis=1), chord


def rk4_f32_stable(a, t, o, oracle):
    """The rows of a float32 table whose reference decision (o, the float64 oracle's iteration on them) does not change when
    the candidate of any of its attempts moves by 2 K_FALLBACK float32 units: a failed attempt stays non-finite or at r <= 0,
    the accepted one stays finite, at r > 0 and on its side of r_capture and r_escape.  From the reference alone."""
    rc, resc = r_plus(abs(a)) * 1.01, 2 * RK4_R_OBS
    stable = np.ones(len(t["names"]), dtype=bool)
    h0 = o["h"] * 2.0 ** (np.maximum(o["attempts"], 1) - 1)
    step = lambda s, l, hh: oracle.rk4_step_kerr(s, l, hh, M, a)  # noqa: E731
    for j in range(int(o["attempts"].max())):
        rows = np.nonzero(o["attempts"] > j)[0]
        with np.errstate(all="ignore"):
            y1, unit, _, _ = sb._step_parts(a, t["st"][rows], t["L"][rows], h0[rows] / 2.0 ** j, step, sb.U32)
            r1, m = y1[:, 0], 2 * sb.K_FALLBACK * unit[:, 0]
            finite = np.isfinite(y1).all(axis=1)
            last = (o["attempts"][rows] == j + 1) & (o["event"][rows] != 0)
            ok_last = finite & np.isfinite(m) & (r1 > m) & (np.abs(r1 - rc) > m) & (np.abs(r1 - resc) > m)
            ok_fail = ~finite | (r1 < -m)
        stable[rows] &= np.where(last, ok_last, ok_fail)
    return stable


def rk4_plain_rows(a, n, seed=0):
    """Ordinary far-field lanes (the `far` class of step_blocks.py, unrounded)."""
    st, L, _, _ = sb.step_class("far", abs(a), n, seed=seed, rounded=False)
    return st, L
