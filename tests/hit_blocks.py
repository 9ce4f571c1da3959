"""What tests/test_hit_blocks_host.py and tests/test_gpu_hit_blocks.py share: the time a stored hit carries, block by block --
the rates t', r', theta' (time_rates, lt_hit_time.hpp), the rule that integrates t' over one step or a part of one
(step_time), and the two-term sum a lane carries them in -- each stated in longdouble, with the classes of states and steps and
the units an error is stated in.  Built on tests/step_blocks.py (the scales S) and tests/disk_blocks.py (real steps, the
Hermite data).

THE REFERENCE is disk.time_rates / disk._hermite / disk.step_time (numpy, float64).  rates_T / step_time_T restate them with
every operation in the precision T (float32: numpy's float32 arithmetic and sine, every operation rounded; float64: the
reference's own bits, asserted by the host test); rates_ld / step_time_ld are the same statements in longdouble.

UNITS.  u = 2^-24 or 2^-53.  At a state (r, theta) with ra = r^2 + a^2, Sigma = ra - a^2 s2, Delta = ra - 2 M r,
P = ra - a L, k_Delta = (ra + 2 M r) / Delta, k_P = (ra + |a L|) / |P| (step_blocks.py: the two cancellations):
    S_t   = [ ra |P| / Delta (1 + k_Delta + k_P) + |a L| + a^2 s2 ] / Sigma
            + 4 a^2 |sin theta| (|t'| + 1) / Sigma
the sum of the magnitudes t' is formed from, plus what an absolute error 2 u of the sine does: d s2 = 2 |s| 2 u, and
dt'/ds2 = a^2 (t' - 1) / Sigma (both Sigma and the numerator carry -a^2 s2).  r' and theta' take step_blocks.scales.
    U_dt(tau) = u (tau h / 6) (S_t(0) + 4 S_t(tau/2) + S_t(tau))
              + (tau h / 6) sum_{t in (tau/2: 4, tau: 1)} w_t (|dt'/dr| E_r(t) + |dt'/dtheta| E_theta(t))
              + u |dt|
with E_x(t) = u sum_j |H_j(t) data_j| + u h (|H_10(t)| S_dx(y0) + |H_11(t)| S_dx(y1)): the unit of the Hermite point the rate is
evaluated at (disk_blocks._herm_abs plus the carry of the end rates' own units through h), and the derivatives of t' by central
difference in longdouble.  The unit bounds ROUNDING, not truncation: the rule is Simpson on a cubic, local error O(h^5)
(test_rule_is_fifth_order keeps that view), and a device that evaluates the same rule is held to this unit whatever h is.

A row is left out where the unit says nothing: a state of the rates, or a step's start or one of its Hermite points, at or
inside 1.001 r_plus, or a non-finite value.  (A step's END may lie inside: a capture step's does, and the rule runs on the
part of it before the cut.)

THE BOUNDS, measured by tests/test_hit_blocks_host.py from rates_T / step_time_T against longdouble and asserted there from
both sides (the ceiling of the worst over every class):
    K_RATE32 = 3, K_RATE64 = 3     t', r', theta' (float32: numpy's float32 sine; float64: numpy's)
    K_DT32   = 2, K_DT64   = 2     dt_step on [0, tau]
A device block is held to twice these (what its form adds: one merged reciprocal for 1 / Sigma and 1 / Delta, fused
multiply-adds, its own sincos).

THE SUM.  A lane adds dt_1 ... dt_n by (sum, e) = TwoSum(t_hi, dt); t_lo = fl(t_lo + e); t_hi = sum, and reads
fl(t_hi + fl(t_lo + part)).  TwoSum is exact: t_hi + dt = sum + e with |e| <= u |sum| <= u A, A = sum |dt_i| (the terms of a
ray are positive: A is the time itself).  So |t_lo| <= i u A (1 + u)^i after i terms, and the only roundings are those of
t_lo + e: each at most u |t_lo + e| <= (i + 1) u^2 A (1 + u)^i -- together below (n^2 / 2 + n) u^2 A (1 + n u).  The read adds
u |t_lo + part| + u |t_hi + (t_lo + part)| <= u (n u A + |part|) (1 + u) + u |total| (1 + u).  With n u < 2^-10:
    |stored - exact| <= u |total| + u |part| + (n^2 / 2 + 3 n) u^2 A        (sum_bound)
against the PLAIN float32 sum's n u A / 2 or so in the mean: at n >= 500 the plain sum misses this bound on most rays, which
is how a test sees a dropped t_lo.
"""
import numpy as np

import disk_blocks as dk
import step_blocks as sb

LD = sb.LD
U32, U64 = sb.U32, sb.U64
N = dk.N
SPINS = dk.SPINS
EXCLUDED_CAP = sb.EXCLUDED_CAP
K_RATE32, K_RATE64 = 3, 3
K_DT32, K_DT64 = 2, 2
MIN_SUM_STEPS = 500


def k_rate(precision):
    return K_RATE32 if precision == 32 else K_RATE64


def k_dt(precision):
    return K_DT32 if precision == 32 else K_DT64


def dtype_of(precision):
    return np.float32 if precision == 32 else np.float64


# ---- the reference's statements in a precision T, and in longdouble --------------------------------------------------------------
def rates_T(M, a, L, r, th, pr, pth, T):
    """disk.time_rates statement by statement, every operation in T (T = longdouble: the yardstick)."""
    r, th, pr, pth, L = (np.asarray(x).astype(T) for x in (r, th, pr, pth, L))
    M, a, two = T(M), T(a), T(2.0)
    s2 = np.sin(th) ** 2
    ra = r * r + a * a
    sigma = ra - a * a * s2
    delta = ra - two * M * r
    p = ra - a * L
    return (ra * p / delta + a * (L - a * s2)) / sigma, delta * pr / sigma, pth / sigma


def _hermite_T(y0, hd0, y1, hd1, t, T):
    t2, t3 = t * t, t * t * t
    return y0 + (T(3.0) * t2 - T(2.0) * t3) * (y1 - y0) + (t3 - T(2.0) * t2 + t) * hd0 + (t3 - t2) * hd1


def step_time_T(M, a, L, y0, y1, h, tau, T):
    """disk.step_time statement by statement in T.  y0, y1 (n,4) (r, theta, p_r, p_theta)."""
    y0, y1 = np.asarray(y0, dtype=np.float64).astype(T), np.asarray(y1, dtype=np.float64).astype(T)
    n = y0.shape[0]
    h, tau, L = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)).astype(T) for x in (h, tau, L))
    t0, r0d, th0d = rates_T(M, a, L, y0[:, 0], y0[:, 1], y0[:, 2], y0[:, 3], T)
    _, r1d, th1d = rates_T(M, a, L, y1[:, 0], y1[:, 1], y1[:, 2], y1[:, 3], T)

    def rate_at(t):
        r = _hermite_T(y0[:, 0], h * r0d, y1[:, 0], h * r1d, t, T)
        th = _hermite_T(y0[:, 1], h * th0d, y1[:, 1], h * th1d, t, T)
        return rates_T(M, a, L, r, th, 0.0, 0.0, T)[0]

    with np.errstate(all="ignore"):
        out = tau * h / T(6.0) * (t0 + T(4.0) * rate_at(T(0.5) * tau) + rate_at(tau))
    return np.where(h == 0, T(0.0), out)


def rates_ld(M, a, L, y):
    """-> (n,3) longdouble t', r', theta' at y (n,4)."""
    y = np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.stack(rates_T(M, a, L, y[:, 0], y[:, 1], y[:, 2], y[:, 3], LD), axis=1)


# ---- units --------------------------------------------------------------------------------------------------------------------------
def _s_t(M, a, L, r, th):
    """S_t (module docstring) at longdouble (r, theta); -> longdouble (n,)."""
    Mq, aq, L = LD(M), LD(a), np.asarray(L, dtype=LD)
    with np.errstate(all="ignore"):
        sn = np.sin(th)
        s2 = sn * sn
        ra = r * r + aq * aq
        sigma = ra - aq * aq * s2
        delta = ra - 2 * Mq * r
        p = ra - aq * L
        kD = (ra + 2 * Mq * r) / delta
        kP = (ra + np.abs(aq * L)) / np.abs(p)
        t = (ra * p / delta + aq * (L - aq * s2)) / sigma
        return (ra * np.abs(p) / delta * (1 + kD + kP) + np.abs(aq * L) + aq * aq * s2) / sigma + \
            4 * aq * aq * np.abs(sn) * (np.abs(t) + 1) / sigma


def _t_rate_ld(M, a, L, r, th):
    return rates_T(M, a, L, r, th, 0.0, 0.0, LD)[0]


def rate_units(M, a, L, y, precision):
    """-> (unit (n,3) float64 for t', r', theta'; keep (n,) bool)."""
    u = dk.u_of(precision)
    y = np.asarray(y, dtype=np.float64)
    st5 = np.stack([y[:, 0], y[:, 1], np.zeros(y.shape[0]), y[:, 2], y[:, 3]], axis=1)
    with dk.mass(M), np.errstate(all="ignore"):
        S = sb.scales(a, st5, L)
        St = _s_t(M, a, L, y[:, 0].astype(LD), y[:, 1].astype(LD)).astype(np.float64)
    unit = u * np.stack([St, S[:, 0], S[:, 1]], axis=1)
    keep = np.isfinite(y).all(axis=1) & (y[:, 0] > 1.001 * dk.r_plus(M, a)) & np.isfinite(unit).all(axis=1)
    return unit, keep


def step_time_ld(M, a, L, y0, y1, h, tau, precision):
    """The rule in longdouble on the steps y0 -> y1 (n,4) and its unit.  -> dict(dt (n,) longdouble, unit (n,) float64, keep (n,))."""
    u = LD(dk.u_of(precision))
    y0, y1 = np.asarray(y0, dtype=np.float64), np.asarray(y1, dtype=np.float64)
    n = y0.shape[0]
    h, tau, L = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in (h, tau, L))
    hq, tq = h.astype(LD), tau.astype(LD)
    st = lambda y: np.stack([y[:, 0], y[:, 1], np.zeros(n), y[:, 2], y[:, 3]], axis=1)
    with dk.mass(M), np.errstate(all="ignore"):
        S0, S1 = np.abs(sb.scales(a, st(y0), L)).astype(LD), np.abs(sb.scales(a, st(y1), L)).astype(LD)
    with np.errstate(all="ignore"):
        d0, d1 = rates_ld(M, a, L, y0), rates_ld(M, a, L, y1)
        data = [(y0[:, i].astype(LD), hq * d0[:, 1 + i], y1[:, i].astype(LD), hq * d1[:, 1 + i]) for i in (0, 1)]
        total, unit = d0[:, 0].copy(), _s_t(M, a, L, *(y0[:, i].astype(LD) for i in (0, 1)))
        unit = u * unit
        r_min = y0[:, 0].astype(LD)
        for t, w in ((tq / 2, 4), (tq, 1)):
            b = dk._basis(t)
            rr, tt = dk._herm(data[0], t), dk._herm(data[1], t)
            r_min = np.minimum(r_min, rr)
            total = total + w * _t_rate_ld(M, a, L, rr, tt)
            e_r = u * dk._herm_abs(data[0], t) + u * hq * (np.abs(b[1]) * S0[:, 0] + np.abs(b[3]) * S1[:, 0])
            e_t = u * dk._herm_abs(data[1], t) + u * hq * (np.abs(b[1]) * S0[:, 1] + np.abs(b[3]) * S1[:, 1])
            dr, dth = LD(1e-6) * np.maximum(np.abs(rr), 1), LD(1e-6)
            ddr = np.abs(_t_rate_ld(M, a, L, rr + dr, tt) - _t_rate_ld(M, a, L, rr - dr, tt)) / (2 * dr)
            ddt = np.abs(_t_rate_ld(M, a, L, rr, tt + dth) - _t_rate_ld(M, a, L, rr, tt - dth)) / (2 * dth)
            unit = unit + w * (u * _s_t(M, a, L, rr, tt) + ddr * e_r + ddt * e_t)
        dt = tq * hq / 6 * total
        unit = np.abs(tq * hq / 6) * unit + u * np.abs(dt)
    dt = np.where(h == 0, LD(0), dt)
    rp = 1.001 * dk.r_plus(M, a)
    keep = np.isfinite(y0).all(axis=1) & np.isfinite(y1).all(axis=1) & (r_min > rp).astype(bool) & np.isfinite(unit.astype(np.float64)) & \
        (h != 0) & (tau != 0)
    return dict(dt=dt, unit=unit.astype(np.float64), keep=keep)


# ---- classes ----------------------------------------------------------------------------------------------------------------------------
RATE_CLASSES = tuple(c for c in sb.RHS_CLASSES if c != "edge") + ("mass",)
_CACHE = {}


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def rate_class(name, spin):
    """-> dict(M, a, y (n,4) (r, theta, p_r, p_theta), L (n,)): float32 values, the same rows for both precisions.  `mass`: the
    `mid` class at M = 2.5 (lengths and L scaled by M, a = spin M)."""
    key = ("rate", name, spin)
    if key not in _CACHE:
        M = 2.5 if name == "mass" else 1.0
        st, L = sb.rhs_class("mid" if name == "mass" else name, abs(spin), N)
        st = st.copy()
        st[:, 0] *= M
        _CACHE[key] = _frozen(dict(M=M, a=float(sb.f32(spin * M)), y=sb.f32(st[:, [0, 1, 3, 4]]), L=sb.f32(L * M)))
    return _CACHE[key]


def rate_classes():
    for spin in SPINS:
        for name in RATE_CLASSES:
            yield spin, name, rate_class(name, spin)


CROSSING_STEP_CLASSES = ("ordinary", "shallow", "inside_isco", "terminal", "mass")
# disk_blocks builds `inside_isco` and `terminal` by carrying a crossing point back by a part of h through the reference's
# right-hand side, which is ZERO at or inside 1.001 r_plus: a point that close to the horizon stays where it is, and the row's
# start lies inside r_cut, where a ray has long ended (r_capture = 1.01 r_plus) and t' has no meaning.  Those rows are counted,
# not hidden: the largest share of a class they may be (disk_blocks' draw has about a fifth and a twentieth), the rest held to the cap.
STARTS_INSIDE = {"crossing/inside_isco": 0.25, "crossing/terminal": 0.10}
TAUS = ("one", "uniform", "tiny", "almost_one")


def taus(n, precision, seed):
    """tau per row: 1, uniform in [0.02, 0.98], 2^-20, 1 - 2^-20 by row index mod 4 (values of the precision)."""
    rng = np.random.default_rng([31, seed])
    k = np.arange(n) % 4
    t = np.where(k == 0, 1.0, np.where(k == 1, rng.uniform(0.02, 0.98, n), np.where(k == 2, 2.0 ** -20, 1.0 - 2.0 ** -20)))
    return dk.as_t(t, precision)


def step_class(source, name, spin, precision):
    """Real steps: -> dict(M, a, y0, y1 (n,4), L, h, tau (n,), ref: step_time_ld of the rows), values of the precision; None where
    the class does not exist at this spin.  source 'crossing': disk_blocks.crossing_class; 'step': step_blocks.step_class with
    the oracle's own RK4 step of the precision."""
    key = ("step", source, name, spin, precision)
    if key in _CACHE:
        return _CACHE[key]
    cols = [0, 1, 3, 4]
    if source == "crossing":
        c = dk.crossing_class(name, spin, precision)
        if c is None:
            return _CACHE.setdefault(key, None)
        M, a, y0, y1, L, h = c["M"], c["a"], c["y0"][:, cols], c["y1"][:, cols], c["L"], c["h"]
    else:
        s = sb.step_class(name, abs(spin), N)  # (drawn for |a|: the class depends on the spin through r_plus alone)
        if s is None:
            return _CACHE.setdefault(key, None)
        st, L, h, _ = s
        M, a = 1.0, spin
        h = np.full(N, float(h))
        y0, y1 = st[:, cols], dk._step(M, a, st, L, h, precision)[:, cols]
        y1 = dk.as_t(y1, precision)
    tau = taus(y0.shape[0], precision, dk.CROSSING_CLASSES.index(name) if source == "crossing" else 50 + sb.STEP_CLASSES.index(name))
    # a step that ends at or inside r_capture ended its ray on its chord there: a hit on it lies before that cut (disk_advance
    # searches [0, t_end]), so its tau is the row's fraction OF the cut -- the rule then runs from an end state that may lie
    # inside the horizon, as the kernels' does
    rcap = 1.01 * dk.r_plus(M, a)
    with np.errstate(all="ignore"):
        cut = np.where(y1[:, 0] <= rcap, np.clip((rcap - y0[:, 0]) / (y1[:, 0] - y0[:, 0]), 0.0, 1.0), 1.0)
        # ... and before the step's cubic in r first reaches r_capture (a hit lies in the annulus, outside that radius; the
        # cubic to an end deep inside the horizon can dip below the chord): on a grid of 1/256
        d0, d1 = rates_ld(M, a, L, y0).astype(np.float64), rates_ld(M, a, L, y1).astype(np.float64)
        grid = np.arange(1, 257) / 256.0
        rr = np.stack([dk._herm((y0[:, 0], h * d0[:, 1], y1[:, 0], h * d1[:, 1]), np.full(y0.shape[0], t)).astype(np.float64) for t in grid], axis=1)
        below = rr <= rcap
        first = np.where(below.any(axis=1), np.argmax(below, axis=1) / 256.0, 1.0)
        # (a row that STARTS at or inside r_capture has no such cut: its tau stays as drawn, and the Hermite points decide)
        cut = np.where((y1[:, 0] <= rcap) & (y0[:, 0] > rcap), np.minimum(cut, first), 1.0)
    tau = dk.as_t(tau * np.where(np.isfinite(cut), cut, 1.0), precision)
    ref = step_time_ld(M, a, L, y0, y1, h, tau, precision)
    return _CACHE.setdefault(key, _frozen(dict(M=M, a=a, y0=np.array(y0), y1=np.array(y1), L=np.array(L), h=np.array(h), tau=tau, ref=_frozen(ref))))


def step_classes(precision):
    for spin in SPINS:
        for source, names in (("crossing", CROSSING_STEP_CLASSES), ("step", sb.STEP_CLASSES)):
            for name in names:
                c = step_class(source, name, spin, precision)
                if c is not None:
                    yield spin, f"{source}/{name}", c


# ---- the two-term sum -------------------------------------------------------------------------------------------------------------------
def two_sum_replay(terms, T, hi=None, lo=None):
    """The lane's statements (DiskTimedStep::advance) on terms (k, n) in T, from (hi, lo) (n,) or zeros: -> (t_hi, t_lo) (n,) T.
    A NaN term is skipped (an iteration the row did not run)."""
    terms = np.asarray(terms, dtype=np.float64)
    n = terms.shape[1]
    hi = np.zeros(n, dtype=T) if hi is None else np.asarray(hi, dtype=np.float64).astype(T)
    lo = np.zeros(n, dtype=T) if lo is None else np.asarray(lo, dtype=np.float64).astype(T)
    for row in terms:
        run = ~np.isnan(row)
        dt = np.where(run, row, 0.0).astype(T)
        s = hi + dt
        bb = s - hi
        lo = np.where(run, lo + ((hi - (s - bb)) + (dt - bb)), lo)
        hi = np.where(run, s, hi)
    return hi, lo


def plain_sum_replay(terms, T):
    terms = np.asarray(terms, dtype=np.float64)
    acc = np.zeros(terms.shape[1], dtype=T)
    for row in terms:
        acc = np.where(np.isnan(row), acc, acc + np.where(np.isnan(row), 0.0, row).astype(T))
    return acc


def sum_bound(terms, part, precision):
    """The bound of the module docstring on fl(t_hi + fl(t_lo + part)) after the non-NaN terms (k, n), in float64."""
    u = dk.u_of(precision)
    terms = np.asarray(terms, dtype=np.float64)
    n = (~np.isnan(terms)).sum(axis=0)
    A = np.nansum(np.abs(terms), axis=0) + np.abs(part)
    total = np.nansum(terms.astype(LD), axis=0) + np.asarray(part, dtype=LD)
    return u * np.abs(total).astype(np.float64) + u * np.abs(part) + (n * n / 2.0 + 3.0 * n) * u * u * A


# ---- the polarization rule where it is hardest (lt_polarization_probe; the rule is disk.polarization) ---------------------------------------
# Per class: M, spin, r_obs (in M; "3rp": 3 r_plus), theta_obs, the hit radii (in units of the ISCO, or of M where given as "M"),
# the field, and what is pinned to zero at the hit.  The existing probe test (tests/test_gpu_polarization.py) draws r from the
# ISCO to 40 at a in {0, 0.9, -0.7}, M = 1, theta_obs in {1, 1.4, pi / 2}: nothing of the below.
POL_FIELD = (0.3, 0.8, 0.5)
POL_CLASSES = {
    "isco_band":  dict(M=1.0, spin=0.998, r_obs=50.0, theta_obs=1.4, r=(1.0, 1.001, "isco")),
    "a998":       dict(M=1.0, spin=0.998, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M")),
    "mass":       dict(M=2.5, spin=0.9, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M")),
    "theta_lo":   dict(M=1.0, spin=0.9, r_obs=50.0, theta_obs=0.05, r=(1.0, 40.0, "M")),
    "theta_hi":   dict(M=1.0, spin=0.9, r_obs=50.0, theta_obs=np.pi - 0.3, r=(1.0, 40.0, "M")),
    "obs_near":   dict(M=1.0, spin=0.9, r_obs="3rp", theta_obs=1.4, r=(1.0, 40.0, "M")),
    "obs_far":    dict(M=1.0, spin=0.9, r_obs=1e4, theta_obs=1.4, r=(1.0, 40.0, "M")),
    "pth0":       dict(M=1.0, spin=0.9, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M"), zero="pth"),
    "pr0":        dict(M=1.0, spin=0.9, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M"), zero="pr"),
    "L0":         dict(M=1.0, spin=0.9, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M"), zero="L"),
    "toroidal":   dict(M=1.0, spin=0.998, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M"), field=(0.0, 1.0, 0.0)),
    "radial":     dict(M=1.0, spin=0.998, r_obs=50.0, theta_obs=1.4, r=(1.0, 40.0, "M"), field=(1.0, 0.0, 0.0)),
}
# Largest |numpy float64 - longdouble| of disk.polarization per class, any component, measured by
# tests/test_hit_blocks_host.py on the CPU (asserted there within a factor 2 either way); the device is held to 4 x.
POL_F64_ERR = {"isco_band": 4.35e-14, "a998": 9.91e-15, "mass": 2.80e-15, "theta_lo": 6.68e-15, "theta_hi": 1.02e-14, "obs_near": 3.03e-15,
               "obs_far": 1.05e-14, "pth0": 8.12e-13, "pr0": 1.52e-15, "L0": 1.92e-15, "toroidal": 8.64e-15, "radial": 5.40e-15}
# (`pth0`: a photon in the plane with the default field's b_z -- records with sin zeta down to 1e-2, where (q, u) lose digits)
POL_PARALLEL_ROWS = 64       # rows of `a998` with the field 1e-3 ... 1e-9 rad from the photon's direction, one call each
POL_S2_SWITCH = 1e-24


def pol_class(name):
    """-> dict(M, a, r_obs, theta_obs, field (b_r, b_phi, b_z), L (n,), hit (n,3), cam (n,2)): null records, computed once."""
    key = ("pol", name)
    if key in _CACHE:
        return _CACHE[key]
    import disk
    c = POL_CLASSES[name]
    M, a = c["M"], c["spin"] * c["M"]
    r_obs = 3.0 * dk.r_plus(M, a) if c["r_obs"] == "3rp" else c["r_obs"] * M
    th = c["theta_obs"]
    rng = np.random.default_rng([41, list(POL_CLASSES).index(name)])
    n = 4 * N
    ri = float(disk.isco(M, a))
    lo, hi = (c["r"][0] * ri, c["r"][1] * ri) if c["r"][2] == "isco" else (ri, c["r"][1] * M)
    r = rng.uniform(lo, hi, n)
    zero = c.get("zero")
    L = np.zeros(n) if zero == "L" else rng.uniform(-5.0, 7.0, n) * M
    pth = np.zeros(n) if zero == "pth" else rng.uniform(-7.0, 7.0, n) * M
    pth_c = rng.uniform(-7.0, 7.0, n) * M

    def p_r2(rr, s, cc, p_theta):
        up = disk._raise_index(M, a, rr, s, cc, (-np.ones(n), np.zeros(n), p_theta, L))
        sigma, delta = rr * rr + a * a * cc * cc, rr * rr - 2 * M * rr + a * a
        return -(-up[0] + p_theta * up[2] + L * up[3]) * sigma / delta

    one, nil = np.ones(n), np.zeros(n)
    if zero == "pr":  # the p_theta at which the null condition leaves p_r = 0: p_r^2 = A - B p_theta^2
        A, B = p_r2(r, one, nil, nil), p_r2(r, one, nil, nil) - p_r2(r, one, nil, one)
        with np.errstate(invalid="ignore"):
            pth = np.where(A > 0, rng.choice([-1.0, 1.0], n) * np.sqrt(A / B), np.nan)
        h2 = np.where(A > 0, 0.0, -1.0)
    else:
        h2 = p_r2(r, one, nil, pth)
    c2 = p_r2(np.full(n, r_obs), np.full(n, np.sin(th)), np.full(n, np.cos(th)), pth_c)
    ok = np.nonzero((h2 >= 0) & (c2 > 0) & ((h2 > 0) | (zero == "pr")))[0][:N]
    assert ok.size == N, (name, ok.size)
    hit = np.stack([r, rng.choice([-1.0, 1.0], n) * np.sqrt(np.maximum(h2, 0.0)), pth], axis=-1)[ok]
    cam = np.stack([-np.sqrt(np.maximum(c2, 0.0)), pth_c], axis=-1)[ok]
    return _CACHE.setdefault(key, _frozen(dict(M=M, a=a, r_obs=r_obs, theta_obs=th, field=c.get("field", POL_FIELD), L=L[ok], hit=hit, cam=cam)))


def pol_field(b):
    import disk
    return disk.BField(b_r=float(b[0]), b_phi=float(b[1]), b_z=float(b[2]))


def pol_reference(c, dtype=np.float64, rows=slice(None), field=None):
    import disk
    with np.errstate(all="ignore"):
        return disk.polarization(c["M"], c["a"], c["r_obs"], c["theta_obs"], c["L"][rows], c["hit"][rows], c["cam"][rows],
                                 pol_field(c["field"] if field is None else field), dtype=dtype)


def photon_direction(c, rows=slice(None)):
    """The received photon's unit direction on the emitter's triad (e_r, e_phi, e_z) in longdouble, and two unit vectors
    that span the plane perpendicular to it -> (k (n,3), p (n,3), q (n,3))."""
    import disk
    hs, L = c["hit"][rows].astype(LD), c["L"][rows].astype(LD)
    er, ept, epp = disk.emitter_frame(LD(c["M"]), LD(c["a"]), hs[:, 0])
    k = np.stack([-er * hs[:, 1], epp * L - ept, hs[:, 2] / hs[:, 0]], axis=1)
    k = k / np.sqrt((k * k).sum(axis=1))[:, None]
    j = np.argmin(np.abs(k), axis=1)  # the axis the direction is farthest from
    e = np.zeros_like(k)
    e[np.arange(k.shape[0]), j] = 1
    p = e - (e * k).sum(axis=1)[:, None] * k
    p = p / np.sqrt((p * p).sum(axis=1))[:, None]
    return k, p, np.cross(k, p)


def tilted_fields(c, rows, delta):
    """One field per row, the photon's direction tilted by the angle delta (n,): -> (b (n,3) float64, s2 (n,) longdouble: sin^2
    zeta of the NORMALISED float64 field against the longdouble direction)."""
    k, p, _ = photon_direction(c, rows)
    b = (k + np.asarray(delta, dtype=LD)[:, None] * p).astype(np.float64)
    bn = b.astype(LD) / np.sqrt((b.astype(LD) ** 2).sum(axis=1))[:, None]
    cr = np.cross(k, bn)
    return b, (cr * cr).sum(axis=1)
