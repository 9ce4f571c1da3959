"""What tests/test_disk_blocks_host.py and tests/test_gpu_disk_blocks.py share: one crossing of the disk's plane on one step
(disk_crossing / disk_advance, lt_disk.hpp) and the closed forms a hit goes through (disk_redshift, wrap_2pi, half_orbits,
disk_emission, disk_shade), each stated in longdouble or mpmath, with the classes of steps, the tables of arguments and the
units an error is stated in.  Built on tests/step_blocks.py (the scales S, the longdouble right-hand side, the mpmath helpers).

STEPS are real: a crossing point on the plane with momenta on the null shell (E = 1: Delta p_r^2 + p_theta^2 = P^2 / Delta -
(L - a)^2, P = r^2 + a^2 - a L) is carried back by a fraction of the class's h, rounded to the precision T of the table, and
y1 is the oracle's own RK4 step of h from there (the float32 oracle's for a float32 table).  Every value a probe is given is a
T, so the device, the oracle and the longdouble statement start from the same numbers.

THE LONGDOUBLE STATEMENT of a crossing (crossing_longdouble): the right-hand side at both ends (step_blocks.
ref_rhs_longdouble), the cubic Hermite polynomial of every component on [0, 1], the root t* of theta(t) = pi/2 on [0, t_end]
by 80 bisections, the components at t*.  pi/2 is the value T has for it (the plane of a float32 trace lies 4.4e-8 off): "on the
plane" is a statement about a T.  It crosses iff theta0 - pi/2 and theta(t_end) - pi/2 differ in sign strictly on the
first side (ltrace.h: landing on the plane from off it counts, leaving it does not); t_end = 1 takes theta1 itself.

UNITS.  u = 2^-24 or 2^-53.  With H_j(t) the four Hermite basis values and (y0, h f0, y1, h f1) the data of component i:
    S_g      = sum_j |H_j(t) data_j| of theta + pi/2 + u-free carry h (|H_10| S_dth(y0) + |H_11| S_dth(y1))
    U_t      = u S_g(t*) / |theta'(t*)| + u t*                                  (the root)
    U_i      = u sum_j |H_j(t*) data_j| + |y_i'(t*)| U_t + u h (|H_10(t*)| S_i(y0) + |H_11(t*)| S_i(y1))   (a hit component)
where S_i is step_blocks.scales: the unit a right-hand side's error is stated in, here carried through h f.
A DECISION is stable where the longdouble crossing radius is farther than 2 K units from r_in and from r_out,
theta(t_end) - pi/2 farther than 2 K u S_g(t_end) from 0, and the cubic has ONE root on [0, t_end].

    g        u g (1 + |Omega xi| / |1 - Omega xi| + (r^1.5 + 3 M sqrt r + 2 |a| sqrt M) / (r^1.5 - 3 M sqrt r + 2 a sqrt M)), mpmath
    wrap     u (|phi| + 2 pi), a distance on the circle, mpmath
    emission u I (ramp_i + 2 s + 0.5 i): the magnitudes the clamped ramp 2 s - 0.5 i is formed from, times I; longdouble from
             the same float32 (r, g)

THE BOUNDS, measured by tests/test_disk_blocks_host.py from the oracle (lto_disk_step, float64 and float32) and from numpy's
float64 disk.redshift / disk.wrap_2pi / the statements of disk.shade against these references alone, rounded up to an
integer and asserted there from both sides:
    K_ROOT64 = 2, K_HIT64 = 4     root and hit state of the float64 oracle
    K_ROOT32 = 2, K_HIT32 = 4     the same of the float32 oracle
    K_G      = 3                  g
    K_WRAP   = 2                  wrap_2pi
    K_EMIT   = 4                  emission
A device block is held to twice these (what its form adds: merged reciprocals, fused multiply-adds, Newton where the oracle
bisects), where it meets the oracle directly to three times, as tests/ray_ends.py.  The device's emission, whose two pow
come from another libm, is held to the count of its own roundings instead (emission_bound).
"""
import numpy as np
import mpmath

import step_blocks as sb

LD = sb.LD
U32, U64 = sb.U32, sb.U64
SPINS = (0.0, 0.5, 0.9, 0.998, -0.7)
MASSES = (1.0, 2.5)
N = 509  # rows per class: no multiple of 64
EXCLUDED_CAP = sb.EXCLUDED_CAP
K_ROOT64, K_HIT64 = 2, 4
K_ROOT32, K_HIT32 = 2, 4
K_G = 3
K_WRAP = 2
K_EMIT = 4


def _ld(x):
    """An mpmath number as the nearest longdouble."""
    hi = float(x)
    return LD(hi) + LD(float(x - mpmath.mpf(hi)))


mpmath.mp.prec = 200
PI_LD = _ld(mpmath.pi)


def k_hit(precision):
    return K_HIT32 if precision == 32 else K_HIT64


def k_root(precision):
    return K_ROOT32 if precision == 32 else K_ROOT64


def u_of(precision):
    return U32 if precision == 32 else U64


def as_t(x, precision):
    """Rounded to the precision of a table, held in float64."""
    return sb.f32(x) if precision == 32 else np.asarray(x, dtype=np.float64)


class mass:
    """step_blocks states its right-hand side and scales for the module's M: a block of rows at another mass runs inside
    `with mass(M):`."""

    def __init__(self, M):
        self.M = float(M)

    def __enter__(self):
        self.keep, sb.M = sb.M, self.M

    def __exit__(self, *exc):
        sb.M = self.keep


def r_plus(M, a):
    return M + np.sqrt(M * M - a * a)


def isco(M, a):
    """The inner edge a disk call resolves r_in <= 0 to: the library's own (host code, no GPU needed).  numpy's cbrt puts
    disk.isco up to 3 ulp beside it."""
    import ltrace
    return float(ltrace.kerr_isco(M, a))


def shell_defect(M, a, y, L):
    """|2 Sigma H| / (P^2 / Delta) of states (n,5): 0 on the null shell.  A traced ray keeps it below 1e-5; a step that
    passed a stage through r_cut (where the reference's right-hand side is zero) leaves it at 1 and far more."""
    y = np.asarray(y, dtype=np.float64)
    r, th, pr, pth = y[:, 0], y[:, 1], y[:, 3], y[:, 4]
    with np.errstate(all="ignore"):
        D, P, s = r * r - 2 * M * r + a * a, r * r + a * a - a * L, np.sin(th)
        return np.abs(D * pr * pr + pth * pth + (L / s - a * s) ** 2 - P * P / D) / (P * P / np.abs(D))


def rule_h(M, a, r, refine=False):
    """The fixed-step tracer's step size at radius r for h_max = 1 (metrics.py:597-611)."""
    rc = 1.01 * r_plus(M, a)
    h = np.full(np.shape(r), 0.5 if refine else 1.0)
    h = np.where(r < 4.0 * rc, np.minimum(h, 0.20 if refine else 0.25), h)
    h = np.where(r < 2.0 * rc, np.minimum(h, 0.08 if refine else 0.10), h)
    return np.where(r < 1.2 * rc, np.minimum(h, 0.03 if refine else 0.05), h)


# ---- Hermite data in longdouble -----------------------------------------------------------------------------------------------
def _basis(t):
    t = np.asarray(t, dtype=LD)
    t2, t3 = t * t, t * t * t
    return 2 * t3 - 3 * t2 + 1, t3 - 2 * t2 + t, -2 * t3 + 3 * t2, t3 - t2  # H00, H10, H01, H11


def _basis_dt(t):
    t = np.asarray(t, dtype=LD)
    t2 = t * t
    return 6 * t2 - 6 * t, 3 * t2 - 4 * t + 1, -6 * t2 + 6 * t, 3 * t2 - 2 * t


def _herm(d, t, basis=_basis):
    """d = (y0, hf0, y1, hf1), each (n,) or (n,5); t (n,)."""
    b = basis(t)
    if d[0].ndim == 2:
        b = [x[:, None] for x in b]
    return b[0] * d[0] + b[1] * d[1] + b[2] * d[2] + b[3] * d[3]


def _herm_abs(d, t):
    b = _basis(t)
    if d[0].ndim == 2:
        b = [x[:, None] for x in b]
    return np.abs(b[0] * d[0]) + np.abs(b[1] * d[1]) + np.abs(b[2] * d[2]) + np.abs(b[3] * d[3])


def crossing_longdouble(M, a, y0, y1, L, h, t_end, r_in, r_out, precision):
    """-> dict(cross, found (n,) bool; t (n,), hit (n,5) longdouble; unit_t (n,), unit (n,5), dth (n,) = |theta'(t*)|, margin (n,) float64: the
    smallest distance of a decision from its threshold in its own unit (inf where none applies))."""
    u = u_of(precision)
    y0 = np.asarray(y0, dtype=np.float64)
    y1 = np.asarray(y1, dtype=np.float64)
    n = y0.shape[0]
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (n,))
    h = np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)).astype(LD)
    t_end = np.broadcast_to(np.asarray(t_end, dtype=np.float64), (n,)).astype(LD)
    with mass(M), np.errstate(all="ignore"):
        f0 = sb.ref_rhs_longdouble(a, y0, L) * h[:, None]
        f1 = sb.ref_rhs_longdouble(a, y1, L) * h[:, None]
        S0 = np.abs(sb.scales(a, y0, L)).astype(LD) * h[:, None]  # (|.|: an end inside the horizon has Delta < 0)
        S1 = np.abs(sb.scales(a, y1, L)).astype(LD) * h[:, None]
    d = (y0.astype(LD), f0, y1.astype(LD), f1)
    th = tuple(x[:, 1] for x in d)

    def carry(t, i=None):
        b = _basis(t)
        if i is None:
            return np.abs(b[1])[:, None] * S0 + np.abs(b[3])[:, None] * S1
        return np.abs(b[1]) * S0[:, i] + np.abs(b[3]) * S1[:, i]

    HALF_PI_LD = LD(as_t(np.pi / 2, precision))  # the plane as T has it: a state is on it when its theta is this value
    with np.errstate(all="ignore"):
        z0 = th[0] - HALF_PI_LD
        z_end = np.where(t_end == 1, th[2] - HALF_PI_LD, _herm(th, t_end) - HALF_PI_LD)
        cross = ((z0 < 0) & (z_end >= 0)) | ((z0 > 0) & (z_end <= 0))
        lo, hi = np.zeros(n, dtype=LD), t_end.copy()
        for _ in range(80):
            mid = (lo + hi) / 2
            gm = _herm(th, mid) - HALF_PI_LD
            same = ((gm < 0) == (z0 < 0)) & (gm != 0)
            lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
        t = (lo + hi) / 2
        hit = _herm(d, t)
        hit[:, 1] = HALF_PI_LD
        dth = np.abs(_herm(th, t, _basis_dt))
        Sg = _herm_abs(th, t) + HALF_PI_LD + carry(t, 1)
        unit_t = u * Sg / dth + u * t
        unit = u * _herm_abs(d, t) + np.abs(_herm(d, t, _basis_dt)) * unit_t[:, None] + u * carry(t)
        found = cross & (hit[:, 0] >= LD(r_in)) & (hit[:, 0] <= LD(r_out))
        Sg_end = _herm_abs(th, t_end) + HALF_PI_LD + carry(t_end, 1)
        m_end = np.where((t_end == 1) | (z0 == 0), np.inf, np.abs(z_end) / (u * Sg_end))
        m_r = np.minimum(np.abs(hit[:, 0] - LD(r_in)), np.abs(hit[:, 0] - LD(r_out))) / unit[:, 0]
        margin = np.where(cross, np.minimum(m_end, m_r), m_end)
    # "the root": the cubic has one on [0, t_end].  Where it has several (theta turns inside the step, within 1e-4 of the plane)
    # bisection and Newton may each find another; such a row is not stable
    c0, c1, c2, c3 = th[0] - HALF_PI_LD, th[1], 3 * (th[2] - th[0]) - 2 * th[1] - th[3], 2 * (th[0] - th[2]) + th[1] + th[3]
    coef = np.stack([c3, c2, c1, c0], axis=1).astype(np.float64)
    te = t_end.astype(np.float64)
    for i in np.nonzero(cross & np.isfinite(coef).all(axis=1))[0]:
        rt = np.roots(coef[i])
        rt = rt[np.abs(rt.imag) <= 1e-7 * (1 + np.abs(rt.real))].real
        if ((rt > -1e-7) & (rt < te[i] + 1e-7)).sum() != 1:
            margin[i] = 0.0
    bad = ~np.isfinite(y0).all(axis=1) | ~np.isfinite(y1).all(axis=1)
    cross, found = cross & ~bad, found & ~bad
    return dict(cross=cross, found=found, t=t, hit=hit, unit_t=unit_t.astype(np.float64), unit=unit.astype(np.float64),
                dth=dth.astype(np.float64),
                margin=np.where(bad, np.inf, margin.astype(np.float64)))


# ---- the classes of steps ---------------------------------------------------------------------------------------------------
CROSSING_CLASSES = ("ordinary", "shallow", "on_plane", "edge_far", "edge_near", "narrow", "inside_isco", "terminal", "still",
                    "nan", "large_L", "mass")
UNSTABLE_CLASSES = ("edge_near",)  # +-1, +-2, +-8 ulp of an edge: exempt from the cap; its stable rows are held like any other's


def _step(M, a, y0, L, h, precision):
    from oracle import oracle
    y1, _ = oracle.rk4_step_kerr(y0, L, h, M, a, f32=precision == 32)
    return y1.astype(np.float64)


def _plane_points(rng, n, M, a, r_lo, r_hi, rho_lo, rho_hi, L_max=None):
    """Crossing points (n,5) at theta = pi/2 on the null shell with |r' / theta'| log-uniform in [rho_lo, rho_hi]; L (n,)."""
    m = 6 * n
    r = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), m))
    L = rng.uniform(-1.0, 1.0, m) * (L_max if L_max is not None else 6.0 * M)
    rho = np.exp(rng.uniform(np.log(rho_lo), np.log(rho_hi), m))
    Delta = r * r - 2 * M * r + a * a
    P = r * r + a * a - a * L
    R = P * P / Delta - (L - a) ** 2
    ok = (R > 1e-3) & (Delta > 0)
    r, L, rho, Delta, R = (x[ok][:n] for x in (r, L, rho, Delta, R))
    assert r.size == n, "too few points on the null shell"
    pr = np.sqrt(R / (Delta + Delta * Delta / (rho * rho))) * rng.choice([-1.0, 1.0], n)
    pth = Delta * np.abs(pr) / rho * rng.choice([-1.0, 1.0], n)
    st = np.stack([r, np.full(n, np.pi / 2), rng.uniform(-6.0, 6.0, n), pr, pth], axis=1)
    return st, L


def _steps_through(rng, M, a, pts, L, h, precision, tau=None):
    """The step of length h that passes through each point at the fraction tau: y0 (T), y1 (T)."""
    n = pts.shape[0]
    tau = rng.uniform(0.05, 0.95, n) if tau is None else tau
    y0 = as_t(_step(M, a, pts, L, -tau * h, 64), precision)
    return y0, as_t(_step(M, a, y0, L, h, precision), precision)


def _edge_rows(rng, M, a, precision, ulps, r_out):
    """Steps whose longdouble crossing radius lies `ulps` ulp (of T) from r_in (first half) or r_out: the start is moved along
    r until it does (three secant passes on the longdouble statement)."""
    r_in = float(as_t(isco(M, a), precision))
    n = N
    edge = np.where(np.arange(n) < n // 2, r_in, float(as_t(r_out, precision)))
    off = np.resize(np.asarray(ulps, dtype=np.float64), n) * np.where((np.arange(n) // 2) % 2 == 0, 1.0, -1.0)
    sp = np.spacing(edge.astype(np.float32)).astype(np.float64) if precision == 32 else np.spacing(edge)
    want = edge + off * sp
    # steep crossings (|r' / theta'| in [0.1, 0.6]: a shallow crossing's radius has a unit of tens of ulp) on the null shell
    L = rng.uniform(-4.0, 4.0, n) * M
    Delta = want * want - 2 * M * want + a * a
    shell = lambda L: (want * want + a * a - a * L) ** 2 / Delta - (L - a) ** 2
    L = np.where(shell(L) > 1e-3, L, 0.0)
    rho = np.exp(rng.uniform(np.log(0.1), np.log(0.6), n))
    pr = np.sqrt(shell(L) / (Delta + Delta * Delta / (rho * rho))) * rng.choice([-1.0, 1.0], n)
    pth = Delta * np.abs(pr) / rho * rng.choice([-1.0, 1.0], n)
    pts = np.stack([want, np.full(n, np.pi / 2), rng.uniform(-6.0, 6.0, n), pr, pth], axis=1)
    h = rule_h(M, a, want)
    tau = rng.uniform(0.2, 0.8, n)
    y0 = as_t(_step(M, a, pts, L, -tau * h, 64), precision)
    L = as_t(L, precision)
    for _ in range(4):
        y1 = as_t(_step(M, a, y0, L, h, precision), precision)
        ref = crossing_longdouble(M, a, y0, y1, L, h, 1.0, 0.0, 1e9, precision)
        y0[:, 0] = as_t(y0[:, 0] + (want - ref["hit"][:, 0].astype(np.float64)), precision)
    y1 = as_t(_step(M, a, y0, L, h, precision), precision)
    return y0, y1, L, h


_CLASSES = {}


def crossing_class(name, a, precision):
    """-> dict(M, a, y0, y1 (n,5), L, h, t_end (n,), terminal (n,) int, r_in (0: the ISCO), r_out, ref: crossing_longdouble of
    the rows, keep (n,): the decision is stable) -- every number a T; computed once and not changed afterwards.  None where the
    class does not exist at this spin."""
    key = (name, a, precision)
    if key in _CLASSES:
        return _CLASSES[key]
    rng = np.random.default_rng([7, CROSSING_CLASSES.index(name), int(round(abs(a) * 1000)), int(a < 0), precision])
    M, r_in_arg, r_out = 1.0, 0.0, 20.0
    n = N
    t_end, terminal = np.ones(n), np.zeros(n, dtype=np.int32)
    if name == "mass":
        if a != 0.9:
            return _CLASSES.setdefault(key, None)
        M, r_out = 2.5, 45.0
    aa = a * M
    ri = isco(M, aa)
    if name in ("ordinary", "mass", "shallow", "large_L"):
        rho = (5.0, 100.0) if name == "shallow" else (0.05, 5.0)
        # (the annulus and a margin on either side: crossings inside the ISCO and beyond r_out are rows too)
        pts, L = _plane_points(rng, n, M, aa, max(0.8 * ri, 1.03 * r_plus(M, aa) * 1.2), 1.3 * r_out, *rho,
                               L_max=None if name != "large_L" else 40.0 * M)
        if name == "large_L":  # the largest |L| that still reaches the annulus: the turning point inside r_out
            pts, L = _plane_points(rng, n, M, aa, ri, r_out, 0.05, 100.0, L_max=1.2 * r_out)
        L = as_t(L, precision)
        h = rule_h(M, aa, pts[:, 0])
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision)
    elif name == "on_plane":
        pts, L = _plane_points(rng, n, M, aa, ri, r_out, 0.05, 5.0)
        L = as_t(L, precision)
        h = rule_h(M, aa, pts[:, 0])
        # the crossing point is the step's start (even rows) or its end (odd rows) ...
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision, tau=(np.arange(n) % 2).astype(np.float64))
        # ... and that theta is set to pi/2 as T has it, and to its neighbours: thirds (start), thirds (end)
        hp = np.float32(np.pi / 2) if precision == 32 else np.float64(np.pi / 2)
        vals = np.array([np.nextafter(hp, hp.__class__(0)), hp, np.nextafter(hp, hp.__class__(4))], dtype=np.float64)
        k = np.arange(n)
        start = k % 2 == 0
        y0[start, 1] = vals[(k[start] // 2) % 3]
        y1[~start, 1] = vals[(k[~start] // 2) % 3]
    elif name in ("edge_far", "edge_near"):
        y0, y1, L, h = _edge_rows(rng, M, aa, precision, (64,) if name == "edge_far" else (1, 2, 8), r_out)
    elif name == "narrow":
        # r_out - r_in = 0.05, wholly inside one step whose two ends lie outside it
        r_in_arg, r_out = 9.0, 9.05
        pts, L = _plane_points(rng, n, M, aa, 8.9, 9.15, 0.5, 60.0)
        h = np.full(n, 1.0)
        tau = rng.uniform(0.3, 0.7, n)
        # ... and 64 rows that turn in r inside it: p_r = 0 on the plane just below r_out, the crossing at mid-step, so that
        # BOTH ends lie above r_out and only the cubic dips into the annulus (what the pre-filter's pad is for)
        k = np.arange(64)
        pts[k, 0] = rng.uniform(9.0485, 9.0498, 64)
        Dk = pts[k, 0] ** 2 - 2 * M * pts[k, 0] + aa * aa
        L[k] = np.where(rng.random(64) < 0.5, -1.0, 1.0) * rng.uniform(1.0, 4.0, 64)
        pts[k, 3] = 0.0
        pts[k, 4] = np.sign(pts[k, 4]) * np.sqrt((pts[k, 0] ** 2 + aa * aa - aa * L[k]) ** 2 / Dk - (L[k] - aa) ** 2)
        tau[k] = 0.5
        L = as_t(L, precision)
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision, tau=tau)
    elif name == "inside_isco":
        if a != 0.998:
            return _CLASSES.setdefault(key, None)
        pts, L = _plane_points(rng, n, M, aa, 1.01 * r_plus(M, aa) * 1.01, 1.05 * ri, 0.05, 20.0, L_max=2.5)
        L = as_t(L, precision)
        h = np.full(n, 0.1)
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision)
    elif name == "terminal":
        # capture chords (a = 0.998: the annulus reaches down to 1.15 r_capture) and escape chords (r_escape = 2 r_obs with
        # r_obs = 12; they cross the plane, never the annulus), the plane crossed before the cut, after it and within rounding of it
        if a != 0.998:
            return _CLASSES.setdefault(key, None)
        m = n // 2
        rcap, resc = 1.01 * r_plus(M, aa), 2.0 * TERMINAL_R_OBS
        m1 = m // 2
        p1, L1 = _plane_points(rng, m1, M, aa, 1.003 * 1.001 * r_plus(M, aa), 1.2 * rcap, 3.0, 200.0, L_max=4.0)
        # ... and the capture steps that do cross the ANNULUS: retrograde rays falling radially through the ISCO cover the
        # 0.16 between it and r_capture within one h = 0.1 (lt_disk.hpp: "rare, not absent")
        pc, Lc = _plane_points(rng, 8 * (m - m1), M, aa, ri, 1.03 * ri, 10.0, 200.0, L_max=4.0)
        fast = np.nonzero(Lc < -1.5)[0][:m - m1]
        assert fast.size == m - m1
        p1, L1 = np.concatenate([p1, pc[fast]]), np.concatenate([L1, Lc[fast]])
        p1[:, 3] = -np.abs(p1[:, 3])
        p2, L2 = _plane_points(rng, n - m, M, aa, 0.97 * resc, 1.025 * resc, 3.0, 200.0)
        p2[:, 3] = np.abs(p2[:, 3])
        pts, L = np.concatenate([p1, p2]), as_t(np.concatenate([L1, L2]), precision)
        h = np.where(np.arange(n) < m, 0.1, 1.0)
        r_out = 11.5  # (a disk call requires r_out < r_obs: no annulus reaches the escape radius 2 r_obs)
        tau = rng.uniform(0.05, 0.95, n)
        tau[m1:m] = rng.uniform(0.02, 0.3, m - m1)
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision, tau=tau)
        target = np.where(np.arange(n) < m, as_t(rcap, precision), as_t(resc, precision))
        denom = y1[:, 0] - y0[:, 0]
        with np.errstate(all="ignore"):
            frac = as_t(np.clip(as_t((target - y0[:, 0]), precision) / denom, 0.0, 1.0), precision)
        ends = (np.where(np.arange(n) < m, y1[:, 0] <= target, y1[:, 0] >= target)) & \
               (np.where(np.arange(n) < m, y0[:, 0] > target, y0[:, 0] < target))
        terminal = np.where(ends, np.where(np.arange(n) < m, -1, 1), 0).astype(np.int32)
        t_end = np.where(ends, frac, 1.0)
        # every 45th terminal row: the cut moved onto the root itself, and one T-ulp to either side
        ref = crossing_longdouble(M, aa, y0, y1, L, h, 1.0, 0.0, 1e9, precision)
        k = np.nonzero(ends)[0][::45]
        sp = np.spacing(ref["t"][k].astype(np.float32)).astype(np.float64) if precision == 32 else np.spacing(ref["t"][k].astype(np.float64))
        t_end[k] = as_t(ref["t"][k].astype(np.float64) + sp * np.resize([-1.0, 0.0, 1.0], k.size), precision)
    elif name == "still":
        pts, L = _plane_points(rng, n, M, aa, ri, r_out, 0.05, 5.0)
        L = as_t(L, precision)
        h = rule_h(M, aa, pts[:, 0])
        y0, _ = _steps_through(rng, M, aa, pts, L, h, precision)
        y0[::3, 1] = as_t(np.pi / 2, precision)  # (a third of them ON the plane)
        y1 = y0.copy()
    elif name == "nan":
        pts, L = _plane_points(rng, n, M, aa, ri, r_out, 0.05, 5.0)
        L = as_t(L, precision)
        h = rule_h(M, aa, pts[:, 0])
        y0, y1 = _steps_through(rng, M, aa, pts, L, h, precision)
        k = np.arange(n)
        y0[k[k % 2 == 0], (k[k % 2 == 0] // 2) % 5] = np.nan
        y1[k[k % 2 == 1], (k[k % 2 == 1] // 2) % 5] = np.nan
    else:
        raise KeyError(name)
    h = as_t(h, precision)
    t_end = as_t(t_end, precision)
    r_in = float(as_t(ri if r_in_arg <= 0 else r_in_arg, precision))
    r_out_t = float(as_t(r_out, precision))
    ref = crossing_longdouble(M, aa, y0, y1, L, h, t_end, r_in, r_out_t, precision)
    k_dec = 2 * k_hit(precision)
    keep = ref["margin"] > k_dec
    c = dict(M=M, a=aa, y0=y0, y1=y1, L=L, h=h, t_end=t_end, terminal=terminal, r_in_arg=r_in_arg, r_in=r_in, r_out=r_out,
             r_out_t=r_out_t, ref=ref, keep=keep, r_obs=TERMINAL_R_OBS if name == "terminal" else 50.0)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _CLASSES.setdefault(key, c)


TERMINAL_R_OBS = 12.0


# ---- the closed forms: tables and references -----------------------------------------------------------------------------------
_G = {}


def g_table():
    """-> list of dict(M, a, r (n,), xi (n,), g (n,) mpmath truth as float64, unit (n,)) per (M, spin): r from the ISCO to 1000,
    xi over [-8 M, 8 M] where 1 - Omega xi >= 0.01."""
    if "t" in _G:
        return _G["t"]
    out = []
    mp = mpmath.mp
    for M in MASSES:
        for s in SPINS:
            a = s * M
            ri = isco(M, a)
            r1 = np.concatenate([[ri, np.nextafter(ri, np.inf), ri * (1 + 1e-9), ri * (1 + 1e-6)], np.exp(np.linspace(np.log(ri * 1.001), np.log(1000.0), 36))])
            xi1 = M * np.array([-8.0, -5.5, -3.0, -1.0, -0.25, 0.0, 1e-9, 0.5, 2.0, 3.7, 5.0, 6.5, 8.0])
            r, xi = (x.ravel() for x in np.meshgrid(r1, xi1, indexing="ij"))
            g, unit, ok = np.empty(r.size), np.empty(r.size), np.zeros(r.size, dtype=bool)
            for i in range(r.size):
                rr, x, Mq, aq = mp.mpf(float(r[i])), mp.mpf(float(xi[i])), mp.mpf(M), mp.mpf(a)
                sM, sr = mp.sqrt(Mq), mp.sqrt(rr)
                r15 = rr * sr
                om = sM / (r15 + aq * sM)
                rad = r15 - 3 * Mq * sr + 2 * aq * sM
                ut = (r15 + aq * sM) / (mp.sqrt(r15) * mp.sqrt(rad))
                den = 1 - om * x
                ok[i] = den >= mp.mpf("0.01")
                gg = 1 / (ut * den)
                g[i] = float(gg)
                unit[i] = float(U64 * gg * (1 + abs(om * x) / abs(den) + (r15 + 3 * Mq * sr + 2 * abs(aq) * sM) / rad))
            out.append(dict(M=M, a=a, r=r[ok], xi=xi[ok], g=g[ok], unit=unit[ok]))
    _G["t"] = out
    return out


def phi_table():
    """-> dict(phi (n,), wrapped (n,) mpmath truth as float64 (of phi mod 2 pi in [0, 2 pi)), unit (n,), half (n,) int64 the
    exact floor(|phi| / pi), near (n,) bool: |phi| / pi lies within the unit of an integer)."""
    if "p" in _G:
        return _G["p"]
    rng = np.random.default_rng(11)
    k = np.arange(-2000, 2001, dtype=np.float64)
    base = np.concatenate([k * (2 * np.pi), k * np.pi])
    phi = np.concatenate([[1e-17, -1e-17, 0.0, -0.0, 1e4, -1e4], base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf),
                          rng.uniform(-1e4, 1e4, 3000), rng.uniform(-30.0, 30.0, 2000)])
    mp = mpmath.mp
    wrapped, half, near = np.empty(phi.size), np.empty(phi.size, dtype=np.int64), np.zeros(phi.size, dtype=bool)
    unit = U64 * (np.abs(phi) + 2 * np.pi)
    two_pi = 2 * mp.pi
    for i, v in enumerate(phi):
        x = mp.mpf(float(v))
        w = x - two_pi * mp.floor(x / two_pi)
        wrapped[i] = float(w)
        q = abs(x) / mp.pi
        half[i] = int(mp.floor(q))
        near[i] = abs(q - mp.nint(q)) * mp.pi <= mp.mpf(float(unit[i]))
    _G["p"] = dict(phi=phi, wrapped=wrapped, unit=unit, half=half, near=near)
    return _G["p"]


def circle_distance(got, want):
    d = np.abs(np.asarray(got, dtype=np.float64) - want)
    return np.minimum(d, np.abs(2 * np.pi - d))


SHADE_CASES = tuple((q, e) for q in (0.0, 3.0, 2.5) for e in (1.0, 2.5, 0.3))


def shade_table(M, a, q, exposure):
    """-> dict(r, g (n,) float32 values as float64, r_in) for one launch: s = g (r_in / r)^(3/4) at and beside every knee of
    the ramp (s = 0, 1/4, 1/2, 3/4, 1), I at and beside 1, and ordinary points."""
    rng = np.random.default_rng([13, int(q * 10), int(exposure * 10), int(round(abs(a) * 1000)), int(M * 10)])
    ri = isco(M, a)
    r = sb.f32(np.exp(rng.uniform(np.log(ri), np.log(60.0 * M), 60)))
    x = ri / r
    rows_r, rows_g = [], []
    offs = np.array([-2, -1, 0, 1, 2])
    for s in (0.0, 0.25, 0.5, 0.75, 1.0):
        g0 = np.asarray(s / x ** 0.75, dtype=np.float32)
        for o in offs:
            gg = g0.copy()
            for _ in range(abs(int(o))):
                gg = np.nextafter(gg, np.float32(np.inf if o > 0 else -np.inf))
            rows_r.append(r)
            rows_g.append(np.maximum(gg, 0).astype(np.float64))
    g1 = np.asarray((1.0 / (exposure * x ** q)) ** 0.25, dtype=np.float32)  # I = 1
    for o in offs:
        gg = g1.copy()
        for _ in range(abs(int(o))):
            gg = np.nextafter(gg, np.float32(np.inf if o > 0 else -np.inf))
        rows_r.append(r)
        rows_g.append(gg.astype(np.float64))
    rows_r.append(sb.f32(np.exp(rng.uniform(np.log(ri), np.log(60.0 * M), 300))))
    rows_g.append(sb.f32(rng.uniform(0.02, 1.9, 300)))
    return dict(r=np.concatenate(rows_r), g=np.concatenate(rows_g), r_in=ri)


def emission_longdouble(r32, g32, r_in, q, exposure):
    """-> (E (n,3) longdouble, unit (n,3) float64 in u = 2^-53) from float32 (r, g) given as float64."""
    r, g = np.asarray(r32, dtype=np.float64).astype(LD), np.asarray(g32, dtype=np.float64).astype(LD)
    x = LD(r_in) / r
    I = LD(exposure) * g ** 4 * x ** LD(q)
    s = g * x ** LD(0.75)
    i = np.arange(3).astype(LD)[None, :]
    lin = 2 * s[:, None] - LD(0.5) * i
    ramp = np.clip(lin, 0, 1)
    terms = 2 * s[:, None] + LD(0.5) * i
    unit = U64 * (I[:, None] * (ramp + terms)).astype(np.float64)
    # (a ramp more than 64 roundings of its terms below its lower knee is 0 whatever the arithmetic: the clamp is exact)
    unit = np.where((lin < -64 * U64 * terms).astype(bool), 0.0, unit)
    return I[:, None] * ramp, unit


def emission_bound(q):
    """The device's emission in units, from its statements (lt_disk.hpp) with every operation within u of its result and
    pow within 2 ulp = 4 u: x = r_in / r carries u, so x^q carries q u and x^0.75 0.75 u;
        I = exposure (g^2 g^2) pow(x, q):  (q + 4 + 2 + 1 + 1 + 1) u = (q + 9) u;   s = g pow(x, 0.75):  (0.75 + 4 + 1) u = 5.75 u;
        E_i = I clamp(2 s - 0.5 i):  |dE| <= (q + 9) u E + I (5.75 u 2 s + u |2 s - 0.5 i|) + u E <= (q + 11) u I (ramp + 2 s + 0.5 i)."""
    return abs(q) + 11.0


def emission_numpy(r32, g32, r_in, q, exposure):
    """The statements of disk.shade (light-path-tracer_amd/disk.py) up to the unclamped emission, float64."""
    r, g = np.asarray(r32, dtype=np.float64), np.asarray(g32, dtype=np.float64)
    x = r_in / r
    intensity = exposure * g ** 4 * x ** q
    s = g * x ** 0.75
    ramp = np.stack([np.clip(2.0 * s - 0.5 * i, 0.0, 1.0) for i in range(3)], axis=-1)
    return intensity[..., None] * ramp


def shade_expected(E, bound):
    """The colour of an emission E (n,3) longdouble known to `bound` (n,3): -> (rgb (n,3) float32, sure3 (n,3) bool, mean (n,)
    float32, sure1 (n,) bool).  A value is sure where E - bound and E + bound round to the same float32."""
    c, lo, hi = (np.clip(v, 0, 1) for v in (E, E - bound, E + bound))
    f = lambda v: v.astype(np.float64).astype(np.float32)
    rgb, sure3 = f(c), f(lo) == f(hi)
    m, b1 = c.sum(axis=1) / 3, (np.minimum(hi - lo, 2 * bound)).sum(axis=1) / 6 + 4 * U64 * c.sum(axis=1) / 3
    return rgb, sure3, f(m), f(np.clip(m - b1, 0, 1)) == f(np.clip(m + b1, 0, 1))


def g_unit(M, a, r, xi):
    """The unit of g (module docstring) in float64, for arguments that are in no table."""
    r, xi = np.asarray(r, dtype=np.float64), np.asarray(xi, dtype=np.float64)
    sM, sr = np.sqrt(M), np.sqrt(r)
    r15 = r * sr
    om = sM / (r15 + a * sM)
    rad = r15 - 3.0 * M * sr + 2.0 * a * sM
    g = np.sqrt(r15) * np.sqrt(rad) / ((r15 + a * sM) * (1.0 - om * xi))
    return U64 * np.abs(g) * (1.0 + np.abs(om * xi) / np.abs(1.0 - om * xi) + (r15 + 3.0 * M * sr + 2.0 * np.abs(a) * sM) / rad)


# ---- one iteration of an integrator with the disk test behind it, by the oracle --------------------------------------------------
ADVANCE_CLASSES = ("ordinary", "shallow", "narrow", "inside_isco", "terminal", "large_L", "mass")
LAMBDA_MAX = 5000.0


def accepted_dp45_h(c):
    """The step size the oracle's DP45 controller settles on from the class's h at each y0: its own reject factors applied until
    it accepts or the attempt ends the ray (as dp45_blocks.accepted_h)."""
    from oracle import oracle
    h = np.array(c["h"], dtype=np.float64)
    for _ in range(200):
        o = oracle.dp45_attempt(c["y0"], c["L"], h, c["M"], c["a"], r_obs=c["r_obs"], lambda_max=LAMBDA_MAX)
        go = (o["decision"] != 2) & (o["event"] == 4) & np.isfinite(o["h_next"]) & (o["h_next"] > 0)
        if not go.any():
            break
        h = np.where(go, o["h_next"], h)
    return h


DP45_CAPTURE_SPIN = 1.0


def dp45_capture_class():
    """Capture steps of DP45 that cross the ANNULUS.  Between r_capture and the ISCO the controller accepts h of 1e-3 ... 2e-2
    (a = 0.998: median 0.02, against the 0.16 between the two radii), so no accepted DP45 step of the spins above both ends a
    ray and is a candidate of the disk test.  At a = M the ISCO is the horizon and r_capture = 1.01 r_plus lies INSIDE the
    annulus: every capture step that crosses the plane before its cut is a hit.  Rows: points on the plane within 0.003 of
    r_capture, falling, carried back up to 0.003; of 16 N such starts the first N whose accepted attempt the oracle ends by
    capture.  float64 (DP45 has no float32 form).  -> the dict of crossing_class, h the accepted step size."""
    key = ("dp45_capture", DP45_CAPTURE_SPIN, 64)
    if key in _CLASSES:
        return _CLASSES[key]
    from oracle import oracle
    M, a, n = 1.0, DP45_CAPTURE_SPIN, 16 * N
    rng = np.random.default_rng([7, 99])
    rcap = 1.01 * r_plus(M, a)
    pts, L = _plane_points(rng, n, M, a, rcap - 0.003, rcap + 0.004, 10.0, 200.0, L_max=4.0)
    pts[:, 3] = -np.abs(pts[:, 3])
    y0 = _step(M, a, pts, L, -rng.uniform(0.05, 0.95, n) * 0.003, 64)
    c = dict(M=M, a=a, y0=y0, L=L, h=np.full(n, 0.01), r_obs=TERMINAL_R_OBS)
    h = accepted_dp45_h(c)
    o = oracle.dp45_attempt(y0, L, h, M, a, r_obs=TERMINAL_R_OBS, lambda_max=LAMBDA_MAX)
    k = np.nonzero((o["decision"] == 2) & (o["event"] == -1) & (y0[:, 0] > 1.002 * 1.001 * r_plus(M, a)))[0][:N]
    assert k.size == N, k.size
    ri = isco(M, a)
    c = dict(M=M, a=a, y0=y0[k], y1=o["next"][k], L=L[k], h=h[k], t_end=np.ones(N), terminal=np.full(N, -1, dtype=np.int32), r_in_arg=0.0,
             r_in=ri, r_out=11.5, r_out_t=11.5, r_obs=TERMINAL_R_OBS)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return _CLASSES.setdefault(key, c)


def advance_oracle(c, precision, dp45=False):
    """What the twin does with one iteration from each y0 of a class: the integrator's iteration (oracle.rk4_iteration, or one
    DP45 attempt of the step size the oracle's controller settles on from the class's h), then lto_disk_step on the step it took.  -> dict(event (n,) the integrator's, moved (n,)
    bool: a step was accepted, h (n,), y1 (n,5) the full step's end, terminal, frac, step: oracle.disk_step's dict, ref:
    crossing_longdouble of that step with the twin's path rule, unit_step (n,5): step_blocks' unit of the step, stable (n,))."""
    from oracle import oracle
    M, a, y0, L = c["M"], c["a"], c["y0"], c["L"]
    f32 = precision == 32
    n = y0.shape[0]
    rcap, resc = 1.01 * r_plus(M, a), 2.0 * c["r_obs"]
    if dp45:
        h = accepted_dp45_h(c)
        o = oracle.dp45_attempt(y0, L, h, M, a, r_obs=c["r_obs"], lambda_max=LAMBDA_MAX)
        event, moved = o["event"], o["decision"] == 2
        y1 = o["next"]
    else:
        o = oracle.rk4_iteration(y0, L, 0.0, M, a, r_obs=c["r_obs"], lambda_max=LAMBDA_MAX, h_max=1.0, f32=f32)
        event, h, moved = o["event"], o["h"].astype(np.float64), (o["attempts"] == 1) & np.isin(o["event"], (4, -1, 1))
        y1 = oracle.rk4_step_kerr(y0, L, h, M, a, f32=f32)[0].astype(np.float64)
    terminal = np.where(event == -1, -1, np.where(event == 1, 1, 0)).astype(np.int32)
    t = np.float32 if f32 else np.float64
    with np.errstate(all="ignore"):
        target = np.where(terminal < 0, t(t(r_plus(M, a)) * t(1.01)) if f32 else rcap, t(resc))
        denom = (y1[:, 0].astype(t) - y0[:, 0].astype(t))
        frac = np.where(denom == 0, 1.0, np.clip((target.astype(t) - y0[:, 0].astype(t)) / denom, 0, 1)).astype(np.float64)
    frac = np.where(terminal == 0, 1.0, frac)
    st = oracle.disk_step(y0, y1, L, h, M, a, c["r_in"], c["r_out_t"], terminal=terminal, frac=frac, is_dp45=dp45, r_obs=c["r_obs"], f32=f32)
    # (a terminal DP45 step: the twin retook the step by RK4 and cut it again; those are the values the root was searched with)
    y1u = np.where(st["cross"][:, None] & (terminal != 0)[:, None] & dp45, st["y1"], y1)
    fru = np.where(st["cross"] & (terminal != 0) & dp45, st["frac"], frac)
    ref = crossing_longdouble(M, a, y0, y1u, L, h, fru, c["r_in"], c["r_out_t"], precision)
    with mass(M):
        step = (lambda s_, L_, h_: oracle.rk4_step_kerr(s_, L_, h_, M, a)) if not dp45 else \
               (lambda s_, L_, h_: (oracle.dp45_attempt(s_, L_, h_, M, a, r_obs=c["r_obs"], lambda_max=LAMBDA_MAX)["next"], np.asarray(s_)[:, :1]))
        _, unit_step, _, _ = sb._step_parts(a, y0, L, h, step, u_of(precision))
    hp = LD(as_t(np.pi / 2, precision))
    with np.errstate(all="ignore"):
        chord = y0[:, 1].astype(LD) + fru.astype(LD) * (y1u[:, 1] - y0[:, 1]).astype(LD) - hp
        z1 = np.where(terminal == 0, y1[:, 1].astype(LD) - hp, chord)
        # the device's own step may differ from the oracle's by 2 K_STEP of the step's unit: a decision is stable where
        # the plane and both edges are clear of that as well
        slack = 2 * sb.K_STEP * unit_step
        clear = (np.abs(z1).astype(np.float64) > 2 * slack[:, 1]) & (np.abs(y0[:, 1] - float(hp)) > 0)
        edge = np.minimum(np.abs(ref["hit"][:, 0].astype(np.float64) - c["r_in"]), np.abs(ref["hit"][:, 0].astype(np.float64) - c["r_out_t"]))
        with np.errstate(divide="ignore"):
            speed = np.abs(y1u[:, 0] - y0[:, 0]) / np.maximum(ref["dth"], 1e-300)  # |dr / dtheta| along the step, roughly
        clear &= ~ref["cross"] | (edge > 2 * (2 * k_hit(precision) * ref["unit"][:, 0] + slack[:, 0] + speed * slack[:, 1]))
        # (an RK4 iteration that retried counts several attempts of the device's loop: not one call of the probe)
        clear &= (ref["margin"] > 2 * k_hit(precision)) & moved & np.isfinite(y1).all(axis=1)
    return dict(event=event, moved=moved, h=h, y1=y1, terminal=terminal, frac=frac, step=st, ref=ref, unit_step=unit_step, stable=clear)
