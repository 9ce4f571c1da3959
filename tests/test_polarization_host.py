"""CPU tests of the polarization rule's numpy statement (disk.polarization, disk.stokes_frame, disk.stokes_lightcurve), the
references tests/test_gpu_polarization.py holds the kernels to.

Truth is independent of the rule and of the Walker-Penrose constant: for every annulus crossing of the dense tracks of
tests/test_hit_time_rule.py (a in {0, 0.9, -0.7}, r_obs = 50, theta_obs = 1.4) the received photon is started at the hit
with k = (-1, -p_r, -p_theta, L) and the electric vector f of the emitter's frame, and the geodesic equation together with
D f / d lambda = 0 is integrated to the camera with scipy's DOP853 (Christoffel symbols from the analytic derivatives of
the Boyer-Lindquist metric; all hits of a spin in one vectorised system, each on its own affine length, the hit's lambda
along the backward ray).  At the camera f is projected on the static observer's tetrad and on the screen basis.  The
crossing itself is refined on the dense track by integrating the oracle's right-hand side from the track point before it.

MEASURED here (56 rays per spin; field (0.3, 0.8, 0.5); 27 / 37 / 22 hits at a = 0 / 0.9 / -0.7, 6 / 9 / 4 of them behind
a plane crossing or in a second slot, none with sin zeta < 0.05):
    change of the truth's (q, u) when rtol goes from 1e-11 to 5e-12: at most 1.5e-12 / 2.1e-12 / 1.5e-12;
        the bound on |dq|, |du| is 10 x the largest of the three, TRUTH_BOUND = 2.1e-11;
    the forward photon at the camera: r, theta, (k_r, k_theta), E and L within 1.3e-10 / 5.4e-9 / 6.6e-11 of r_obs, theta_obs
        and (-p_r, -p_theta), 1, L of the camera's record -- the tracks' own tolerance (rtol 1e-11, amplified behind a plane
        crossing); asserted at 1e-8;
    disk.polarization against the truth, on the truth's own ends (the arrival point and momenta of the forward photon):
        largest |dq|, |du| 3.3e-12 / 3.8e-12 / 1.8e-12, bound TRUTH_BOUND;
    on the camera's record, which differs from the truth's end by the offsets above: 2.0e-12 / 9.9e-11 / 2.1e-12, each within
        TRUTH_BOUND + sum_i |d(q, u)/dx_i| |offset_i| (the closed form's own sensitivity to the camera end, by central
        differences; 1.2e-10 where the 9.9e-11 is);
    kappa at the camera end against kappa at the hit, relative to |kappa|: 2.0e-11 / 1.2e-10 / 8.1e-12; kappa's own change on
        halving the tolerance is 9.8e-12 / 5.8e-11 / 2.6e-12 (it carries |f| and a factor r_obs, which (q, u) do not), so its
        bound by the same rule is KAPPA_BOUND = 5.9e-10.
The hit is put back on the null shell (p_r from H = 0) before it is transported: the dense track drifts off it by its
tolerance, kappa is conserved along null rays only, and without that step the comparison shows a systematic 3e-12 ... 2e-11.
"""
import numpy as np
import pytest

import disk as diskmod
import ltrace
from oracle import oracle
from test_hit_time_rule import M, R_OBS, SPINS, THETA_OBS, tracks

HALF_PI = np.pi / 2
FIELD = diskmod.BField(0.3, 0.8, 0.5, 0.7)
SIN_ZETA_MIN = 0.05
TRUTH_BOUND = 2.1e-11        # 10 x the measured change of the truth's (q, u) on halving its tolerance (header)
KAPPA_BOUND = 5.9e-10        # the same rule for kappa / |kappa|, whose own change on halving is larger (header)
ARRIVAL_TOL = 1e-8
R_OUT = 20.0

_HITS, _TRUTH = {}, {}


# ---- the metric and its derivatives -------------------------------------------------------------------------------------
def metric(a, r, th):
    """g (4, 4, n), d_r g, d_theta g of the Boyer-Lindquist metric (t, r, theta, phi), analytic."""
    s, c = np.sin(th), np.cos(th)
    s2 = s * s
    sig = r * r + a * a * c * c
    dlt = r * r - 2 * M * r + a * a
    dsig_th = -2 * a * a * s * c
    z = np.zeros_like(r)
    w = (sig - 2 * r * r) / (sig * sig)          # d_r (r / Sigma)
    g_tt, g_tt_r, g_tt_th = -1 + 2 * M * r / sig, 2 * M * w, -2 * M * r * dsig_th / (sig * sig)
    g_tp = -2 * M * a * r * s2 / sig
    g_tp_r = -2 * M * a * s2 * w
    g_tp_th = -2 * M * a * r * (2 * s * c * sig - s2 * dsig_th) / (sig * sig)
    g_rr, g_rr_r, g_rr_th = sig / dlt, (2 * r * dlt - sig * (2 * r - 2 * M)) / (dlt * dlt), dsig_th / dlt
    g_pp = (r * r + a * a) * s2 + 2 * M * a * a * r * s2 * s2 / sig
    g_pp_r = 2 * r * s2 + 2 * M * a * a * s2 * s2 * w
    g_pp_th = 2 * (r * r + a * a) * s * c + 2 * M * a * a * r * (4 * s2 * s * c * sig - s2 * s2 * dsig_th) / (sig * sig)

    def mat(tt, tp, rr, thth, pp):
        return np.array([[tt, z, z, tp], [z, rr, z, z], [z, z, thth, z], [tp, z, z, pp]])

    return mat(g_tt, g_tp, g_rr, sig, g_pp), mat(g_tt_r, g_tp_r, g_rr_r, 2 * r, g_pp_r), mat(g_tt_th, g_tp_th, g_rr_th, dsig_th, g_pp_th)


def raise_index(g, v):
    """g^{mu nu} v_nu for the block-diagonal metric g (4, 4, n)."""
    det = g[0, 0] * g[3, 3] - g[0, 3] * g[0, 3]
    return np.array([(g[3, 3] * v[0] - g[0, 3] * v[3]) / det, v[1] / g[1, 1], v[2] / g[2, 2], (g[0, 0] * v[3] - g[0, 3] * v[0]) / det])


def transport_rhs(a, y):
    """d / d lambda of (r, theta, k^mu, f^mu) (10, n): x' = k, k' = -Gamma(k, k), f' = -Gamma(k, f)."""
    r, th, k, f = y[0], y[1], y[2:6], y[6:10]
    g, gr, gth = metric(a, r, th)
    dk = k[1] * gr + k[2] * gth                   # k^alpha d_alpha g
    out = np.empty_like(y)
    out[0], out[1] = k[1], k[2]
    for v, lo in ((k, 2), (f, 6)):
        dv = v[1] * gr + v[2] * gth
        low = 0.5 * (np.einsum("mbn,bn->mn", dk, v) + np.einsum("man,an->mn", dv, k))
        low[1] -= 0.5 * np.einsum("an,abn,bn->n", k, gr, v)
        low[2] -= 0.5 * np.einsum("an,abn,bn->n", k, gth, v)
        out[lo:lo + 4] = -raise_index(g, low)
    return out


def test_christoffels_against_central_differences():
    rng = np.random.default_rng(1)
    r, th = rng.uniform(2.5, 50.0, 40), rng.uniform(0.3, 2.8, 40)
    for a in SPINS:
        g, gr, gth = metric(a, r, th)
        h = 1e-5
        fd_r = (metric(a, r + h, th)[0] - metric(a, r - h, th)[0]) / (2 * h)
        fd_th = (metric(a, r, th + h)[0] - metric(a, r, th - h)[0]) / (2 * h)
        scale = 1 + np.abs(g)
        assert np.max(np.abs(gr - fd_r) / scale) <= 1e-8 and np.max(np.abs(gth - fd_th) / scale) <= 1e-8


# ---- the hits of the dense tracks ----------------------------------------------------------------------------------------
def refined_hits(a, rays=None):
    """The annulus crossings (r_in = ISCO, r_out = 20) of the dense tracks, refined: per hit dict(ray, slot (its index among
    the ray's annulus crossings), planes (plane crossings before it), lam (its lambda along the backward ray), L,
    hit (r, p_r, p_theta), cam (p_r, p_theta at the camera), i (index of the track point before it))."""
    from scipy.integrate import solve_ivp
    key = (a, None if rays is None else tuple(np.concatenate(rays)))
    if key in _HITS:
        return _HITS[key]
    r_in = float(diskmod.isco(M, a))
    out = []
    for tr in tracks(a, rays):
        lam, y = tr["lam"], tr["y"]
        z = y[2] - HALF_PI
        slot = 0
        for k, i in enumerate(np.nonzero(((z[:-1] < 0) & (z[1:] >= 0)) | ((z[:-1] > 0) & (z[1:] <= 0)))[0]):
            ev = lambda t, s: s[2] - HALF_PI
            sol = solve_ivp(lambda t, s: oracle.rhs8(1, M, a, s), (lam[i], lam[i + 1]), y[:, i], method="DOP853", rtol=1e-12, atol=1e-14,
                            events=ev, dense_output=True)
            if not len(sol.t_events[0]):
                continue
            s = sol.y_events[0][0]
            # back onto the null shell: the track drifts off H = 0 by its tolerance, and kappa is conserved along null rays only
            up = diskmod._raise_index(M, a, s[1], 1.0, 0.0, (-1.0, 0.0, s[6], y[7, 0]))
            dlt = s[1] * s[1] - 2 * M * s[1] + a * a
            s[5] = np.sign(s[5]) * np.sqrt(-(-up[0] + s[6] * up[2] + y[7, 0] * up[3]) * s[1] * s[1] / dlt)
            if r_in <= s[1] <= R_OUT:
                out.append(dict(ray=tr["ray"], slot=slot, planes=k, lam=float(sol.t_events[0][0]), L=float(y[7, 0]),
                                hit=np.array([s[1], s[5], s[6]]), cam=np.array([y[5, 0], y[6, 0]]), i=int(i)))
                slot += 1
    _HITS[key] = out
    return out


def transport_truth(a, hits, rtol=1e-11, field=FIELD):
    """Brute-force transport of every hit's (k, f) to the camera -> dict(qu (n, 2), sin_zeta, arrive (n, 4): r, theta, k_r,
    k_theta at the end, kappa_hit, kappa_cam (n, 2))."""
    from scipy.integrate import solve_ivp
    hs = np.array([h["hit"] for h in hits])
    L = np.array([h["L"] for h in hits])
    lam = np.array([h["lam"] for h in hits])
    k, f, s2, _ = diskmod.emission_vector(M, a, L, hs, field)
    n = len(hits)
    y0 = np.concatenate([[hs[:, 0], np.full(n, HALF_PI)], np.array(k), np.array(f)]).reshape(-1)
    sol = solve_ivp(lambda s, y: (transport_rhs(a, y.reshape(10, n)) * lam).reshape(-1), (0.0, 1.0), y0, method="DOP853",
                    rtol=rtol, atol=1e-3 * rtol)
    y = sol.y[:, -1].reshape(10, n)
    r, th, kk, ff = y[0], y[1], y[2:6], y[6:10]
    g = metric(a, r, th)[0]
    k_low = np.einsum("abn,bn->an", g, kk)
    # the screen at the arrival point, from the arrived photon itself; f on it by the metric
    kc, f1, f2, _ = diskmod.camera_screen(M, a, r, th, k_low[3], np.stack([-k_low[1], -k_low[2]], axis=-1))
    x = np.einsum("an,abn,bn->n", np.array(f1), g, ff)
    yy = np.einsum("an,abn,bn->n", np.array(f2), g, ff)
    n2 = x * x + yy * yy
    s_th, c_th = np.sin(th), np.cos(th)
    return dict(qu=np.stack([(x * x - yy * yy) / n2, 2 * x * yy / n2], axis=-1), sin_zeta=np.sqrt(s2),
                arrive=np.stack([r, th, k_low[1], k_low[2]], axis=-1), e_t=k_low[0], L=k_low[3],
                kappa_hit=np.stack(diskmod.walker_penrose(a, hs[:, 0], 1.0, 0.0, k, f), axis=-1),
                kappa_cam=np.stack(diskmod.walker_penrose(a, r, s_th, c_th, kk, ff), axis=-1))


def truth(a, rays=None):
    """refined_hits(a, rays) and their transported truth at rtol 1e-11, cached."""
    key = (a, None if rays is None else tuple(np.concatenate(rays)))
    if key not in _TRUTH:
        hits = refined_hits(a, rays)
        _TRUTH[key] = (hits, transport_truth(a, hits))
    return _TRUTH[key]


def closed_form(a, hits, field=FIELD, dtype=np.float64):
    return diskmod.polarization(M, a, R_OBS, THETA_OBS, np.array([h["L"] for h in hits]), np.array([h["hit"] for h in hits]),
                                np.array([h["cam"] for h in hits]), field, dtype)


# ---- 1, 2: the rule against the truth ---------------------------------------------------------------------------------------
def camera_sensitivity(a, hits, offsets):
    """Per hit, sum_i |d(q, u) / d x_i| |offset_i| over the camera's (r_obs, theta_obs, p_r, p_theta), by central differences
    of the closed form: how far (q, u) may move when the camera end is off by `offsets` (n, 4)."""
    L, hs = np.array([h["L"] for h in hits]), np.array([h["hit"] for h in hits])
    cam = np.array([h["cam"] for h in hits])
    base = np.stack([np.full(len(hits), R_OBS), np.full(len(hits), THETA_OBS), cam[:, 0], cam[:, 1]], axis=-1)
    out = np.zeros((len(hits), 2))
    for i in range(4):
        d = np.zeros(4)
        d[i] = 1e-6
        hi, lo = base + d, base - d
        f = lambda x: diskmod.polarization(M, a, x[:, 0], x[:, 1], L, hs, x[:, 2:], FIELD)[:, :2]
        out += np.abs(f(hi) - f(lo)) / 2e-6 * np.abs(offsets[:, i:i + 1])
    return out


@pytest.mark.parametrize("a", SPINS)
def test_rule_against_transported_truth(a):
    hits, t = truth(a)
    assert len(hits) >= 20 and sum(h["slot"] > 0 or h["planes"] > 0 for h in hits) >= 2
    keep = t["sin_zeta"] >= SIN_ZETA_MIN
    assert keep.sum() >= 0.98 * len(hits)
    L, hs = np.array([h["L"] for h in hits]), np.array([h["hit"] for h in hits])
    cam = np.array([h["cam"] for h in hits])
    arr = t["arrive"]
    # the reading of the photon: it arrives at the camera with the reversed momenta of the camera's own record
    offsets = np.stack([arr[:, 0] - R_OBS, arr[:, 1] - THETA_OBS, -arr[:, 2] - cam[:, 0], -arr[:, 3] - cam[:, 1]], axis=-1)
    off = max(np.max(np.abs(offsets)), np.max(np.abs(t["e_t"] + 1.0)), np.max(np.abs(t["L"] - L)))
    # the rule on the truth's own ends, and on the camera's record (which the track meets to `offsets`)
    own = diskmod.polarization(M, a, arr[:, 0], arr[:, 1], L, hs, -arr[:, 2:4], FIELD)
    got = closed_form(a, hits)
    d_own = np.abs(own[keep, :2] - t["qu"][keep])
    d_rec = np.abs(got[keep, :2] - t["qu"][keep])
    allow = TRUTH_BOUND + camera_sensitivity(a, hits, offsets)[keep]
    nk = np.linalg.norm(t["kappa_hit"], axis=-1, keepdims=True)
    kap = np.max(np.abs(t["kappa_cam"] - t["kappa_hit"]) / nk)
    print(f"a {a}: {len(hits)} hits ({int((~keep).sum())} with sin zeta < {SIN_ZETA_MIN}); arrival off by at most {off:.2e}; "
          f"largest |dq|, |du| {d_own.max():.2e} on the truth's ends, {d_rec.max():.2e} on the camera's record (allowed "
          f"{allow[np.unravel_index(np.argmax(d_rec), d_rec.shape)]:.2e} there); kappa conserved to {kap:.2e} of |kappa|")
    assert off <= ARRIVAL_TOL
    assert d_own.max() <= TRUTH_BOUND
    assert np.all(d_rec <= allow)
    assert kap <= KAPPA_BOUND
    assert np.array_equal(got[:, 2:], own[:, 2:]) and np.max(np.abs(got[:, 2] - t["sin_zeta"])) == 0.0
    assert np.max(np.abs(got[:, 0] ** 2 + got[:, 1] ** 2 - 1.0)) <= 1e-12 and np.all((got[:, 3] >= 0) & (got[:, 3] <= 1))


# ---- 3: mirror symmetry ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", [(0.0, 0.0, 1.0), (0.6, -0.8, 0.0)], ids=["vertical", "in-plane"])
@pytest.mark.parametrize("a", SPINS)
def test_equatorial_mirror(a, field):
    """theta_obs = pi / 2: the ray at screen angle t and its mirror image through the equatorial plane (screen angle
    pi - t: p_theta reversed everywhere) have equal q and opposite u, for a field that the reflection maps to +- itself."""
    rng = np.random.default_rng(3)
    n = 200
    r_hit = rng.uniform(float(diskmod.isco(M, a)), 20.0, n)
    pr, pth, L = rng.uniform(-1.2, 1.2, n), rng.uniform(-6.0, 6.0, n), rng.uniform(-5.0, 6.0, n)
    cam = np.stack([-rng.uniform(0.9, 1.0, n), rng.uniform(-6.0, 6.0, n)], axis=-1)
    b = diskmod.BField(*field, 0.7)
    up = diskmod.polarization(M, a, R_OBS, HALF_PI, L, np.stack([r_hit, pr, pth], axis=-1), cam, b)
    dn = diskmod.polarization(M, a, R_OBS, HALF_PI, L, np.stack([r_hit, pr, -pth], axis=-1), cam * [1.0, -1.0], b)
    assert np.max(np.abs(up[:, 0] - dn[:, 0])) <= 1e-10 and np.max(np.abs(up[:, 1] + dn[:, 1])) <= 1e-10
    assert np.array_equal(up[:, 2:], dn[:, 2:]) and np.abs(up[:, 1]).max() > 0.5


# ---- 4 - 7: the Stokes sums --------------------------------------------------------------------------------------------------
def synth_pol(shape, seed):
    """Random polarization records (shape + (4,)) float32: unit (q, u), sin zeta and mu in [0, 1]."""
    rng = np.random.default_rng(seed)
    chi2 = rng.uniform(0.0, 2 * np.pi, shape)
    return np.stack([np.cos(chi2), np.sin(chi2), rng.uniform(0.0, 1.0, shape), rng.uniform(0.0, 1.0, shape)], axis=-1).astype(np.float32)


def _records(seed=7, shape=(40, 37, 4)):
    from test_hotspot_records_host import synth
    hits, n_hits = synth(*shape, seed, float(diskmod.isco(M, 0.9)), 20.0)
    return hits, n_hits, synth_pol(shape, seed + 100)


SPOT = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5, exposure=2.0, with_disk=True)
TIMES = 5.0 + 7.5 * np.arange(6)


def test_stokes_intensity_is_the_lightcurve():
    hits, n_hits, pol = _records()
    lc = diskmod.lightcurve(M, 0.9, hits, n_hits, SPOT, TIMES)
    st = diskmod.stokes_lightcurve(M, 0.9, hits, n_hits, pol, SPOT, TIMES, FIELD)
    assert st.shape == (6, 3) and np.array_equal(st[:, 0], lc[:, 0])
    assert np.all(np.abs(st[:, 1:]) <= FIELD.pol_frac * st[:, :1]) and np.abs(st[:, 1:]).min() > 0
    fr = diskmod.stokes_frame(M, 0.9, hits, n_hits, pol, diskmod.ThinDisk(), SPOT, 20.0, FIELD)
    assert fr.shape == hits.shape[:2] + (3,) and fr.dtype == np.float32
    assert np.all(np.hypot(fr[..., 1], fr[..., 2]) <= FIELD.pol_frac * fr[..., 0] * (1 + 1e-6))
    assert np.all(fr[n_hits == 0] == 0) and np.all(fr[n_hits > 0, 0] > 0)


def test_unpolarized_is_exactly_zero():
    hits, n_hits, pol = _records()
    b0 = diskmod.BField(0.3, 0.8, 0.5, 0.0)
    assert np.all(diskmod.stokes_lightcurve(M, 0.9, hits, n_hits, pol, SPOT, TIMES, b0)[:, 1:] == 0)
    assert np.all(diskmod.stokes_frame(M, 0.9, hits, n_hits, pol, diskmod.ThinDisk(), SPOT, 20.0, b0)[..., 1:] == 0)


def test_field_reversal_changes_no_bit():
    neg = diskmod.BField(-FIELD.b_r, -FIELD.b_phi, -FIELD.b_z, FIELD.pol_frac)
    for a in SPINS:
        hits = refined_hits(a)
        assert closed_form(a, hits, FIELD).tobytes() == closed_form(a, hits, neg).tobytes()


def test_whole_periods_change_no_bit():
    """Frames a whole number of orbital periods apart: the spot is at the same place to float64 rounding (~1e-15 of a
    value), far below the float32 a frame is stored in, so Q and U repeat with the intensity, bit for bit."""
    hits, n_hits, pol = _records()
    a = 0.9
    period = 2 * np.pi / float(diskmod.omega(M, a, SPOT.r_spot))
    f0 = diskmod.stokes_frame(M, a, hits, n_hits, pol, diskmod.ThinDisk(), SPOT, 64.0, FIELD)
    for k in (1, 3):
        fk = diskmod.stokes_frame(M, a, hits, n_hits, pol, diskmod.ThinDisk(), SPOT, 64.0 + k * period, FIELD)
        assert fk.tobytes() == f0.tobytes()
    half = diskmod.stokes_frame(M, a, hits, n_hits, pol, diskmod.ThinDisk(), SPOT, 64.0 + 0.5 * period, FIELD)
    assert (half != f0).any(axis=-1).sum() > 100


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------------
def _calls():
    cam = ltrace.Camera(64, 48, 0.7, 0.5, 0.0, 0.0, 50.0, 1.4)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    hits, n_hits, pol = _records(shape=(6, 5, 2))
    d, s = ltrace.default_disk(), ltrace.default_hotspot()
    return lambda b: [lambda: ltrace.trace_disk_pol(cam, met, ltrace.default_opts(), d, b),
                      lambda: ltrace.trace_batch_kerr_disk_pol(1.0, 0.9, 50.0, [0.1], [0.2], 1.4, 5000.0, d, b),
                      lambda: ltrace.polarization_probe(met, 50.0, 1.4, [2.0], [[8.0, -0.5, 1.0]], [[-0.99, 2.0]], b),
                      lambda: ltrace.shade_stokes(hits, n_hits, pol, met, d, s, b, 0.0),
                      lambda: ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, b, 0.0, 1.0, 4)]


def test_default_field():
    b = ltrace.default_bfield()
    assert (b.b_r, b.b_phi, b.b_z, b.pol_frac) == (0.0, 0.0, 1.0, 0.7)
    lt = diskmod.BField(0.3, 0.8, 0.5, 0.25).to_lt()
    assert (lt.b_r, lt.b_phi, lt.b_z, lt.pol_frac) == (0.3, 0.8, 0.5, 0.25)
    assert ltrace.load().lt_version() == 200


def test_refusals():
    """Without a GPU every new compute entry point returns LT_ERR_NO_DEVICE; with one, a zero field and a polarization
    fraction outside [0, 1] are LT_ERR_INVALID_ARG."""
    calls = _calls()
    if ltrace.device_count() <= 0:
        for call in calls(ltrace.default_bfield()) + calls(ltrace.default_bfield(b_z=0.0)):
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE
        return
    for bad in (ltrace.default_bfield(b_z=0.0), ltrace.default_bfield(pol_frac=1.5), ltrace.default_bfield(pol_frac=-0.1),
                ltrace.default_bfield(b_r=float("nan"))):
        for call in calls(bad):
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_INVALID_ARG
