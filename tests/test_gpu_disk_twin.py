"""GPU tests of the accretion disk's hit rule against its step-exact CPU twin (oracle.trace_batch_kerr_disk).

tests/test_gpu_disk.py and tests/test_gpu_disk_images.py compare the disk kernels with the TRUE geodesic, so their
budgets have to absorb the integrator's own truncation error (RK4: 3e-2 in r with a 10 % tail).  The twin applies the
rule of include/ltrace.h to the accepted states of the oracle's own RK4 / DP45 tracer -- every step tested, no radius
pre-filter, no streak gate, the root by 64 halvings -- so the only difference left is the arithmetic's: float64
rounding and the kernels' Newton root against the twin's bisection.  Every number the disk produces is pinned at that
level, with no tail.

Budgets (eps_r, eps_phi, eps_theta): |dr| <= (eps_r + |r'/theta'| eps_theta) e^(pi k) and likewise for phi, k = plane
crossings of the ray before the hit (a deviation grows by e^pi per half orbit, tests/test_gpu_disk_images.py).
MEASURED on the MI355X (build 975d7207b2c9; profiles/disk_twin_975d7207b2c9.json holds the per-case figures), GPU
minus twin, 3 456 rays per case, opaque and thin entry points, every stored slot, rays not excluded:
                                         max |dr|   max |dphi|  max |dg|   max nr     max nphi    fa median / p99
    a=0.9   th=1.4    r=50   out=20      2.6e-7     1.7e-8      4.5e-9     2.5e-9     2.4e-9      7e-16 / 2.3e-10
    a=0.9   th=1.4    r=50   out=40      3.1e-7     1.7e-8      4.5e-9     2.5e-9     2.4e-9      6e-16 / 2.5e-10
    a=-0.7  th=1.2    r=50   out=20      7.0e-7     1.8e-8      8.7e-9     5.2e-9     4.9e-9      6e-16 / 1.0e-9
    a=0.998 th=1.45   r=50   out=20      4.0e-7     7.3e-8      4.1e-9     1.8e-9     1.7e-9      7e-16 / 1.1e-10
    a=0     th=1.45   r=1000 out=20      1.0e-7     9.8e-9      3.0e-9     1.1e-9     1.1e-9      1e-15 / 9.3e-11
    a=0.9   th=pi-1.4 r=50   out=20      2.6e-7     1.7e-8      4.7e-9     2.4e-9     2.4e-9      7e-16 / 2.5e-10
nr = |dr| / ((1 + |r'/theta'|) e^(pi k)), nphi likewise: the model's own unit.  The figures are RK4 float64's; DP45-exact
and plain DP45 give the same to two digits (the difference is the crossing's arithmetic, not the integrator's), and
status, n_hits, winding and rhs_evals equal the twin's on every ray not excluded, in all 24 float64 runs.  Slot 1 sits
at nr 1e-10, slots 2 and 3 at 1e-13 and below: e^(pi k) overstates the growth, so the later slots are held harder than
slot 0.  The largest raw |dr| belong to rays that cross the plane at a shallow angle (|r'/theta'| up to ~100).
BUDGETS, 10 x the largest nr / nphi: eps_r = 5.2e-8, eps_phi = 4.9e-8, eps_theta = 5.2e-8 (BUDGET64 in
test_oracle_disk.py) -- 600 times under the ceilings set beforehand (eps_r <= 3e-5, eps_phi, eps_theta <= 1e-5, a
thousandth of test_gpu_disk.py's RK4 budget).
RK4 float32 against the float64 twin, slot 0 of the primary hits: no ray of 20 626 with another hit count (budget
1e-3), none beyond 3e-4 in r (condition: at most 1 %); (median, p99) of |dr| from (2.5e-6, 3.5e-5) at a = 0.998 to
(1.1e-5, 1.9e-4) at r_obs = 1000, of |dphi| from (1.3e-7, 9.7e-7) to (7.6e-7, 4.3e-6).  Q32 is 4 x each case's own.
The frame path agrees with the twin rounded to float32 bit for bit on all 7 680 pixels (allowed: 2 ulp + budget).
"""
import numpy as np
import pytest

import disk as diskmod
import disk_blocks as dk
import ltrace
from oracle import oracle  # noqa: F401
from test_oracle_disk import (BUDGET64, CASES, CASE_IDS, E_PI, FRAME_H, FRAME_W, M, crossing_k, excluded, fans,  # noqa: F401
                              frame_fov, frame_twin, hit_slots, lam_max, twin)

pytestmark = pytest.mark.gpu

# float32 RK4 against the float64 twin: exclusion margins (eps_r, eps_theta) = the ceiling 3e-4 and a third of it (theta
# ~ pi/2 at a crossing where r ~ 10: the same relative size); per case ((median, p99) of slot 0's |dr|, of its |dphi|) over
# the primary hits, 4 x the measured quantiles (header)
EXCL32 = (3e-4, 1e-4)
Q32 = [((1.2e-5, 1.2e-4), (1.1e-6, 6.5e-6)),
       ((1.9e-5, 1.6e-4), (7.8e-7, 6.5e-6)),
       ((1.3e-5, 6.3e-5), (5.2e-7, 3.9e-6)),
       ((9.9e-6, 1.4e-4), (1.3e-6, 1.9e-5)),
       ((4.6e-5, 7.5e-4), (3.1e-6, 1.8e-5)),
       ((1.3e-5, 1.2e-4), (1.1e-6, 7.0e-6))]
FLIPS32 = 1e-3  # the project's float32 class-flip budget


def dphi(a, b):
    return np.abs((a - b + np.pi) % (2 * np.pi) - np.pi)


def g_bound(a, r, xi, br):
    """How far g may move when r moves by br: g is a closed form of (r, xi)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        g0 = diskmod.redshift(M, a, r, xi)
        lo, hi = diskmod.redshift(M, a, np.maximum(r - br, 1e-3), xi), diskmod.redshift(M, a, r + br, xi)
    return 1.5 * np.maximum(np.abs(lo - g0), np.abs(hi - g0)) + 1e-12 * np.abs(g0)


def slot_errors(ci, images, tw, rays, n_slots):
    """GPU slots (n, m, 3) against the twin's for the rays in `rays` (bool), slots below n_slots (n,): -> dict of flat
    arrays over those (ray, slot) pairs: ray, slot, dr, dphi, dg, k, s_r, s_phi, nr = |dr| / ((1 + s_r) e^(pi k)),
    nphi likewise (the figures the budgets are ten times the maxima of)."""
    hs = hit_slots(tw, images.shape[1])
    m = images.shape[1]
    sel = rays[:, None] & (np.arange(m)[None, :] < n_slots[:, None])
    i, j = np.nonzero(sel)
    t = tw["images"][:, :m]
    dr = np.abs(images[i, j, 0] - t[i, j, 0])
    dp = dphi(images[i, j, 1], t[i, j, 1])
    dg = np.abs(images[i, j, 2] - t[i, j, 2])
    k, s_r, s_phi = hs["k"][i, j], hs["s_r"][i, j], hs["s_phi"][i, j]
    return dict(ray=i, slot=j, dr=dr, dphi=dp, dg=dg, k=k, s_r=s_r, s_phi=s_phi, nr=dr / ((1 + s_r) * E_PI ** k),
                nphi=dp / ((1 + s_phi) * E_PI ** k), hs=hs)


def describe(ci, tw, e, idx):
    """The twin's diagnostics of the offending (ray, slot) pairs, for the failure message."""
    a, tho, ro, rout = CASES[ci]
    rc4 = 4.0 * 1.01 * (M + np.sqrt(M * M - a * a))
    lines = []
    for q in idx[:6]:
        i, j = int(e["ray"][q]), int(e["slot"][q])
        hs = e["hs"]
        lines.append(f"ray {i} slot {j}: dr {e['dr'][q]:.3e} dphi {e['dphi'][q]:.3e} dg {e['dg'][q]:.3e} k {e['k'][q]} "
                     f"s_r {e['s_r'][q]:.3g} | twin step {hs['step'][i, j]:.0f} t {hs['t'][i, j]:.6f} h {hs['h'][i, j]:.4g} "
                     f"r {hs['r0'][i, j]:.5f} -> {hs['r1'][i, j]:.5f} "
                     f"{'streak region' if hs['r0'][i, j] >= rc4 else 'banded'} terminal {hs['terminal'][i, j]:.0f}")
    return "\n".join(lines)


def check_slots(ci, a, images, tw, rays, n_slots, budget, xi):
    """Asserts every selected slot within the budget; returns the error table (for the measurement script)."""
    eps_r, eps_phi, eps_th = budget
    e = slot_errors(ci, images, tw, rays, n_slots)
    scale = E_PI ** e["k"]
    br = (eps_r + e["s_r"] * eps_th) * scale
    bp = (eps_phi + e["s_phi"] * eps_th) * scale
    bg = g_bound(a, tw["images"][e["ray"], e["slot"], 0], xi[e["ray"]], br)
    print(f"case {ci}: {e['dr'].size} slots, max |dr| {e['dr'].max():.3e} |dphi| {e['dphi'].max():.3e} |dg| {e['dg'].max():.3e}; "
          f"normalised max r {e['nr'].max():.3e} phi {e['nphi'].max():.3e}")
    bad = np.nonzero((e["dr"] > br) | (e["dphi"] > bp) | (e["dg"] > bg))[0]
    assert bad.size == 0, f"{bad.size} of {e['dr'].size} slots outside the budget {budget}\n" + describe(ci, tw, e, bad)
    return e


def check_g_closed_form(a, images, xi):
    """g is disk.redshift of the r the call returns, within the unit of tests/disk_blocks.py: 2 K_G units for the device's g and
    K_G for numpy's -- a few 1e-15 relative; 2e-13 at the ISCO of a = 0.998, where the radicand r^1.5 - 3 M sqrt r + 2 a sqrt M
    cancels by a factor of a hundred."""
    r, g = images[..., 0], images[..., 2]
    on = ~np.isnan(r)
    xi_on = np.broadcast_to(xi.reshape((-1,) + (1,) * (r.ndim - 1)), r.shape)[on]
    ref = diskmod.redshift(M, a, r[on], xi_on)
    bound = 3 * dk.K_G * dk.g_unit(M, a, r[on], xi_on)
    assert np.all(np.abs(g[on] - ref) <= bound), float(np.max(np.abs(g[on] - ref) / bound))


def check_fa(fa_gpu, fa_tw, rays):
    both = rays & ~np.isnan(fa_gpu) & ~np.isnan(fa_tw)
    assert np.array_equal(np.isnan(fa_gpu[rays]), np.isnan(fa_tw[rays]))
    d = np.abs(fa_gpu[both] - fa_tw[both])
    # the project's float64 parity: median 1e-10, p99 1e-8
    assert np.median(d) <= 1e-10 and np.quantile(d, 0.99) <= 1e-8, (np.median(d), np.quantile(d, 0.99))


def run_gpu(ci, integ, prec):
    a, tho, ro, rout = CASES[ci]
    al, th, ar, _ = fans(ro, rout)
    d = ltrace.default_disk(r_out=rout)
    opq = ltrace.trace_batch_kerr_disk(M, a, ro, al, th, tho, lam_max(ro), d, axis_refines=ar, integrator=integ,
                                       precision=prec)
    thin = ltrace.trace_batch_kerr_disk_images(M, a, ro, al, th, tho, lam_max(ro), d, max_images=8, axis_refines=ar,
                                               integrator=integ, precision=prec)
    return opq, thin


def compare_exact(ci, integ, opq, thin, budget=BUDGET64):
    """The float64 paths whose steps are the oracle's (RK4, DP45-exact) against the twin: everything, no tail.
    -> (error table of the opaque call, of the thin call, excluded share)."""
    a, tho, ro, rout = CASES[ci]
    r_in = float(diskmod.isco(M, a))
    tname = "rk4" if integ == "rk4" else "dp45"
    t_opq, t_thin = twin(ci, tname, True), twin(ci, tname, False)
    ex = excluded(t_thin, r_in, rout, budget[0], budget[2])
    ok = ~ex
    share = ex.mean()
    print(f"case {ci} {integ}: {ex.sum()} of {ex.size} rays excluded ({100 * share:.2f} %)")
    assert share <= 0.02
    xi = t_thin["xi"]
    # opaque: the ray ends at its first hit
    for k in ("status", "winding", "rhs_evals"):
        diff = np.nonzero(ok & (opq[k] != t_opq[k]))[0]
        assert diff.size == 0, (k, diff[:8], opq[k][diff[:8]], t_opq[k][diff[:8]])
    check_fa(opq["fa"], t_opq["fa"], ok)
    on = opq["status"] == ltrace.STATUS_DISK
    assert np.all(np.isnan(opq["disk"][~on])) and not np.any(np.isnan(opq["disk"][on]))
    assert np.all(np.isnan(opq["fa"][on]))
    e1 = check_slots(ci, a, opq["disk"][:, None, :], t_opq, ok & on, on.astype(np.int64), budget, xi)
    check_g_closed_form(a, opq["disk"], xi)
    # thin: the ray goes on; the plain tracer's fa, winding, status, evaluations
    for k in ("status", "winding", "rhs_evals", "n_hits"):
        diff = np.nonzero(ok & (thin[k] != t_thin[k]))[0]
        assert diff.size == 0, (k, diff[:8], thin[k][diff[:8]], t_thin[k][diff[:8]])
    check_fa(thin["fa"], t_thin["fa"], ok)
    ns = np.minimum(thin["n_hits"], 8).astype(np.int64)
    used = np.arange(8)[None, :] < ns[:, None]
    assert np.all(np.isnan(thin["images"][~used])) and not np.any(np.isnan(thin["images"][used]))
    ph = thin["images"][..., 1][used]
    assert np.all((ph >= 0) & (ph < 2 * np.pi))
    e2 = check_slots(ci, a, thin["images"], t_thin, ok, ns, budget, xi)
    check_g_closed_form(a, thin["images"], xi)
    return e1, e2, share


@pytest.mark.parametrize("integ", ["rk4", "dp45_exact"])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_float64_against_twin(ci, integ):
    opq, thin = run_gpu(ci, integ, 64)
    compare_exact(ci, integ, opq, thin)


def compare_dp45(ci, opq, thin):
    """Plain DP45 (float32 step-size controller): its accept / reject sequence is not the reference's, so hit counts
    and slot 0 against the DP45 twin under test_gpu_disk.py's DP45 budget.  -> (|dr|, |dphi|) of slot 0."""
    from test_gpu_disk import BUDGET
    eps_r, eps_phi, eps_th, tail = BUDGET[("dp45_exact", 64)]
    assert tail == 0.0
    a, tho, ro, rout = CASES[ci]
    r_in = float(diskmod.isco(M, a))
    t_thin = twin(ci, "dp45", False)
    ok = ~excluded(t_thin, r_in, rout, eps_r, eps_th)
    print(f"case {ci} dp45: {(~ok).sum()} of {ok.size} rays excluded")
    diff = np.nonzero(ok & (thin["n_hits"] != t_thin["n_hits"]))[0]
    assert diff.size == 0, (diff[:8], thin["n_hits"][diff[:8]], t_thin["n_hits"][diff[:8]])
    assert np.array_equal((opq["status"] == ltrace.STATUS_DISK)[ok], (t_thin["n_hits"] > 0)[ok])
    rays = ok & (t_thin["n_hits"] > 0)
    e = slot_errors(ci, thin["images"][:, :1], t_thin, rays, np.ones(ok.size, np.int64))
    scale = E_PI ** e["k"]
    print(f"case {ci} dp45: slot 0 max |dr| {e['dr'].max():.3e} |dphi| {e['dphi'].max():.3e}")
    bad = np.nonzero((e["dr"] > (eps_r + e["s_r"] * eps_th) * scale) | (e["dphi"] > (eps_phi + e["s_phi"] * eps_th) * scale))[0]
    assert bad.size == 0, f"{bad.size} of {e['dr'].size} outside the budget\n" + describe(ci, t_thin, e, bad)
    assert opq["disk"][rays, :2].tobytes() == np.ascontiguousarray(thin["images"][rays, 0, :2]).tobytes()
    return e


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_plain_dp45_against_twin(ci):
    opq, thin = run_gpu(ci, "dp45", 64)
    compare_dp45(ci, opq, thin)


def compare_f32(ci, opq, thin):
    """RK4 float32 against the float64 RK4 twin.  -> (flip share, |dr|, |dphi| of slot 0 where both have the hit)."""
    a, tho, ro, rout = CASES[ci]
    r_in = float(diskmod.isco(M, a))
    t_thin = twin(ci, "rk4", False)
    ok = ~excluded(t_thin, r_in, rout, EXCL32[0], EXCL32[1])
    flips = ok & (thin["n_hits"] != t_thin["n_hits"])
    share = flips.sum() / ok.sum()
    assert np.array_equal(opq["status"] == ltrace.STATUS_DISK, thin["n_hits"] > 0)
    rays = ok & (thin["n_hits"] > 0) & (t_thin["n_hits"] > 0) & ~flips
    e = slot_errors(ci, thin["images"][:, :1], t_thin, rays, np.ones(ok.size, np.int64))
    first = e["k"] == 0
    dr, dp = e["dr"][first], e["dphi"][first]
    beyond = float((dr > 3e-4).mean())
    print(f"case {ci} rk4 f32: {(~ok).sum()} excluded, flips {flips.sum()} of {ok.sum()} ({share:.2e}); slot 0 of {dr.size} primary hits: "
          f"|dr| median {np.median(dr):.3e} p99 {np.quantile(dr, 0.99):.3e} max {dr.max():.3e}, "
          f"|dphi| median {np.median(dp):.3e} p99 {np.quantile(dp, 0.99):.3e}; beyond 3e-4: {beyond:.4f}")
    assert share <= FLIPS32, (int(flips.sum()), int(ok.sum()))
    assert beyond <= 0.01
    (dr_med, dr_p99), (dp_med, dp_p99) = Q32[ci]
    assert np.median(dr) <= dr_med and np.quantile(dr, 0.99) <= dr_p99, (np.median(dr), np.quantile(dr, 0.99))
    assert np.median(dp) <= dp_med and np.quantile(dp, 0.99) <= dp_p99, (np.median(dp), np.quantile(dp, 0.99))
    g_ref = diskmod.redshift(M, a, thin["images"][rays, 0, 0], t_thin["xi"][rays])
    assert np.all(np.abs(thin["images"][rays, 0, 2] - g_ref) <= 1e-6 * np.abs(g_ref))  # xi is a float32 here
    return share, dr, dp


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_rk4_float32_against_twin(ci):
    opq, thin = run_gpu(ci, "rk4", 32)
    compare_f32(ci, opq, thin)


# ---- the frame path: the prologue's own initial conditions in the same chain ------------------------------------------
def frame_camera():
    a, tho, ro, rout = CASES[0]
    hfov, vfov = frame_fov()
    return ltrace.Camera(FRAME_W, FRAME_H, hfov, vfov, 0.0, 0.0, ro, tho), hfov, vfov


def compare_frame(opq, thin, budget=BUDGET64):
    a, tho, ro, rout = CASES[0]
    r_in = float(diskmod.isco(M, a))
    t_opq, t_thin = frame_twin(True, 3), frame_twin(False, 3)
    ex = excluded(t_thin, r_in, rout, budget[0], budget[2])
    ok = ~ex
    print(f"frame: {ex.sum()} of {ex.size} pixels excluded")
    assert ex.mean() <= 0.02
    n = FRAME_W * FRAME_H
    assert np.array_equal(np.asarray(opq["status"]).ravel()[ok], t_opq["status"][ok])
    assert np.array_equal(np.asarray(thin["status"]).ravel()[ok], t_thin["status"][ok])
    assert np.array_equal(np.asarray(thin["n_hits"]).ravel().astype(np.int64)[ok], np.minimum(t_thin["n_hits"], 255)[ok])
    hs = hit_slots(t_thin, 3)
    eps_r, eps_phi, eps_th = budget
    worst = 0.0
    for name, got, tw, m in (("render_disk", np.asarray(opq["disk"]).reshape(n, 1, 3), t_opq, 1),
                             ("render_disk_images", np.asarray(thin["images"]).reshape(n, 3, 3), t_thin, 3)):
        ref = tw["images"][:, :m]
        ref32 = ref.astype(np.float32)
        ns = np.minimum(tw["n_hits"], m)
        used = ok[:, None] & (np.arange(m)[None, :] < ns[:, None])
        assert np.all(np.isnan(got[ok][np.isnan(ref32[ok])]))
        scale = E_PI ** hs["k"][:, :m]
        br = (eps_r + np.nan_to_num(hs["s_r"][:, :m]) * eps_th) * scale
        bp = (eps_phi + np.nan_to_num(hs["s_phi"][:, :m]) * eps_th) * scale
        xi = np.broadcast_to(tw["xi"][:, None], (n, m))
        bg = g_bound(a, ref[..., 0], xi, br)
        for c, b in ((0, br), (1, bp), (2, bg)):
            err = np.abs(got[..., c].astype(np.float64) - ref32[..., c].astype(np.float64))
            if c == 1:
                err = np.minimum(err, 2 * np.pi - err)
            tol = 2 * np.spacing(np.abs(ref32[..., c])).astype(np.float64) + b
            bad = used & ~(err <= tol)
            worst = max(worst, float(np.max((err / np.spacing(np.abs(ref32[..., c])))[used])))
            assert not bad.any(), (name, c, int(bad.sum()), np.argwhere(bad)[:4], err[bad][:4], tol[bad][:4])
    print(f"frame: worst slot error {worst:.2f} float32 ulp")


def test_frame_against_twin():
    a, tho, ro, rout = CASES[0]
    cam, hfov, vfov = frame_camera()
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    o = ltrace.default_opts(integrator="rk4", precision=64, tb_symmetry=0)
    opq = ltrace.render_disk(cam, met, o, ltrace.default_disk(r_out=rout), want=("status", "disk"))
    thin = ltrace.render_disk_images(cam, met, o, ltrace.default_disk(r_out=rout), max_images=3,
                                     want=("status", "images", "n_hits"))
    compare_frame(opq, thin)
