"""CPU tests of the disk's step-exact twin (oracle.trace_batch_kerr_disk, oracle/lt_oracle.c): the reference that
tests/test_gpu_disk_twin.py holds the kernels to is itself pinned here, without a GPU.  It changes no step of the
oracle's tracers; its primary hits lie within the existing budgets of the independent truth (the dense DP45 of
tests/test_gpu_disk.py); it obeys the symmetries of the problem; and the fans the GPU test uses reach the places where
a kernel can be wrong: both edges of the annulus, RK4's streak region, hits behind an earlier crossing, higher-order
images, a hit on the very step that ends the ray."""
import numpy as np
import pytest

import disk as diskmod
from oracle import oracle
from test_gpu_disk import BUDGET, _Tally, _truth

M = 1.0
E_PI = float(np.exp(np.pi))
# (a, theta_obs, r_obs, r_out)
CASES = [(0.9, 1.4, 50.0, 20.0),
         (0.9, 1.4, 50.0, 40.0),          # an outer edge deep in RK4's streak region, close under r_obs
         (-0.7, 1.2, 50.0, 20.0),
         (0.998, 1.45, 50.0, 20.0),       # r_in = 1.237, just outside the capture radius: the 0.05 / 0.10 step bands
         (0.0, 1.45, 1000.0, 20.0),       # a far observer: DP45 starts at h = 0.01 r_obs
         (0.9, np.pi - 1.4, 50.0, 20.0)]  # the observer below the plane
CASE_IDS = [f"a{a:g}-th{t:.3g}-r{r:g}-out{o:g}" for a, t, r, o in CASES]

# float64 (eps_r, eps_phi, eps_theta): 10 x the largest GPU - twin difference measured on the MI355X, in the model's unit
# (tests/test_gpu_disk_twin.py's header has the figures).  Here they set the exclusion margins.
BUDGET64 = (5.2e-8, 4.9e-8, 5.2e-8)


def lam_max(r_obs):
    return max(5000.0, 6.0 * r_obs)


def fans(r_obs, r_out):
    """Deterministic rays -> (alpha, screen angle, axis_refine, in the critical-curve fan).  Per screen angle (16, evenly
    spaced from 0, so 0 and pi/2 are among them): 128 alphas over the disk's image and 64 impact parameters r_obs
    tan(alpha) from 4 to 8 around the critical curve; the fans of two of the angles once more as axis-refine rays."""
    ang = np.arange(16) * (2 * np.pi / 16)
    amax = 1.3 * np.arctan(r_out / r_obs)
    one = np.concatenate([np.linspace(0.02 * amax, amax, 128), np.arctan(np.linspace(4.0, 8.0, 64) / r_obs)])
    al, th = np.tile(one, 16), np.repeat(ang, one.size)
    crit = np.tile(np.arange(one.size) >= 128, 16)
    extra = np.isin(th, ang[[1, 10]])
    ar = np.concatenate([np.zeros(al.size, np.uint8), np.ones(int(extra.sum()), np.uint8)])
    return np.concatenate([al, al[extra]]), np.concatenate([th, th[extra]]), ar, np.concatenate([crit, crit[extra]])


_TWIN = {}


def twin(ci, integ, opaque):
    """The twin's answer for case ci, cached (and left unchanged by every user).  integ: 'rk4' or 'dp45'."""
    key = (ci, integ, bool(opaque))
    if key not in _TWIN:
        a, tho, ro, rout = CASES[ci]
        al, th, ar, _ = fans(ro, rout)
        _TWIN[key] = oracle.trace_batch_kerr_disk(M, a, ro, al, th, tho, lam_max(ro), float(diskmod.isco(M, a)), rout,
                                                  integ, 8, opaque, axis_refines=ar)
    return _TWIN[key]


def crossing_k(tw):
    """-> (recorded, on_path, k): per recorded sign change, whether it lies on the ray's path and how many crossings of
    the plane the ray made before it."""
    cr = tw["cross"]
    rec = ~np.isnan(cr[..., 0])
    on = rec & (np.nan_to_num(cr[..., 10]) == 1.0)
    return rec, on, np.cumsum(on, axis=1) - on


def excluded(tw, r_in, r_out, eps_r, eps_th):
    """Rays left out of the strict comparison, by the twin's diagnostics alone: a plane crossing within
    (eps_r + |r'/theta'| eps_theta) e^(pi k) of an edge of the annulus; a turning point of theta within eps_theta
    e^(pi k) of the plane near the annulus; a sign change on a terminal step at a radius where it could be a hit."""
    cr = tw["cross"]
    rec, on, k = crossing_k(tw)
    r, s_r = np.nan_to_num(cr[..., 5]), np.nan_to_num(cr[..., 7])
    margin = (eps_r + s_r * eps_th) * E_PI ** k
    edge = np.minimum(np.abs(r - r_in), np.abs(r - r_out)) <= margin
    term = rec & (np.nan_to_num(cr[..., 9]) != 0.0) & (r >= r_in - margin) & (r <= r_out + margin)
    return (on & edge).any(1) | term.any(1) | (tw["graze"] <= eps_th) | (tw["n_cross"] > cr.shape[1])


def hit_slots(tw, m=8):
    """Per ray, the first m hits' diagnostics: dict of (n, m) arrays (k, s_r, s_phi, step, t, h, r0, r1), NaN past the
    ray's hits."""
    cr = tw["cross"]
    rec, on, k = crossing_k(tw)
    hit = rec & (np.nan_to_num(cr[..., 11]) == 1.0)
    order = np.argsort(~hit, axis=1, kind="stable")[:, :m]
    valid = np.take_along_axis(hit, order, 1)
    out = {"k": np.where(valid, np.take_along_axis(k, order, 1), 0)}
    for name, col in (("step", 0), ("t", 1), ("h", 2), ("r0", 3), ("r1", 4), ("s_r", 7), ("s_phi", 8), ("terminal", 9)):
        out[name] = np.where(valid, np.take_along_axis(cr[..., col], order, 1), np.nan)
    return out


FRAME_W, FRAME_H = 96, 80


def frame_fov():
    vfov = np.radians(40.0)
    return 2 * np.arctan(np.tan(vfov / 2) * FRAME_W / FRAME_H), vfov


def frame_twin(opaque, max_images):
    """The twin on the rays of the first case's 96 x 80 frame: oracle.pixel_angles (alpha as the float32 the reference
    stores, the axis-refine columns), as oracle.lookup traces them."""
    a, tho, ro, rout = CASES[0]
    hfov, vfov = frame_fov()
    al, th, cols = oracle.pixel_angles(FRAME_H, FRAME_W, hfov, vfov)
    ar = np.broadcast_to(cols[None, :], al.shape).astype(np.uint8)
    return oracle.trace_batch_kerr_disk(M, a, ro, al.astype(np.float64).ravel(), th.ravel(), tho, lam_max(ro),
                                        float(diskmod.isco(M, a)), rout, "rk4", max_images, opaque,
                                        axis_refines=ar.ravel())


INTEGS = ("rk4", "dp45")


@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_no_change_of_a_step(ci, integ):
    """Thin mode: fa, n_half, status and rhs_evals of every ray are the plain tracer's, byte for byte; opaque mode: the
    same for every ray without a hit."""
    a, tho, ro, rout = CASES[ci]
    al, th, ar, _ = fans(ro, rout)
    plain = oracle.trace_batch_kerr(M, a, ro, al, th, tho, lam_max(ro), axis_refines=ar, integrator=integ)
    thin, opq = twin(ci, integ, False), twin(ci, integ, True)
    miss = opq["status"] != 2
    assert np.array_equal(miss, thin["n_hits"] == 0) and 0 < miss.sum() < miss.size
    for k, ref in zip(("fa", "winding", "status", "rhs_evals"), plain):
        assert thin[k].tobytes() == ref.tobytes(), k
        assert opq[k][miss].tobytes() == ref[miss].tobytes(), k
    # a ray the opaque disk stopped: no final angle, fewer evaluations, slot 0 of the thin run
    hit = ~miss
    assert np.all(np.isnan(opq["fa"][hit])) and np.all(opq["rhs_evals"][hit] <= thin["rhs_evals"][hit])
    assert opq["images"][hit, 0].tobytes() == thin["images"][hit, 0].tobytes()
    assert np.all(opq["n_hits"][hit] == 1) and np.all(np.isnan(opq["images"][:, 1:]))


@pytest.mark.parametrize("integ", INTEGS)
def test_primary_hits_against_the_independent_truth(integ):
    """A sample of the twin's primary hits from two cases within test_gpu_disk.py's budgets of the dense DP45 truth."""
    key = ("rk4", 64) if integ == "rk4" else ("dp45_exact", 64)
    tally = _Tally(*key)
    for ci in (0, 2):
        a, tho, ro, rout = CASES[ci]
        al, th, ar, crit = fans(ro, rout)
        tw = twin(ci, integ, False)
        hs = hit_slots(tw, 1)
        prim = np.nonzero((tw["n_hits"] > 0) & (hs["k"][:, 0] == 0) & ~crit & (ar == 0))[0]
        for i in prim[7::max(1, prim.size // 14)][:14]:
            tr = _truth(M, a, ro, tho, al[i], th[i], float(diskmod.isco(M, a)), rout)
            if tr is None or not tr["hit"] or not tr["first"]:
                continue
            tally.hit(tr, tw["images"][i, 0, 0], tw["images"][i, 0, 1], (ci, int(i)))
            g = diskmod.redshift(M, a, tw["images"][i, 0, 0], tr["xi"])
            assert abs(tw["images"][i, 0, 2] - g) <= 1e-12 * abs(g)
    assert tally.n >= 20
    tally.check()


@pytest.mark.parametrize("integ", INTEGS)
def test_a_ray_in_the_plane_never_hits(integ):
    al = np.array([0.05, 0.2, 0.3, 0.05, 0.2, 0.3])
    th = np.array([np.pi / 2] * 3 + [-np.pi / 2] * 3)
    for opaque in (False, True):
        tw = oracle.trace_batch_kerr_disk(M, 0.9, 50.0, al, th, np.pi / 2, 5000.0, float(diskmod.isco(M, 0.9)), 20.0,
                                          integ, 8, opaque)
        assert np.all(tw["n_hits"] == 0) and np.all(tw["n_cross"] == 0) and np.all(tw["status"] != 2)
        assert np.all(np.isnan(tw["images"]))


def _sym_rays(angles=range(1, 8)):
    ang = np.array(angles) * (np.pi / 8)  # strictly between 0 and pi: the mirror image is another ray
    al = np.tile(np.linspace(0.03, 0.42, 60), ang.size)
    return al, np.repeat(ang, 60)


@pytest.mark.parametrize("integ", INTEGS)
def test_schwarzschild_left_right_symmetry(integ):
    """a = 0: the fans at screen angles theta and -theta give the same r_hit."""
    al, th = _sym_rays()
    r_in = float(diskmod.isco(M, 0.0))
    p = oracle.trace_batch_kerr_disk(M, 0.0, 50.0, al, th, 1.45, 5000.0, r_in, 20.0, integ, 8, False)
    q = oracle.trace_batch_kerr_disk(M, 0.0, 50.0, al, -th, 1.45, 5000.0, r_in, 20.0, integ, 8, False)
    ok = ~(excluded(p, r_in, 20.0, BUDGET64[0], BUDGET64[2]) | excluded(q, r_in, 20.0, BUDGET64[0], BUDGET64[2]))
    assert ok.mean() > 0.95 and (p["n_hits"][ok] > 0).sum() > 60
    assert np.array_equal(p["n_hits"][ok], q["n_hits"][ok])
    hit = ok & (p["n_hits"] > 0)
    assert np.max(np.abs(p["images"][hit, 0, 0] - q["images"][hit, 0, 0])) <= 1e-9
    # phi mirrors too
    d = np.abs((p["images"][hit, 0, 1] + q["images"][hit, 0, 1]) % (2 * np.pi))
    assert np.max(np.minimum(d, 2 * np.pi - d)) <= 1e-9


def _mirror_pair(integ):
    """The twin at (theta_obs, screen angle theta) and at (pi - theta_obs, pi - theta), a = 0.9.  Without the screen
    angles +-pi/2: there p_theta is sqrt of a difference that cancels to rounding noise (~1e-7) in the reference's
    initial conditions and takes its sign from cos(theta) = 6e-17 > 0 on both sides, so those two rays are not
    each other's mirror image (their r_hit differ by ~1e-7)."""
    al, th = _sym_rays((1, 2, 3, 5, 6, 7))
    th = np.concatenate([th, -th])
    al = np.concatenate([al, al])
    a, tho = 0.9, 1.4
    r_in = float(diskmod.isco(M, a))
    p = oracle.trace_batch_kerr_disk(M, a, 50.0, al, th, tho, 5000.0, r_in, 20.0, integ, 8, False)
    q = oracle.trace_batch_kerr_disk(M, a, 50.0, al, np.pi - th, np.pi - tho, 5000.0, r_in, 20.0, integ, 8, False)
    return p, q, r_in


def test_observer_below_the_plane_mirrors_the_one_above():
    """theta_obs -> pi - theta_obs with the screen angle mirrored (theta -> pi - theta): same r_hit, same g, to 1e-9.
    RK4: its step depends on r alone, so the mirrored ray takes the mirrored steps."""
    p, q, r_in = _mirror_pair("rk4")
    ok = ~(excluded(p, r_in, 20.0, BUDGET64[0], BUDGET64[2]) | excluded(q, r_in, 20.0, BUDGET64[0], BUDGET64[2]))
    assert ok.mean() > 0.95 and (p["n_hits"][ok] > 0).sum() > 120
    assert np.array_equal(p["n_hits"][ok], q["n_hits"][ok])
    hit = ok & (p["n_hits"] > 0)
    assert np.max(np.abs(p["images"][hit, 0, 0] - q["images"][hit, 0, 0])) <= 1e-9
    assert np.max(np.abs(p["images"][hit, 0, 2] - q["images"][hit, 0, 2])) <= 1e-9


def test_observer_below_the_plane_dp45():
    """The reference's DP45 is NOT mirror symmetric: its error norm scales theta's error by |theta|, which is not
    |pi - theta|, so the mirrored ray takes other steps (the plain tracer's final angles differ by up to 4e-4).  The
    mirrored hits then agree as two DP45 runs of one geodesic do: within test_gpu_disk.py's DP45 budget of each other."""
    eps_r, eps_phi, eps_th, _ = BUDGET[("dp45_exact", 64)]
    p, q, r_in = _mirror_pair("dp45")
    ok = ~(excluded(p, r_in, 20.0, eps_r, eps_th) | excluded(q, r_in, 20.0, eps_r, eps_th))
    assert ok.mean() > 0.9 and (p["n_hits"][ok] > 0).sum() > 120
    assert np.array_equal(p["n_hits"][ok], q["n_hits"][ok])
    hs = hit_slots(p, 1)
    hit = ok & (p["n_hits"] > 0) & (hs["k"][:, 0] == 0)
    assert np.all(np.abs(p["images"][hit, 0, 0] - q["images"][hit, 0, 0]) <= 2 * (eps_r + hs["s_r"][hit, 0] * eps_th))


# ---- the fans can tell right from wrong -------------------------------------------------------------------------------
# Smallest counts per case.  Where a case cannot reach the figure every case should reach (40 / 40 / 40 / 20 / 40 / 10),
# its own row says what it does reach, and why:
#  - later: rays with an earlier plane crossing outside the annulus and a hit afterwards.  With r_out = 40 under
#    r_obs = 50 nearly every first crossing already lies inside the annulus; only rays that first cross inside r_in do
#    otherwise (4 of them).
#  - n2 / n3: rays of the critical-curve fan with two / three hits.  Higher-order crossings lie at r of a few M.  For
#    a = 0 (r_in = 6) and a = -0.7 (r_in = 8.14) the ISCO is outside most of them, so those cases see few second and no
#    third images whatever the sampling (the a = 0 case therefore checks slot 0 and little else); a = 0.998 at 83 degrees has 4 third images among its critical-curve rays.
FAN_MINIMA = {  # near r_out, near r_in, streak, later, n2, n3
    0: (40, 40, 40, 20, 40, 10),
    1: (40, 40, 40, 4, 40, 10),
    2: (40, 40, 40, 20, 40, 0),
    3: (40, 40, 40, 20, 40, 4),
    4: (40, 40, 40, 20, 2, 0),
    5: (40, 40, 40, 20, 40, 10),
}


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_fans_reach_where_kernels_go_wrong(ci):
    a, _, ro, rout = CASES[ci]
    r_in = float(diskmod.isco(M, a))
    rc4 = 4.0 * 1.01 * (M + np.sqrt(M * M - a * a))  # RK4's far-field streak runs above this radius
    _, _, _, crit = fans(ro, rout)
    tw = twin(ci, "rk4", False)
    cr = tw["cross"]
    rec, on, k = crossing_k(tw)
    hit = rec & (np.nan_to_num(cr[..., 11]) == 1.0)
    r = np.nan_to_num(cr[..., 5])
    missed = on & ~hit
    earlier_miss = (np.cumsum(missed, axis=1) - missed) > 0
    got = (int((hit & (np.abs(r - rout) <= 1.0)).sum()), int((hit & (np.abs(r - r_in) <= 0.5)).sum()),
           int((hit & (np.nan_to_num(cr[..., 3]) > rc4)).sum()), int((hit & earlier_miss).any(1).sum()),
           int((crit & (tw["n_hits"] >= 2)).sum()), int((crit & (tw["n_hits"] >= 3)).sum()))
    print(ci, got)
    assert all(g >= m for g, m in zip(got, FAN_MINIMA[ci])), (got, FAN_MINIMA[ci])
    assert tw["n_cross"].max() <= cr.shape[1]


@pytest.mark.parametrize("integ", INTEGS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_exclusions_stay_under_two_percent(ci, integ):
    a, _, ro, rout = CASES[ci]
    ex = excluded(twin(ci, integ, False), float(diskmod.isco(M, a)), rout, BUDGET64[0], BUDGET64[2])
    assert ex.mean() <= 0.02, ex.mean()


def test_frame_exclusions_stay_under_two_percent():
    a, _, ro, rout = CASES[0]
    tw = frame_twin(False, 3)
    assert tw["n_hits"].size == FRAME_W * FRAME_H and (tw["n_hits"] > 0).sum() > 500 and (tw["n_hits"] > 1).sum() > 20
    assert excluded(tw, float(diskmod.isco(M, a)), rout, BUDGET64[0], BUDGET64[2]).mean() <= 0.02


# A hit on the very step that ends the ray.  Searched for in the a = 0.998 case (r_in = 1.237 M, capture at 1.074 M): the
# case's own RK4 fan holds three rays whose capture step (h = 0.1, from r = 1.3 ... 1.4 to inside the horizon) crosses the
# plane inside the annulus before the ray reaches the capture radius.  This is the one whose first crossing it is, kept
# by name.  None was found under DP45, whose steps there are shorter.
TERMINAL_RAY = dict(a=0.998, theta_obs=1.45, r_obs=50.0, r_out=20.0, alpha=0.0595147927162206, theta=3 * np.pi / 2)


def test_a_hit_on_the_capture_step():
    c = TERMINAL_RAY
    r_in = float(diskmod.isco(M, c["a"]))
    al, th = np.array([c["alpha"]]), np.array([c["theta"]])
    plain = oracle.trace_batch_kerr(M, c["a"], c["r_obs"], al, th, c["theta_obs"], 5000.0, integrator="rk4")
    assert plain[2][0] == -1
    for opaque in (False, True):
        tw = oracle.trace_batch_kerr_disk(M, c["a"], c["r_obs"], al, th, c["theta_obs"], 5000.0, r_in, c["r_out"], "rk4",
                                          8, opaque)
        assert tw["n_cross"][0] == 1 and tw["n_hits"][0] == 1
        row = dict(zip(oracle.DISK_CROSS_FIELDS, tw["cross"][0, 0]))
        assert row["terminal"] == -1 and row["hit"] == 1 and row["on_path"] == 1 and row["t"] <= row["frac"]
        assert r_in <= row["r"] <= c["r_out"] and row["r1"] < 1.01 * (M + np.sqrt(M * M - c["a"] ** 2)) < row["r0"]
        assert tw["images"][0, 0, 0] == row["r"]
        # the hit's step is the ray's last: the opaque ray has taken every step of the plain one
        assert 4 * (row["step"] + 1) == plain[3][0] == tw["rhs_evals"][0]
        assert tw["status"][0] == (2 if opaque else -1)
    # the search itself, on the case's fan: hits on a capture step
    cr = twin(3, "rk4", False)["cross"]
    cap = (np.nan_to_num(cr[..., 9]) == -1.0) & (np.nan_to_num(cr[..., 11]) == 1.0)
    assert cap.any(1).sum() >= 3
    cr = twin(3, "dp45", False)["cross"]
    assert not ((np.nan_to_num(cr[..., 9]) == -1.0) & (np.nan_to_num(cr[..., 11]) == 1.0)).any()
