"""GPU tests of the optically thin disk (lt_render_disk_images, lt_trace_batch_kerr_disk_images).

The mode changes no step and stops no ray, so most of it is checked by identity: every non-image output is
lt_render's, slot 0 is lt_render_disk's hit, and the colour is disk.shade_images of the plain frame.  The hits
themselves are checked against ground truth independent of the kernels: each ray starts from the oracle's initial
conditions (oracle.kerr_ic), is integrated by the oracle's dense DP45 at rtol 1e-11 / atol 1e-13, and EVERY crossing
of the plane inside the annulus is found on the cubic Hermite of the dense step with the oracle's right-hand side."""
import os
import subprocess
import sys

import numpy as np
import pytest

import disk as diskmod
import ltrace
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = np.pi / 2
R_OUT = 20.0

# Slot-0 budgets, (eps_r, eps_phi, eps_theta, tail) per (integrator, precision): tests/test_gpu_disk.py's, which says
# where they come from.  A crossing point moves along the track by delta_theta / |theta'| for an error delta_theta of
# theta, so |r_hit - r_true| <= eps_r + |r' / theta'| eps_theta and likewise for phi; RK4 allows a tail of 10 % of the
# hits outside the budget (rays that pass within a few M of the hole, where the fixed step loses them) and needs a
# median |dr| below 1e-3.
BUDGET = {("rk4", 32): (3e-2, 1e-2, 1e-2, 0.10), ("rk4", 64): (3e-2, 1e-2, 1e-2, 0.10),
          ("dp45_exact", 64): (1e-3, 1e-4, 3e-4, 0.0)}
# Slot 1 of DP45-exact.  A secondary image is a ray that swung round the hole by about one more half orbit before
# it reached the disk; near the photon orbit a deviation grows by e^gamma per half orbit with the Lyapunov exponent
# gamma = pi for Schwarzschild (and no larger than that for these spins and inclinations), so slot 1's budget is
# e^pi ~ 23 times slot 0's, applied where the secondary hit is the track's second crossing of the plane (one half
# orbit after the first).  Later crossings are only counted (hit / no-hit).
E_PI = float(np.exp(np.pi))
BUDGET_SLOT1 = tuple(E_PI * x for x in BUDGET[("dp45_exact", 64)][:3]) + (0.0,)

_TRUTH = {}


def _truth(M, a, r_obs, theta_obs, alpha, theta, r_in, r_out):
    key = (M, a, r_obs, theta_obs, float(alpha), float(theta), r_in, r_out)
    if key not in _TRUTH:
        _TRUTH[key] = _truth_uncached(M, a, r_obs, theta_obs, alpha, theta, r_in, r_out)
    return _TRUTH[key]


def _truth_uncached(M, a, r_obs, theta_obs, alpha, theta, r_in, r_out):
    """The oracle's answer for one ray: dict(hits [dict(r, phi, k (index of the crossing among all plane crossings),
    s_r, s_phi)] in order along the ray, crossings [(r, s_r)] of the plane anywhere, grazes [(|theta - pi/2|, k)] at
    the turning points of theta near the annulus, k = plane crossings before it, xi = p_phi); None: no initial state."""
    ok, st5, p_t, p_phi = oracle.kerr_ic(M, a, r_obs, alpha, theta, theta_obs)
    if not ok:
        return None
    s0 = np.array([0.0, st5[0], st5[1], st5[2], p_t, st5[3], st5[4], p_phi])
    r_plus = M + np.sqrt(M * M - a * a)
    mp = 60000
    t, y, status, _ = oracle.integrate_dense(1, M, a, s0, lambda_max=max(5000.0, 6.0 * r_obs),
                                             r_stop_inner=1.01 * r_plus, r_stop_outer=2.0 * r_obs, rtol=1e-11,
                                             atol=1e-13, max_step=1.0, max_points=mp)
    assert len(t) < mp, "oracle track truncated"
    r, th = y[1], y[2]
    z = th - HALF_PI
    turn = np.nonzero(np.sign(np.diff(z[:-1])) != np.sign(np.diff(z[1:])))[0] + 1
    turn = turn[(r[turn] >= r_in - 1.0) & (r[turn] <= r_out + 1.0)]
    idx = np.nonzero(((z[:-1] < 0) & (z[1:] >= 0)) | ((z[:-1] > 0) & (z[1:] <= 0)))[0]
    grazes = [(float(abs(z[j])), int(np.searchsorted(idx, j))) for j in turn]
    hits, crossings = [], []
    for k, i in enumerate(idx):
        h = t[i + 1] - t[i]
        f0, f1 = oracle.rhs8(1, M, a, y[:, i]) * h, oracle.rhs8(1, M, a, y[:, i + 1]) * h

        def herm(c, u):
            u2, u3 = u * u, u * u * u
            return ((2 * u3 - 3 * u2 + 1) * y[c, i] + (u3 - 2 * u2 + u) * f0[c] + (-2 * u3 + 3 * u2) * y[c, i + 1]
                    + (u3 - u2) * f1[c])
        lo, hi, glo = 0.0, 1.0, z[i]
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            gm = herm(2, mid) - HALF_PI
            if (gm < 0) == (glo < 0) and gm != 0:
                lo, glo = mid, gm
            else:
                hi = mid
        u = 0.5 * (lo + hi)
        rc = herm(1, u)
        d = oracle.rhs8(1, M, a, (1 - u) * y[:, i] + u * y[:, i + 1])
        s_r, s_phi = abs(d[1] / d[2]), abs(d[3] / d[2])
        crossings.append((rc, s_r))
        if r_in <= rc <= r_out:
            hits.append(dict(r=rc, phi=herm(3, u), k=k, s_r=s_r, s_phi=s_phi))
    return dict(hits=hits, crossings=crossings, grazes=grazes, xi=p_phi)


def _count_may_differ(tr, r_in, r_out, eps_r, eps_th):
    """True if the budget lets the GPU's hit count differ from the oracle's: a crossing close enough to an edge of the
    annulus to move across it, or a turning point of theta within eps_theta of the plane near the annulus (a graze
    that the integrated track may turn into two crossings, or the reverse).  After k crossings of the plane the ray
    has swung round the hole k half orbits more than a primary one, and the budget grows by e^(pi k) (BUDGET_SLOT1)."""
    if any(zt <= eps_th * E_PI ** k for zt, k in tr["grazes"]):
        return True
    return any(min(abs(rc - r_in), abs(rc - r_out)) <= (eps_r + s_r * eps_th) * E_PI ** k
               for k, (rc, s_r) in enumerate(tr["crossings"]))


class _Tally:
    """Hits against a budget; rays outside it (and unexplained count disagreements) make up at most its tail."""

    def __init__(self, key, budget):
        self.key = key
        self.eps_r, self.eps_phi, self.eps_th, self.tail = budget
        self.n, self.dr, self.out = 0, [], []

    def hit(self, h, rh, ph, where):
        dphi = abs((ph - h["phi"] + np.pi) % (2 * np.pi) - np.pi)
        self.n += 1
        self.dr.append(abs(rh - h["r"]))
        if abs(rh - h["r"]) > self.eps_r + h["s_r"] * self.eps_th or dphi > self.eps_phi + h["s_phi"] * self.eps_th:
            self.out.append((where, float(rh), float(ph), h["r"], h["phi"], h["s_r"]))

    def disagree(self, where):
        self.n += 1
        self.out.append((where, "hit count"))

    def check(self, min_n=10):
        assert self.n >= min_n, (self.key, self.n)
        assert len(self.out) <= self.tail * self.n, (self.key, f"{len(self.out)} of {self.n} outside the budget", self.out[:4])
        if self.tail and self.dr:
            assert np.median(self.dr) <= 1e-3, (self.key, np.median(self.dr))


def _rays(r_obs, n, seed):
    """The first half over the disk image (test_gpu_disk.py's sample), the second around the critical curve (impact
    parameters 4 ... 8 M), where the higher-order images lie."""
    rng = np.random.default_rng(seed)
    amax = 1.3 * np.arctan(R_OUT / r_obs)
    al = np.concatenate([rng.uniform(0.02 * amax, amax, n - n // 2),
                         rng.uniform(np.arctan(4.0 / r_obs), np.arctan(8.0 / r_obs), n // 2)])
    return al, rng.uniform(0.0, 2 * np.pi, n)


CASES = [(0.9, 1.2), (0.9, 1.45), (-0.7, 1.2), (-0.7, 1.45), (0.0, 1.45)]


@pytest.mark.parametrize("integ,prec", [("rk4", 32), ("rk4", 64), ("dp45_exact", 64)])
@pytest.mark.parametrize("a,theta_obs", CASES)
def test_batch_hits_against_oracle(integ, prec, a, theta_obs):
    M, r_obs = 1.0, 50.0
    n = 240
    alphas, thetas = _rays(r_obs, n, seed=int(1000 * (a + 1)) + int(100 * theta_obs))
    r_in = ltrace.kerr_isco(M, a)
    d = ltrace.default_disk(r_out=R_OUT)
    out = ltrace.trace_batch_kerr_disk_images(M, a, r_obs, alphas, thetas, theta_obs, max(5000.0, 6.0 * r_obs), d,
                                              max_images=8, integrator=integ, precision=prec)
    # every non-image output is the plain batch twin's
    fa, w = np.empty(alphas.size), np.empty(alphas.size, dtype=np.int64)
    st = np.empty(alphas.size, dtype=np.int8)
    ltrace.trace_batch_kerr(M, a, r_obs, alphas, thetas, theta_obs, max(5000.0, 6.0 * r_obs), None, fa, w,
                            integrator=integ, precision=prec, out_status=st)
    assert out["fa"].tobytes() == fa.tobytes() and out["winding"].tobytes() == w.tobytes()
    assert out["status"].tobytes() == st.tobytes()
    n_hits = out["n_hits"]
    assert np.all(n_hits >= 0) and (n_hits >= 2).sum() > 10, "rays sampled near the critical curve must see a second image"
    key = (integ, prec)
    slot0 = _Tally((key, 0), BUDGET[key])
    slot1 = _Tally((key, 1), BUDGET_SLOT1)
    counts = _Tally((key, "count"), BUDGET[key])
    for i, (al, th) in enumerate(zip(alphas, thetas)):
        tr = _truth(M, a, r_obs, theta_obs, al, th, r_in, R_OUT)
        if tr is None:
            continue
        img = out["images"][i]
        k = min(int(n_hits[i]), 8)
        assert np.all(np.isnan(img[k:]))
        if k:
            assert np.all((img[:k, 1] >= 0) & (img[:k, 1] < 2 * np.pi))
            g_ref = diskmod.redshift(M, a, img[:k, 0], tr["xi"])
            np.testing.assert_allclose(img[:k, 2], g_ref, rtol=1e-6)
        hits = tr["hits"]
        if int(n_hits[i]) != len(hits):
            if not _count_may_differ(tr, r_in, R_OUT, counts.eps_r, counts.eps_th):
                counts.disagree(i)
            continue
        counts.n += 1
        # the primary image (first crossing of the plane) of the disk sample, under test_gpu_disk.py's budgets
        if hits and hits[0]["k"] == 0 and i < n - n // 2:
            slot0.hit(hits[0], img[0, 0], img[0, 1], i)
        if integ == "dp45_exact" and len(hits) > 1 and hits[0]["k"] == 0 and hits[1]["k"] == 1:
            slot1.hit(hits[1], img[1, 0], img[1, 1], i)
    slot0.check()
    counts.check()
    if integ == "dp45_exact":
        slot1.check(min_n=5)


def test_records_independent_of_max_images():
    M, a, r_obs, theta_obs = 1.0, 0.9, 50.0, 1.3
    alphas, thetas = _rays(r_obs, 4096, seed=11)
    d = ltrace.default_disk(r_out=R_OUT)
    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        outs = {m: ltrace.trace_batch_kerr_disk_images(M, a, r_obs, alphas, thetas, theta_obs, 5000.0, d, max_images=m,
                                                       integrator=integ, precision=prec) for m in (1, 3, 8)}
        n_hits = outs[8]["n_hits"]
        for m, o in outs.items():
            assert o["n_hits"].tobytes() == n_hits.tobytes()
            assert o["fa"].tobytes() == outs[8]["fa"].tobytes()
            assert o["images"].shape == (alphas.size, m, 3)
            assert o["images"].tobytes() == np.ascontiguousarray(outs[8]["images"][:, :m]).tobytes()
            for j in range(m):
                assert np.all(np.isnan(o["images"][n_hits <= j, j]))
                assert not np.any(np.isnan(o["images"][n_hits > j, j]))
        assert (n_hits > 1).sum() > 20, np.bincount(n_hits)     # n_hits > max_images = 1
        # the opaque disk stops at slot 0: the same crossing, bit for bit.  g is float64 here and comes from the same
        # formula in another kernel, where the compiler may fuse its multiply-adds differently: a few ulp (the frame
        # outputs, float32, are compared bit for bit in test_frame_identity_with_opaque_disk).
        opq = ltrace.trace_batch_kerr_disk(M, a, r_obs, alphas, thetas, theta_obs, 5000.0, d, integrator=integ,
                                           precision=prec)
        assert np.array_equal(opq["status"] == ltrace.STATUS_DISK, n_hits > 0)
        on = n_hits > 0
        assert opq["disk"][on, :2].tobytes() == np.ascontiguousarray(outs[1]["images"][on, 0, :2]).tobytes()
        g0, g1 = opq["disk"][on, 2], outs[1]["images"][on, 0, 2]
        assert np.all(np.abs(g0 - g1) <= 4 * np.spacing(g0))


# ---- frames ------------------------------------------------------------------------------------------------------
def _frame_setup(W, H):
    fov = np.radians(40.0)
    hfov = 2 * np.arctan(np.tan(fov / 2) * W / H)
    cam = ltrace.Camera(W, H, hfov, fov, 0.0, 0.0, 50.0, 1.4)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    rng = np.random.default_rng(W * 7 + H)
    bg = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8).astype(np.float32) / 255.0
    return cam, met, bg


_FRAMES = {}


def _frames(W, H, integ, prec):
    key = (W, H, integ, prec)
    if key not in _FRAMES:
        cam, met, bg = _frame_setup(W, H)
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        plain = ltrace.render(cam, met, o, background=bg)
        opaque = ltrace.render_disk(cam, met, o, ltrace.default_disk(), background=bg)
        thin = ltrace.render_disk_images(cam, met, o, ltrace.default_disk(), max_images=3, background=bg)
        _FRAMES[key] = (cam, met, bg, plain, opaque, thin)
    return _FRAMES[key]


FRAME_CASES = [(W, H, i, p) for W, H in ((256, 256), (320, 192)) for i, p in (("rk4", 32), ("rk4", 64), ("dp45_exact", 64))]
STAT_KEYS = ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid")


@pytest.mark.parametrize("W,H,integ,prec", FRAME_CASES)
def test_frame_identity_with_render(W, H, integ, prec):
    cam, met, bg, plain, opaque, thin = _frames(W, H, integ, prec)
    for k in ("fa", "winding", "status", "steps"):
        assert np.asarray(plain[k]).tobytes() == np.asarray(thin[k]).tobytes(), k
    none = thin["n_hits"] == 0
    assert 0 < none.sum() < none.size
    for k in ("rgb", "rgba"):
        assert np.asarray(plain[k])[none].tobytes() == np.asarray(thin[k])[none].tobytes(), k
    for k in STAT_KEYS:
        assert plain["stats"][k] == thin["stats"][k], k
    assert thin["stats"]["disk"] == int((thin["n_hits"] > 0).sum())
    assert thin["stats"]["disk_hits"] == int(thin["n_hits"].astype(np.int64).sum())


@pytest.mark.parametrize("W,H,integ,prec", FRAME_CASES)
def test_frame_identity_with_opaque_disk(W, H, integ, prec):
    cam, met, bg, plain, opaque, thin = _frames(W, H, integ, prec)
    on = opaque["status"] == ltrace.STATUS_DISK
    assert on.sum() > 100
    assert np.array_equal(thin["n_hits"] >= 1, on)
    assert thin["images"][on, 0].tobytes() == np.ascontiguousarray(opaque["disk"][on]).tobytes()
    assert (thin["n_hits"] >= 2).sum() > 0, "the frame must show a higher-order image"


@pytest.mark.parametrize("W,H,integ,prec", FRAME_CASES)
def test_frame_colour(W, H, integ, prec):
    cam, met, bg, plain, opaque, thin = _frames(W, H, integ, prec)
    r_in = ltrace.kerr_isco(1.0, 0.9)
    ref = diskmod.shade_images(plain["rgb"], thin["images"], thin["n_hits"], r_in)
    got = thin["rgb"]
    ulp = np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)))
    assert np.all(np.abs(got - ref) <= 2 * ulp)
    ref8 = (ref * np.float32(255.0)).astype(np.uint8)
    assert np.all(np.abs(thin["rgba"][..., :3].astype(int) - ref8.astype(int)) <= 1)
    assert np.all(thin["rgba"][..., 3] == 255)


def test_frame_without_background_and_gray():
    """No background: base 0, so the frame is the disk's light alone.  A 1-channel background: the mean of each E_j."""
    W, H = 192, 128
    cam, met, bg = _frame_setup(W, H)
    o = ltrace.default_opts(integrator="rk4", precision=32, tb_symmetry=0)
    r_in = ltrace.kerr_isco(1.0, 0.9)
    dark = ltrace.render_disk_images(cam, met, o, ltrace.default_disk(), max_images=3)
    assert np.all(dark["rgb"][dark["n_hits"] == 0] == 0.0)
    ref = diskmod.shade_images(np.zeros((H, W, 3), np.float32), dark["images"], dark["n_hits"], r_in)
    assert np.all(np.abs(dark["rgb"] - ref) <= 2 * np.spacing(np.maximum(ref, np.float32(1e-30))))
    gray = bg.mean(axis=2).astype(np.float32)
    plain = ltrace.render(cam, met, o, background=gray)
    thin = ltrace.render_disk_images(cam, met, o, ltrace.default_disk(), max_images=3, background=gray)
    assert thin["rgb"].shape == (H, W)
    ref = diskmod.shade_images(plain["rgb"], thin["images"], thin["n_hits"], r_in, channels=1)
    assert np.all(np.abs(thin["rgb"] - ref) <= 2 * np.spacing(np.maximum(ref, np.float32(1e-30))))


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{root!r}, {pkg!r}]
import ltrace
rng = np.random.default_rng(3)
al = np.concatenate([rng.uniform(0.01, 0.5, 6000), rng.uniform(np.arctan(4.0 / 50.0), np.arctan(8.0 / 50.0), 6000)])
th = rng.uniform(0.0, 2 * np.pi, al.size)
res = {{}}
for integ, prec in (("rk4", 32), ("rk4", 64)):
    o = ltrace.trace_batch_kerr_disk_images(1.0, 0.9, 50.0, al, th, 1.3, 5000.0, ltrace.default_disk(), max_images=3,
                                            integrator=integ, precision=prec)
    for k in ("images", "n_hits", "fa", "status"):
        res[f"{{integ}}{{prec}}_{{k}}"] = o[k]
np.savez({out!r}, **res)
"""


def test_ghost_lanes_change_no_record(tmp_path):
    """LT_D_LONG=8 sends nearly every RK4 wavefront through the ghost-lane phase, whose twin lanes must not write
    records or counts: the batch results are byte-identical to a default run's (each in a fresh process)."""
    res = {}
    for name, env in (("default", {}), ("ghost", {"LT_D_LONG": "8"})):
        out = str(tmp_path / f"{name}.npz")
        code = _CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "light-path-tracer_amd"), out=out)
        e = dict(os.environ)
        e.pop("LT_D_LONG", None)
        e.update(env)
        subprocess.run([sys.executable, "-c", code], env=e, check=True, timeout=600)
        res[name] = np.load(out)
    for k in res["default"].files:
        assert res["default"][k].tobytes() == res["ghost"][k].tobytes(), k
    assert (res["default"]["rk432_n_hits"] >= 2).sum() > 50


def _upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(d.ptr, a.ctypes.data, a.nbytes, 1), "hipMemcpy H2D")
    return d


def test_frame_partitions_reassemble():
    """Three partitions through a block_owner table, rendered by lt_render_disk_images_dev into one device buffer per
    output, un-permuted by lt_scatter_rows_indexed_dev: byte-identical to the single frame."""
    import hipmini
    W, H = 256, 256
    cam, met, bg, plain, opaque, thin = _frames(W, H, "rk4", 32)
    row_block = 16
    nb = (H + row_block - 1) // row_block
    owner = np.array([(b * 5 + 2) % 3 for b in range(nb)], dtype=np.uint16)
    kinds = {"fa": (np.float32, ()), "winding": (np.uint16, ()), "status": (np.int8, ()), "steps": (np.uint32, ()),
             "images": (np.float32, (3, 3)), "n_hits": (np.uint8, ()), "rgb": (np.float32, (3,)),
             "rgba": (np.uint8, (4,))}
    recv = {k: hipmini.DeviceArray((H, W) + sh, dt) for k, (dt, sh) in kinds.items()}
    d_bg = _upload(bg)
    stats = _upload(np.zeros(ltrace.STAT_WORDS, dtype=np.uint64))
    index, row0 = [], 0
    for p in range(3):
        o = ltrace.default_opts(integrator="rk4", precision=32, tb_symmetry=0, n_parts=3, part=p, row_block=row_block,
                                block_owner=owner)
        rows = ltrace.owned_rows(H, row_block, owner, p)
        at = {k: recv[k].ptr + row0 * W * int(np.prod(sh, dtype=np.int64)) * np.dtype(dt).itemsize
              for k, (dt, sh) in kinds.items()}
        ltrace.render_disk_images_dev(cam, met, o, ltrace.default_disk(), max_images=3, d_bg=d_bg.ptr, bg_channels=3,
                                      d_fa=at["fa"], d_w=at["winding"], d_status=at["status"], d_steps=at["steps"],
                                      d_images=at["images"], d_n_hits=at["n_hits"], d_rgb=at["rgb"], d_rgba=at["rgba"],
                                      d_stats=stats.ptr)
        index.append(rows)
        row0 += rows.size
    hipmini.device_synchronize()
    assert row0 == H
    idx = _upload(np.concatenate(index).astype(np.int64))
    for k, (dt, sh) in kinds.items():
        full = hipmini.DeviceArray((H, W) + sh, dt)
        row_bytes = W * int(np.prod(sh, dtype=np.int64)) * np.dtype(dt).itemsize
        ltrace.scatter_rows_indexed_dev(recv[k].ptr, full.ptr, idx.ptr, H, H, row_bytes)
        hipmini.device_synchronize()
        assert full.get().tobytes() == np.ascontiguousarray(thin[k]).tobytes(), k
    st = stats.get()
    assert int(st[ltrace.STAT_DISK]) == thin["stats"]["disk"] and int(st[ltrace.STAT_RAYS]) == W * H
    assert int(st[ltrace.STAT_DISK_HITS]) == thin["stats"]["disk_hits"]


def test_refusals():
    cam = ltrace.Camera(16, 16, 0.5, 0.5, 0.0, 0.0, 50.0, 1.4)
    kerr = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    o = ltrace.default_opts()
    d = ltrace.default_disk()
    al, th = np.array([0.1]), np.array([0.0])
    for m in (0, 9, -1):
        with pytest.raises(ltrace.LtraceError) as e:
            ltrace.render_disk_images(cam, kerr, o, d, max_images=m)
        assert e.value.code == ltrace.ERR_INVALID_ARG
        with pytest.raises(ltrace.LtraceError) as e:
            ltrace.trace_batch_kerr_disk_images(1.0, 0.9, 50.0, al, th, 1.4, 5000.0, d, max_images=m)
        assert e.value.code == ltrace.ERR_INVALID_ARG
    isco = ltrace.kerr_isco(1.0, 0.9)
    for bad in (ltrace.default_disk(r_in=isco - 0.1), ltrace.default_disk(r_out=80.0)):
        with pytest.raises(ltrace.LtraceError) as e:
            ltrace.render_disk_images(cam, kerr, o, bad)
        assert e.value.code == ltrace.ERR_INVALID_ARG
        with pytest.raises(ltrace.LtraceError) as e:
            ltrace.trace_batch_kerr_disk_images(1.0, 0.9, 50.0, al, th, 1.4, 5000.0, bad)
        assert e.value.code == ltrace.ERR_INVALID_ARG
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    with pytest.raises(ltrace.LtraceError) as e:
        ltrace.render_disk_images(cam, schw, o, d)
    assert e.value.code == ltrace.ERR_UNSUPPORTED
    with pytest.raises(ltrace.LtraceError) as e:
        ltrace.render_disk_images(cam, kerr, ltrace.default_opts(schedule="queue"), d)
    assert e.value.code == ltrace.ERR_UNSUPPORTED


def test_cli_writes_png(tmp_path):
    import matplotlib.image as mpimg
    import image_lens
    from metrics import Kerr
    png = tmp_path / "thin.png"
    cmd = [sys.executable, os.path.join(ROOT, "light-path-tracer_amd", "image_lens.py"), "--a", "0.9",
           "--disk-images", "3", "--theta-obs", "80", "--synthetic", "256", "256", "--output", str(png)]
    subprocess.run(cmd, check=True, cwd=str(tmp_path), timeout=600)
    img8 = np.rint(mpimg.imread(str(png)) * 255.0).astype(np.uint8)
    vfov = np.radians(40.0)
    src = image_lens.synthetic_background(256, 256)
    out = image_lens.render_frame(src, Kerr(1.0, 0.9), 100.0, (vfov, vfov), theta_obs=np.radians(80.0),
                                  disk=diskmod.TransparentDisk(), want=("status", "rgba"))
    assert out["disk_images"].shape == (256, 256, 3, 3)
    assert (out["disk_hits"] >= 2).sum() > 0
    on = out["disk_hits"] > 0
    assert on.sum() > 100
    assert np.array_equal(img8[on][:, :3], out["rgba"][on][:, :3])
