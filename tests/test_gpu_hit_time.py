"""GPU tests of the hit times and the hot spot (lt_trace_disk_hits, lt_trace_batch_kerr_disk_hits, lt_step_time_probe,
lt_shade_hotspot, lt_hotspot_lightcurve).

Identity: the timed trace takes lt_render_disk_images' steps, so everything the two share is equal bit for bit.  The
device's step rule is held to disk.step_time; the stored times to the oracle's dense truth (tests/test_hit_time_rule.py
builds the tracks) within a budget in the model of tests/test_gpu_disk.py: a hit whose position along the track is off
by the integrator's r budget is off in time by |t' / r'| times that, times e^(pi k) behind k plane crossings.

MEASURED on the MI355X (build 7351b710453e; profiles/hit_time_7351b710453e.json):
    step rule, float32 against disk.step_time, 8 742 steps, tau = 1 and random: largest relative difference 1.04e-5
        (float64: within 1e-12);
    stored times against the dense truth, 224 rays per spin (1 / 1 / 3 excluded), slot 0 and slot 1, DP45-exact and
        RK4 float64 alike: every error inside the position term |t'/r'| (eps_r + |r'/theta'| eps_theta) e^(pi k) of the
        integrator's own r budget, so nothing is left for eps_t: eps_t = 0, no RK4 ray in its tail allowance;
        raw |dt - dt_true| median 1.7e-4 ... 2.0e-4 / max 7.9e-3 (DP45-exact), median 7e-6 ... 4.8e-5 / max 0.12 (RK4);
    RK4 float32 against float64, slot 0, (median, p99) of |dt|: (8.8e-6, 3.4e-5) a = 0, (1.2e-5, 6.9e-5) a = 0.9,
        (1.1e-5, 4.8e-5) a = -0.7 -- of light-travel times of 30 ... 200 M;
    the frame path in float64 (test_frame_times_against_the_truth), 149 of 150 sampled pixels, 149 slot-0 and 13 slot-1
        times: none outside the bound; raw |dt - dt_true| median 4.6e-5 / max 0.17 (RK4), median 1.3e-4 / max 3.0e-3
        (DP45-exact).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import disk as diskmod
import ltrace
from oracle import oracle
from test_hit_time_rule import M, R_OBS, SPINS, THETA_OBS, pairs, tracks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PI = np.pi / 2
E_PI = float(np.exp(np.pi))
# the fan rays and cases of tests/test_gpu_disk_twin.py (its generator restated): (a, theta_obs, r_obs, r_out)
CASES = [(0.9, 1.4, 50.0, 20.0),
         (0.9, 1.4, 50.0, 40.0),   # an outer edge deep in RK4's streak region: where turning the streak off could show
         (-0.7, 1.2, 50.0, 20.0)]
CASE_IDS = [f"a{a:g}-th{t:.3g}-r{r:g}-out{o:g}" for a, t, r, o in CASES]
CONFIGS = [("rk4", 32), ("rk4", 64), ("dp45_exact", 64)]
CONFIG_IDS = [f"{i}-{p}" for i, p in CONFIGS]
FRAME_W, FRAME_H = 96, 80
# (eps_r, eps_theta, tail) of tests/test_gpu_disk.py's BUDGET, DESIGN.md 10b
R_BUDGET = {"rk4": (3e-2, 1e-2, 0.10), "dp45_exact": (1e-3, 3e-4, 0.0)}
# Measured (header), asserted at the stated multiple.
EPS_T = {"dp45_exact": 0.0, "rk4": 0.0}   # x 10
PROBE32_REL = 1.05e-5                                              # x 4
Q32 = [(8.8e-6, 3.4e-5), (1.24e-5, 6.92e-5), (1.09e-5, 4.84e-5)]                                                          # per spin (median, p99) of |dt32 - dt64|, x 4
MEASURE = os.environ.get("LT_HIT_TIME_MEASURE")  # a path: the figures the tests print are also written there as JSON


def lam_max(r_obs):
    return max(5000.0, 6.0 * r_obs)


def fans(r_obs, r_out):
    """Per screen angle (16, evenly spaced from 0): 128 alphas over the disk's image and 64 impact parameters r_obs
    tan(alpha) from 4 to 8 around the critical curve; the fans of two of the angles once more as axis-refine rays."""
    ang = np.arange(16) * (2 * np.pi / 16)
    amax = 1.3 * np.arctan(r_out / r_obs)
    one = np.concatenate([np.linspace(0.02 * amax, amax, 128), np.arctan(np.linspace(4.0, 8.0, 64) / r_obs)])
    al, th = np.tile(one, 16), np.repeat(ang, one.size)
    extra = np.isin(th, ang[[1, 10]])
    ar = np.concatenate([np.zeros(al.size, np.uint8), np.ones(int(extra.sum()), np.uint8)])
    return np.concatenate([al, al[extra]]), np.concatenate([th, th[extra]]), ar


def frame_fov():
    vfov = np.radians(40.0)
    return 2 * np.arctan(np.tan(vfov / 2) * FRAME_W / FRAME_H), vfov


def frame_setup(integ="rk4", prec=32, **kw):
    a, tho, ro, rout = CASES[0]
    hfov, vfov = frame_fov()
    cam = ltrace.Camera(FRAME_W, FRAME_H, hfov, vfov, 0.0, 0.0, ro, tho)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    return cam, met, ltrace.default_opts(integrator=integ, precision=prec, **kw), ltrace.default_disk(r_out=rout)


_FRAME = {}


def frame_hits(integ="rk4", prec=32):
    """The 96 x 80 frame of the first case, 3 images, per configuration (default RK4 float32): the timed trace's outputs,
    cached and left unchanged."""
    if (integ, prec) not in _FRAME:
        cam, met, o, d = frame_setup(integ, prec)
        _FRAME[integ, prec] = ltrace.trace_disk_hits(cam, met, o, d, max_images=3)
    return _FRAME[integ, prec]


_RECORD = {}


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


# ---- identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
def test_batch_identity(ci, integ, prec):
    a, tho, ro, rout = CASES[ci]
    al, th, ar = fans(ro, rout)
    d = ltrace.default_disk(r_out=rout)
    args = (M, a, ro, al, th, tho, lam_max(ro), d)
    kw = dict(max_images=4, axis_refines=ar, integrator=integ, precision=prec)
    ref, got = ltrace.trace_batch_kerr_disk_images(*args, **kw), ltrace.trace_batch_kerr_disk_hits(*args, **kw)
    assert (ref["n_hits"] > 0).sum() > 1000 and (ref["n_hits"] > 1).sum() > 40
    assert np.ascontiguousarray(got["hits"][..., :3]).tobytes() == ref["images"].tobytes()
    for k in ("n_hits", "fa", "winding", "status", "rhs_evals"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    dt = got["hits"][..., 3]
    stored = np.arange(4)[None, :] < ref["n_hits"][:, None]
    assert np.array_equal(np.isnan(dt), ~stored)
    # light needs at least the straight-line time to the disk's outer edge, and later hits are later
    assert np.all(dt[stored] > ro - rout) and np.all(dt[stored] < 20 * ro)
    two = ref["n_hits"] > 1
    assert np.all(dt[two, 1] > dt[two, 0])


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_frame_identity(integ, prec):
    cam, met, o, d = frame_setup(integ, prec)
    ref = ltrace.render_disk_images(cam, met, o, d, max_images=3)
    got = frame_hits(integ, prec)
    assert np.ascontiguousarray(got["hits"][..., :3]).tobytes() == ref["images"].tobytes()
    for k in ("n_hits", "fa", "winding", "status", "steps"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    for k in ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "disk", "disk_hits"):
        assert got["stats"][k] == ref["stats"][k], k
    assert ref["stats"]["disk_hits"] > 1000


_DUMP = """
import sys
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
import numpy as np, ltrace
from test_gpu_hit_time import frame_setup
cam, met, o, d = frame_setup(sys.argv[2], int(sys.argv[3]))
out = ltrace.trace_disk_hits(cam, met, o, d, max_images=3)
np.savez(sys.argv[1], **{{k: np.asarray(v) for k, v in out.items() if k != "stats"}})
"""


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_ghost_phase_changes_nothing(tmp_path, integ, prec):
    """LT_D_LONG=8 (read once per process, so a child): every long wave spends its steps in the ghost-lane phase; the
    records, times included, are the default's byte for byte."""
    path = str(tmp_path / "ghost.npz")
    src = _DUMP.format(pkg=os.path.join(ROOT, "light-path-tracer_amd"), root=ROOT, tests=os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", src, path, integ, str(prec)], check=True, env=dict(os.environ, LT_D_LONG="8"), timeout=120)
    got, ref = np.load(path), frame_hits(integ, prec)
    for k in ("hits", "n_hits", "fa", "winding", "status", "steps"):
        assert got[k].tobytes() == np.asarray(ref[k]).tobytes(), k


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_partitions_reassemble(integ, prec):
    whole = frame_hits(integ, prec)
    full = {k: np.empty_like(np.asarray(whole[k])) for k in ("hits", "n_hits", "fa", "status")}
    for part in range(3):
        cam, met, o, d = frame_setup(integ, prec, n_parts=3, part=part, row_block=16)
        out = ltrace.trace_disk_hits(cam, met, o, d, max_images=3)
        rows = ltrace.global_rows(FRAME_H, 16, 3, part)
        for k in full:
            full[k][rows] = out[k]
    for k in full:
        assert full[k].tobytes() == np.asarray(whole[k]).tobytes(), k


# ---- the device's step rule -------------------------------------------------------------------------------------------
def test_step_rule_probe():
    """~4 000 consecutive-point pairs of the CPU test's tracks, tau = 1 and random, against disk.step_time: float64 to
    1e-12 relative, float32 to 4 x the measured largest relative difference."""
    rng = np.random.default_rng(11)
    worst32 = 0.0
    n = 0
    for a in SPINS:
        met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
        L, y0, y1, h = [], [], [], []
        for tr in tracks(a)[::3]:
            l, p0, p1, hh, _ = pairs(tr)
            keep = rng.random(hh.size) < 0.2
            L.append(np.full(keep.sum(), l)); y0.append(p0[keep]); y1.append(p1[keep]); h.append(hh[keep])
        L, y0, y1, h = np.concatenate(L), np.concatenate(y0), np.concatenate(y1), np.concatenate(h)
        n += h.size
        for tau in (np.ones(h.size), rng.uniform(0.02, 0.98, h.size)):
            ref = diskmod.step_time(M, a, L, y0, y1, h, tau)
            d64 = ltrace.step_time_probe(met, L, y0, y1, h, tau, precision=64)
            assert np.max(np.abs(d64 - ref) / np.abs(ref)) <= 1e-12
            d32 = ltrace.step_time_probe(met, L, y0, y1, h, tau, precision=32)
            worst32 = max(worst32, float(np.max(np.abs(d32 - ref) / np.abs(ref))))
    assert 3000 <= n <= 6000
    print(f"step rule, float32 against disk.step_time: largest relative difference {worst32:.3e} over {2 * n} steps")
    record("probe32_rel", worst32)
    assert worst32 <= 4 * PROBE32_REL


# ---- the stored times against the truth ---------------------------------------------------------------------------------
_TRUTH = {}


def fan():
    """Deterministic rays for the comparison with the truth: 8 screen angles x (26 alphas over the disk's image + 2 impact
    parameters between the critical curve and the direct image's inner edge) = 224 rays."""
    ang = 0.2 + np.arange(8) * (2 * np.pi / 8)
    amax = 1.3 * np.arctan(20.0 / R_OBS)
    one = np.concatenate([np.linspace(0.05 * amax, amax, 26), np.arctan(np.array([5.6, 6.4]) / R_OBS)])
    return np.tile(one, ang.size), np.repeat(ang, one.size)


def truth(a, rays=None):
    """Per ray of `rays` (alphas, screen angles; default fan()) (r_in = ISCO, r_out = 20; the dense tracks as tests/test_hit_time_rule.py builds them): the
    annulus crossings of the dense track in order, as (k, r, t, |r'/theta'|, |t'/r'|) with k the plane crossings before it; every plane crossing's (r, |r'/theta'|,
    k); graze, the closest approach to the plane at a turning point of theta near the annulus."""
    key = (a, None if rays is None else tuple(np.concatenate(rays)))
    if key in _TRUTH:
        return _TRUTH[key]
    r_in, r_out = float(diskmod.isco(M, a)), 20.0
    out = []
    for tr in tracks(a, fan() if rays is None else rays):
        lam, y = tr["lam"], tr["y"]
        z = y[2] - HALF_PI
        turn = np.nonzero(np.sign(np.diff(z[:-1])) != np.sign(np.diff(z[1:])))[0] + 1
        turn = turn[(y[1][turn] >= r_in - 1.0) & (y[1][turn] <= r_out + 1.0)]
        graze = float(np.min(np.abs(z[turn]))) if turn.size else np.inf
        hits, planes = [], []
        for k, i in enumerate(np.nonzero(((z[:-1] < 0) & (z[1:] >= 0)) | ((z[:-1] > 0) & (z[1:] <= 0)))[0]):
            h = lam[i + 1] - lam[i]
            f0, f1 = oracle.rhs8(1, M, a, y[:, i]) * h, oracle.rhs8(1, M, a, y[:, i + 1]) * h
            herm = lambda c, u: diskmod._hermite(y[c, i], f0[c], y[c, i + 1], f1[c], u)
            lo, hi, glo = 0.0, 1.0, z[i]
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                gm = herm(2, mid) - HALF_PI
                if (gm < 0) == (glo < 0) and gm != 0:
                    lo, glo = mid, gm
                else:
                    hi = mid
            u = 0.5 * (lo + hi)
            d = oracle.rhs8(1, M, a, (1 - u) * y[:, i] + u * y[:, i + 1])
            rc, s_r = herm(1, u), abs(d[1] / d[2])
            planes.append((rc, s_r, k))
            if r_in <= rc <= r_out:
                hits.append((k, rc, abs(herm(0, u)), s_r, abs(d[0] / d[1])))
        out.append(dict(ray=tr["ray"], hits=hits, planes=planes, graze=graze))
    _TRUTH[key] = out
    return out


def may_differ(t, r_in, r_out, eps_r, eps_th):
    """tests/test_gpu_disk.py's _may_differ, from the truth alone: a graze, or a plane crossing within the r budget of an
    edge of the annulus."""
    if t["graze"] <= eps_th:
        return True
    return any(min(abs(rc - r_in), abs(rc - r_out)) <= (eps_r + s_r * eps_th) * E_PI ** k for rc, s_r, k in t["planes"])


def gpu_times(a, integ, prec):
    al, th = fan()
    return ltrace.trace_batch_kerr_disk_hits(M, a, R_OBS, al, th, THETA_OBS, lam_max(R_OBS), ltrace.default_disk(r_out=20.0),
                                             max_images=2, integrator=integ, precision=prec)


@pytest.mark.parametrize("integ", ("dp45_exact", "rk4"))
@pytest.mark.parametrize("a", SPINS)
def test_times_against_the_truth(a, integ):
    """Slot 0, and slot 1 where it exists: |dt_gpu - dt_true| <= (eps_t + |t'/r'| (eps_r + |r'/theta'| eps_theta)) e^(pi k)."""
    eps_r, eps_th, tail = R_BUDGET[integ]
    r_in = float(diskmod.isco(M, a))
    tr = truth(a)
    # Exclusions are decided by the truth alone, before any GPU value is read, and are at most 2 % of the case.  RK4's own
    # r budget would put 3 ... 5 % of these rays within reach of an edge (12 % with the e^(pi k) growth), so both
    # integrators exclude by DP45's margins, and an RK4 ray that lands on the other side of an edge counts into RK4's
    # 10 % tail allowance with the rays of its primary-image tail.
    keep = [t for t in tr if not may_differ(t, r_in, 20.0, *R_BUDGET["dp45_exact"][:2])]
    assert len(keep) >= 0.98 * len(tr), (len(keep), len(tr))
    out = gpu_times(a, integ, 64)
    n, outside, resid, raw, slots = 0, 0, [], [], [0, 0]
    for t in keep:
        i = t["ray"]
        if min(out["n_hits"][i], 2) != min(len(t["hits"]), 2):
            n += 1
            outside += 1
            continue
        for j, (k, rc, tt, s_r, t_r) in enumerate(t["hits"][:2]):
            model = t_r * (eps_r + s_r * eps_th)
            err = abs(out["hits"][i, j, 3] - tt)
            n += 1
            slots[j] += 1
            resid.append(max(err / E_PI ** k - model, 0.0))
            raw.append(err)
            if err > (10 * EPS_T[integ] + model) * E_PI ** k:
                outside += 1
    resid = np.array(resid)
    print(f"a {a} {integ}: {slots[0]} slot-0 and {slots[1]} slot-1 times, {len(tr) - len(keep)} rays excluded; error beyond the "
          f"position model: max {resid.max():.3e}, p90 {np.quantile(resid, 0.9):.3e}; outside {outside} of {n}")
    print(f"    raw |dt_gpu - dt_true|: median {np.median(raw):.3e}, max {np.max(raw):.3e}")
    record(f"eps_t/{integ}/a{a:g}", dict(raw_median=np.median(raw), raw_max=np.max(raw), max=resid.max(), p90=np.quantile(resid, 0.9), slot0=slots[0], slot1=slots[1],
                                         outside=outside, n=n))
    assert slots[0] >= 25
    assert outside <= tail * n, (outside, n)


FRAME_SAMPLE, FRAME_SAMPLE_POOL = 150, 1536


def frame_truth():
    """The frame's sample for the comparison with the truth, from the truth alone: the pixels of the 96 x 80 frame in a
    seeded random order, the first FRAME_SAMPLE_POOL of them traced by the oracle from oracle.pixel_angles' rays, and of
    those whose dense track crosses the annulus at least once the first FRAME_SAMPLE.  -> [(row, column, truth() entry)]."""
    a = CASES[0][0]
    al, th, _ = oracle.pixel_angles(FRAME_H, FRAME_W, *frame_fov())
    order = np.random.default_rng(17).permutation(FRAME_W * FRAME_H)[:FRAME_SAMPLE_POOL]
    rays = (al.ravel()[order].astype(np.float64), th.ravel()[order])
    with_hit = [(int(order[t["ray"]] // FRAME_W), int(order[t["ray"]] % FRAME_W), t) for t in truth(a, rays) if t["hits"]]
    assert len(with_hit) >= FRAME_SAMPLE, len(with_hit)
    return with_hit[:FRAME_SAMPLE]


def frame_sample_kept():
    """frame_truth() without the rays that may_differ() excludes by DP45's margins; the cap of 2 % is a condition of the
    test (tests/test_hit_time_rule.py checks it without a GPU)."""
    a = CASES[0][0]
    sample = frame_truth()
    keep = [s for s in sample if not may_differ(s[2], float(diskmod.isco(M, a)), CASES[0][3], *R_BUDGET["dp45_exact"][:2])]
    assert len(keep) >= 0.98 * len(sample), (len(keep), len(sample))
    return sample, keep


@pytest.mark.parametrize("integ", ("rk4", "dp45_exact"))
def test_frame_times_against_the_truth(integ):
    """test_times_against_the_truth for the frame path in float64 (lt_trace_disk_hits, k_epilogue_disk_hits<double>), after
    tests/test_gpu_disk.py::test_frame_disk_pixels: 150 sampled pixels, slot 0 and slot 1 where present,
    |dt_gpu - dt_true| <= (10 eps_t + |t'/r'| (eps_r + |r'/theta'| eps_theta)) e^(pi k) + spacing(float32(dt_true)), the
    last because a frame stores the time in float32."""
    eps_r, eps_th, tail = R_BUDGET[integ]
    sample, keep = frame_sample_kept()      # decided before any GPU value is read
    out = frame_hits(integ, 64)
    n, outside, raw, slots = 0, 0, [], [0, 0]
    for iy, ix, t in keep:
        if min(out["n_hits"][iy, ix], 2) != min(len(t["hits"]), 2):
            n += 1
            outside += 1
            continue
        for j, (k, rc, tt, s_r, t_r) in enumerate(t["hits"][:2]):
            err = abs(float(out["hits"][iy, ix, j, 3]) - tt)
            n += 1
            slots[j] += 1
            raw.append(err)
            if not err <= (10 * EPS_T[integ] + t_r * (eps_r + s_r * eps_th)) * E_PI ** k + float(np.spacing(np.float32(tt))):
                outside += 1
    print(f"frame, a {CASES[0][0]} {integ}: {slots[0]} slot-0 and {slots[1]} slot-1 times, {len(sample) - len(keep)} pixels excluded; "
          f"outside {outside} of {n}; raw |dt_gpu - dt_true|: median {np.median(raw):.3e}, max {np.max(raw):.3e}")
    record(f"frame_times/{integ}", dict(raw_median=np.median(raw), raw_max=np.max(raw), slot0=slots[0], slot1=slots[1], outside=outside, n=n,
                                        excluded=len(sample) - len(keep)))
    assert slots[0] >= 100
    assert outside <= tail * n, (outside, n)


@pytest.mark.parametrize("si", range(len(SPINS)))
def test_float32_times(si):
    """RK4 float32 against RK4 float64 on the rays where both store the same hits: median and p99 of slot 0's |dt|."""
    a = SPINS[si]
    o32, o64 = gpu_times(a, "rk4", 32), gpu_times(a, "rk4", 64)
    same = (o32["n_hits"] == o64["n_hits"]) & (o64["n_hits"] > 0)
    assert same.sum() >= 25
    d = np.abs(o32["hits"][same, 0, 3] - o64["hits"][same, 0, 3])
    med, p99 = float(np.median(d)), float(np.quantile(d, 0.99))
    print(f"a {a}: float32 - float64 slot-0 times over {same.sum()} rays: median {med:.3e}, p99 {p99:.3e}")
    record(f"q32/a{a:g}", (med, p99))
    assert med <= 4 * Q32[si][0] and p99 <= 4 * Q32[si][1]


# ---- symmetry, RK4 float64 ------------------------------------------------------------------------------------------------
def _sym_rays(angles=(1, 2, 3, 4, 5, 6, 7)):
    ang = np.array(angles) * (np.pi / 8)
    return np.tile(np.linspace(0.03, 0.42, 60), ang.size), np.repeat(ang, 60)


def _times(a, al, th, tho):
    return ltrace.trace_batch_kerr_disk_hits(M, a, 50.0, al, th, tho, 5000.0, ltrace.default_disk(r_out=20.0), max_images=2,
                                             integrator="rk4", precision=64)


def _same_times(p, q):
    both = (p["n_hits"] == q["n_hits"]) & (p["n_hits"] > 0)
    # (a ray whose mirror image counts other hits sits on an edge of the annulus to rounding: at most a few)
    assert both.sum() >= 0.97 * (p["n_hits"] > 0).sum() and both.sum() > 60
    assert np.max(np.abs(p["hits"][both, 0, 3] - q["hits"][both, 0, 3])) <= 1e-9


def test_schwarzschild_left_right_symmetry():
    al, th = _sym_rays()
    _same_times(_times(0.0, al, th, 1.45), _times(0.0, al, -th, 1.45))


def test_observer_below_the_plane():
    """theta_obs -> pi - theta_obs with the screen angle mirrored; without the screen angles +-pi/2, which
    tests/test_oracle_disk.py names as ill-conditioned."""
    al, th = _sym_rays((1, 2, 3, 5, 6, 7))
    al, th = np.concatenate([al, al]), np.concatenate([th, -th])
    _same_times(_times(0.9, al, th, 1.4), _times(0.9, al, np.pi - th, np.pi - 1.4))


# ---- shading and the light curve ------------------------------------------------------------------------------------------
def _ulps(x, ref):
    return np.abs(x.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30)).astype(np.float32))


SPOT = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5, exposure=2.0, with_disk=True)


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("with_base", (False, True))
def test_shade_against_numpy(with_base, channels):
    f = frame_hits()
    cam, met, o, d = frame_setup()
    a = CASES[0][0]
    dk = diskmod.ThinDisk(r_out=20.0)
    base = None
    if with_base:
        base = np.random.default_rng(2).uniform(0.0, 0.5, (FRAME_H, FRAME_W) + ((3,) if channels == 3 else ())).astype(np.float32)
    for t_obs in (0.0, 60.0, 333.25):
        got = ltrace.shade_hotspot(f["hits"], f["n_hits"], met, d, SPOT.to_lt(), t_obs, base=base, channels=channels)
        ref = diskmod.shade_hotspot(M, a, f["hits"], f["n_hits"], dk, SPOT, t_obs, base=base, channels=channels)
        assert got["rgb"].shape == ref.shape
        assert np.max(_ulps(got["rgb"], ref)) <= 2
        # RGBA8 = floor(255 rgb): equal except where the float value lies within 2 ulp of a rounding boundary
        c3 = ref if channels == 3 else np.repeat(ref[..., None], 3, axis=-1)
        want = (c3 * np.float32(255.0)).astype(np.uint8)
        x = c3.astype(np.float64) * 255.0
        near = np.abs(x - np.rint(x)) <= 2 * 255.0 * np.spacing(c3).astype(np.float64) + 1e-12
        assert np.all((got["rgba"][..., :3] == want) | near) and np.all(got["rgba"][..., 3] == 255)
    assert (ref > 0).sum() > 500


def test_dark_spot_is_the_thin_disk_frame():
    cam, met, o, d = frame_setup()
    ref = ltrace.render_disk_images(cam, met, o, d, max_images=3, want=("rgb",))
    f = frame_hits()
    got = ltrace.shade_hotspot(f["hits"], f["n_hits"], met, d, ltrace.default_hotspot(exposure=0.0, with_disk=1), 12.0)
    assert got["rgb"].tobytes() == ref["rgb"].tobytes() and (ref["rgb"] > 0).sum() > 500


def test_lightcurve():
    import ctypes as C
    import hipmini
    f = frame_hits()
    cam, met, o, d = frame_setup()
    a = CASES[0][0]
    spot = SPOT.to_lt()
    lc = ltrace.hotspot_lightcurve(f["hits"], f["n_hits"], met, d, spot, 5.0, 7.5, 64)
    ref = diskmod.lightcurve(M, a, f["hits"], f["n_hits"], SPOT, 5.0 + 7.5 * np.arange(64))
    assert np.all(ref[:, 0] > 0) and ref[:, 0].max() > 3 * ref[:, 0].min()
    assert np.max(np.abs(lc - ref) / np.abs(ref)) <= 1e-12
    assert ltrace.hotspot_lightcurve(f["hits"], f["n_hits"], met, d, spot, 5.0, 7.5, 64).tobytes() == lc.tobytes()
    dev = {}
    for name in ("hits", "n_hits"):
        host = np.ascontiguousarray(f[name])
        dev[name] = hipmini.DeviceArray(host.shape, host.dtype)
        assert hipmini.hip().hipMemcpy(C.c_void_p(dev[name].ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1) == 0   # host to device
    d_out = hipmini.DeviceArray((64, 3), np.float64)
    ltrace.hotspot_lightcurve_dev(dev["hits"].ptr, dev["n_hits"].ptr, FRAME_H, FRAME_W, 3, met, d, spot, 5.0, 7.5, 64, d_out.ptr)
    assert d_out.get().tobytes() == lc.tobytes()   # (the blocking copy orders behind the default stream's kernels)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    cam, met, o, d = frame_setup()
    f = frame_hits()

    def code(fn):
        with pytest.raises(ltrace.LtraceError) as ei:
            fn()
        return ei.value.code

    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, M, 0.0)
    assert code(lambda: ltrace.trace_disk_hits(cam, schw, o, d)) == ltrace.ERR_UNSUPPORTED
    oq = frame_setup(schedule="queue")[2]
    assert code(lambda: ltrace.trace_disk_hits(cam, met, oq, d)) == ltrace.ERR_UNSUPPORTED
    for m in (0, 9):
        assert code(lambda: ltrace.trace_disk_hits(cam, met, o, d, max_images=m)) == ltrace.ERR_INVALID_ARG
        assert code(lambda: ltrace.trace_batch_kerr_disk_hits(M, 0.9, 50.0, [0.1], [0.2], 1.4, 5000.0, d, max_images=m)) == ltrace.ERR_INVALID_ARG
    for sigma in (0.0, -1.0):
        bad = ltrace.default_hotspot(sigma=sigma)
        assert code(lambda: ltrace.shade_hotspot(f["hits"], f["n_hits"], met, d, bad, 0.0)) == ltrace.ERR_INVALID_ARG
        assert code(lambda: ltrace.hotspot_lightcurve(f["hits"], f["n_hits"], met, d, bad, 0.0, 1.0, 4)) == ltrace.ERR_INVALID_ARG
    assert code(lambda: ltrace.shade_hotspot(f["hits"], f["n_hits"], schw, d, ltrace.default_hotspot(), 0.0)) == ltrace.ERR_UNSUPPORTED


# ---- command line ---------------------------------------------------------------------------------------------------------
def test_cli_sequence(tmp_path):
    import matplotlib.image as mpimg
    out = str(tmp_path / "spot.png")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "light-path-tracer_amd"))
    subprocess.run([sys.executable, os.path.join(ROOT, "light-path-tracer_amd", "image_lens.py"), "--a", "0.9", "--theta-obs", "80",
                    "--r-obs", "50", "--disk-images", "3", "--synthetic", "64", "48", "--hotspot", "8", "0.5", "1.5", "--times", "0", "10",
                    "3", "--output", out], check=True, env=env, timeout=120)
    frames = [mpimg.imread(str(tmp_path / f"spot_{i:04d}.png")) for i in range(3)]
    assert all(f.shape[:2] == (48, 64) for f in frames)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    lc = np.load(str(tmp_path / "spot_lightcurve.npy"))
    assert lc.shape == (3, 3) and np.all(lc[:, 0] > 0)
