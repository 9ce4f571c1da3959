"""CPU tests of the hit-time rule and the hot spot's numpy statements (disk.step_time, disk.shade_hotspot,
disk.lightcurve), the references tests/test_gpu_hit_time.py holds the kernels to.

Truth for time is independent of the rule: the oracle's 8-D dense DP45 (oracle.integrate_dense, rtol 1e-11 / atol 1e-13,
max_step 1) carries coordinate time as a state component.  The rule is applied to consecutive points of those tracks
(so the states are exact to 1e-11 and what is measured is the quadrature alone) and compared with the track's own time
difference, per step and summed along the track.

MEASURED here (168 tracks, a in {0, 0.9, -0.7}, r_obs = 50, theta_obs = 1.4; per spin 4 screen angles x (8 rays over
the disk's image + 6 impact parameters 4 ... 8 around the critical curve); 65 390 steps of length <= 1):
    largest per-step error 1.7e-9 / 2.9e-9 / 2.6e-9 (a = 0 / 0.9 / -0.7);
    largest per-track error 5.6e-8 / 8.1e-8 / 7.5e-8 absolute, 9e-10 of the elapsed time;
    doubling the step raises the median per-step error by 34.4 / 35.5 / 35.3 (2^5 = 32: the rule is local O(h^5)).
The assertions are 10 x the measured maxima, the project's habit.
"""
import numpy as np
import pytest

import disk as diskmod
import ltrace
from oracle import oracle

M = 1.0
R_OBS, THETA_OBS = 50.0, 1.4
SPINS = (0.0, 0.9, -0.7)
STEP_ERR_MAX = 2.9e-9    # measured (header); asserted at 10 x
TRACK_ERR_MAX = 8.1e-8

_TRACKS = {}


def fan():
    """Deterministic rays: 4 screen angles x (8 alphas over the disk's image + 6 impact parameters 4 ... 8 around the
    critical curve) = 56 rays."""
    ang = np.array([0.3, 1.9, 3.5, 5.1])
    amax = 1.3 * np.arctan(20.0 / R_OBS)
    one = np.concatenate([np.linspace(0.05 * amax, amax, 8), np.arctan(np.linspace(4.0, 8.0, 6) / R_OBS)])
    return np.tile(one, ang.size), np.repeat(ang, one.size)


def tracks(a, rays=None):
    """The dense tracks of the rays (alphas, screen angles; default: fan()) for spin a, cached: list of dict(ray (index into fan()), lam (n,), y (8, n): t, r, theta, phi, p_t, p_r,
    p_theta, p_phi)."""
    key = (a, None if rays is None else tuple(np.concatenate(rays)))
    if key not in _TRACKS:
        out = []
        r_plus = M + np.sqrt(M * M - a * a)
        for i, (al, th) in enumerate(zip(*(fan() if rays is None else rays))):
            ok, st5, p_t, p_phi = oracle.kerr_ic(M, a, R_OBS, al, th, THETA_OBS)
            if not ok:
                continue
            s0 = np.array([0.0, st5[0], st5[1], st5[2], p_t, st5[3], st5[4], p_phi])
            lam, y, _, _ = oracle.integrate_dense(1, M, a, s0, lambda_max=5000.0, r_stop_inner=1.01 * r_plus,
                                                  r_stop_outer=2.0 * R_OBS, rtol=1e-11, atol=1e-13, max_step=1.0,
                                                  max_points=60000)
            assert len(lam) < 60000
            out.append(dict(ray=i, lam=np.asarray(lam), y=np.asarray(y)))
        _TRACKS[key] = out
    return _TRACKS[key]


def pairs(tr, stride=1):
    """Consecutive points of one track, every stride-th: (L, y0 (n, 4), y1 (n, 4), h (n,), dt_true (n,))."""
    y, lam = tr["y"][:, ::stride], tr["lam"][::stride]
    s4 = y[[1, 2, 5, 6]].T
    return y[7, 0], s4[:-1], s4[1:], np.diff(lam), np.abs(np.diff(y[0]))


def step_errors(a, trs, stride):
    err, med, track, t_end = [], [], [], []
    for tr in trs:
        L, y0, y1, h, dt_true = pairs(tr, stride)
        dt = diskmod.step_time(M, a, L, y0, y1, h)
        e = np.abs(dt - dt_true)
        err.append(e)
        med.append(np.median(e[h > 0.5]) if np.any(h > 0.5) else np.nan)
        track.append(abs(dt.sum() - dt_true.sum()))
        t_end.append(dt_true.sum())
    return dict(err=np.concatenate(err), err_med=np.array(med), track=np.array(track), t_end=np.array(t_end))


@pytest.mark.parametrize("a", SPINS)
def test_rule_against_the_dense_truth(a):
    trs = tracks(a)
    assert len(trs) >= 50
    e = step_errors(a, trs, 1)
    print(f"a {a}: {e['err'].size} steps, max per-step error {e['err'].max():.3e}, max per-track error {e['track'].max():.3e}")
    assert e["err"].max() <= 10 * STEP_ERR_MAX
    assert e["track"].max() <= 10 * TRACK_ERR_MAX
    # time runs forward along the backward ray in the tracers' convention
    assert all(np.all(np.diff(tr["y"][0]) * np.sign(tr["y"][0, -1]) > 0) for tr in trs)


@pytest.mark.parametrize("a", SPINS)
def test_rule_is_fifth_order(a):
    """Every second point doubles h: the per-step error grows by about 2^5 (median over each track's full-size steps,
    then over the tracks)."""
    trs = tracks(a)
    e1, e2 = step_errors(a, trs, 1), step_errors(a, trs, 2)
    ok = np.isfinite(e1["err_med"]) & np.isfinite(e2["err_med"]) & (e1["err_med"] > 1e-13)
    ratio = np.median(e2["err_med"][ok] / e1["err_med"][ok])
    print(f"a {a}: median error ratio on doubling the step {ratio:.1f}")
    assert 16.0 <= ratio <= 64.0


def test_partial_steps_add_up():
    """[0, tau] plus the rule on the remainder (the step from the cubic's state at tau, of length (1 - tau) h) equals
    tau = 1 to the rule's own error; h = 0 gives 0."""
    a = 0.9
    rng = np.random.default_rng(5)
    for tr in tracks(a)[::6]:
        L, y0, y1, h, _ = pairs(tr)
        tau = rng.uniform(0.05, 0.95, h.size)
        whole = diskmod.step_time(M, a, L, y0, y1, h)
        part = diskmod.step_time(M, a, L, y0, y1, h, tau)
        # the state at tau: the step's cubic Hermite in every component, with the tracers' derivatives
        lam = tr["lam"]
        ym = np.empty_like(y0)
        f0 = np.array([oracle.rhs8(1, M, a, tr["y"][:, i]) for i in range(h.size)])[:, [1, 2, 5, 6]] * h[:, None]
        f1 = np.array([oracle.rhs8(1, M, a, tr["y"][:, i + 1]) for i in range(h.size)])[:, [1, 2, 5, 6]] * h[:, None]
        for c in range(4):
            ym[:, c] = diskmod._hermite(y0[:, c], f0[:, c], y1[:, c], f1[:, c], tau)
        rest = diskmod.step_time(M, a, L, ym, y1, (1.0 - tau) * h)
        assert np.max(np.abs(part + rest - whole)) <= 10 * STEP_ERR_MAX
        assert np.all(diskmod.step_time(M, a, L, y0, y1, 0.0 * h, tau) == 0.0)
        assert lam.size == h.size + 1


def test_frame_sample_excludes_few():
    """The sample of tests/test_gpu_hit_time.py::test_frame_times_against_the_truth is drawn and thinned from the truth
    alone, so its condition -- 150 pixels with a crossing, at most 2 % of them excluded -- is checked here, without a GPU."""
    import test_gpu_hit_time as g
    sample, keep = g.frame_sample_kept()
    assert len(sample) == g.FRAME_SAMPLE and len(keep) >= 0.98 * len(sample)
    assert len({(iy, ix) for iy, ix, _ in sample}) == len(sample)
    assert sum(len(t["hits"]) > 1 for _, _, t in keep) >= 5      # slot 1 is compared as well


def _hits(seed=3, shape=(12, 10, 3)):
    """A synthetic hit buffer: r in [2, 20], phi in [0, 2 pi), g in [0.2, 1.4], dt in [40, 200]; about a third of the
    slots unused (NaN), leading slots first."""
    rng = np.random.default_rng(seed)
    R, W, m = shape
    hits = np.stack([rng.uniform(2.0, 20.0, shape), rng.uniform(0.0, 2 * np.pi, shape), rng.uniform(0.2, 1.4, shape),
                     rng.uniform(40.0, 200.0, shape)], axis=-1).astype(np.float32)
    n_hits = rng.integers(0, m + 2, (R, W)).astype(np.uint8)
    hits[np.arange(m)[None, None, :] >= n_hits[..., None]] = np.nan
    return hits, n_hits


def test_wide_spot_without_disk_is_g4_ramp():
    hits, n_hits = _hits()
    a = 0.9
    spot = diskmod.HotSpot(r_spot=8.0, phi0=0.4, sigma=1e9, exposure=0.05, with_disk=False)
    rgb = diskmod.shade_hotspot(M, a, hits, n_hits, diskmod.ThinDisk(), spot, 17.0)
    g = np.where(np.isnan(hits[..., 2]), 0.0, hits[..., 2].astype(np.float64))
    ref = sum(0.05 * g[..., j, None] ** 4 * np.clip(2.0 * g[..., j, None] - 0.5 * np.arange(3), 0.0, 1.0) for j in range(3))
    assert np.max(np.abs(rgb - np.clip(ref, 0.0, 1.0))) <= 2e-7
    assert np.array_equal(diskmod.shade_hotspot(M, a, hits, None, diskmod.ThinDisk(), spot, 17.0), rgb)


def test_lightcurve_is_periodic():
    hits, n_hits = _hits(seed=4)
    a = 0.9
    spot = diskmod.HotSpot(r_spot=7.0, phi0=1.0, sigma=1.5, exposure=1.0)
    period = 2 * np.pi / diskmod.omega(M, a, spot.r_spot)
    t = np.linspace(0.0, 90.0, 7)
    lc0, lc1 = diskmod.lightcurve(M, a, hits, n_hits, spot, t), diskmod.lightcurve(M, a, hits, n_hits, spot, t + period)
    assert lc0.shape == (7, 3) and np.all(lc0[:, 0] > 0) and np.ptp(lc0[:, 0]) > 0
    assert np.max(np.abs(lc1 - lc0) / np.abs(lc0)) <= 1e-12


@pytest.mark.parametrize("channels", (1, 3))
def test_dark_spot_with_disk_is_the_thin_disk(channels):
    hits, n_hits = _hits(seed=6)
    a = -0.7
    dk = diskmod.ThinDisk(q=2.5, exposure=0.3)
    base = np.random.default_rng(1).uniform(0, 0.4, hits.shape[:2] + ((3,) if channels == 3 else ())).astype(np.float32)
    got = diskmod.shade_hotspot(M, a, hits, n_hits, dk, diskmod.HotSpot(exposure=0.0, with_disk=True), 5.0, base=base,
                                channels=channels)
    ref = diskmod.shade_images(base, hits[..., :3], n_hits, dk.inner_edge(M, a), q=2.5, exposure=0.3, channels=channels)
    assert np.array_equal(got, ref)


def test_no_device_is_refused():
    """Without a GPU every new entry point returns LT_ERR_NO_DEVICE."""
    if ltrace.device_count() > 0:
        pytest.skip("a GPU is visible")
    cam = ltrace.Camera(64, 48, 0.7, 0.5, 0.0, 0.0, 50.0, 1.4)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    hits, n_hits = _hits()
    calls = [lambda: ltrace.trace_disk_hits(cam, met, ltrace.default_opts(), ltrace.default_disk()),
             lambda: ltrace.trace_batch_kerr_disk_hits(1.0, 0.9, 50.0, [0.1], [0.2], 1.4, 5000.0, ltrace.default_disk()),
             lambda: ltrace.step_time_probe(met, 1.0, [[10, 1.5, -1, 0]], [[9, 1.5, -1, 0]], 1.0),
             lambda: ltrace.shade_hotspot(hits, n_hits, met, ltrace.default_disk(), ltrace.default_hotspot(), 0.0),
             lambda: ltrace.hotspot_lightcurve(hits, n_hits, met, ltrace.default_disk(), ltrace.default_hotspot(), 0.0, 1.0, 4)]
    for call in calls:
        with pytest.raises(ltrace.LtraceError) as ei:
            call()
        assert ei.value.code == ltrace.ERR_NO_DEVICE
