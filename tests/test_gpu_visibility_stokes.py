"""The polarized visibility kernels (lt_visibility_stokes.hpp) through lt_disk_visibility_stokes[_dev] and
lt_hotspot_visibility_stokes[_dev].  The longdouble reference and the bounds are tests/test_visibility_stokes_host.py's
(its header derives them); the hit records, their references and the baselines are test_gpu_visibility.py's -- the cases of
test_diskmap_host.CASES: 257 x 331 x 8 (a second, partial pass of the stride loop, W odd), 260 x 300 x 3, 3 x 70 x 5,
1 x 1 x 1, counts above max_images -- with test_polarization_host.synth_pol records of the same shapes, and the 96 x 80
trace of test_gpu_diskmap.py.

Batches.  (time, plane) is flattened into pairs and a workgroup accumulates LT_VISIBILITY_STOKES_BATCH_PAIRS = 5 of them,
three terms each.  With split_orders the 8 planes of one time of "big" span two batches; the 3 planes of "mid" against 5
pairs make every batch cross a time boundary.  Launches: the partials of one batch at 1024 baselines take
256 x 15 x 1024 x 16 B = 60 MiB of the 64 MiB workspace, so the 25 pairs of the many-baselines test run as five launches.

The link to the Stokes light curve, derived.  On records with g in [1, 1.4] the colour ramp is (1, 1, 1) and the light curve's
per-slot light is m = ((e + e) + e) / 3 with e = w_I: two roundings (e + e is exact), so m = w_I (1 + 2 x 2^-53).  Its Q term
is (w q) m with w q the same float64 number as the visibility's (Pi sz sz) q; the visibility rounds the last product once,
the light curve rounds it once or fuses it into its sum: one 2^-53 on either side.  So corresponding terms differ by at most
(2 + 2) 2^-53 |term|, c = 4, and |term| <= Pi w_I (1 + 2^-23) <= w_I with the Pi = 0.6 of these tests.  Both then add the
same n terms in their own orders, n 2^-53 of the sum of |terms| as in test_gpu_visibility.py's link to the light curve:
(4 + n) 2^-53 sum w_I for Q and U, and for I (whose terms differ by the mean's 2 x 2^-53 alone) all the more.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES, LC_GRIDS, grid_times
from test_gpu_diskmap import SEQ, upload
from test_gpu_visibility import TIME_GRIDS, lt_spot, setup
from test_hotspot_records_host import isco_ref, lc_bound
from test_polarization_host import synth_pol
from test_spectrum_host import DISK_EXPOSURE, SPOT, U
from test_visibility_host import BASELINES, phase_bound
from test_visibility_stokes_host import FIELD, StokesVisibilityReference, check_visibility_stokes, stack_stokes

pytestmark = pytest.mark.gpu
LD = np.longdouble
_POL = {}


def setup_stokes(name):
    """test_gpu_visibility.setup plus the polarization records, their reference and the field."""
    c, hits, n_hits, ref, vref, met, dk = setup(name)
    if name not in _POL:
        pol = synth_pol((c.R, c.W, c.m), c.seed + 100)
        _POL[name] = (pol, StokesVisibilityReference(vref, pol, FIELD.pol_frac))
    return c, hits, n_hits, _POL[name][0], ref, _POL[name][1], met, dk, FIELD.to_lt()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_polarized_visibilities_against_the_reference(name):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    spot = SPOT(c.M)
    pb = phase_bound(c.R, c.W)
    disk_w = ref.disk_weights(float(isco_ref(c.M, c.a)), 3.0, DISK_EXPOSURE)
    spot_w = {float(t): ref.spot_weights(c.M, c.a, spot, t) for g in TIME_GRIDS for t in grid_times(g)}
    worst = dict(disk=np.zeros(3), spot=np.zeros(3))
    for split in (False, True):
        counts = sref.vref.counts(split)
        planes = c.m if split else 1
        want_disk = sref.visibility(disk_w, BASELINES, split)
        want_spot = [stack_stokes([sref.visibility(spot_w[float(t)], BASELINES, split) for t in grid_times(lcg)]) for lcg in TIME_GRIDS]
        for nh in (n_hits, None) if name in ("big", "strip") else (n_hits if split else None,):
            got = ltrace.disk_visibility_stokes(hits, nh, pol, met, dk, fld, BASELINES, split)
            assert got.shape == (planes, 3, 9) and np.all(got[..., 0].imag == 0.0)
            worst["disk"] = np.maximum(worst["disk"], check_visibility_stokes(got, want_disk, counts, 1e-12, pb))
            for lcg, ws in zip(TIME_GRIDS, want_spot):
                got = ltrace.hotspot_visibility_stokes(hits, nh, pol, met, dk, lt_spot(spot), fld, BASELINES, split, *lcg)
                assert got.shape == (lcg[2], planes, 3, 9) and np.all(got[..., 0].imag == 0.0)
                worst["spot"] = np.maximum(worst["spot"], check_visibility_stokes(got, ws, counts, lc_bound(c.M, c.a, spot, grid_times(lcg), c.r_out), pb))
    for who, excess in worst.items():
        print(f"{name} {who}: I, Q, U against longdouble, {excess[0]:.4f}, {excess[1]:.4f}, {excess[2]:.4f} of their bounds")
        assert max(excess) <= 1


# ---- 2. the I plane has the unpolarized bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "strip"))
def test_i_plane_has_the_unpolarized_bits(name):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    spot = lt_spot(SPOT(c.M))
    for split in (False, True):
        for nh in (n_hits, None):
            got = ltrace.disk_visibility_stokes(hits, nh, pol, met, dk, fld, BASELINES, split)
            assert np.ascontiguousarray(got[..., 0, :]).tobytes() == ltrace.disk_visibility(hits, nh, met, dk, BASELINES, split).tobytes()
            for lcg in TIME_GRIDS + [LC_GRIDS[0]]:                         # 3, 2 and 6 times: with the planes, whole and ragged batches
                got = ltrace.hotspot_visibility_stokes(hits, nh, pol, met, dk, spot, fld, BASELINES, split, *lcg)
                plain = ltrace.hotspot_visibility(hits, nh, met, dk, spot, BASELINES, split, *lcg)
                assert np.ascontiguousarray(got[..., 0, :]).tobytes() == plain.tobytes(), (split, lcg)
                assert np.any(got[..., 1, :] != 0) and np.any(got[..., 2, :] != 0)


# ---- 3. rows do not depend on their batch, baselines not on their company ----------------------------------------------------
def test_rows_do_not_depend_on_their_batch():
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes("big")
    assert ltrace.visibility_stokes_batch_pairs() == 5 and c.m == 8
    t_start, dt = 333.25, 0.1                                             # (i dt is not exact: an fma would give another time)
    run = lambda t0, n, split=True: ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, lt_spot(SPOT(c.M)), fld, BASELINES, split, t0, dt, n)
    whole = run(t_start, 3)                                               # 24 pairs: four full batches and a ragged fifth
    assert whole.shape == (3, 8, 3, 9) and np.all(whole[:, :, 0, 0].real > 0)
    assert run(t_start, 3).tobytes() == whole.tobytes()                   # a second call differs in no bit
    for i in range(3):                                                    # alone: 8 pairs, other batch boundaries
        assert run(t_start + i * dt, 1)[0].tobytes() == whole[i].tobytes(), i
    assert len({whole[i].tobytes() for i in range(3)}) == 3               # the rows are different rows
    unsplit = run(t_start, 7, False)                                      # 7 pairs: a batch of 5 and a ragged one of 2
    assert unsplit.shape == (7, 1, 3, 9)
    for i in range(7):
        assert run(t_start + i * dt, 1, False)[0].tobytes() == unsplit[i].tobytes(), i
    assert run(t_start, 7, False).tobytes() == unsplit.tobytes()


@pytest.mark.parametrize("n_b", (1024, 300))
def test_many_baselines_and_each_alone(n_b):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes("strip")
    uv = np.random.default_rng(n_b).uniform(-0.5, 0.5, (n_b, 2))
    uv[0], uv[-1] = (0.0, 0.0), (0.5, -0.5)
    spot, lcg = SPOT(c.M), LC_GRIDS[1]                                    # 5 times x 5 planes: 25 pairs, five batches
    assert c.m == 5 and lcg[2] == 5
    # one batch at 1024 baselines leaves no room for a second: more than one launch
    per_batch = ltrace.VISIBILITY_BLOCKS * 15 * n_b * 16
    assert (ltrace.VISIBILITY_WORKSPACE_BYTES // per_batch < 5) and (n_b != 1024 or ltrace.VISIBILITY_WORKSPACE_BYTES // per_batch == 1)
    run = lambda b: ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, lt_spot(spot), fld, b, True, *lcg)
    whole = run(uv)
    assert whole.shape == (5, c.m, 3, n_b)
    want = stack_stokes([sref.visibility(ref.spot_weights(c.M, c.a, spot, t), uv, True) for t in grid_times(lcg)])
    excess = check_visibility_stokes(whole, want, sref.vref.counts(True), lc_bound(c.M, c.a, spot, grid_times(lcg), c.r_out), phase_bound(c.R, c.W))
    still = ltrace.disk_visibility_stokes(hits, None, pol, met, dk, fld, uv, False)
    want = sref.visibility(ref.disk_weights(float(isco_ref(c.M, c.a)), 3.0, DISK_EXPOSURE), uv, False)
    excess_disk = check_visibility_stokes(still, want, sref.vref.counts(False), 1e-12, phase_bound(c.R, c.W))
    print(f"strip, {n_b} baselines: spot {np.round(excess, 4).tolist()}, disk {np.round(excess_disk, 4).tolist()} of their bounds")
    assert max(excess) <= 1 and max(excess_disk) <= 1
    picks = sorted({0, 1, 63, 64, 127, 128, 255, 256, 257, n_b - 2, n_b - 1} | {(n_b * k) // 6 for k in range(1, 6)})
    assert len(picks) == 16
    for b in picks:                                                       # alone it is pass 0, work-item 0
        alone = run(uv[b:b + 1])
        assert alone[..., 0].tobytes() == np.ascontiguousarray(whole[..., b]).tobytes(), b
        assert np.array_equal(ltrace.disk_visibility_stokes(hits, None, pol, met, dk, fld, uv[b:b + 1], False)[0, :, 0], still[0, :, b])
    for i in range(5):                                                    # every row alone: another batch, another launch
        row = ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, lt_spot(spot), fld, uv, True, lcg[0] + i * lcg[1], lcg[1], 1)
        assert row.tobytes() == whole[i:i + 1].tobytes()


# ---- 4. exact phases and weights ------------------------------------------------------------------------------------------------
def test_exact_phases_and_weights_on_the_device():
    """Synthetic records of weight g^4 (the disk with q = 0 and exposure 1, as test_exact_phases_on_the_device): four pixels in
    a row with equal g, sin zeta = 1 and Pi = 0.5, so w_Q = (0.5 q) w and w_U = (0.5 u) w are exact for q, u in {0, 1, -1}."""
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(q=0.0, exposure=1.0)
    fld = ltrace.default_bfield(pol_frac=0.5)
    g = np.float32(0.75)                                                  # (g^2)^2 = 81 / 256: small multiples of w are exact
    w = (float(g) * float(g)) ** 2
    uv = np.array([(0.25, 0.0), (0.5, 0.0), (0.0, 0.0), (-0.25, 0.0), (0.0, 0.25), (0.25, 0.5)])
    hits = np.full((1, 4, 2, 4), np.nan, dtype=np.float32)
    hits[0, :, 0] = [8.0, 1.0, g, 100.0]
    plain = ltrace.disk_visibility(hits, None, met, dk, uv, True)
    assert np.array_equal(plain[0], [0, 0, 4 * w, 0, 4 * w, 0])

    def run(q, u, split=True, h=hits):
        pol = np.full(h.shape, np.nan, dtype=np.float32)
        pol[0, :, 0] = np.stack(np.broadcast_arrays(np.float32(q), np.float32(u), np.float32(1.0), np.float32(0.5)), axis=-1)
        return ltrace.disk_visibility_stokes(h, None, pol, met, dk, fld, uv, split)

    for q, u in ((1, 0), (0, 1), (-1, 0), (0, -1)):
        V = run(q, u)
        assert V.shape == (2, 3, 6) and np.all(V[1] == 0) and np.array_equal(V[0, 0], plain[0])
        assert np.array_equal(V[0, 1], (0.5 * q) * plain[0]) and np.array_equal(V[0, 2], (0.5 * u) * plain[0])
        assert V[0, 1 if q else 2, 2] == 0.5 * (q + u) * 4 * w and np.all(V[0, 2 if q else 1] == 0)
    # one record per phase: at u = 1/4 the pixels' phases are 1, -i, -1, i, so Q~ = 0.5 w (1 + 1) and U~ = 0.5 w (-i - i)
    V = run([1, 0, -1, 0], [0, 1, 0, -1])
    assert V[0, 0, 0] == 0 and V[0, 1, 0] == w and V[0, 2, 0] == -1j * w
    assert V[0, 1, 2] == 0 and V[0, 2, 2] == 0 and V[0, 1, 3] == w and V[0, 2, 3] == 1j * w          # (0, 0), and the conjugate at -1/4
    # a second slot with the opposite polarization, unsplit: the slots are added before the phase, Q and U cancel to +0
    both = hits.copy()
    both[0, :, 1] = hits[0, :, 0]
    pol = np.empty(both.shape, dtype=np.float32)
    pol[0, :, 0], pol[0, :, 1] = (1.0, 0.0, 1.0, 0.5), (-1.0, 0.0, 1.0, 0.5)
    V = ltrace.disk_visibility_stokes(both, None, pol, met, dk, fld, uv, False)
    assert V.shape == (1, 3, 6) and V[0, 0, 2] == 8 * w and np.all(V[0, 1:] == 0)
    V = ltrace.disk_visibility_stokes(both, None, pol, met, dk, fld, uv, True)
    assert np.array_equal(V[0, 1], 0.5 * plain[0]) and np.array_equal(V[1, 1], -0.5 * plain[0])
    spot = ltrace.default_hotspot(r_spot=8.0, sigma=4.0)                  # equal records, equal weights: the same ratios
    Vs = ltrace.hotspot_visibility_stokes(both, None, pol, met, dk, spot, fld, uv, True, 50.0, 1.0, 2)
    assert Vs.shape == (2, 2, 3, 6) and np.all(Vs[:, 0, 0, 2].real > 0)
    assert np.array_equal(Vs[:, 0, 1], 0.5 * Vs[:, 0, 0]) and np.array_equal(Vs[:, 1, 1], -0.5 * Vs[:, 1, 0]) and np.all(Vs[:, :, 2] == 0)


# ---- 5. unpolarized light ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip"))
def test_unpolarized_light(name):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    dark = ltrace.default_bfield(b_r=0.3, b_phi=-0.5, b_z=1.0, pol_frac=0.0)
    spot = lt_spot(SPOT(c.M))
    for split in (False, True):
        V = ltrace.disk_visibility_stokes(hits, n_hits, pol, met, dk, dark, BASELINES, split)
        assert np.all(V[:, 1:] == 0) and np.ascontiguousarray(V[:, 0]).tobytes() == ltrace.disk_visibility(hits, n_hits, met, dk, BASELINES, split).tobytes()
        V = ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, spot, dark, BASELINES, split, *LC_GRIDS[0])
        lit = ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, spot, fld, BASELINES, split, *LC_GRIDS[0])
        assert np.all(V[:, :, 1:] == 0) and np.any(lit[:, :, 1:] != 0)
        assert np.ascontiguousarray(V[:, :, 0]).tobytes() == np.ascontiguousarray(lit[:, :, 0]).tobytes()


# ---- 6. Hermitian symmetry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip"))
def test_hermitian_symmetry_to_the_bit(name):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    uv = np.concatenate([BASELINES, np.random.default_rng(5).uniform(-0.5, 0.5, (55, 2))])
    for split in (False, True):
        a = ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, lt_spot(SPOT(c.M)), fld, uv, split, *LC_GRIDS[0])
        b = ltrace.hotspot_visibility_stokes(hits, n_hits, pol, met, dk, lt_spot(SPOT(c.M)), fld, -uv, split, *LC_GRIDS[0])
        assert np.array_equal(b.real, a.real) and np.array_equal(b.imag, -a.imag)
        assert all(np.any(a[:, :, s].imag != 0) for s in range(3))
        a = ltrace.disk_visibility_stokes(hits, n_hits, pol, met, dk, fld, uv, split)
        b = ltrace.disk_visibility_stokes(hits, n_hits, pol, met, dk, fld, -uv, split)
        assert np.array_equal(b.real, a.real) and np.array_equal(b.imag, -a.imag)


# ---- 7. the link to the Stokes light curve --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "strip", "one"))
def test_zero_baseline_is_the_stokes_light_curve(name):
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    spot = lt_spot(SPOT(c.M))
    assert FIELD.pol_frac * (1 + 2.0 ** -23) <= 1                         # |w_Q|, |w_U| <= w_I (header)
    bright = hits.copy()
    bright[..., 2] = (1.0 + 0.4 * (hits[..., 2].astype(np.float64) - 0.15) / 1.25).astype(np.float32)     # g into [1, 1.4]: the ramp is (1, 1, 1)
    stored = np.arange(c.m) < np.minimum(n_hits, c.m)[..., None]
    assert bright[..., 2][stored].min() >= 1.0 and bright[..., 2][stored].max() <= np.float32(1.4)
    n_all = int(stored.sum())
    worst = 0.0
    for lcg in LC_GRIDS[:2]:                                              # (times whose i dt is exact: the light curve may use an fma)
        V = ltrace.hotspot_visibility_stokes(bright, n_hits, pol, met, dk, spot, fld, BASELINES[:1], False, *lcg)
        lc = ltrace.hotspot_lightcurve_stokes(bright, n_hits, pol, met, dk, spot, fld, *lcg)
        assert V.shape == (lcg[2], 1, 3, 1) and lc.shape == (lcg[2], 3) and np.all(V.imag == 0) and np.all(lc[:, 0] > 0)
        diff = np.abs(V[:, 0, :, 0].real.astype(LD) - lc.astype(LD))
        bound = (4 + n_all) * U * lc[:, :1].astype(LD)
        worst = max(worst, float(np.max(diff / bound)))
        assert np.all(diff <= bound)
        assert name == "one" or np.all(lc[:, 1:] != 0)
    print(f"{name}: V(0, 0) of I, Q, U against the Stokes light curve, {worst:.4f} of (4 + n) 2^-53 sum I")


# ---- 8. device pointers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "one"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes(name)
    d_hits, d_n, d_pol = upload(hits), upload(n_hits), upload(pol)
    spot = lt_spot(SPOT(c.M))
    lcg = LC_GRIDS[0]
    as_complex = lambda d: np.ascontiguousarray(d.get()).view(np.complex128)[..., 0]
    for split, counts in ((False, True), (True, False)):
        shape = (c.m if split else 1, 3, 9, 2)
        nh, d_nh = (n_hits, d_n.ptr) if counts else (None, 0)
        d_out = hipmini.DeviceArray((1,) + shape, np.float64)
        ltrace.disk_visibility_stokes_dev(d_hits.ptr, d_nh, d_pol.ptr, c.R, c.W, c.m, met, dk, fld, BASELINES, split, d_out.ptr)
        assert as_complex(d_out)[0].tobytes() == ltrace.disk_visibility_stokes(hits, nh, pol, met, dk, fld, BASELINES, split).tobytes()
        d_out = hipmini.DeviceArray((lcg[2],) + shape, np.float64)
        ltrace.hotspot_visibility_stokes_dev(d_hits.ptr, d_nh, d_pol.ptr, c.R, c.W, c.m, met, dk, spot, fld, BASELINES, split, *lcg, d_out.ptr)
        assert as_complex(d_out).tobytes() == ltrace.hotspot_visibility_stokes(hits, nh, pol, met, dk, spot, fld, BASELINES, split, *lcg).tobytes()


# ---- 9. one real trace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [None, 2])
def test_render_sequence_returns_the_recentred_entry_points_outputs(S):
    import image_lens
    from metrics import Kerr
    M, a = SEQ["M"], SEQ["a"]
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    spot = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5)
    times = 100.0 + 25.0 * np.arange(3)
    kerr = Kerr(M=M, a=a, integrator="rk4", precision=32)
    k = 1 if S is None else S
    render = lambda **kw: image_lens.render_sequence(None, kerr, SEQ["r_obs"], SEQ["fov"], tdisk, spot, times, shape=SEQ["shape"],
                                                     theta_obs=SEQ["theta_obs"], samples=S, **kw)
    before = render(bfield=FIELD)                                          # the path the new code is not on
    assert "visibility_stokes" not in before and "disk_visibility_stokes" not in before and "visibility" not in before
    assert "visibility_stokes" not in render(baselines=diskmod.Baselines.radial(12, 0.5, 30.0))      # no field, no new keys
    met, dk, fld = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt(), FIELD.to_lt()
    outs = {}
    for split in (False, True):
        bl = diskmod.Baselines.radial(12, 0.5, 30.0, split_orders=split)
        out = render(bfield=FIELD, baselines=bl)
        planes = SEQ["max_images"] if split else 1
        assert out["visibility_stokes"].shape == (3, planes, 3, 12) and out["disk_visibility_stokes"].shape == (planes, 3, 12)
        assert out["visibility_stokes"].dtype == np.complex128 and out["disk_visibility_stokes"].dtype == np.complex128
        assert out["pol"].shape == out["hits"].shape == (SEQ["shape"][0] * k, SEQ["shape"][1] * k, SEQ["max_images"], 4)
        # every key of the call without baselines keeps its bytes (the trace and the re-shades are deterministic)
        for key, value in before.items():
            if key != "stats":
                assert np.asarray(out[key]).tobytes() == np.asarray(value).tobytes(), key
        uv = bl.uv / np.float64(k)
        rec = (out["hits"], out["n_hits"], out["pol"], met, dk)
        dyn = ltrace.hotspot_visibility_stokes(*rec, spot.to_lt(), fld, uv, split, 100.0, 25.0, 3)
        still = ltrace.disk_visibility_stokes(*rec, fld, uv, split)
        assert np.array_equal(out["visibility_stokes"], bl.recentre(dyn, SEQ["shape"], k))
        assert np.array_equal(out["disk_visibility_stokes"], bl.recentre(still, SEQ["shape"], k))
        # the unpolarized keys are the unpolarized entry points', and the new keys' I planes are their bytes
        plain = bl.recentre(ltrace.hotspot_visibility(out["hits"], out["n_hits"], met, dk, spot.to_lt(), uv, split, 100.0, 25.0, 3), SEQ["shape"], k)
        plain_disk = bl.recentre(ltrace.disk_visibility(out["hits"], out["n_hits"], met, dk, uv, split), SEQ["shape"], k)
        assert out["visibility"].tobytes() == plain.tobytes() and out["disk_visibility"].tobytes() == plain_disk.tobytes()
        assert np.ascontiguousarray(out["visibility_stokes"][:, :, 0]).tobytes() == out["visibility"].tobytes()
        assert np.ascontiguousarray(out["disk_visibility_stokes"][:, 0]).tobytes() == out["disk_visibility"].tobytes()
        slc = ltrace.hotspot_lightcurve_stokes(*rec, spot.to_lt(), fld, 100.0, 25.0, 3) / np.float64(k * k)
        assert out["stokes_lightcurve"].tobytes() == slc.tobytes()
        # the net polarization never exceeds Pi, and it moves
        for V in (out["visibility_stokes"], out["disk_visibility_stokes"]):
            frac = diskmod.fractional_polarization(V)[..., 0]
            lit = V[..., 0, 0] != 0
            assert np.all(lit[..., :2]) and np.all(np.abs(frac[lit]) <= FIELD.pol_frac * (1 + 1e-6)) and np.all(np.abs(frac[lit]) > 0)
        assert len({np.ascontiguousarray(out["visibility_stokes"][i, :, 1]).tobytes() for i in range(3)}) == 3
        outs[split] = out
    per, one = outs[True], outs[False]
    scale = np.abs(one["visibility_stokes"][:, :, :1, :1])
    assert np.all(np.abs(per["visibility_stokes"].sum(axis=1, keepdims=True) - one["visibility_stokes"]) <= 1e-12 * scale)
    scale = np.abs(one["disk_visibility_stokes"][0, 0, 0])
    assert np.all(np.abs(per["disk_visibility_stokes"].sum(axis=0) - one["disk_visibility_stokes"][0]) <= 1e-12 * scale)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, pol, ref, sref, met, dk, fld = setup_stokes("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    good_spot = lt_spot(SPOT(c.M))
    good_uv = np.ascontiguousarray(BASELINES)

    def call(form, hits_=hits, pol_=pol, met_=met, disk_=dk, emit=None, field_=fld, R=c.R, W=c.W, m=c.m, uv_=good_uv, n_b=None, t_start=0.0, dt=1.0,
             n_times=2, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full((4, 8, 3, 1025, 2), -7.0)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        head = (ptr(hits_), ptr(n_hits), ptr(pol_), R, W, m, ref_(met_), ref_(disk_))
        uv_args = (ptr(uv_), (0 if uv_ is None else uv_.shape[0]) if n_b is None else n_b, 1)
        o = None if null_out else ptr(out)
        if form == "disk":
            rc = lib.lt_disk_visibility_stokes(*head, ref_(field_), *uv_args, o)
        else:
            rc = lib.lt_hotspot_visibility_stokes(*head, ref_(good_spot if emit is None else emit), ref_(field_), *uv_args, t_start, dt, n_times, o)
        if rc != ltrace.OK:
            assert np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    for form in ("disk", "spot"):
        assert call(form)[0] == ltrace.OK
    nan, inf = float("nan"), float("inf")
    INV = ltrace.ERR_INVALID_ARG
    with_uv = lambda i, u, v: np.concatenate([good_uv[:i], [(u, v)], good_uv[i:]])
    long_uv = np.zeros((1025, 2))
    head = [(dict(hits_=None), INV, "null"), (dict(met_=None), INV, "null"), (dict(disk_=None), INV, "null")]
    frame = [(dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"), (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), INV, "bad metric"),
             (dict(R=0), INV, "empty frame"), (dict(W=-3), INV, "empty frame"), (dict(m=0), INV, "max_images"), (dict(m=9), INV, "max_images")]
    emitter = dict(disk=([], []),
                   spot=([(dict(emit="null"), INV, "null")],
                         [(dict(emit=ltrace.default_hotspot(sigma=0.0)), INV, "sigma"), (dict(emit=ltrace.default_hotspot(r_spot=-1.0)), INV, "r_spot")]))
    tail = [(dict(disk_=ltrace.default_disk(q=nan)), INV, "disk q"), (dict(disk_=ltrace.default_disk(exposure=-1.0)), INV, "disk q"),
            (dict(uv_=None, n_b=9), INV, "null uv"), (dict(n_b=0), INV, "n_baselines"), (dict(uv_=long_uv), INV, "n_baselines"),
            (dict(uv_=with_uv(3, 0.5000001, 0.0)), INV, "baseline 3"), (dict(uv_=with_uv(9, 0.0, -0.5000001)), INV, "baseline 9"),
            (dict(uv_=with_uv(0, nan, 0.0)), INV, "baseline 0"), (dict(uv_=with_uv(1, 0.0, inf)), INV, "baseline 1")]
    polarized = [(dict(pol_=None), INV, "null pol"), (dict(field_="null"), INV, "null metric / field"),
                 (dict(field_=ltrace.default_bfield(b_r=0.0, b_phi=0.0, b_z=0.0)), INV, "the field"),
                 (dict(field_=ltrace.default_bfield(b_z=inf)), INV, "the field"), (dict(field_=ltrace.default_bfield(pol_frac=1.5)), INV, "pol_frac"),
                 (dict(field_=ltrace.default_bfield(pol_frac=nan)), INV, "pol_frac")]
    times = [(dict(n_times=-1), INV, "n_times"), (dict(n_times=65536), INV, "n_times"), (dict(t_start=nan), INV, "t_start"), (dict(dt=inf), INV, "t_start")]
    last = [(dict(null_out=True), INV, "null out")]
    for form in ("disk", "spot"):
        nulls, fields = emitter[form]
        seq = head + nulls + frame + fields + tail + polarized + ([] if form == "disk" else times) + last
        for i, (kw, code, word) in enumerate(seq):
            rc, msg = call(form, **kw)
            assert rc == code and word in msg, (form, kw, rc, msg)
            for kw2, _, word2 in seq[i + 1:]:                           # with a later fault present as well, the earlier one decides
                if set(kw) & set(kw2) or word2.split()[0] == word.split()[0]:
                    continue
                rc, msg = call(form, **kw, **kw2)
                assert rc == code and word in msg, (form, kw, kw2, rc, msg)
    rc, msg = call("spot", pol_=None, field_="null")                     # (both begin with "null": the records come first)
    assert rc == INV and "null pol" in msg
    # no times: nothing to do, nothing written, even without an output
    assert call("spot", n_times=0)[0] == ltrace.OK and call("spot", n_times=0, null_out=True)[0] == ltrace.OK
    d_hits, d_pol = upload(hits), upload(pol)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.hotspot_visibility_stokes_dev(d_hits.ptr, 0, d_pol.ptr, c.R, c.W, c.m, met, dk, good_spot, fld, good_uv, True, 0.0, 1.0, 2, 0)
    assert ei.value.code == INV and "null out" in str(ei.value)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.disk_visibility_stokes_dev(d_hits.ptr, 0, 0, c.R, c.W, c.m, met, dk, fld, good_uv, False, 0)
    assert ei.value.code == INV and "null pol" in str(ei.value)
