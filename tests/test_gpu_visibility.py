"""The visibility kernels (lt_visibility.hpp) through lt_disk_visibility[_dev], lt_hotspot_visibility[_dev] and
lt_diskmap_visibility[_dev].  Baselines, the longdouble reference and the bounds are tests/test_visibility_host.py's (its
header derives the bounds); the records are test_diskmap_host.CASES' -- 257 x 331 x 8 (a second, partial pass of the stride
loop, W odd), 260 x 300 x 3, 3 x 70 x 5, 1 x 1 x 1, counts above max_images -- and the 96 x 80 trace of test_gpu_diskmap.py.

Batches.  A workgroup accumulates LT_VISIBILITY_BATCH_TERMS = 16 (time, plane) terms at once, so with split_orders on
the max_images = 8 case ltrace.visibility_batch_times gives 16 // 8 = 2 times, the smallest batch there is: 4 times run
as two batches.  Launches: the partials of one batch of 15 terms at 1024 baselines take 256 x 15 x 1024 x 16 B = 60 MiB of
the 64 MiB workspace, so the 5 times of the many-baselines test on the max_images = 5 case (batches of 3) run as two
launches as well.

The links to what exists, derived.  V(0, 0) adds the weights a spectrum bins (c = 1 and s = 0 exactly, the fused
multiply-add adds w itself): both add the same n_terms non-negative numbers in their own orders, so they lie within
(4 + n_terms) 2^-53 relative of each other, as a spectrum's rows and the light curve do (test_gpu_spectrum.py).  The
triangle inequality: |V(b)| <= flux and V(0, 0) >= flux up to the errors of their own sums and phases -- the weights are
the same numbers on both sides, so no term_bound -- hence |V(b)| <= V(0, 0) (1 + 2 (phase_bound + n_terms 2^-53) + 4 x 2^-53),
the last for the modulus taken in float64.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES, LC_GRIDS, grid_times, make_map, map_lc_bound, records
from test_gpu_diskmap import SEQ, traced, upload
from test_hotspot_records_host import isco_ref, lc_bound
from test_spectrum_host import DISK_EXPOSURE, GRIDS, MAP_VARIANTS, SPOT, SpectrumReference, U
from test_visibility_host import BASELINES, VisibilityReference, check_visibility, phase_bound

pytestmark = pytest.mark.gpu
LD = np.longdouble
TIME_GRIDS = [LC_GRIDS[0][:2] + (3,), LC_GRIDS[1][:2] + (2,)]             # (t_start, dt, n_times): the light curves' first two, shortened
_REF = {}


def setup(name):
    c = CASES[name]
    hits, n_hits, _ = records(name)
    if name not in _REF:
        ref = SpectrumReference(hits, n_hits)
        _REF[name] = (ref, VisibilityReference(ref, c.W))
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a)
    dk = ltrace.default_disk(r_out=c.r_out, exposure=DISK_EXPOSURE)      # r_in 0: the ISCO, resolved by the library
    return c, hits, n_hits, _REF[name][0], _REF[name][1], met, dk


def lt_spot(spot):
    return ltrace.default_hotspot(r_spot=spot[0], phi0=spot[1], sigma=spot[2], exposure=spot[3], with_disk=int(spot[4]))


def stack(wants):
    """[(re, im, flux) per time] -> (re, im, flux) with a leading time axis."""
    return tuple(np.stack(x) for x in zip(*wants))


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_visibilities_against_the_reference(name):
    c, hits, n_hits, ref, vref, met, dk = setup(name)
    spot = SPOT(c.M)
    pb = phase_bound(c.R, c.W)
    disk_w = ref.disk_weights(float(isco_ref(c.M, c.a)), 3.0, DISK_EXPOSURE)
    spot_w = {float(t): ref.spot_weights(c.M, c.a, spot, t) for g in TIME_GRIDS for t in grid_times(g)}
    maps = [make_map(c, v) for v in MAP_VARIANTS]
    worst = dict(disk=0.0, spot=0.0, map=0.0)
    for split in (False, True):
        counts = vref.counts(split)
        dm = maps[int(split)]                                             # Keplerian unsplit, rigid split
        want_disk = vref.visibility(disk_w, BASELINES, split)
        want_spot = [stack([vref.visibility(spot_w[float(t)], BASELINES, split) for t in grid_times(lcg)]) for lcg in TIME_GRIDS]
        want_map = [stack([vref.visibility(ref.map_weights(c.M, c.a, dm, t), BASELINES, split) for t in grid_times(lcg)]) for lcg in TIME_GRIDS]
        for nh in (n_hits, None) if name in ("big", "strip") else (n_hits if split else None,):
            got = ltrace.disk_visibility(hits, nh, met, dk, BASELINES, split)
            assert got.shape == (c.m if split else 1, 9) and np.all(got[:, 0].imag == 0.0)
            worst["disk"] = max(worst["disk"], check_visibility(got, want_disk, counts, 1e-12, pb))
            for lcg, ws, wm in zip(TIME_GRIDS, want_spot, want_map):
                got = ltrace.hotspot_visibility(hits, nh, met, dk, lt_spot(spot), BASELINES, split, *lcg)
                assert got.shape == (lcg[2], c.m if split else 1, 9) and np.all(got[..., 0].imag == 0.0)
                worst["spot"] = max(worst["spot"], check_visibility(got, ws, counts, lc_bound(c.M, c.a, spot, grid_times(lcg), c.r_out), pb))
                got = ltrace.diskmap_visibility(hits, nh, met, dk, dm.to_lt(), dm.texels, BASELINES, split, *lcg)
                assert np.all(got[..., 0].imag == 0.0)
                worst["map"] = max(worst["map"], check_visibility(got, wm, counts, map_lc_bound(c.M, c.a, dm, grid_times(lcg), float(diskmod.isco(c.M, c.a))), pb))
    for who, excess in worst.items():
        print(f"{name} {who}: visibility against longdouble, {excess:.4f} of its bound")
        assert excess <= 1


# ---- 2. many baselines: ownership beyond one per work-item, a ragged last pass, two launches ---------------------------------
@pytest.mark.parametrize("n_b", (1024, 300))
def test_many_baselines_and_each_alone(n_b):
    c, hits, n_hits, ref, vref, met, dk = setup("strip")
    uv = np.random.default_rng(n_b).uniform(-0.5, 0.5, (n_b, 2))
    uv[0], uv[-1] = (0.0, 0.0), (0.5, -0.5)
    spot, lcg = SPOT(c.M), LC_GRIDS[1]                                    # 5 times: batches of 3 with the 5 planes
    assert ltrace.visibility_batch_times(True, c.m) == 3
    run = lambda b: ltrace.hotspot_visibility(hits, n_hits, met, dk, lt_spot(spot), b, True, *lcg)
    whole = run(uv)
    assert whole.shape == (5, c.m, n_b)
    want = stack([vref.visibility(ref.spot_weights(c.M, c.a, spot, t), uv, True) for t in grid_times(lcg)])
    excess = check_visibility(whole, want, vref.counts(True), lc_bound(c.M, c.a, spot, grid_times(lcg), c.r_out), phase_bound(c.R, c.W))
    still = ltrace.disk_visibility(hits, None, met, dk, uv, False)
    excess_disk = check_visibility(still, vref.visibility(ref.disk_weights(float(isco_ref(c.M, c.a)), 3.0, DISK_EXPOSURE), uv, False),
                                   vref.counts(False), 1e-12, phase_bound(c.R, c.W))
    print(f"strip, {n_b} baselines: spot {excess:.4f}, disk {excess_disk:.4f} of their bounds")
    assert excess <= 1 and excess_disk <= 1
    picks = sorted({0, 1, 63, 64, 127, 128, 255, 256, 257, n_b - 2, n_b - 1} | {(n_b * k) // 6 for k in range(1, 6)})
    assert len(picks) == 16
    for b in picks:                                                       # alone it is pass 0, work-item 0
        alone = run(uv[b:b + 1])
        assert alone[..., 0].tobytes() == np.ascontiguousarray(whole[..., b]).tobytes(), b
        assert ltrace.disk_visibility(hits, None, met, dk, uv[b:b + 1], False)[0, 0] == still[0, b]
    for i in range(5):                                                    # every row alone: another batch, another launch
        assert ltrace.hotspot_visibility(hits, n_hits, met, dk, lt_spot(spot), uv, True, lcg[0] + i * lcg[1], lcg[1], 1).tobytes() == whole[i:i + 1].tobytes()


# ---- 3. reproducible and batch-independent -------------------------------------------------------------------------------------
@pytest.mark.parametrize("emitter", ("spot", "map"))
def test_rows_do_not_depend_on_their_batch(emitter):
    c, hits, n_hits, ref, vref, met, dk = setup("big")
    per_batch = ltrace.visibility_batch_times(True, c.m)
    assert per_batch == ltrace.VISIBILITY_BATCH_TERMS // 8 == 2           # the smallest batch there is
    n_times = per_batch + 2                                               # one batch plus two more times
    t_start, dt = 333.25, 0.1                                             # (i dt is not exact: an fma would give another time)
    if emitter == "spot":
        run = lambda t0, n, split=True: ltrace.hotspot_visibility(hits, n_hits, met, dk, lt_spot(SPOT(c.M)), BASELINES, split, t0, dt, n)
    else:
        dm = make_map(c, MAP_VARIANTS[0])
        run = lambda t0, n, split=True: ltrace.diskmap_visibility(hits, n_hits, met, dk, dm.to_lt(), dm.texels, BASELINES, split, t0, dt, n)
    whole = run(t_start, n_times)
    assert whole.shape == (n_times, 8, 9) and np.all(whole[..., 0].real > 0)
    assert run(t_start, n_times).tobytes() == whole.tobytes()             # a second call differs in no bit
    for i in range(n_times):
        assert run(t_start + i * dt, 1)[0].tobytes() == whole[i].tobytes(), i
    assert len({whole[i].tobytes() for i in range(n_times)}) == n_times   # the rows are different rows
    three = run(t_start, 3)                                               # a ragged last batch
    assert three.tobytes() == whole[:3].tobytes()
    unsplit = run(t_start, 19, False)                                     # 16 + 3 times in one plane
    assert ltrace.visibility_batch_times(False, c.m) == 16
    for i in (0, 15, 16, 18):
        assert run(t_start + i * dt, 1, False)[0].tobytes() == unsplit[i].tobytes(), i


# ---- 4. exact phases ---------------------------------------------------------------------------------------------------------------
def test_exact_phases_on_the_device():
    """Synthetic records of weight g^4: the disk with q = 0 and exposure 1 (pow(x, 0) = 1, so the weight is (g^2)^2 in float64
    and the sums are predicted to the bit).  Four pixels in a row with equal g at u = 1/4: the phases are 1, -i, -1, i."""
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(q=0.0, exposure=1.0)
    g = np.float32(0.75)                                                  # (g^2)^2 = 81 / 256: small multiples of w are exact
    w = (float(g) * float(g)) ** 2
    rec = np.array([8.0, 1.0, g, 100.0], dtype=np.float32)
    uv = np.array([(0.25, 0.0), (0.5, 0.0), (0.0, 0.0), (-0.25, 0.0), (0.0, 0.25), (0.25, 0.5)])
    hits = np.full((1, 4, 2, 4), np.nan, dtype=np.float32)
    hits[0, :, 0] = rec
    V = ltrace.disk_visibility(hits, None, met, dk, uv, True)
    assert V.shape == (2, 6) and np.all(V[1] == 0)
    assert V[0, 0] == 0 and V[0, 1] == 0 and V[0, 2] == 4 * w and V[0, 3] == 0 and V[0, 4] == 4 * w and V[0, 5] == 0
    spot = ltrace.default_hotspot(r_spot=8.0, sigma=4.0)
    Vs = ltrace.hotspot_visibility(hits, None, met, dk, spot, uv, False, 50.0, 1.0, 2)       # equal records, equal weights: the same zeros
    assert np.all(Vs[:, 0, [0, 1, 3, 5]] == 0) and np.all(Vs[:, 0, 2].real > 0) and np.all(Vs[:, 0, 2].imag == 0)
    hits[0, 1::2, 0] = np.nan                                             # weights (w, 0, w, 0)
    V = ltrace.disk_visibility(hits, None, met, dk, uv, False)
    assert V.shape == (1, 6) and V[0, 1] == 2 * w and V[0, 0] == 0 and V[0, 2] == 2 * w
    # the same row inside a larger frame, from column 1 of row 1 on: every phase turned by a quarter cycle per pixel of offset
    big = np.full((3, 7, 2, 4), np.nan, dtype=np.float32)
    big[1, 1:5, 0] = rec
    big[1, 1:5, 1] = rec                                                  # and a second slot: 2 w per pixel, unsplit
    n_hits = np.zeros((3, 7), dtype=np.uint8)
    n_hits[1, 1:5] = 2
    V = ltrace.disk_visibility(big, n_hits, met, dk, uv, False)
    assert V[0, 0] == 0 and V[0, 1] == 0 and V[0, 2] == 8 * w and V[0, 4] == 8 * (-1j) * w and V[0, 5] == 0


# ---- 5. Hermitian symmetry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip"))
def test_hermitian_symmetry_to_the_bit(name):
    c, hits, n_hits, ref, vref, met, dk = setup(name)
    uv = np.concatenate([BASELINES, np.random.default_rng(5).uniform(-0.5, 0.5, (55, 2))])
    for split in (False, True):
        a = ltrace.hotspot_visibility(hits, n_hits, met, dk, lt_spot(SPOT(c.M)), uv, split, *LC_GRIDS[0])
        b = ltrace.hotspot_visibility(hits, n_hits, met, dk, lt_spot(SPOT(c.M)), -uv, split, *LC_GRIDS[0])
        assert np.array_equal(b.real, a.real) and np.array_equal(b.imag, -a.imag)
        assert np.any(a.imag != 0)


# ---- 6. the links to what exists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "strip", "one"))
def test_zero_baseline_is_the_spectrum_and_the_light_curve(name):
    c, hits, n_hits, ref, vref, met, dk = setup(name)
    spot, dm = lt_spot(SPOT(c.M)), make_map(c, MAP_VARIANTS[0])
    worst = 0.0
    for split in (False, True):
        sp = diskmod.Spectrum(*GRIDS[1], split_orders=split).to_lt()
        n_terms = vref.counts(split)
        for lcg in LC_GRIDS[:2]:
            pairs = ((ltrace.hotspot_visibility(hits, n_hits, met, dk, spot, BASELINES, split, *lcg), ltrace.hotspot_spectrum(hits, n_hits, met, dk, spot, sp, *lcg)),
                     (ltrace.diskmap_visibility(hits, n_hits, met, dk, dm.to_lt(), dm.texels, BASELINES, split, *lcg),
                      ltrace.diskmap_spectrum(hits, n_hits, met, dk, dm.to_lt(), dm.texels, sp, *lcg)),
                     (ltrace.disk_visibility(hits, n_hits, met, dk, BASELINES, split)[None], ltrace.disk_spectrum(hits, n_hits, met, dk, sp)[None]))
            for V, spectrum in pairs:
                rows = spectrum.astype(LD).sum(axis=-1)                   # (times, planes)
                flux = V[..., 0].real.astype(LD)
                assert np.all(V[..., 0].imag == 0.0) and np.all((rows > 0) == (n_terms > 0)) and np.all((flux > 0) == (n_terms > 0))
                rel = np.abs(flux - rows) / np.where(rows > 0, rows, LD(1))
                worst = max(worst, float(np.max(rel / ((4 + n_terms) * U))))
                assert np.all(rel <= (4 + n_terms) * U)
                # the triangle inequality on non-negative weights
                bound = 2 * (phase_bound(c.R, c.W) + n_terms * U) + 4 * U
                assert np.all(np.abs(V) <= (V[..., 0].real * (1 + bound))[..., None])
    # the light curve's column 0, with the ramp at (1, 1, 1)
    bright = hits.copy()
    bright[..., 2] = (1.0 + 0.4 * (hits[..., 2].astype(np.float64) - 0.15) / 1.25).astype(np.float32)     # g into [1, 1.4]
    stored = np.arange(c.m) < np.minimum(n_hits, c.m)[..., None]
    assert bright[..., 2][stored].min() >= 1.0 and bright[..., 2][stored].max() <= np.float32(1.4)
    n_all = int(stored.sum())
    for lcg in LC_GRIDS[:2]:                                              # (times whose i dt is exact: the light curve may use an fma)
        pairs = ((ltrace.hotspot_visibility(bright, n_hits, met, dk, spot, BASELINES[:1], False, *lcg), ltrace.hotspot_lightcurve(bright, n_hits, met, dk, spot, *lcg)),
                 (ltrace.diskmap_visibility(bright, n_hits, met, dk, dm.to_lt(), dm.texels, BASELINES[:1], False, *lcg),
                  ltrace.diskmap_lightcurve(bright, n_hits, met, dk, dm.to_lt(), dm.texels, *lcg)))
        for V, lc in pairs:
            assert np.all(lc[:, 0] > 0)
            rel = np.abs(V[:, 0, 0].real.astype(LD) - lc[:, 0].astype(LD)) / lc[:, 0].astype(LD)
            worst = max(worst, float(np.max(rel / ((4 + n_all) * U))))
            assert np.all(rel <= (4 + n_all) * U)
    print(f"{name}: V(0, 0) against the spectrum's rows and the light curve, {worst:.4f} of (4 + n_terms) 2^-53")


# ---- 7. device pointers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "one"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c, hits, n_hits, ref, vref, met, dk = setup(name)
    d_hits, d_n = upload(hits), upload(n_hits)
    spot, dm = lt_spot(SPOT(c.M)), make_map(c, MAP_VARIANTS[1])
    d_tex = upload(dm.texels)
    lcg = LC_GRIDS[0]
    as_complex = lambda d: np.ascontiguousarray(d.get()).view(np.complex128)[..., 0]
    for split, counts in ((False, True), (True, False)):
        shape = (c.m if split else 1, 9, 2)
        nh, d_nh = (n_hits, d_n.ptr) if counts else (None, 0)
        d_out = hipmini.DeviceArray((1,) + shape, np.float64)
        ltrace.disk_visibility_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, BASELINES, split, d_out.ptr)
        assert as_complex(d_out)[0].tobytes() == ltrace.disk_visibility(hits, nh, met, dk, BASELINES, split).tobytes()
        d_out = hipmini.DeviceArray((lcg[2],) + shape, np.float64)
        ltrace.hotspot_visibility_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, spot, BASELINES, split, *lcg, d_out.ptr)
        assert as_complex(d_out).tobytes() == ltrace.hotspot_visibility(hits, nh, met, dk, spot, BASELINES, split, *lcg).tobytes()
        d_out = hipmini.DeviceArray((lcg[2],) + shape, np.float64)
        ltrace.diskmap_visibility_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm.to_lt(), d_tex.ptr, BASELINES, split, *lcg, d_out.ptr)
        assert as_complex(d_out).tobytes() == ltrace.diskmap_visibility(hits, nh, met, dk, dm.to_lt(), dm.texels, BASELINES, split, *lcg).tobytes()


# ---- 8. one real trace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [None, 2])
@pytest.mark.parametrize("emitter", ("spot", "map"))
def test_render_sequence_returns_the_recentred_entry_points_outputs(emitter, S):
    import image_lens
    from metrics import Kerr
    M, a = SEQ["M"], SEQ["a"]
    r_in = float(diskmod.isco(M, a))
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    spot = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5) if emitter == "spot" else None
    dmap = None if emitter == "spot" else diskmod.DiskMap(diskmod.spiral_map(32, 128, r_min=r_in, r_max=SEQ["r_out"]), r_min=r_in,
                                                         r_max=SEQ["r_out"], exposure=0.5)
    times = 100.0 + 25.0 * np.arange(3)
    kerr = Kerr(M=M, a=a, integrator="rk4", precision=32)
    outs = {}
    for split in (False, True):
        bl = diskmod.Baselines.radial(12, 0.5, 30.0, split_orders=split)
        out = image_lens.render_sequence(None, kerr, SEQ["r_obs"], SEQ["fov"], tdisk, spot, times, shape=SEQ["shape"], theta_obs=SEQ["theta_obs"],
                                         samples=S, diskmap=dmap, baselines=bl, spectrum=diskmod.Spectrum(0.3, 1.2, 7) if split else None)
        k = 1 if S is None else S
        planes = SEQ["max_images"] if split else 1
        assert out["visibility"].shape == (3, planes, 12) and out["disk_visibility"].shape == (planes, 12)
        assert out["visibility"].dtype == np.complex128 and out["disk_visibility"].dtype == np.complex128
        assert out["hits"].shape == (SEQ["shape"][0] * k, SEQ["shape"][1] * k, SEQ["max_images"], 4)
        assert ("spectrum" in out) == split
        met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
        uv = bl.uv / np.float64(k)
        if emitter == "spot":
            dyn = ltrace.hotspot_visibility(out["hits"], out["n_hits"], met, dk, spot.to_lt(), uv, split, 100.0, 25.0, 3)
        else:
            dyn = ltrace.diskmap_visibility(out["hits"], out["n_hits"], met, dk, dmap.to_lt(), dmap.texels, uv, split, 100.0, 25.0, 3)
        assert np.array_equal(out["visibility"], bl.recentre(dyn, SEQ["shape"], k))
        assert np.array_equal(out["disk_visibility"], bl.recentre(ltrace.disk_visibility(out["hits"], out["n_hits"], met, dk, uv, split), SEQ["shape"], k))
        assert len({out["visibility"][i].tobytes() for i in range(3)}) == 3                           # the visibilities move
        assert np.all(out["visibility"][:, :2, 0].real > 0) and np.all(out["visibility"][..., 0].imag == 0)
        outs[split] = out
    per, one = outs[True], outs[False]
    assert np.all(np.abs(per["visibility"][:, 1]).sum(axis=-1) > 0)                                   # the first lensed image holds light
    scale = np.abs(one["visibility"][:, :, :1])
    assert np.all(np.abs(per["visibility"].sum(axis=1, keepdims=True) - one["visibility"]) <= 1e-12 * scale)
    assert np.all(np.abs(per["disk_visibility"].sum(axis=0) - one["disk_visibility"][0]) <= 1e-12 * np.abs(one["disk_visibility"][0, 0]))


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, ref, vref, met, dk = setup("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    good_map = make_map(c, MAP_VARIANTS[0])
    good_spot = lt_spot(SPOT(c.M))
    good_uv = np.ascontiguousarray(BASELINES)

    def call(form, hits_=hits, met_=met, disk_=dk, emit=None, tex=good_map.texels, R=c.R, W=c.W, m=c.m, uv_=good_uv, n_b=None, t_start=0.0,
             dt=1.0, n_times=2, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full((4, 8, 1025, 2), -7.0)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        head = (ptr(hits_), ptr(n_hits), R, W, m, ref_(met_), ref_(disk_))
        uv_args = (ptr(uv_), (0 if uv_ is None else uv_.shape[0]) if n_b is None else n_b, 1)
        o = None if null_out else ptr(out)
        if form == "disk":
            rc = lib.lt_disk_visibility(*head, *uv_args, o)
        elif form == "spot":
            rc = lib.lt_hotspot_visibility(*head, ref_(good_spot if emit is None else emit), *uv_args, t_start, dt, n_times, o)
        else:
            rc = lib.lt_diskmap_visibility(*head, ref_(good_map.to_lt() if emit is None else emit), ptr(tex), *uv_args, t_start, dt, n_times, o)
        if rc != ltrace.OK:
            assert np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    for form in ("disk", "spot", "map"):
        assert call(form)[0] == ltrace.OK
    nan, inf = float("nan"), float("inf")
    INV = ltrace.ERR_INVALID_ARG
    with_uv = lambda i, u, v: np.concatenate([good_uv[:i], [(u, v)], good_uv[i:]])
    long_uv = np.zeros((1025, 2))
    map_with = lambda **kw: diskmod.DiskMap(good_map.texels, **{**dict(r_min=good_map.r_min, r_max=good_map.r_max, rotation=good_map.rotation,
                                                                       exposure=good_map.exposure), **kw}).to_lt()
    rot7 = good_map.to_lt()
    rot7.rotation = 7
    head = [(dict(hits_=None), INV, "null"), (dict(met_=None), INV, "null"), (dict(disk_=None), INV, "null")]
    frame = [(dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"), (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), INV, "bad metric"),
             (dict(R=0), INV, "empty frame"), (dict(W=-3), INV, "empty frame"), (dict(m=0), INV, "max_images"), (dict(m=9), INV, "max_images")]
    emitter = dict(disk=([], []),
                   spot=([(dict(emit="null"), INV, "null")],
                         [(dict(emit=ltrace.default_hotspot(sigma=0.0)), INV, "sigma"), (dict(emit=ltrace.default_hotspot(r_spot=-1.0)), INV, "r_spot")]),
                   map=([(dict(emit="null"), INV, "null"), (dict(tex=None), INV, "null")],
                        [(dict(emit=map_with(r_min=0.0)), INV, "r_min"), (dict(emit=map_with(exposure=-1.0)), INV, "map exposure"),
                         (dict(emit=rot7), INV, "rotation")]))
    tail = [(dict(disk_=ltrace.default_disk(q=nan)), INV, "disk q"), (dict(disk_=ltrace.default_disk(exposure=-1.0)), INV, "disk q"),
            (dict(uv_=None, n_b=9), INV, "null uv"), (dict(n_b=0), INV, "n_baselines"), (dict(uv_=long_uv), INV, "n_baselines"),
            (dict(uv_=with_uv(3, 0.5000001, 0.0)), INV, "baseline 3"), (dict(uv_=with_uv(9, 0.0, -0.5000001)), INV, "baseline 9"),
            (dict(uv_=with_uv(0, nan, 0.0)), INV, "baseline 0"), (dict(uv_=with_uv(1, 0.0, inf)), INV, "baseline 1")]
    times = [(dict(n_times=-1), INV, "n_times"), (dict(n_times=65536), INV, "n_times"), (dict(t_start=nan), INV, "t_start"), (dict(dt=inf), INV, "t_start")]
    last = [(dict(null_out=True), INV, "null out")]
    for form in ("disk", "spot", "map"):
        nulls, fields = emitter[form]
        seq = head + nulls + frame + fields + tail + ([] if form == "disk" else times) + last
        for i, (kw, code, word) in enumerate(seq):
            rc, msg = call(form, **kw)
            assert rc == code and word in msg, (form, kw, rc, msg)
            for kw2, _, word2 in seq[i + 1:]:                           # with a later fault present as well, the earlier one decides
                if set(kw) & set(kw2) or word2.split()[0] == word.split()[0]:
                    continue
                rc, msg = call(form, **kw, **kw2)
                assert rc == code and word in msg, (form, kw, kw2, rc, msg)
    # no times: nothing to do, nothing written, even without an output
    for form in ("spot", "map"):
        assert call(form, n_times=0)[0] == ltrace.OK and call(form, n_times=0, null_out=True)[0] == ltrace.OK
    d_hits = upload(hits)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.hotspot_visibility_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, good_spot, good_uv, True, 0.0, 1.0, 2, 0)
    assert ei.value.code == INV and "null out" in str(ei.value)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.disk_visibility_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, with_uv(2, 0.7, 0.0), False, 0)
    assert ei.value.code == INV and "baseline 2" in str(ei.value)
