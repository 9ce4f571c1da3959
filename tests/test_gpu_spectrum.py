"""The spectrum kernels (lt_spectrum.hpp) through lt_disk_spectrum[_dev], lt_hotspot_spectrum[_dev] and
lt_diskmap_spectrum[_dev].  Grids, the longdouble reference and the bounds are tests/test_spectrum_host.py's (its header
derives the bounds); the records are test_diskmap_host.CASES' -- 257 x 331 x 8 (a second, partial pass of the stride loop,
W odd), 260 x 300 x 3, 3 x 70 x 5, 1 x 1 x 1, counts above max_images -- and the 96 x 80 trace of test_gpu_diskmap.py.

Batches.  The first stage's partials are LT_SPECTRUM_BLOCKS histograms of float64 per time inside
LT_SPECTRUM_WORKSPACE_BYTES: at the largest key count, 8 planes of 514 columns, ltrace.spectrum_batch_times gives
64 MiB / (256 x 4112 x 8 B) = 7 times, so 9 times run as two batches (7 + 2) and nothing needs lowering for the test.

The link to the light curve (test_rows_sum_to_the_light_curve), derived: with every g in [1, 1.4] the ramp is (1, 1, 1),
the light curve's term is (I + I + I) / 3 -- two roundings, within 2 x 2^-53 of I -- and both sides add the same n_terms
non-negative terms in their own orders: within (4 + n_terms) 2^-53 relative of each other.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES, LC_GRIDS, grid_times, make_map, map_lc_bound, records
from test_gpu_diskmap import SEQ, traced, upload
from test_hotspot_records_host import isco_ref, lc_bound
from test_spectrum_host import DISK_EXPOSURE, EDGE_GRID, GRIDS, MAP_VARIANTS, SPOT, SpectrumReference, U, check_spectrum, edge_values

pytestmark = pytest.mark.gpu
LD = np.longdouble
BIG_GRID = GRIDS[3]                                           # 512 bins: split on the max_images = 8 case it has 4112 keys
_REF = {}


def setup(name):
    c = CASES[name]
    hits, n_hits, _ = records(name)
    if name not in _REF:
        _REF[name] = SpectrumReference(hits, n_hits)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a)
    dk = ltrace.default_disk(r_out=c.r_out, exposure=DISK_EXPOSURE)      # r_in 0: the ISCO, resolved by the library
    return c, hits, n_hits, _REF[name], met, dk


def lt_spot(spot):
    return ltrace.default_hotspot(r_spot=spot[0], phi0=spot[1], sigma=spot[2], exposure=spot[3], with_disk=int(spot[4]))


def lt_spec(grid, split=False):
    return diskmod.Spectrum(*grid, split_orders=split).to_lt()


# ---- 1. against the reference ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_spectra_against_the_reference(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    spot = SPOT(c.M)
    r_in = float(isco_ref(c.M, c.a))
    disk_w = ref.disk_weights(r_in, 3.0, DISK_EXPOSURE)
    spot_w = {float(t): ref.spot_weights(c.M, c.a, spot, t) for g in LC_GRIDS for t in grid_times(g)}
    maps = [make_map(c, v) for v in MAP_VARIANTS]
    map_w = {(vi, float(t)): ref.map_weights(c.M, c.a, dm, t) for vi, dm in enumerate(maps) for g in LC_GRIDS[:2] for t in grid_times(g)}
    worst = dict(disk=(0.0, 0.0), spot=(0.0, 0.0), map=(0.0, 0.0))
    note = lambda who, pair: worst.__setitem__(who, max(worst[who], pair))
    for grid in GRIDS:
        for split in (False, True):
            sp = lt_spec(grid, split)
            counts = ref.keys(grid, split)[3]
            vi, dm = int(split), maps[int(split)]                         # Keplerian unsplit, rigid split
            want_disk = ref.bin(disk_w, grid, split)
            want_spot = [np.stack([ref.bin(spot_w[float(t)], grid, split) for t in grid_times(lcg)]) for lcg in LC_GRIDS]
            want_map = [np.stack([ref.bin(map_w[(vi, float(t))], grid, split) for t in grid_times(lcg)]) for lcg in LC_GRIDS[:2]]
            for nh in (n_hits, None) if grid == BIG_GRID else (n_hits if split else None,):
                note("disk", check_spectrum(ltrace.disk_spectrum(hits, nh, met, dk, sp), want_disk, counts, 1e-12))
                for lcg, want in zip(LC_GRIDS, want_spot):
                    got = ltrace.hotspot_spectrum(hits, nh, met, dk, lt_spot(spot), sp, *lcg)
                    note("spot", check_spectrum(got, want, counts, lc_bound(c.M, c.a, spot, grid_times(lcg), c.r_out)))
                for lcg, want in zip(LC_GRIDS[:2], want_map):
                    got = ltrace.diskmap_spectrum(hits, nh, met, dk, dm.to_lt(), dm.texels, sp, *lcg)
                    note("map", check_spectrum(got, want, counts, map_lc_bound(c.M, c.a, dm, grid_times(lcg), float(diskmod.isco(c.M, c.a)))))
    if c.m == 8:
        assert ref.keys(BIG_GRID, True)[3].size == 4112                  # the largest key count there is
    for who, (excess, rel) in worst.items():
        print(f"{name} {who}: spectrum against longdouble, largest relative difference {rel:.2e}, {excess:.3f} of its bound")
        assert excess <= 1


# ---- 2. reproducible and batch-independent -------------------------------------------------------------------------------------
@pytest.mark.parametrize("emitter", ("spot", "map"))
def test_rows_do_not_depend_on_their_batch(emitter):
    c, hits, n_hits, ref, met, dk = setup("big")
    sp = lt_spec(BIG_GRID, True)
    per_batch = ltrace.spectrum_batch_times(sp, c.m)
    assert per_batch == ltrace.SPECTRUM_WORKSPACE_BYTES // (ltrace.SPECTRUM_BLOCKS * 4112 * 8) == 7
    n_times = per_batch + 2                                              # two batches, the second partial
    t_start, dt = 333.25, 0.1                                            # (i dt is not exact: an fma would give another time)
    if emitter == "spot":
        run = lambda t0, n: ltrace.hotspot_spectrum(hits, n_hits, met, dk, lt_spot(SPOT(c.M)), sp, t0, dt, n)
    else:
        dm = make_map(c, MAP_VARIANTS[0])
        run = lambda t0, n: ltrace.diskmap_spectrum(hits, n_hits, met, dk, dm.to_lt(), dm.texels, sp, t0, dt, n)
    whole = run(t_start, n_times)
    assert whole.shape == (n_times, 8, 514) and np.all(whole.sum(axis=(1, 2)) > 0)
    assert run(t_start, n_times).tobytes() == whole.tobytes()             # a second call differs in no bit
    for i in range(n_times):
        alone = run(t_start + i * dt, 1)
        assert alone[0].tobytes() == whole[i].tobytes(), i
    assert len({whole[i].tobytes() for i in range(n_times)}) == n_times   # the rows are different rows
    small = lt_spec(GRIDS[0], False)                                      # one batch of a small grid against the rows alone
    if emitter == "spot":
        a = ltrace.hotspot_spectrum(hits, None, met, dk, lt_spot(SPOT(c.M)), small, t_start, dt, 3)
        b = [ltrace.hotspot_spectrum(hits, None, met, dk, lt_spot(SPOT(c.M)), small, t_start + i * dt, dt, 1)[0] for i in range(3)]
        assert a.tobytes() == np.stack(b).tobytes()


# ---- 3. exact edges on the device ------------------------------------------------------------------------------------------------
def test_exact_edges_on_the_device():
    """The host test's grid and g values in otherwise synthetic records of weight g^4: the disk with q = 0 and exposure 1
    (pow(x, 0) = 1, so the weight is (g^2)^2 in float64 and the sums are predicted to the bit), a one-texel map of 1 and
    exposure 1 (m is 1 within 2 ulp), and the spot (the populated columns)."""
    g, cols = edge_values()
    n = g.size
    hits = np.empty((1, n, 2, 4), dtype=np.float32)
    hits[..., 0], hits[..., 1], hits[..., 3] = 8.0, 1.0, 100.0
    hits[0, :, 0, 2], hits[0, :, 1, 2] = g, g[::-1]                       # slot 1: the same values in the other order
    n_hits = np.full((1, n), 2, dtype=np.uint8)
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(q=0.0, exposure=1.0)
    g4 = (g.astype(np.float64) * g.astype(np.float64)) ** 2
    want = np.zeros((2, 10))
    for plane, order in enumerate((np.arange(n), np.arange(n)[::-1])):
        for i in order:                                                   # lane order within the slot
            if cols[i] >= 0:
                want[plane, cols[i]] += g4[i]
    assert np.count_nonzero(want[0]) == 4 and np.array_equal(want[0] > 0, want[1] > 0)
    split, whole = lt_spec(EDGE_GRID, True), lt_spec(EDGE_GRID, False)
    got = ltrace.disk_spectrum(hits, n_hits, met, dk, split)
    assert got.tobytes() == want.tobytes()
    got = ltrace.disk_spectrum(hits, None, met, dk, whole)                # (slot 0 then slot 1 per column; two terms each way)
    assert got.shape == (1, 10) and np.all(np.abs(got[0] - want.sum(axis=0)) <= 4 * U * want.sum(axis=0))
    assert np.array_equal(got[0] > 0, want[0] > 0)
    dm = diskmod.DiskMap(np.ones((1, 1), np.float32), r_min=2.0, r_max=20.0, exposure=1.0)
    got = ltrace.diskmap_spectrum(hits, n_hits, met, dk, dm.to_lt(), dm.texels, split, 50.0, 1.0, 2)
    assert got.shape == (2, 2, 10) and np.array_equal(got > 0, np.stack([want > 0] * 2))
    assert np.all(np.abs(got - want) <= 4 * U * want)
    spot = ltrace.default_hotspot(r_spot=8.0, sigma=4.0)
    got = ltrace.hotspot_spectrum(hits, n_hits, met, dk, spot, split, 50.0, 1.0, 2)
    assert np.array_equal(got > 0, np.stack([want > 0] * 2)) and np.all(got <= want)      # exp(...) <= 1


# ---- 4. the link to the existing light curve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "strip", "one"))
def test_rows_sum_to_the_light_curve(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    bright = hits.copy()
    bright[..., 2] = (1.0 + 0.4 * (hits[..., 2].astype(np.float64) - 0.15) / 1.25).astype(np.float32)     # g into [1, 1.4]
    stored = np.arange(c.m) < np.minimum(n_hits, c.m)[..., None]
    assert bright[..., 2][stored].min() >= 1.0 and bright[..., 2][stored].max() <= np.float32(1.4)
    n_terms = int(stored.sum())
    spot, dm = lt_spot(SPOT(c.M)), make_map(c, MAP_VARIANTS[0])
    worst = 0.0
    for lcg in LC_GRIDS[:2]:                                              # (times whose i dt is exact: the light curve may use an fma)
        for grid, split in ((GRIDS[1], False), (GRIDS[0], True)):
            sp = lt_spec(grid, split)
            pairs = ((ltrace.hotspot_spectrum(bright, n_hits, met, dk, spot, sp, *lcg), ltrace.hotspot_lightcurve(bright, n_hits, met, dk, spot, *lcg)),
                     (ltrace.diskmap_spectrum(bright, n_hits, met, dk, dm.to_lt(), dm.texels, sp, *lcg),
                      ltrace.diskmap_lightcurve(bright, n_hits, met, dk, dm.to_lt(), dm.texels, *lcg)))
            for spectrum, lc in pairs:
                rows = spectrum.astype(LD).sum(axis=(1, 2))
                assert np.all(lc[:, 0] > 0)
                rel = np.abs(rows - lc[:, 0].astype(LD)) / lc[:, 0].astype(LD)
                worst = max(worst, float(rel.max()))
                assert np.all(rel <= (4 + n_terms) * U)
    print(f"{name}: spectrum rows against the light curve's column 0, largest relative difference {worst:.2e}, bound {(4 + n_terms) * U:.2e}")


# ---- 5. device pointers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "one"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c, hits, n_hits, ref, met, dk = setup(name)
    d_hits, d_n = upload(hits), upload(n_hits)
    spot, dm = lt_spot(SPOT(c.M)), make_map(c, MAP_VARIANTS[1])
    d_tex = upload(dm.texels)
    lcg = LC_GRIDS[0]
    for grid, split, counts in ((GRIDS[0], False, True), (BIG_GRID, True, False), (GRIDS[1], True, True)):
        sp = lt_spec(grid, split)
        shape = (c.m if split else 1, grid[2] + 2)
        nh, d_nh = (n_hits, d_n.ptr) if counts else (None, 0)
        d_out = hipmini.DeviceArray((1,) + shape, np.float64)
        ltrace.disk_spectrum_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, sp, d_out.ptr)
        assert d_out.get()[0].tobytes() == ltrace.disk_spectrum(hits, nh, met, dk, sp).tobytes()
        d_out = hipmini.DeviceArray((lcg[2],) + shape, np.float64)
        ltrace.hotspot_spectrum_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, spot, sp, *lcg, d_out.ptr)
        assert d_out.get().tobytes() == ltrace.hotspot_spectrum(hits, nh, met, dk, spot, sp, *lcg).tobytes()
        d_out = hipmini.DeviceArray((lcg[2],) + shape, np.float64)
        ltrace.diskmap_spectrum_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm.to_lt(), d_tex.ptr, sp, *lcg, d_out.ptr)
        assert d_out.get().tobytes() == ltrace.diskmap_spectrum(hits, nh, met, dk, dm.to_lt(), dm.texels, sp, *lcg).tobytes()


# ---- 6. one real trace --------------------------------------------------------------------------------------------------------------
def test_traced_line_and_dynamic_spectrum():
    hits, n_hits, met, dk = traced()
    M, a = SEQ["M"], SEQ["a"]
    grid = diskmod.Spectrum()
    centres = grid.energies(1.0)
    line = ltrace.disk_spectrum(hits, n_hits, met, dk, grid.to_lt())
    assert line.shape == (1, 98) and line[0, 0] == 0 and line[0, -1] == 0
    assert line[0, 1:-1][centres > 1.0].sum() > 0 and line[0, 1:-1][centres < 0.7].sum() > 0          # the blue horn at 80 deg, the red wing
    want = diskmod.disk_spectrum(M, a, hits, n_hits, diskmod.ThinDisk(r_out=SEQ["r_out"]), grid)
    assert np.all(np.abs(line - want) <= 1e-11 * want) and np.array_equal(line > 0, want > 0)
    spot = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5, exposure=1.0)
    period = 2 * np.pi / float(diskmod.omega(M, a, 9.0))
    n = 16
    dyn = ltrace.hotspot_spectrum(hits, n_hits, met, dk, spot.to_lt(), grid.to_lt(), 100.0, period / n, n)
    flux = dyn[:, 0, 1:-1]
    assert np.all(flux.sum(axis=1) > 0)
    mean_g = (flux * centres).sum(axis=1) / flux.sum(axis=1)
    print(f"traced 96 x 80 frame, spot at r = 9: flux-weighted mean g over one period {mean_g.min():.3f} ... {mean_g.max():.3f}")
    assert mean_g.max() - mean_g.min() >= 0.1
    per = ltrace.hotspot_spectrum(hits, n_hits, met, dk, spot.to_lt(), diskmod.Spectrum(split_orders=True).to_lt(), 100.0, period / n, n)
    assert per.shape == (n, SEQ["max_images"], 98) and per[:, 1].sum() > 0                           # the first lensed image holds light
    assert np.all(np.abs(per.sum(axis=1) - dyn[:, 0]) <= 1e-12 * dyn[:, 0])


@pytest.mark.parametrize("S", [None, 2])
@pytest.mark.parametrize("emitter", ("spot", "map"))
def test_render_sequence_returns_the_entry_points_outputs(emitter, S):
    import image_lens
    from metrics import Kerr
    M, a = SEQ["M"], SEQ["a"]
    r_in = float(diskmod.isco(M, a))
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    spot = diskmod.HotSpot(r_spot=9.0, phi0=0.5, sigma=1.5) if emitter == "spot" else None
    dmap = None if emitter == "spot" else diskmod.DiskMap(diskmod.spiral_map(32, 128, r_min=r_in, r_max=SEQ["r_out"]), r_min=r_in,
                                                         r_max=SEQ["r_out"], exposure=0.5)
    times = 100.0 + 25.0 * np.arange(3)
    grid = diskmod.Spectrum(0.3, 1.2, 7, split_orders=emitter == "map")
    out = image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk, spot, times,
                                     shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], samples=S, diskmap=dmap, spectrum=grid)
    k = 1 if S is None else S
    planes = SEQ["max_images"] if grid.split_orders else 1
    assert out["spectrum"].shape == (3, planes, 9) and out["disk_spectrum"].shape == (planes, 9)
    assert out["hits"].shape == (SEQ["shape"][0] * k, SEQ["shape"][1] * k, SEQ["max_images"], 4)
    met, dk, sp = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt(), grid.to_lt()
    if emitter == "spot":
        dyn = ltrace.hotspot_spectrum(out["hits"], out["n_hits"], met, dk, spot.to_lt(), sp, 100.0, 25.0, 3)
    else:
        dyn = ltrace.diskmap_spectrum(out["hits"], out["n_hits"], met, dk, dmap.to_lt(), dmap.texels, sp, 100.0, 25.0, 3)
    assert np.array_equal(out["spectrum"], dyn / np.float64(k * k))
    assert np.array_equal(out["disk_spectrum"], ltrace.disk_spectrum(out["hits"], out["n_hits"], met, dk, sp) / np.float64(k * k))
    assert np.all(out["spectrum"].sum(axis=(1, 2)) > 0) and out["disk_spectrum"].sum() > 0
    assert len({out["spectrum"][i].tobytes() for i in range(3)}) == 3                               # the spectrum moves


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, ref, met, dk = setup("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    good_map = make_map(c, MAP_VARIANTS[0])
    good_spot = lt_spot(SPOT(c.M))
    good_spec = lt_spec(GRIDS[0], True)

    def call(form, hits_=hits, met_=met, disk_=dk, emit=None, tex=good_map.texels, R=c.R, W=c.W, m=c.m, spec_=good_spec, t_start=0.0, dt=1.0,
             n_times=2, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full((4, 8, 514), -7.0)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        head = (ptr(hits_), ptr(n_hits), R, W, m, ref_(met_), ref_(disk_))
        o = None if null_out else ptr(out)
        if form == "disk":
            rc = lib.lt_disk_spectrum(*head, ref_(spec_), o)
        elif form == "spot":
            rc = lib.lt_hotspot_spectrum(*head, ref_(good_spot if emit is None else emit), ref_(spec_), t_start, dt, n_times, o)
        else:
            rc = lib.lt_diskmap_spectrum(*head, ref_(good_map.to_lt() if emit is None else emit), ptr(tex), ref_(spec_), t_start, dt, n_times, o)
        if rc != ltrace.OK:
            assert np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    for form in ("disk", "spot", "map"):
        assert call(form)[0] == ltrace.OK
    nan, inf = float("nan"), float("inf")
    INV = ltrace.ERR_INVALID_ARG
    spec = lambda **kw: ltrace.default_spectrum(**{**dict(g_min=0.3, g_max=1.2, n_bins=7, split_orders=1), **kw})
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
            (dict(spec_="null"), INV, "null spec"), (dict(spec_=spec(g_min=0.0)), INV, "g_min"), (dict(spec_=spec(g_min=nan)), INV, "g_min"),
            (dict(spec_=spec(g_max=0.3)), INV, "g_min"), (dict(spec_=spec(g_max=inf)), INV, "g_min"),
            (dict(spec_=spec(n_bins=0)), INV, "n_bins"), (dict(spec_=spec(n_bins=513)), INV, "n_bins")]
    times = [(dict(n_times=-1), INV, "n_times"), (dict(n_times=65536), INV, "n_times"), (dict(t_start=nan), INV, "t_start"), (dict(dt=inf), INV, "t_start")]
    last = [(dict(null_out=True), INV, "null out")]
    for form in ("disk", "spot", "map"):
        nulls, fields = emitter[form]
        seq = head + nulls + frame + fields + tail + ([] if form == "disk" else times) + last
        for i, (kw, code, word) in enumerate(seq):
            rc, msg = call(form, **kw)
            assert rc == code and word in msg, (form, kw, rc, msg)
            for kw2, _, word2 in seq[i + 1:]:                           # with a later fault present as well, the earlier one decides
                if set(kw) & set(kw2) or word2 == word:
                    continue
                rc, msg = call(form, **kw, **kw2)
                assert rc == code and word in msg, (form, kw, kw2, rc, msg)
    # a bad grid with bad times: the grid decides; no times: nothing to do, nothing written, even without an output
    for form in ("spot", "map"):
        out_untouched = call(form, n_times=0)
        assert out_untouched[0] == ltrace.OK and call(form, n_times=0, null_out=True)[0] == ltrace.OK
    d_hits = upload(hits)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.hotspot_spectrum_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, good_spot, good_spec, 0.0, 1.0, 2, 0)
    assert ei.value.code == INV and "null out" in str(ei.value)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.disk_spectrum_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, spec(n_bins=600), 0)
    assert ei.value.code == INV and "n_bins" in str(ei.value)
