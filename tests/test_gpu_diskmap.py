"""The rotating emissivity map's kernels (lt_diskmap.hpp) through lt_shade_diskmap[_dev], lt_shade_diskmap_aa[_dev] and
lt_diskmap_lightcurve[_dev].  Cases, tables, variants, the longdouble reference and the bounds are
tests/test_diskmap_host.py's (its header derives the bounds); the records are synthetic at the sizes that reach the
kernels' edges -- 257 x 331 x 8 (a second, partial pass of the light curve's 65 536-pixel stride, W odd), 260 x 300 x 3,
3 x 70 x 5, 1 x 1 x 1, counts above max_images -- and one real 96 x 80 trace for the cross-check against the hot spot's
kernel, which pins the signs of rotation and delay.

The cross-check's bound (test_rigid_gaussian_table_is_the_hot_spot), derived: a rigid table whose texels are the spot's
Gaussian w at t = 0, turning at the spot's Omega, is the spot up to the bilinear interpolation of w.  Linear interpolation
over a cell of size h errs by at most h^2 / 8 max|w''|; |d^2 w / dr^2| <= 1 / sigma^2 and |d^2 w / dpsi^2| <=
1.74 r_max r_s / sigma^2 over the annulus; the float32 texels add 2^-24 (w <= 1):
    B = h_r^2 / (8 sigma^2) + h_phi^2 1.74 r_max r_s / (8 sigma^2) + 2^-24,    |d rgb| <= sum_j exposure g_j^4 B + 2 ulp
per pixel and channel (ramp <= 1; the clamp to [0, 1] does not increase a difference).  B = 1.0e-3 at 256 x 1024.

Mass scaling (test_scaling_with_mass).  Doubling r, dt, t, r_min, r_max and a at M = 2 and halving omega_p is exact in
binary floating point, and under rigid rotation every intermediate of the rule is then the M = 1 one or its exact double /
half: the light curve differs in no bit.  Under Keplerian rotation Omega(r) is computed from r with two square roots,
sqrt(2 r) is not the double of a float64 sqrt(r), so the phase differs in its last bits and the curves agree within twice
the light curve's bound (each is within the bound of the exact curve); both are asserted.

MEASURED on an MI355X (gfx950), the figures the tests print:
    frames against longdouble: no float32 differs (0.00 ulp) on big, mid, strip and one; bound 2.  The traced frame against
        the numpy statement: 1.00 ulp (bound 2), 10 533 lit, unsaturated values;
    light curves against longdouble, largest relative difference / its bound, all at the Keplerian 37 x 64 table and t = 1e5:
        big 1.3e-14 / 4.1e-10, mid 8.0e-15 / 8.1e-11, strip 1.7e-13 / 1.1e-10, one 1.2e-12 / 4.1e-10; never above 4 % of a bound;
        the traced frame 5.0e-14 / 6.5e-9;
    sum of a frame against the light curve: at most 1.4e-8 (bound 2^-23 = 1.19e-7), brightest pixel 0.40;
    M = 1 against M = 2: rigid, no bit differs; Keplerian, at most 2.1e-14 relative (bound 2.2e-10 there);
    rigid Gaussian table against lt_shade_hotspot on the traced frame: B = 9.26e-4, largest difference 0.36 of the pixel's
        bound, the brightest spot pixel 1058 times its bound.
"""
import ctypes as C

import numpy as np
import pytest

import aa
import disk as diskmod
import ltrace
from test_diskmap_host import (CASES, DISK_EXPOSURE, LC_GRIDS, MAP_EXPOSURE, TABLES, VARIANTS, MapReference, base_of, grid_times, make_map,
                               map_lc_bound, records, table)
from test_hotspot_records_host import isco_ref, lc_excess, synth, ulps

pytestmark = pytest.mark.gpu
LD = np.longdouble
_TRACE = {}


def setup(name):
    c = CASES[name]
    hits, n_hits, ref = records(name)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a)
    dk = ltrace.default_disk(r_out=c.r_out, exposure=DISK_EXPOSURE)      # r_in 0: the ISCO, resolved by the library
    return c, hits, n_hits, ref, met, dk


def upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(a.ctypes.data), a.nbytes, 1), "hipMemcpy H2D")
    return d


def check_rgba(rgba, ref32):
    """RGBA8 = floor(255 rgb), equal except where the float value lies within 2 ulp of a rounding boundary; alpha 255."""
    c3 = ref32 if ref32.ndim == 3 else np.repeat(ref32[..., None], 3, axis=-1)
    want = (c3 * np.float32(255.0)).astype(np.uint8)
    x = c3.astype(np.float64) * 255.0
    near = np.abs(x - np.rint(x)) <= 2 * 255.0 * np.spacing(c3).astype(np.float64) + 1e-12
    assert np.all((rgba[..., :3] == want) | near) and np.all(rgba[..., 3] == 255)


def replicate(a, S):
    return np.repeat(np.repeat(a, S, axis=0), S, axis=1)


# ---- 1. frames against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_frames_against_the_reference(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(isco_ref(c.M, c.a))
    worst, inside = 0.0, 0
    for v in VARIANTS:
        dmap, base = make_map(c, v), base_of(c, v)
        got = ltrace.shade_diskmap(hits, n_hits if v.counts else None, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base,
                                   channels=v.channels)
        want = ref.frame(c.M, c.a, dmap, v.t_obs, r_in, 3.0, DISK_EXPOSURE, base=base, channels=v.channels).astype(np.float32)
        assert got["rgb"].shape == want.shape and got["rgb"].dtype == np.float32
        worst = max(worst, float(np.max(ulps(got["rgb"], want))))
        check_rgba(got["rgba"], want)
        inside += int(((want > (0 if base is None else base)) & (want < 1)).sum())
    print(f"{name}: frames against longdouble, largest difference {worst:.2f} ulp of float32; {inside} lit, unsaturated values")
    assert worst <= 2
    assert inside >= (1 if c.R * c.W == 1 else 0.2 * c.R * c.W)


# ---- 2. light curves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lightcurve_against_the_reference(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(diskmod.isco(c.M, c.a))
    for v in VARIANTS[:2] if c.R * c.W > 1000 else VARIANTS:
        dmap = make_map(c, v)
        for grid in LC_GRIDS:
            times = grid_times(grid)
            lc = ltrace.diskmap_lightcurve(hits, n_hits if v.counts else None, met, dk, dmap.to_lt(), dmap.texels, *grid)
            assert lc.shape == (grid[2], 3)
            again = ltrace.diskmap_lightcurve(hits, n_hits if v.counts else None, met, dk, dmap.to_lt(), dmap.texels, *grid)
            assert again.tobytes() == lc.tobytes()                       # a second run differs in no bit
            want = ref.lightcurve(c.M, c.a, dmap, times)
            bound = map_lc_bound(c.M, c.a, dmap, times, r_in)
            excess, rel = lc_excess(lc, want, bound)
            print(f"{name} {v.rotation} {TABLES[v.table]} t = {grid[0]:g} ...: light curve against longdouble, largest relative "
                  f"difference {rel:.2e}, bound {bound:.2e}")
            assert np.all(want[:, 0] > 0)
            assert excess <= 1


@pytest.mark.parametrize("name", list(CASES))
def test_frame_sums_to_the_lightcurve(name):
    """Without disk and base, one channel, unclamped (the reference's brightest pixel is below 1): a frame's pixels are the
    light curve's terms rounded to float32, so their sums agree to 2^-23 (non-negative terms, each within 2^-24)."""
    c, hits, n_hits, ref, met, dk = setup(name)
    ix, iy = np.meshgrid(np.arange(c.W), np.arange(c.R))
    worst = 0.0
    for v in (VARIANTS[1], VARIANTS[4]):                                  # rigid 37 x 64 and Keplerian 5 x 1, both without the disk
        dmap = make_map(c, v, exposure=0.02)
        brightest = float(ref.frame(c.M, c.a, dmap, v.t_obs, 0.0, channels=1, clamp=False).max())
        assert brightest < 1
        rgb = ltrace.shade_diskmap(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, channels=1, want=("rgb",))["rgb"].astype(LD)
        lc = ltrace.diskmap_lightcurve(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, 1.0, 1)[0].astype(LD)
        assert lc[0] > 0
        for col, wgt in enumerate((1, ix, iy)):
            s = (rgb * wgt).sum()
            assert abs(s - lc[col]) <= LD(2.0 ** -23) * lc[col]
            if lc[col] > 0:
                worst = max(worst, float(abs(s - lc[col]) / lc[col]))
    print(f"{name}: brightest pixel {brightest:.3f}; sum of the frame against the light curve, largest relative difference {worst:.2e}")


def test_scaling_with_mass():
    """Records and map at M = 1, a = 0.6 against (r, dt, t, r_min, r_max, a) doubled and omega_p halved at M = 2 (doubling
    is exact in float32 and float64, so the two inputs state one scene).  Rigid rotation: no bit of the light curve
    differs.  Keplerian rotation: Omega(r) is recomputed from the doubled r and rounds differently (file header), so the
    curves agree within twice the light curve's bound."""
    R, W, m, M, a, r_out = 260, 300, 2, 1.0, 0.6, 20.0
    r_in = ltrace.kerr_isco(M, a)
    hits, n_hits = synth(R, W, m, 41, r_in, r_out)
    twice = hits.copy()
    twice[..., 0] *= 2
    twice[..., 3] *= 2
    one = (ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), ltrace.default_disk(r_in=r_in, r_out=r_out))
    two = (ltrace.Metric(ltrace.METRIC_KERR, 0, 2 * M, 2 * a), ltrace.default_disk(r_in=2 * r_in, r_out=2 * r_out))
    for rotation in ("rigid", "kepler"):
        for shape in ((37, 64), (2, 3)):
            m1 = diskmod.DiskMap(table(shape), r_min=3.0, r_max=17.0, rotation=rotation, omega_p=0.03125, exposure=MAP_EXPOSURE)
            m2 = diskmod.DiskMap(table(shape), r_min=6.0, r_max=34.0, rotation=rotation, omega_p=0.015625, exposure=MAP_EXPOSURE)
            for grid in LC_GRIDS[:3]:
                l1 = ltrace.diskmap_lightcurve(hits, n_hits, *one, m1.to_lt(), m1.texels, *grid)
                l2 = ltrace.diskmap_lightcurve(twice, n_hits, *two, m2.to_lt(), m2.texels, 2 * grid[0], 2 * grid[1], grid[2])
                rel = float(np.max(np.abs(l2 - l1) / l1))
                bound = map_lc_bound(M, a, m1, grid_times(grid), r_in)
                print(f"M = 1 against M = 2, {rotation} {shape} t = {grid[0]:g} ...: largest relative difference {rel:.2e} (bound {bound:.2e})")
                assert np.all(l1 > 0)
                if rotation == "rigid":
                    assert l2.tobytes() == l1.tobytes()
                else:
                    assert rel <= 2 * bound                            # two computed curves, each within the bound of the exact one
            if rotation == "rigid":
                f1 = ltrace.shade_diskmap(hits, n_hits, *one, m1.to_lt(), m1.texels, 333.25, want=("rgb",))["rgb"]
                f2 = ltrace.shade_diskmap(twice, n_hits, *two, m2.to_lt(), m2.texels, 666.5, want=("rgb",))["rgb"]
                assert ((f1 > 0) & (f1 < 1)).sum() > 0.2 * f1.size and float(np.max(ulps(f2, f1))) <= 2


# ---- 3. a dark map is the hot spot with no light ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "strip", "one"))
def test_a_dark_map_is_a_dark_spot(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    dark = ltrace.default_hotspot(exposure=0.0, with_disk=1)
    lit = 0
    for v in VARIANTS[:4]:
        dmap = make_map(c, v)
        dmap.with_disk, dmap.texels = True, np.zeros_like(dmap.texels)
        base, nh = base_of(c, v), n_hits if v.counts else None
        got = ltrace.shade_diskmap(hits, nh, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base, channels=v.channels)
        want = ltrace.shade_hotspot(hits, nh, met, dk, dark, v.t_obs, base=base, channels=v.channels)
        assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["rgba"], want["rgba"])
        lit += int((want["rgb"] > (0 if base is None else base)).sum())
    assert lit > 0
    # the aa forms at S = 2, on the case's records read as fine records where the shape allows, else on repeated ones
    S = 2
    fh, fn = (hits, n_hits) if c.R % S == 0 and c.W % S == 0 else (replicate(hits, S), replicate(n_hits, S))
    dmap = make_map(c, VARIANTS[0])
    dmap.texels = np.zeros_like(dmap.texels)
    fb = np.random.default_rng(5).uniform(0.0, 0.5, fh.shape[:2] + (3,)).astype(np.float32)
    got = ltrace.shade_diskmap_aa(fh, fn, S, met, dk, dmap.to_lt(), dmap.texels, 333.25, base=fb)
    want = ltrace.shade_hotspot_aa(fh, fn, S, met, dk, dark, 333.25, base=fb)
    assert np.array_equal(got["rgb"], want["rgb"]) and np.array_equal(got["rgba"], want["rgba"])


# ---- 4. supersampled frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R,W,m", [(2, 37, 51, 3), (3, 19, 29, 8), (4, 13, 21, 5)])
def test_aa_is_the_resolve_of_the_fine_frame(S, R, W, m):
    """R W is no multiple of 256 / S^2 (64, 28, 16), so the last workgroup is partial and slots straddle output rows."""
    assert (R * W) % (256 // (S * S)) != 0
    M, a, r_out = 1.0, 0.9, 20.0
    hits, n_hits = synth(R * S, W * S, m, 80 + S, float(diskmod.isco(M, a)), r_out)
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), ltrace.default_disk(r_out=r_out, exposure=DISK_EXPOSURE)
    rng = np.random.default_rng(S)
    differs = 0
    for v in VARIANTS[:4]:
        dmap = make_map(CASES["big"], v)
        base = rng.uniform(0.0, 0.5, (R * S, W * S) + ((3,) if v.channels == 3 else ())).astype(np.float32) if v.base else None
        nh = n_hits if v.counts else None
        fine = ltrace.shade_diskmap(hits, nh, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base, channels=v.channels)
        got = ltrace.shade_diskmap_aa(hits, nh, S, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base, channels=v.channels)
        want = aa.resolve(fine["rgb"], S)
        assert got["rgb"].shape == want.shape == ((R, W, 3) if v.channels == 3 else (R, W)) and got["rgb"].dtype == np.float32
        assert np.array_equal(got["rgb"], want)
        check_rgba(got["rgba"], want)
        differs += int(not np.array_equal(want, fine["rgb"][::S, ::S]))
        # device pointers give the host form's bytes
        import hipmini
        d_hits, d_n, d_tex = upload(hits), upload(n_hits), upload(dmap.texels)
        d_base = upload(base) if base is not None else None
        d_rgb, d_rgba = hipmini.DeviceArray(want.shape, np.float32), hipmini.DeviceArray((R, W, 4), np.uint8)
        ltrace.shade_diskmap_aa_dev(d_hits.ptr, d_n.ptr if v.counts else 0, R, W, S, m, met, dk, dmap.to_lt(), d_tex.ptr, v.t_obs,
                                    d_base=d_base.ptr if d_base else 0, channels=v.channels, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
        assert d_rgb.get().tobytes() == got["rgb"].tobytes() and d_rgba.get().tobytes() == got["rgba"].tobytes()
    assert differs == 4                                                   # a mean, not a pick


@pytest.mark.parametrize("name", ("strip", "one"))
def test_aa_of_one_sample_and_of_repeated_records(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    for v in VARIANTS[:4]:
        dmap, base, nh = make_map(c, v), base_of(c, v), n_hits if v.counts else None
        one = ltrace.shade_diskmap(hits, nh, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base, channels=v.channels)
        s1 = ltrace.shade_diskmap_aa(hits, nh, 1, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base, channels=v.channels)
        assert s1["rgb"].tobytes() == one["rgb"].tobytes() and s1["rgba"].tobytes() == one["rgba"].tobytes()
        for S in (2, 3, 8):
            # every sub-sample is the same float32 x; k x is exact in float64 for k <= 64, so the mean is x
            rep = ltrace.shade_diskmap_aa(replicate(hits, S), None if nh is None else replicate(nh, S), S, met, dk, dmap.to_lt(),
                                          dmap.texels, v.t_obs, base=None if base is None else replicate(base, S), channels=v.channels)
            assert rep["rgb"].tobytes() == one["rgb"].tobytes() and rep["rgba"].tobytes() == one["rgba"].tobytes()


@pytest.mark.parametrize("name", ("big", "one"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c, hits, n_hits, ref, met, dk = setup(name)
    d_hits, d_n = upload(hits), upload(n_hits)
    for v in VARIANTS[:4]:
        dmap, base = make_map(c, v), base_of(c, v)
        d_tex = upload(dmap.texels)
        grid = LC_GRIDS[0]
        lc = ltrace.diskmap_lightcurve(hits, n_hits if v.counts else None, met, dk, dmap.to_lt(), dmap.texels, *grid)
        d_out = hipmini.DeviceArray((grid[2], 3), np.float64)
        ltrace.diskmap_lightcurve_dev(d_hits.ptr, d_n.ptr if v.counts else 0, c.R, c.W, c.m, met, dk, dmap.to_lt(), d_tex.ptr, *grid, d_out.ptr)
        assert d_out.get().tobytes() == lc.tobytes()      # (the blocking copy orders behind the default stream's kernels)
        host = ltrace.shade_diskmap(hits, n_hits if v.counts else None, met, dk, dmap.to_lt(), dmap.texels, v.t_obs, base=base,
                                    channels=v.channels)
        d_base = upload(base) if base is not None else None
        d_rgb, d_rgba = hipmini.DeviceArray(host["rgb"].shape, np.float32), hipmini.DeviceArray((c.R, c.W, 4), np.uint8)
        ltrace.shade_diskmap_dev(d_hits.ptr, d_n.ptr if v.counts else 0, c.R, c.W, c.m, met, dk, dmap.to_lt(), d_tex.ptr, v.t_obs,
                                 d_base=d_base.ptr if d_base else 0, channels=v.channels, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
        assert d_rgb.get().tobytes() == host["rgb"].tobytes() and d_rgba.get().tobytes() == host["rgba"].tobytes()


# ---- 5., 6. one real trace -----------------------------------------------------------------------------------------------------
SEQ = dict(M=1.0, a=0.9, r_obs=50.0, theta_obs=np.radians(80.0), fov=(2 * np.arctan(np.tan(np.radians(20.0)) * 96 / 80), np.radians(40.0)),
           shape=(80, 96), r_out=20.0, max_images=3)


def traced():
    """The 96 x 80 frame: a = 0.9, theta_obs = 80 deg, r_obs = 50, three images, RK4 float32 -- traced once."""
    if not _TRACE:
        cam = ltrace.Camera(SEQ["shape"][1], SEQ["shape"][0], SEQ["fov"][0], SEQ["fov"][1], 0.0, 0.0, SEQ["r_obs"], SEQ["theta_obs"])
        met = ltrace.Metric(ltrace.METRIC_KERR, 0, SEQ["M"], SEQ["a"])
        dk = ltrace.default_disk(r_out=SEQ["r_out"])
        opts = ltrace.default_opts(integrator="rk4", precision=32, schedule="direct", tb_symmetry=0)
        out = ltrace.trace_disk_hits(cam, met, opts, dk, max_images=SEQ["max_images"], want=("hits", "n_hits"))
        _TRACE.update(hits=np.array(out["hits"]), n_hits=np.array(out["n_hits"]), met=met, dk=dk)
    return _TRACE["hits"], _TRACE["n_hits"], _TRACE["met"], _TRACE["dk"]


def test_rigid_gaussian_table_is_the_hot_spot():
    hits, n_hits, met, dk = traced()
    M, a = SEQ["M"], SEQ["a"]
    r_s, phi0, sigma, exposure, t_obs = 9.0, 0.5, 1.5, 1.0, 333.25
    n_r, n_phi = 256, 1024
    stored = np.arange(hits.shape[2]) < np.minimum(n_hits, hits.shape[2])[..., None]
    assert stored.sum() > 1000
    r_lo, r_hi = float(hits[..., 0][stored].min()), float(hits[..., 0][stored].max())
    h_r = (r_hi - r_lo) / (n_r - 2)
    r_min, r_max = r_lo - h_r, r_hi + h_r                                 # the records' range and a texel on each side
    h_phi = 2 * np.pi / n_phi
    dmap = diskmod.DiskMap(diskmod.spots_map(n_r, n_phi, r_min, r_max, [(r_s, phi0, sigma)]), r_min=r_min, r_max=r_max, rotation="rigid",
                           omega_p=np.sqrt(M) / (r_s ** 1.5 + a * np.sqrt(M)), exposure=exposure, with_disk=False)
    spot = ltrace.default_hotspot(r_spot=r_s, phi0=phi0, sigma=sigma, exposure=exposure, with_disk=0)
    got = ltrace.shade_diskmap(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, t_obs, want=("rgb",))["rgb"]
    want = ltrace.shade_hotspot(hits, n_hits, met, dk, spot, t_obs, want=("rgb",))["rgb"]
    B = h_r ** 2 / (8 * sigma ** 2) + h_phi ** 2 * 1.74 * r_max * r_s / (8 * sigma ** 2) + 2.0 ** -24
    g4 = np.where(stored, hits[..., 2].astype(np.float64), 0.0) ** 4
    bound = exposure * g4.sum(axis=-1) * B                                # (rows, W): the same for the three channels
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    slack = 2 * np.spacing(np.maximum(np.abs(want), np.float32(1e-30))).astype(np.float64)
    lit = bound > 0
    worst = float(np.max(diff[lit] / (bound[lit][:, None] + slack[lit])))
    signal = float(np.max(want[lit].max(axis=-1) / bound[lit]))
    print(f"rigid Gaussian table {n_r} x {n_phi} against lt_shade_hotspot: B = {B:.2e}; largest difference {worst:.2f} of the pixel's bound; "
          f"the brightest spot pixel is {signal:.0f} times its bound")
    assert np.all(diff <= bound[..., None] + slack)
    assert signal >= 100                                                   # otherwise the comparison says nothing


def test_traced_frame_against_the_numpy_statement():
    hits, n_hits, met, dk = traced()
    M, a = SEQ["M"], SEQ["a"]
    r_in = float(diskmod.isco(M, a))
    dmap = diskmod.DiskMap(diskmod.spiral_map(64, 256, arms=2, pitch=0.35, contrast=0.8, r_min=r_in, r_max=SEQ["r_out"]), r_min=r_in,
                           r_max=SEQ["r_out"], rotation="kepler", exposure=0.5)
    tdisk = diskmod.ThinDisk(r_out=SEQ["r_out"])
    worst, inside = 0.0, 0
    for t_obs in (333.25, 1e5):
        got = ltrace.shade_diskmap(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, t_obs, want=("rgb",))["rgb"]
        want = diskmod.shade_diskmap(M, a, hits, n_hits, tdisk, dmap, t_obs)
        worst = max(worst, float(np.max(ulps(got, want))))
        inside += int(((want > 0) & (want < 1)).sum())
    print(f"traced 96 x 80 frame, Keplerian spiral: largest difference from disk.shade_diskmap {worst:.2f} ulp of float32; {inside} lit, unsaturated values")
    assert worst <= 2 and inside > 1000
    # the light curve against the longdouble reference on the same records, the bound with the records' own delays
    ref = MapReference(hits, n_hits)
    stored = np.arange(hits.shape[2]) < np.minimum(n_hits, hits.shape[2])[..., None]
    dts = hits[..., 3][stored]
    r_lo = float(hits[..., 0][stored].min())
    for grid in LC_GRIDS[:3]:
        times = grid_times(grid)
        lc = ltrace.diskmap_lightcurve(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, *grid)
        bound = map_lc_bound(M, a, dmap, times, min(r_in, r_lo), dt_range=(float(dts.min()), float(dts.max())))
        excess, rel = lc_excess(lc, ref.lightcurve(M, a, dmap, times), bound)
        print(f"traced frame, t = {grid[0]:g} ...: light curve against longdouble, largest relative difference {rel:.2e}, bound {bound:.2e}")
        assert excess <= 1


@pytest.mark.parametrize("S", [None, 2])
def test_render_sequence_returns_the_entry_points_outputs(S):
    import image_lens
    from metrics import Kerr
    M, a = SEQ["M"], SEQ["a"]
    r_in = float(diskmod.isco(M, a))
    dmap = diskmod.DiskMap(diskmod.spiral_map(32, 128, r_min=r_in, r_max=SEQ["r_out"]), r_min=r_in, r_max=SEQ["r_out"], exposure=0.5)
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    times = 100.0 + 25.0 * np.arange(3)
    out = image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk, None, times,
                                     shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], samples=S, diskmap=dmap)
    k = 1 if S is None else S
    assert out["hits"].shape == (SEQ["shape"][0] * k, SEQ["shape"][1] * k, SEQ["max_images"], 4)
    assert out["frames"].shape == (3,) + SEQ["shape"] + (3,) and out["rgba"].shape == (3,) + SEQ["shape"] + (4,)
    assert out.get("samples") == S
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
    for i, t in enumerate(times):
        if S is None:
            f = ltrace.shade_diskmap(out["hits"], out["n_hits"], met, dk, dmap.to_lt(), dmap.texels, float(t))
        else:
            f = ltrace.shade_diskmap_aa(out["hits"], out["n_hits"], S, met, dk, dmap.to_lt(), dmap.texels, float(t))
        assert np.array_equal(out["frames"][i], f["rgb"]) and np.array_equal(out["rgba"][i], f["rgba"])
    lc = ltrace.diskmap_lightcurve(out["hits"], out["n_hits"], met, dk, dmap.to_lt(), dmap.texels, 100.0, 25.0, 3)
    assert np.array_equal(out["lightcurve"], lc / np.array([k * k, k ** 3, k ** 3], dtype=np.float64))
    assert np.all(out["lightcurve"][:, 0] > 0) and len({out["frames"][i].tobytes() for i in range(3)}) == 3     # the picture moves


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, ref, met, dk = setup("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    good = make_map(c, VARIANTS[0])
    S = 1

    def call(form="frame", hits_=hits, met_=met, disk_=dk, lt=None, tex=good.texels, R=c.R, W=c.W, m=c.m, S_=S, channels=3, t_obs=333.25,
             t_start=0.0, dt=1.0, n_times=2):
        """-> (code, message); the outputs of a refused call are untouched."""
        lt = lt or good.to_lt()
        rgb, rgba, out = np.full((c.R, c.W, 3), -7.0, np.float32), np.full((c.R, c.W, 4), 77, np.uint8), np.full((4, 3), -7.0)
        head = (ptr(hits_), ptr(n_hits), R, W)
        mid = (m, C.byref(met_) if met_ is not None else None, C.byref(disk_) if disk_ is not None else None,
               C.byref(lt) if lt != "null" else None, ptr(tex))
        if form == "frame":
            rc = lib.lt_shade_diskmap(*head, *mid, t_obs, None, channels, ptr(rgb), ptr(rgba))
        elif form == "aa":
            rc = lib.lt_shade_diskmap_aa(*head, S_, *mid, t_obs, None, channels, ptr(rgb), ptr(rgba))
        else:
            rc = lib.lt_diskmap_lightcurve(*head, *mid, t_start, dt, n_times, ptr(out))
        if rc != ltrace.OK:
            assert np.all(rgb == -7.0) and np.all(rgba == 77) and np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    for form in ("frame", "aa", "curve"):
        assert call(form)[0] == ltrace.OK
    bad = lambda **kw: good.__class__(good.texels, **{**dict(r_min=good.r_min, r_max=good.r_max, rotation=good.rotation, omega_p=good.omega_p,
                                                             exposure=good.exposure), **kw}).to_lt()
    nan, inf = float("nan"), float("inf")
    rot7 = good.to_lt()
    rot7.rotation = 7
    rigid_nan = bad(rotation="rigid", omega_p=nan)
    sizes = good.to_lt()
    sizes.n_r, sizes.n_phi = 1 << 14, 1 << 13                             # 2^27 texels: refused before the table is read
    zero = good.to_lt()
    zero.n_phi = 0
    # (keywords, code, a word of the message), in the header's order; every later fault is also present in `worse`
    steps = [(dict(hits_=None), ltrace.ERR_INVALID_ARG, "null"), (dict(met_=None), ltrace.ERR_INVALID_ARG, "null"),
             (dict(disk_=None), ltrace.ERR_INVALID_ARG, "null"), (dict(lt="null"), ltrace.ERR_INVALID_ARG, "null"),
             (dict(tex=None), ltrace.ERR_INVALID_ARG, "null"),
             (dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"),
             (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), ltrace.ERR_INVALID_ARG, "bad metric"),
             (dict(R=0), ltrace.ERR_INVALID_ARG, "empty frame"), (dict(W=-3), ltrace.ERR_INVALID_ARG, "empty frame"),
             (dict(m=0), ltrace.ERR_INVALID_ARG, "max_images"), (dict(m=9), ltrace.ERR_INVALID_ARG, "max_images"),
             (dict(lt=bad(r_min=0.0)), ltrace.ERR_INVALID_ARG, "r_min"), (dict(lt=bad(r_max=good.r_min)), ltrace.ERR_INVALID_ARG, "r_min"),
             (dict(lt=bad(r_max=inf)), ltrace.ERR_INVALID_ARG, "r_min"), (dict(lt=bad(r_min=nan)), ltrace.ERR_INVALID_ARG, "r_min"),
             (dict(lt=rigid_nan), ltrace.ERR_INVALID_ARG, "omega_p"),
             (dict(lt=bad(exposure=-1.0)), ltrace.ERR_INVALID_ARG, "map exposure"), (dict(lt=bad(exposure=inf)), ltrace.ERR_INVALID_ARG, "map exposure"),
             (dict(lt=zero), ltrace.ERR_INVALID_ARG, "texels"), (dict(lt=sizes), ltrace.ERR_INVALID_ARG, "texels"),
             (dict(lt=rot7), ltrace.ERR_INVALID_ARG, "rotation"),
             (dict(disk_=ltrace.default_disk(q=nan)), ltrace.ERR_INVALID_ARG, "disk q"),
             (dict(disk_=ltrace.default_disk(exposure=-1.0)), ltrace.ERR_INVALID_ARG, "disk q")]
    last = dict(frame=[(dict(channels=2), "channels"), (dict(t_obs=nan), "t_obs"), (dict(t_obs=inf), "t_obs")],
                curve=[(dict(n_times=-1), "n_times"), (dict(n_times=65536), "n_times"), (dict(t_start=nan), "t_start"), (dict(dt=inf), "t_start")])
    last["aa"] = last["frame"]
    for form in ("frame", "aa", "curve"):
        seq = steps + [(kw, ltrace.ERR_INVALID_ARG, word) for kw, word in last[form]]
        for i, (kw, code, word) in enumerate(seq):
            rc, msg = call(form, **kw)
            assert rc == code and word in msg, (form, kw, rc, msg)
            # with a later fault present as well, the earlier one still decides
            for kw2, _, word2 in seq[i + 1:]:
                if set(kw) & set(kw2) or word2 == word:
                    continue
                rc, msg = call(form, **kw, **kw2)
                assert rc == code and word in msg, (form, kw, kw2, rc, msg)
    # Keplerian rotation ignores omega_p
    assert call(lt=bad(rotation="kepler", omega_p=nan))[0] == ltrace.OK
    # the aa forms look at samples right after the device, before everything else
    for S_ in (0, -1, 9):
        rc, msg = call("aa", S_=S_, met_=schw, hits_=None)
        assert rc == ltrace.ERR_INVALID_ARG and "samples" in msg
    # no times: nothing to do, nothing written; a null out with times is refused last
    assert call("curve", n_times=0)[0] == ltrace.OK
    d_hits, d_tex = upload(hits), upload(good.texels)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.diskmap_lightcurve_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, good.to_lt(), d_tex.ptr, 0.0, 1.0, 2, 0)
    assert ei.value.code == ltrace.ERR_INVALID_ARG and "null out" in str(ei.value)
