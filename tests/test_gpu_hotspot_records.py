"""GPU tests of the hot spot's kernels (k_shade_hotspot, k_lightcurve_partial, k_lightcurve_final; lt_shade_hotspot,
lt_shade_hotspot_dev, lt_hotspot_lightcurve, lt_hotspot_lightcurve_dev) on synthetic hit records.

The kernels are functions of the caller's records, so the records come from tests/test_hotspot_records_host.py's
generator at the smallest sizes that reach each edge, and the expected values from its longdouble reference:
    257 x 331 (85 067 pixels, max_images 8): more than the light curve's 65 536-pixel pass and no multiple of 256 -- blocks
        0 ... 75 take a second pass, block 76 a partial one, the rest one; W odd and != R, so p mod W and p div W differ;
    1 x 1; 3 x 70 (less than one block); 256 x 256 (exactly one pass); 260 x 300 with max_images 1.
n_hits runs to 12, above every max_images, as the timed trace's counts do.

Bounds (derived in the host file's header; none comes from the kernels): frames 2 ulp of float32 against the reference,
1 ulp between frames one orbital period apart; light curve lc_bound(); sum of a frame against the light curve 2^-23.

MEASURED on the MI355X (build 7351b710453e; profiles/hotspot_records_7351b710453e.json):
    frames against the reference: at most 1.00 ulp of float32 (big, single), 0.00 ulp (one, strip, pass); bound 2;
    light curve against the reference, largest relative difference of the three columns / bound, at t = 5 ..., 1e5 ..., -3e4 ...:
        big-main    2.7e-16 / 2.0e-12,  6.2e-14 / 2.6e-10,  3.1e-14 / 7.8e-11;
        big-narrow  7.1e-15 / 4.0e-11,  1.8e-12 / 9.9e-9,   1.1e-12 / 3.0e-9;
        one-wide    8.4e-15 / 1.2e-12,  2.8e-12 / 5.7e-11,  1.0e-12 / 1.8e-11;
        strip       9.3e-16 / 1.2e-12,  3.7e-13 / 4.2e-11,  5.5e-14 / 1.4e-11;
        pass-isco   1.8e-15 / 2.0e-12,  7.7e-14 / 2.6e-10,  1.7e-14 / 8.0e-11;
        single-isco 2.3e-15 / 3.7e-12,  2.6e-13 / 7.0e-10,  9.1e-14 / 2.1e-10;
    sum of a frame against the light curve: 4.7e-10 (big), 5.6e-8 (one: a single term, bound 2^-24), 2.1e-8 (strip), 1.7e-9
        (pass), 1.3e-9 (single); bound 2^-23 = 1.19e-7; brightest pixel 0.30;
    frames 1 and 3 periods apart: no bit differs (bound 1 ulp); M = 1 against M = 2: no bit differs, frames and flux.
"""
import ctypes as C
import os

import numpy as np
import pytest

import ltrace
from test_hotspot_records_host import LD, TWO_PI_LD, Reference, lc_bound, lc_excess, omega_ref, synth, ulps

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_HOTSPOT_RECORDS_MEASURE")   # a path: the figures the tests print are also written there as JSON
T_OBS = (0.0, 333.25, 1e5, -3e4)
# Light-curve grids (t_start, dt, n): every t_start + i dt is exact in float64, so the kernel's t_start + dt i is the
# reference's time whether or not the compiler fuses it.  16 times on the two large frames, 64 elsewhere.
GRIDS_16 = ((5.0, 7.5, 6), (1e5, 11.0, 5), (-3e4, 13.0, 5))
GRIDS_64 = ((5.0, 7.5, 40), (1e5, 11.0, 12), (-3e4, 13.0, 12))


def spot_of(M, a, k):
    """Spots as (r_spot, phi0, sigma, exposure, with_disk): the existing test's; one at 1.2 ISCO; narrow without the disk;
    wide."""
    isco = ltrace.kerr_isco(M, a)
    return {"main": (9.0, 0.5, 1.5, 2.0, 1), "isco": (1.2 * isco, 0.3, 1.5, 2.0, 1), "narrow": (1.2 * isco, 2.5, 0.3, 1.5, 0),
            "wide": (1.2 * isco, 1.0, 4.0, 1.0, 1), "wide-dark": (1.2 * isco, 4.0, 4.0, 0.6, 0)}[k]


# name: (R, W, max_images, M, a, r_out, seed, spots, light-curve grids)
CASES = {"big": (257, 331, 8, 1.0, 0.9, 20.0, 31, ("main", "narrow"), GRIDS_16),
         "one": (1, 1, 2, 1.0, 0.9, 20.0, 32, ("wide",), GRIDS_64),     # (a seed whose pixel holds more hits than slots)
         "strip": (3, 70, 5, 1.0, 0.0, 20.0, 34, ("wide-dark",), GRIDS_64),
         "pass": (256, 256, 2, 1.0, -0.7, 20.0, 35, ("isco",), GRIDS_64),
         "single": (260, 300, 1, 2.0, 1.2, 40.0, 36, ("isco",), GRIDS_16)}
CASE_SPOTS = [(c, s) for c, v in CASES.items() for s in v[7]]
CASE_SPOT_IDS = [f"{c}-{s}" for c, s in CASE_SPOTS]
DISK_EXPOSURE = 0.25   # keeps most lit pixels of a frame with the disk below 1, where a wrong value shows

_CASE, _RECORD = {}, {}


class Case:
    def __init__(self, name):
        self.name = name
        self.R, self.W, self.m, self.M, self.a, self.r_out, seed, self.spots, self.grids = CASES[name]
        self.r_in = ltrace.kerr_isco(self.M, self.a)
        self.hits, self.n_hits = synth(self.R, self.W, self.m, seed, self.r_in, self.r_out)
        self.ref = Reference(self.hits, self.n_hits)
        self.met = ltrace.Metric(ltrace.METRIC_KERR, 0, self.M, self.a)
        self.disk = ltrace.default_disk(r_out=self.r_out, exposure=DISK_EXPOSURE)   # r_in 0: the ISCO, resolved by the library
        self.base = {1: np.random.default_rng(seed).uniform(0.0, 0.5, (self.R, self.W)).astype(np.float32),
                     3: np.random.default_rng(seed + 1).uniform(0.0, 0.5, (self.R, self.W, 3)).astype(np.float32)}

    def frame_ref(self, spot, t_obs, base=None, channels=3):
        return self.ref.frame(self.M, self.a, spot, t_obs, self.r_in, 3.0, DISK_EXPOSURE, base=base, channels=channels).astype(np.float32)

    def shade(self, spot, t_obs, n_hits="own", hits=None, **kw):
        return ltrace.shade_hotspot(self.hits if hits is None else hits, self.n_hits if isinstance(n_hits, str) else n_hits, self.met,
                                    self.disk, lt_spot(spot), t_obs, **kw)

    def curve(self, spot, grid, n_hits="own", hits=None):
        return ltrace.hotspot_lightcurve(self.hits if hits is None else hits, self.n_hits if isinstance(n_hits, str) else n_hits, self.met,
                                         self.disk, lt_spot(spot), *grid)


def case(name):
    """The records, reference and base images of one case, built once and left unchanged."""
    if name not in _CASE:
        _CASE[name] = Case(name)
    return _CASE[name]


def lt_spot(spot):
    return ltrace.default_hotspot(r_spot=float(spot[0]), phi0=float(spot[1]), sigma=float(spot[2]), exposure=float(spot[3]),
                                  with_disk=int(spot[4]))


def record(key, value):
    _RECORD[key] = max(_RECORD.get(key, 0.0), float(value))
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1)


def upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(a.ctypes.data), a.nbytes, 1), "hipMemcpy H2D")
    return d


def check_rgba(rgba, ref32):
    """The existing test's rule: RGBA8 = floor(255 rgb), equal except where the float value lies within 2 ulp of a rounding
    boundary; alpha 255."""
    c3 = ref32 if ref32.ndim == 3 else np.repeat(ref32[..., None], 3, axis=-1)
    want = (c3 * np.float32(255.0)).astype(np.uint8)
    x = c3.astype(np.float64) * 255.0
    near = np.abs(x - np.rint(x)) <= 2 * 255.0 * np.spacing(c3).astype(np.float64) + 1e-12
    assert np.all((rgba[..., :3] == want) | near) and np.all(rgba[..., 3] == 255)


# ---- 1. frames against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sk", CASE_SPOTS, ids=CASE_SPOT_IDS)
def test_frames_against_the_reference(name, sk):
    c = case(name)
    spot = spot_of(c.M, c.a, sk)
    worst, inside = 0.0, 0
    for t_obs in T_OBS:
        for channels in (1, 3):
            for base in (None, c.base[channels]):
                got = c.shade(spot, t_obs, base=base, channels=channels)
                ref = c.frame_ref(spot, t_obs, base=base, channels=channels)
                assert got["rgb"].shape == ref.shape and got["rgb"].dtype == np.float32
                worst = max(worst, float(np.max(ulps(got["rgb"], ref))))
                check_rgba(got["rgba"], ref)
                inside += int(((ref > (0 if base is None else base)) & (ref < 1)).sum())
    print(f"{name}-{sk}: frames against longdouble, largest difference {worst:.2f} ulp of float32; {inside} lit, unsaturated values")
    record(f"frame_ulp/{name}-{sk}", worst)
    assert worst <= 2
    assert inside >= (1 if c.R * c.W == 1 else 0.1 * 16 * c.R * c.W)


@pytest.mark.parametrize("name", ("big", "strip"))
def test_gray_base_single_outputs(name):
    """A gray base with only the RGBA8 frame, and with only the float frame: each is the pair's."""
    c = case(name)
    spot = spot_of(c.M, c.a, c.spots[0])
    both = c.shade(spot, 333.25, base=c.base[1])
    assert both["rgb"].shape == (c.R, c.W) and both["rgba"].shape == (c.R, c.W, 4)
    rgba = c.shade(spot, 333.25, base=c.base[1], want=("rgba",))
    rgb = c.shade(spot, 333.25, base=c.base[1], want=("rgb",))
    assert set(rgba) == {"rgba"} and set(rgb) == {"rgb"}
    assert rgba["rgba"].tobytes() == both["rgba"].tobytes() and rgb["rgb"].tobytes() == both["rgb"].tobytes()


# ---- 2. the light curve against the reference -----------------------------------------------------------------------------
@pytest.mark.parametrize("name,sk", CASE_SPOTS, ids=CASE_SPOT_IDS)
def test_lightcurve_against_the_reference(name, sk):
    c = case(name)
    spot = spot_of(c.M, c.a, sk)
    for grid in c.grids:
        times = grid[0] + grid[1] * np.arange(grid[2])
        lc = c.curve(spot, grid)
        assert lc.shape == (grid[2], 3)
        ref = c.ref.lightcurve(c.M, c.a, spot, times)
        bound = lc_bound(c.M, c.a, spot, times, c.r_out)
        excess, rel = lc_excess(lc, ref, bound)
        print(f"{name}-{sk} t = {grid[0]:g} ...: light curve against longdouble, largest relative difference {rel:.2e}, bound {bound:.2e}")
        record(f"lc_rel/{name}-{sk}/t{grid[0]:g}", rel)
        record(f"lc_bound/{name}-{sk}/t{grid[0]:g}", bound)
        assert np.all(ref[:, 0] > 0)
        assert excess <= 1


# ---- 3. reproducible bits, device pointers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "one", "single"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c = case(name)
    spot = spot_of(c.M, c.a, c.spots[0])
    d_hits, d_n = upload(c.hits), upload(c.n_hits)
    grid = c.grids[0]
    lc = c.curve(spot, grid)
    assert c.curve(spot, grid).tobytes() == lc.tobytes()
    for dn in (d_n.ptr, 0):
        d_out = hipmini.DeviceArray((grid[2], 3), np.float64)
        ltrace.hotspot_lightcurve_dev(d_hits.ptr, dn, c.R, c.W, c.m, c.met, c.disk, lt_spot(spot), *grid, d_out.ptr)
        assert d_out.get().tobytes() == lc.tobytes()      # (the blocking copy orders behind the default stream's kernels)
    for channels in (1, 3):
        for base in (None, c.base[channels]):
            host = c.shade(spot, 333.25, base=base, channels=channels)
            assert c.shade(spot, 333.25, base=base, channels=channels)["rgb"].tobytes() == host["rgb"].tobytes()
            d_base = upload(base) if base is not None else None
            for dn in (d_n.ptr, 0):
                d_rgb, d_rgba = hipmini.DeviceArray(host["rgb"].shape, np.float32), hipmini.DeviceArray((c.R, c.W, 4), np.uint8)
                ltrace.shade_hotspot_dev(d_hits.ptr, dn, c.R, c.W, c.m, c.met, c.disk, lt_spot(spot), 333.25,
                                         d_base=d_base.ptr if d_base else 0, channels=channels, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
                assert d_rgb.get().tobytes() == host["rgb"].tobytes() and d_rgba.get().tobytes() == host["rgba"].tobytes()
    # either output alone
    d_rgb = hipmini.DeviceArray((c.R, c.W, 3), np.float32)
    ltrace.shade_hotspot_dev(d_hits.ptr, d_n.ptr, c.R, c.W, c.m, c.met, c.disk, lt_spot(spot), 333.25, d_rgb=d_rgb.ptr)
    assert d_rgb.get().tobytes() == c.shade(spot, 333.25, channels=3)["rgb"].tobytes()


# ---- 4. what n_hits means -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_n_hits_semantics(name):
    c = case(name)
    spot = spot_of(c.M, c.a, c.spots[0])
    grid = c.grids[1][:2] + (4,)
    assert (c.n_hits > c.m).any()
    frame, lc = c.shade(spot, 1e5, base=c.base[3]), c.curve(spot, grid)
    # the NaN padding makes "leading non-NaN slots" and min(n_hits, max_images) the same slots, counts above max_images included
    for nh in (None, np.minimum(c.n_hits, c.m)):
        f2, l2 = c.shade(spot, 1e5, n_hits=nh, base=c.base[3]), c.curve(spot, grid, n_hits=nh)
        assert f2["rgb"].tobytes() == frame["rgb"].tobytes() and f2["rgba"].tobytes() == frame["rgba"].tobytes()
        assert l2.tobytes() == lc.tobytes()
    # with n_hits given, what lies in the slots behind it is never read: finite garbage changes nothing -- records that
    # sit on the spot at the light curve's first time, as bright as a record gets
    on_spot = float((LD(spot[1]) + omega_ref(c.M, c.a, spot[0]) * (LD(grid[0]) - 50)) % TWO_PI_LD)
    dirty = c.hits.copy()
    dirty[np.arange(c.m)[None, None, :] >= c.n_hits[..., None]] = np.array([spot[0], on_spot, 1.3, 50.0], dtype=np.float32)
    changed = not np.array_equal(np.isnan(dirty), np.isnan(c.hits))
    assert changed or c.R * c.W == 1
    f3, l3 = c.shade(spot, 1e5, hits=dirty, base=c.base[3]), c.curve(spot, grid, hits=dirty)
    assert f3["rgb"].tobytes() == frame["rgb"].tobytes() and l3.tobytes() == lc.tobytes()
    if changed:   # ... and without n_hits it is read
        assert c.curve(spot, grid, hits=dirty, n_hits=None).tobytes() != lc.tobytes()


# ---- 5. the two kernels agree with each other --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_frame_sums_to_the_lightcurve(name):
    """Without disk and base, one channel, unclamped (the reference's brightest pixel is below 1): a frame's pixels are
    the light curve's terms rounded to float32, so their sums agree to 2^-23 (non-negative terms, each within 2^-24)."""
    c = case(name)
    spot = (1.2 * c.r_in, 0.7, 1.5 * c.M, 0.05, 0)
    ix, iy = np.meshgrid(np.arange(c.W), np.arange(c.R))
    worst = 0.0
    for t_obs in (333.25, 1e5):
        brightest = float(c.ref.frame(c.M, c.a, spot, t_obs, c.r_in, channels=1).max())
        assert brightest < 1
        rgb = c.shade(spot, t_obs, channels=1, want=("rgb",))["rgb"].astype(LD)
        lc = c.curve(spot, (t_obs, 1.0, 1))[0].astype(LD)
        assert lc[0] > 0
        for col, wgt in enumerate((1, ix, iy)):
            s = (rgb * wgt).sum()
            assert abs(s - lc[col]) <= LD(2.0 ** -23) * lc[col]
            if lc[col] > 0:
                worst = max(worst, float(abs(s - lc[col]) / lc[col]))
        print(f"{name} t = {t_obs:g}: brightest pixel {brightest:.3f}; sum of the frame against the light curve, largest relative difference {worst:.2e}")
    record(f"frame_vs_lc/{name}", worst)


# ---- 6. the orbit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "pass", "single"))
def test_orbital_period(name):
    """Omega from the test's own formula: a frame one and three periods later is the same frame (1 ulp of float32), half
    a period later it is another one.  Pins the sign of a (pass: a = -0.7) and the powers of M (single: M = 2)."""
    c = case(name)
    spot = spot_of(c.M, c.a, c.spots[0])
    om = omega_ref(c.M, c.a, spot[0])
    t0 = 333.25
    f0 = c.shade(spot, t0, channels=3, want=("rgb",))["rgb"]
    worst = 0.0
    for k in (1, 3):
        fk = c.shade(spot, float(t0 + k * TWO_PI_LD / om), channels=3, want=("rgb",))["rgb"]
        worst = max(worst, float(np.max(ulps(fk, f0))))
    print(f"{name}: frames 1 and 3 periods apart, largest difference {worst:.2f} ulp of float32")
    record(f"period_ulp/{name}", worst)
    assert worst <= 1
    half = c.shade(spot, float(t0 + TWO_PI_LD / om / 2), channels=3, want=("rgb",))["rgb"]
    assert np.any(half != f0, axis=-1).sum() > 100


def test_scaling_with_mass():
    """Records and spot at M = 1, a = 0.6 against (r, dt, r_spot, sigma, t, a) all doubled at M = 2 with the disk's r_in
    doubled: the same picture and the same flux.  (Doubling is exact in float32, so the two inputs state one scene.)"""
    R, W, m, M, a, r_out = 260, 300, 2, 1.0, 0.6, 20.0
    r_in = ltrace.kerr_isco(M, a)
    hits, n_hits = synth(R, W, m, 41, r_in, r_out)
    twice = hits * np.array([2, 1, 1, 2], dtype=np.float32)
    spot = (1.2 * r_in, 0.4, 1.5, 2.0, 1)
    spot2 = (2 * spot[0], spot[1], 2 * spot[2], spot[3], spot[4])
    one = (ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), ltrace.default_disk(r_in=r_in, r_out=r_out, exposure=DISK_EXPOSURE))
    two = (ltrace.Metric(ltrace.METRIC_KERR, 0, 2 * M, 2 * a), ltrace.default_disk(r_in=2 * r_in, r_out=2 * r_out, exposure=DISK_EXPOSURE))
    worst = 0.0
    for t_obs in (333.25, -3e4):
        f1 = ltrace.shade_hotspot(hits, n_hits, *one, lt_spot(spot), t_obs, want=("rgb",))["rgb"]
        f2 = ltrace.shade_hotspot(twice, n_hits, *two, lt_spot(spot2), 2 * t_obs, want=("rgb",))["rgb"]
        assert ((f1 > 0) & (f1 < 1)).sum() > 0.2 * f1.size
        worst = max(worst, float(np.max(ulps(f2, f1))))
    print(f"M = 1 against M = 2: frames, largest difference {worst:.2f} ulp of float32")
    record("scaling_ulp", worst)
    assert worst <= 2
    for grid in GRIDS_16:
        l1 = ltrace.hotspot_lightcurve(hits, n_hits, *one, lt_spot(spot), *grid)
        l2 = ltrace.hotspot_lightcurve(twice, n_hits, *two, lt_spot(spot2), 2 * grid[0], 2 * grid[1], grid[2])
        bound = lc_bound(M, a, spot, grid[0] + grid[1] * np.arange(grid[2]), r_out)
        rel = float(np.max(np.abs(l2[:, 0] - l1[:, 0]) / l1[:, 0]))
        print(f"M = 1 against M = 2, t = {grid[0]:g} ...: flux, largest relative difference {rel:.2e}, bound {bound:.2e}")
        record(f"scaling_flux_rel/t{grid[0]:g}", rel)
        assert np.all(l1[:, 0] > 0) and rel <= bound


# ---- 7. refusals and no-ops ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_library_working():
    c = case("strip")
    spot = spot_of(c.M, c.a, c.spots[0])
    s = lt_spot(spot)
    ref = c.frame_ref(spot, 333.25)

    def still_works():
        assert np.max(ulps(c.shade(spot, 333.25, want=("rgb",))["rgb"], ref)) <= 2

    def refused(fn):
        with pytest.raises(ltrace.LtraceError) as ei:
            fn()
        assert ei.value.code == ltrace.ERR_INVALID_ARG
        still_works()

    still_works()
    empty = ltrace.hotspot_lightcurve(c.hits, c.n_hits, c.met, c.disk, s, 5.0, 7.5, 0)
    assert empty.shape == (0, 3)
    still_works()
    refused(lambda: ltrace.hotspot_lightcurve(c.hits, c.n_hits, c.met, c.disk, s, 5.0, 7.5, 65536))
    refused(lambda: ltrace.shade_hotspot(c.hits, c.n_hits, c.met, c.disk, s, 0.0, channels=2))
    for bad in (np.nan, np.inf, -np.inf):
        refused(lambda: ltrace.shade_hotspot(c.hits, c.n_hits, c.met, c.disk, s, bad))
        refused(lambda: ltrace.hotspot_lightcurve(c.hits, c.n_hits, c.met, c.disk, s, bad, 1.0, 4))
        refused(lambda: ltrace.hotspot_lightcurve(c.hits, c.n_hits, c.met, c.disk, s, 0.0, bad, 4))
    nine = np.concatenate([c.hits, c.hits[:, :, :4]], axis=2)
    assert nine.shape == (c.R, c.W, 9, 4)
    refused(lambda: ltrace.shade_hotspot(nine, c.n_hits, c.met, c.disk, s, 0.0))
    refused(lambda: ltrace.hotspot_lightcurve(nine, c.n_hits, c.met, c.disk, s, 0.0, 1.0, 4))
