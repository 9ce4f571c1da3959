"""The disk movie (include/ltrace.h, "a disk movie"): an extended-precision reference of the rule, the CPU tests that hold
disk.shade_diskmovie / disk.diskmovie_lightcurve to it, the library's exports and bindings, the flare generator and the
refusals that need no GPU.  tests/test_gpu_diskmovie.py imports the cases, the reference and the bounds from here and
holds the kernels (lt_diskmovie.hpp) to them.

Records come from test_hotspot_records_host.synth through test_diskmap_host.records (the map's four cases).
MovieReference extends MapReference: it is written from the header's five steps in np.longdouble (64-bit mantissa here),
sums included, with the true 2 pi; it calls nothing of disk.py.

Bounds, derived and not measured:
    frames: as the map's -- float32 output of a value good to ~1e-12 relative: 1 ulp of float32 for the numpy statement,
        2 ulp for the kernel (two roundings plus contraction);
    light curve: every term is non-negative (texels in [0.5, 1.5], m a convex combination of them).  Two things are
        rounded in float64 before a table is read.
        (a) The phase Omega (t_em - T_q) of each frame of the pair.  t_em = t - dt, T_q = t0 + q dt_frame, their
        difference and the product are each rounded; |T_q| <= |t0| + n_frames dt_frame for a held movie and
        <= |t_em| + dt_frame for a loop, so the phase is off by at most 8 2^-53 Omega (|t_em| + |t0| + n_frames dt_frame),
        the map's factor 8 (which holds the wrap with the float64 2 pi) on a larger time.  It is amplified as the map's:
        a step du in u = psi n_phi / 2 pi moves a bilinear value by at most du (T_max - T_min), relative to at least T_min;
        the blend of two such values moves by no more.  This is map_lc_bound of the movie's tables plus the same
        expression for the time |t0| + n_frames dt_frame.
        (b) The blend weight f_t.  s = (t_em - t0) / dt_frame takes three roundings (t_em, the difference, the quotient):
        |ds| <= 4 2^-53 (|t_em| + |t0|) / dt_frame.  The rule is continuous in t_em across every floor and clamp (header),
        so a rounding of s that crosses one moves m by |ds| |m_q1 - m_q0| <= |ds| (T_max - T_min) all the same, relative
        to at least T_min:
            rel <= map_lc_bound + 8 2^-53 Omega (|t0| + n_frames dt_frame) (n_phi / 2 pi) (T_max - T_min) / T_min
                   + 4 2^-53 max(|t_em| + |t0|) / dt_frame (T_max - T_min) / T_min                        (movie_lc_bound)

MEASURED here, disk.py against the reference (the cases and variants below):
    frames: no float32 differs (0.00 ulp) on any of the four cases;
    light curve, |lc - ref| / |ref| over the three columns where it comes nearest to its bound: big 2.4e-16 (bound 1.7e-12,
        rigid loop, t = 600), mid 1.5e-14 (8.3e-11, Keplerian hold, t = 1e5), strip 1.5e-13 (2.9e-11, one rigid held frame,
        t = 1e5), one 6.2e-13 (1.8e-11, one rigid held frame, t = -3e4): never above 3.5 % of a bound.
"""
import ctypes
import re
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES, DISK_EXPOSURE, LC_GRIDS, MAP_EXPOSURE, MapReference, base_of, grid_times, map_lc_bound, records, table
from test_hotspot_records_host import DT_RANGE, isco_ref, lc_excess, synth, ulps

LD = np.longdouble
TWO_PI_LD = 2 * np.arccos(LD(-1))

# ---- cases: the map's records; movies, variants, times -------------------------------------------------------------------
TABLES = [(2, 3), (37, 64)]
T0, DT_FRAME = 64.0, 128.0          # dyadic: T_q = 64 + 128 q is exact, and so is T_q + dt for a float32 dt
# n_frames, table, rotation, boundary, with n_hits, with base, channels, with_disk, range inside the records' r range, times
Variant = namedtuple("Variant", "n_frames table rotation boundary counts base channels with_disk inside t_obs")
# emission times t_obs - dt, dt in [30, 400]: 80 -> all before frame 0;  600 -> [200, 570], inside five frames (64 ... 576),
# past the end of two (64, 192) and of one;  "epoch" -> the first stored slot exactly on frame 1's (or the only frame's)
# epoch;  2000 -> all beyond;  1e5 and -3e4 far outside.
VARIANTS = [Variant(5, 1, "kepler", "hold", True, True, 3, True, False, (600.0, "epoch", 1e5)),
            Variant(5, 1, "rigid", "loop", False, False, 1, False, False, (80.0, 600.0, -3e4)),
            Variant(2, 0, "kepler", "loop", True, False, 3, False, True, ("epoch", 2000.0, 1e5)),
            Variant(1, 1, "rigid", "hold", False, True, 1, True, True, (80.0, 600.0)),
            Variant(2, 1, "kepler", "hold", True, True, 1, False, False, (80.0, 2000.0, -3e4)),
            Variant(1, 0, "kepler", "loop", True, False, 3, True, False, (600.0, "epoch"))]
MOVIE_LC_GRIDS = LC_GRIDS + [(600.0, 9.0, 4), (80.0, 16.0, 3)]
BIG_LC_GRIDS = [(600.0, 9.0, 2), (1e5, 11.0, 2), (-3e4, 13.0, 1)]       # the large cases: five times per variant


def movie_table(n_frames, shape, seed=11):
    """Texels (n_frames, n_r, n_phi) uniform in [0.5, 1.5], float32: the map's table() per frame, each its own."""
    return np.stack([table(shape, seed=seed + 17 * k) for k in range(n_frames)])


def make_movie(c, v, exposure=MAP_EXPOSURE, t0=T0, dt_frame=DT_FRAME):
    """The disk.DiskMovie of variant v on case c's records; the annulus and the pattern speed are test_diskmap_host.make_map's."""
    r_in = float(diskmod.isco(c.M, c.a))
    lo, hi = (r_in + 2.0 * c.M, c.r_out - 5.0 * c.M) if v.inside else (0.5 * r_in, c.r_out + c.M)
    return diskmod.DiskMovie(movie_table(v.n_frames, TABLES[v.table]), t0=t0, dt_frame=dt_frame, boundary=v.boundary, r_min=lo, r_max=hi,
                             rotation=v.rotation, omega_p=0.03 / c.M, exposure=exposure, with_disk=v.with_disk)


def observer_time(t, ref, movie):
    """A variant's time: a number, or "epoch" -- the first stored slot's emission time exactly on an epoch (frame 1's, or
    the only frame's): T_q + dt is exact in float64 for the dyadic clock."""
    if t != "epoch":
        return float(t)
    T_q = movie.t0 + min(1, movie.n_frames - 1) * movie.dt_frame
    t_obs = float(T_q) + float(ref.dt[0])
    assert LD(t_obs) - ref.dt[0] == LD(T_q)
    return t_obs


# ---- the reference ------------------------------------------------------------------------------------------------------
class MovieReference(MapReference):
    """MapReference with a movie as the emitter: weight() is the header's steps 1 to 5 of "a disk movie" in longdouble;
    map_emission, frame and lightcurve are inherited and take a disk.DiskMovie where they took a disk.DiskMap."""

    def _bilinear(self, movie, k, psi):
        """The map's steps 3 to 5 on frame k (n_stored,) at psi, in longdouble."""
        T = movie.texels.astype(LD)
        _, n_r, n_phi = T.shape
        r_min, r_max = LD(movie.r_min), LD(movie.r_max)
        v = np.clip((self.r - r_min) / (r_max - r_min) * n_r - LD(0.5), LD(0), LD(n_r - 1))
        i0 = np.minimum(np.floor(v).astype(np.int64), n_r - 1)
        i1 = np.minimum(i0 + 1, n_r - 1)
        f_r = v - i0
        u = psi * (n_phi / TWO_PI_LD) - LD(0.5)
        fl = np.floor(u)
        k0 = np.mod(fl.astype(np.int64), n_phi)
        k1 = np.mod(k0 + 1, n_phi)
        f_p = u - fl
        return (1 - f_r) * ((1 - f_p) * T[k, i0, k0] + f_p * T[k, i0, k1]) + f_r * ((1 - f_p) * T[k, i1, k0] + f_p * T[k, i1, k1])

    def pair(self, movie, t_obs):
        """Steps 1 to 3: (t_em, q0, q1, f_t, k0, k1)."""
        n = movie.n_frames
        t_em = LD(t_obs) - self.dt
        s = (t_em - LD(movie.t0)) / LD(movie.dt_frame)
        if movie.boundary == "hold":
            q0 = np.clip(np.floor(s), LD(0), LD(n - 1))
            q1 = np.minimum(q0 + 1, LD(n - 1))
            f_t = np.clip(s - q0, LD(0), LD(1))
            k0, k1 = q0, q1
        else:
            q0 = np.floor(s)
            q1 = q0 + 1
            f_t = s - q0
            k0, k1 = (np.clip(q - n * np.floor(q / n), LD(0), LD(n - 1)) for q in (q0, q1))
        return t_em, q0, q1, f_t, k0.astype(np.int64), k1.astype(np.int64)

    def weight(self, M, a, movie, t_obs):
        """(n_stored,): the movie's blended value m of every stored slot at observer time t_obs (steps 1 to 5)."""
        t_em, q0, q1, f_t, k0, k1 = self.pair(movie, t_obs)
        if movie.rotation == "rigid":
            om = LD(movie.omega_p)
        else:
            om = np.sqrt(LD(M)) / (self.r * np.sqrt(self.r) + LD(a) * np.sqrt(LD(M)))

        def look(q, k):
            x = self.ph - om * (t_em - (LD(movie.t0) + q * LD(movie.dt_frame)))
            psi = x - TWO_PI_LD * np.floor(x / TWO_PI_LD)
            psi = np.where((psi >= TWO_PI_LD) | (psi < 0), LD(0), psi)
            return self._bilinear(movie, k, psi)

        m0, m1 = look(q0, k0), look(q1, k1)
        m = (1 - f_t) * m0 + f_t * m1
        if movie.boundary == "hold":
            m = np.where(q1 == q0, m0, m)
        inside = (self.r32.astype(np.float64) >= np.float64(movie.r_min)) & (self.r32.astype(np.float64) <= np.float64(movie.r_max))
        return np.where(inside, m, LD(0))


_MOVIE_REF = {}


def movie_records(name):
    """(hits, n_hits, MovieReference) of one of the map's cases, made once."""
    if name not in _MOVIE_REF:
        hits, n_hits, _ = records(name)
        _MOVIE_REF[name] = (hits, n_hits, MovieReference(hits, n_hits))
    return _MOVIE_REF[name]


def movie_lc_bound(M, a, movie, times, r_in, dt_range=DT_RANGE):
    """The light curve's relative bound (header) over `times`, dt anywhere in dt_range."""
    t = np.asarray(times, dtype=np.float64)
    T = movie.texels.astype(np.float64)
    tables = diskmod.DiskMap(T.reshape(-1, T.shape[2]), r_min=movie.r_min, r_max=movie.r_max, rotation=movie.rotation, omega_p=movie.omega_p)
    om = abs(movie.omega_p) if movie.rotation == "rigid" else float(np.sqrt(M) / (r_in ** 1.5 + a * np.sqrt(M)))
    slope = (T.max() - T.min()) / T.min()
    t_em = max(np.max(np.abs(t - dt_range[0])), np.max(np.abs(t - dt_range[1])))
    clock = abs(movie.t0) + movie.n_frames * movie.dt_frame
    return (map_lc_bound(M, a, tables, times, r_in, dt_range) + 8 * 2.0 ** -53 * om * clock * (T.shape[2] / (2 * np.pi)) * slope
            + 4 * 2.0 ** -53 * (t_em + abs(movie.t0)) / movie.dt_frame * slope)


# ---- CPU tests: the numpy statement against the reference -----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_numpy_frames_against_the_reference(name):
    c = CASES[name]
    hits, n_hits, ref = movie_records(name)
    r_in = float(isco_ref(c.M, c.a))
    dk = diskmod.ThinDisk(r_out=c.r_out, exposure=DISK_EXPOSURE)
    worst, inside, outside_slots, two, one = 0.0, 0, 0, 0, 0
    for v in VARIANTS:
        movie, base = make_movie(c, v), base_of(c, v)
        for t in v.t_obs[:1] if c.R * c.W > 1000 else v.t_obs:      # (the large cases: one time per variant)
            t_obs = observer_time(t, ref, movie)
            got = diskmod.shade_diskmovie(c.M, c.a, hits, n_hits if v.counts else None, dk, movie, t_obs, base=base, channels=v.channels)
            want = ref.frame(c.M, c.a, movie, t_obs, r_in, dk.q, dk.exposure, base=base, channels=v.channels)
            assert got.shape == want.shape and got.dtype == np.float32
            worst = max(worst, float(np.max(ulps(got, want))))
            if t == v.t_obs[0]:                                       # counted once per variant, as the map's test counts
                w32 = want.astype(np.float32)
                inside += int(((w32 > (0 if base is None else base)) & (w32 < 1)).sum())
            _, q0, q1, f_t, _, _ = ref.pair(movie, t_obs)
            two += int(((q1 != q0) & (f_t > 0) & (f_t < 1)).sum())
            one += int((q1 == q0).sum())
            if t == "epoch":
                assert f_t[0] == 0 and q0[0] == min(1, movie.n_frames - 1)
        if v.inside:
            outside_slots += int(((ref.r32 < movie.r_min) | (ref.r32 > movie.r_max)).sum())
    print(f"{name}: disk.shade_diskmovie against longdouble, largest difference {worst:.2f} ulp of float32; {inside} lit, unsaturated values; "
          f"{two} slots blend two frames, {one} hold one")
    assert worst <= 1
    if c.R * c.W > 1:
        assert inside >= 0.2 * c.R * c.W       # lit and not saturated: pixels that say something
        assert outside_slots > 0 and two > 0 and one > 0
    else:
        assert inside >= 1


@pytest.mark.parametrize("name", list(CASES))
def test_every_frame_says_something(name):
    """The condition the GPU test rests on, for the reference alone: per variant and time at least 0.2 R W lit, unsaturated
    values (1 for the one-pixel case) -- m is a convex combination of texels in [0.5, 1.5], as the map's at these exposures."""
    c = CASES[name]
    hits, n_hits, ref = movie_records(name)
    r_in = float(isco_ref(c.M, c.a))
    dk = diskmod.ThinDisk(r_out=c.r_out, exposure=DISK_EXPOSURE)
    for v in VARIANTS[:3]:
        movie, base = make_movie(c, v), base_of(c, v)
        t_obs = observer_time(v.t_obs[0], ref, movie)
        m = ref.weight(c.M, c.a, movie, t_obs)
        assert np.all((m == 0) | ((m >= 0.5) & (m <= 1.5)))
        w32 = ref.frame(c.M, c.a, movie, t_obs, r_in, dk.q, dk.exposure, base=base, channels=v.channels).astype(np.float32)
        inside = int(((w32 > (0 if base is None else base)) & (w32 < 1)).sum())
        assert inside >= (0.2 * c.R * c.W if c.R * c.W > 1 else 1)


@pytest.mark.parametrize("name", list(CASES))
def test_numpy_lightcurve_against_the_reference(name):
    c = CASES[name]
    hits, n_hits, ref = movie_records(name)
    r_in = float(diskmod.isco(c.M, c.a))
    big = c.R * c.W > 1000
    for v in VARIANTS[:2] if big else VARIANTS:
        movie = make_movie(c, v)
        for grid in BIG_LC_GRIDS if big else MOVIE_LC_GRIDS:
            times = grid_times(grid)
            lc = diskmod.diskmovie_lightcurve(c.M, c.a, hits, n_hits if v.counts else None, movie, times)
            want = ref.lightcurve(c.M, c.a, movie, times)
            bound = movie_lc_bound(c.M, c.a, movie, times, r_in)
            excess, rel = lc_excess(lc, want, bound)
            print(f"{name} {v.rotation} {v.boundary} {v.n_frames} x {TABLES[v.table]} t = {grid[0]:g} ...: disk.diskmovie_lightcurve against "
                  f"longdouble, largest relative difference {rel:.2e}, bound {bound:.2e}")
            assert np.all(want[:, 0] > 0)
            assert excess <= 1


def test_numpy_aa_is_the_resolve_of_the_fine_frame():
    import aa
    c, v = CASES["strip"], VARIANTS[0]
    movie, dk = make_movie(c, v), diskmod.ThinDisk(r_out=c.r_out, exposure=DISK_EXPOSURE)
    fh, fn = synth(c.R * 2, 20, c.m, 92, float(diskmod.isco(c.M, c.a)), c.r_out)
    fine = diskmod.shade_diskmovie(c.M, c.a, fh, fn, dk, movie, 600.0, channels=1)
    got = diskmod.shade_diskmovie_aa(c.M, c.a, fh, fn, dk, movie, 600.0, 2, channels=1)
    assert got.shape == (c.R, 10) and got.dtype == np.float32 and np.array_equal(got, aa.resolve(fine, 2))


# ---- CPU tests: properties of the rule ---------------------------------------------------------------------------------------
def test_one_held_frame_is_the_map():
    c, v = CASES["strip"], VARIANTS[3]
    hits, n_hits, _ = movie_records("strip")
    movie = make_movie(c, v, t0=0.0, dt_frame=3.7)
    for t in (333.25, 1e5, -3e4):
        assert np.array_equal(diskmod.movie_intensity(c.M, c.a, hits, movie, t), diskmod.map_intensity(c.M, c.a, hits, movie.frame(0), t),
                              equal_nan=True)


def test_the_rule_is_continuous_across_epochs_and_ends():
    """m just below and just above every epoch, and at both ends of a held movie, differs by the step times the slope."""
    c = CASES["strip"]
    for v in (VARIANTS[0], VARIANTS[1], VARIANTS[2]):
        movie = make_movie(c, v)
        r = np.full(7, 0.5 * (movie.r_min + movie.r_max))
        phi = np.linspace(0.1, 6.0, 7)
        om = 0.03
        for q in range(-1, movie.n_frames + 2):
            T = movie.t0 + q * movie.dt_frame
            eps = 1e-7
            lo, at, hi = (diskmod.sample_movie(movie, r, phi, om, T + d) for d in (-eps, 0.0, eps))
            step = eps * (1.0 / movie.dt_frame + om * 64 / (2 * np.pi)) * 1.0 * 4        # d(f_t) + d(psi) n_phi / 2 pi, times T_max - T_min
            assert np.max(np.abs(lo - at)) <= step and np.max(np.abs(hi - at)) <= step, (v, q)


def test_loop_and_hold():
    c = CASES["strip"]
    hits, n_hits, _ = movie_records("strip")
    loop = make_movie(c, VARIANTS[1]._replace(rotation="rigid"))
    loop.omega_p = 0.0
    period = loop.n_frames * loop.dt_frame
    a, b = (diskmod.movie_intensity(c.M, c.a, hits, loop, t) for t in (600.0, 600.0 + period))
    assert np.array_equal(a, b, equal_nan=True)
    assert not np.array_equal(a, diskmod.movie_intensity(c.M, c.a, hits, loop, 600.0 + loop.dt_frame), equal_nan=True)
    hold = make_movie(c, VARIANTS[0]._replace(rotation="rigid"))
    hold.omega_p = 0.0
    first = diskmod.DiskMovie(hold.texels[:1], t0=hold.t0, dt_frame=hold.dt_frame, r_min=hold.r_min, r_max=hold.r_max, rotation="rigid",
                              exposure=hold.exposure)
    last = diskmod.DiskMovie(hold.texels[-1:], t0=hold.t0, dt_frame=hold.dt_frame, r_min=hold.r_min, r_max=hold.r_max, rotation="rigid",
                             exposure=hold.exposure)
    assert np.array_equal(diskmod.movie_intensity(c.M, c.a, hits, hold, 80.0), diskmod.movie_intensity(c.M, c.a, hits, first, 80.0), equal_nan=True)
    assert np.array_equal(diskmod.movie_intensity(c.M, c.a, hits, hold, 2000.0), diskmod.movie_intensity(c.M, c.a, hits, last, 2000.0), equal_nan=True)


def test_flare_movie():
    """The flare's light peaks at t_peak and is the floor's light far from it; the clump rides on the rotation."""
    kw = dict(n_r=24, n_phi=96, r_min=4.0, r_max=16.0, r_s=9.0, phi_s=1.0, sigma=1.5, t_peak=200.0, t_width=30.0, dt_frame=10.0, t0=0.0,
              floor=0.1, amplitude=2.0, M=1.0, a=0.9)
    mv = diskmod.flare_movie(41, **kw)
    assert mv.texels.shape == (41, 24, 96) and mv.texels.dtype == np.float32 and mv.boundary == "hold" and mv.rotation == "kepler"
    assert (mv.t0, mv.dt_frame, mv.r_min, mv.r_max) == (0.0, 10.0, 4.0, 16.0)
    light = mv.texels.astype(np.float64).sum(axis=(1, 2))
    assert np.argmax(light) == 20 and light[0] == pytest.approx(0.1 * 24 * 96, rel=1e-6) and light[40] == pytest.approx(light[0], rel=1e-6)
    assert np.all(np.diff(light[:21]) >= 0) and np.all(np.diff(light[20:]) <= 0) and light[20] > 1.3 * light[0]
    # at t_peak the clump is round about (r_s, phi_s); a frame later the ring at r_s has carried it on by Omega dt_frame
    i = int((9.0 - 4.0) / 0.5)                                          # the row whose centre is 9.25
    k_peak = np.argmax(mv.texels[20, i])
    assert abs((k_peak + 0.5) * 2 * np.pi / 96 - 1.0) < 2 * np.pi / 96
    r_row = 4.0 + (i + 0.5) * 0.5
    want = 1.0 + float(diskmod.omega(1.0, 0.9, r_row)) * 50.0
    assert abs((np.argmax(mv.texels[25, i]) + 0.5) * 2 * np.pi / 96 - want) < 2 * np.pi / 96
    # through records: every slot sees the flare at its own emission time, so with one delay the curve peaks at t_peak + dt
    hits, n_hits = synth(24, 40, 3, 77, 4.0, 16.0)
    hits[..., 3] = np.where(np.isnan(hits[..., 3]), np.nan, np.float32(100.0))
    times = 100.0 + 10.0 * np.arange(41)
    lc = diskmod.diskmovie_lightcurve(1.0, 0.9, hits, n_hits, mv, times)[:, 0]
    quiet = diskmod.diskmovie_lightcurve(1.0, 0.9, hits, n_hits, diskmod.flare_movie(41, **dict(kw, amplitude=0.0)), times[:1])[0, 0]
    assert abs(times[np.argmax(lc)] - 300.0) <= 20.0 and lc.max() > 1.3 * quiet
    assert lc[0] == pytest.approx(quiet, rel=1e-6) and lc[-1] == pytest.approx(quiet, rel=1e-6)
    rigid = diskmod.flare_movie(3, **dict(kw, rotation="rigid", omega_p=0.01, boundary="loop", exposure=0.5, with_disk=False))
    assert (rigid.rotation, rigid.omega_p, rigid.boundary, rigid.exposure, rigid.with_disk) == ("rigid", 0.01, "loop", 0.5, False)


# ---- exports, bindings, the struct ------------------------------------------------------------------------------------------
def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(ltrace.DiskMovie) == 2 * 8 + 2 * 4 == 24
    d = ltrace.default_diskmovie()
    assert (d.t0, d.dt_frame, d.n_frames, d.boundary) == (0.0, 1.0, 1, 0)
    d = ltrace.default_diskmovie(boundary="loop", n_frames=7)
    assert d.boundary == ltrace.MOVIE_LOOP == 1 and d.n_frames == 7 and ltrace.MOVIE_HOLD == 0
    movie = diskmod.DiskMovie(movie_table(4, (5, 3)), t0=-2.5, dt_frame=0.75, boundary="loop", r_min=3.0, r_max=9.0, rotation="rigid",
                              omega_p=0.02, exposure=0.5, with_disk=False)
    lt, mv = movie.to_lt()
    assert (lt.r_min, lt.r_max, lt.omega_p, lt.exposure, lt.n_r, lt.n_phi, lt.rotation, lt.with_disk) == (3.0, 9.0, 0.02, 0.5, 5, 3, 1, 0)
    assert (mv.t0, mv.dt_frame, mv.n_frames, mv.boundary) == (-2.5, 0.75, 4, 1)
    assert ctypes.sizeof(ltrace.DiskMap) == 48          # the map's struct is untouched


def test_exports_and_bindings():
    header = (Path(__file__).resolve().parents[1] / "include" / "ltrace.h").read_text()
    declared = sorted(set(re.findall(r"\b(lt_\w*diskmovie\w*)\s*\(", header)))
    want = sorted([f"lt_{stem}{suffix}" for stem in ("shade_diskmovie", "shade_diskmovie_aa", "diskmovie_lightcurve", "diskmovie_spectrum",
                                                      "diskmovie_visibility") for suffix in ("", "_dev")] + ["lt_default_diskmovie"])
    assert declared == want
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name) and name in ltrace.SIGNATURES, name
    for name in declared[1:]:                                            # the map's signature with the movie after the map
        res, args = ltrace.SIGNATURES[name]
        tres, targs = ltrace.SIGNATURES[name.replace("diskmovie", "diskmap")]
        at = targs.index(ctypes.POINTER(ltrace.DiskMap)) + 1
        assert res == tres and args == targs[:at] + [ctypes.POINTER(ltrace.DiskMovie)] + targs[at:], name
    assert ltrace.SIGNATURES["lt_default_diskmovie"] == (None, [ctypes.POINTER(ltrace.DiskMovie)])
    for fn in ("shade_diskmovie", "shade_diskmovie_aa", "diskmovie_lightcurve", "diskmovie_spectrum", "diskmovie_visibility"):
        assert callable(getattr(ltrace, fn)) and callable(getattr(ltrace, fn + "_dev")) and callable(getattr(diskmod, fn))
    for fn in ("sample_movie", "movie_intensity", "movie_emission", "flare_movie"):
        assert callable(getattr(diskmod, fn))
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
        met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
        movie = diskmod.DiskMovie(movie_table(2, (2, 3)))
        dm, mv = movie.to_lt()
        sp, uv = ltrace.default_spectrum(), np.array([[0.1, 0.0]])
        calls = (lambda: ltrace.shade_diskmovie(hits, n_hits, met, d, dm, mv, movie.texels, 0.0),
                 lambda: ltrace.shade_diskmovie_aa(hits, n_hits, 2, met, d, dm, mv, movie.texels, 0.0),
                 lambda: ltrace.diskmovie_lightcurve(hits, n_hits, met, d, dm, mv, movie.texels, 0.0, 1.0, 4),
                 lambda: ltrace.diskmovie_spectrum(hits, n_hits, met, d, dm, mv, movie.texels, sp, 0.0, 1.0, 4),
                 lambda: ltrace.diskmovie_visibility(hits, n_hits, met, d, dm, mv, movie.texels, uv, False, 0.0, 1.0, 4),
                 lambda: ltrace.shade_diskmovie_dev(8, 0, 4, 4, 2, met, d, dm, mv, 8, 0.0),
                 lambda: ltrace.shade_diskmovie_aa_dev(8, 0, 2, 2, 2, 2, met, d, dm, mv, 8, 0.0),
                 lambda: ltrace.diskmovie_lightcurve_dev(8, 0, 4, 4, 2, met, d, dm, mv, 8, 0.0, 1.0, 4, 8),
                 lambda: ltrace.diskmovie_spectrum_dev(8, 0, 4, 4, 2, met, d, dm, mv, 8, sp, 0.0, 1.0, 4, 8),
                 lambda: ltrace.diskmovie_visibility_dev(8, 0, 4, 4, 2, met, d, dm, mv, 8, uv, False, 0.0, 1.0, 4, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE


# ---- refusals that need no device ---------------------------------------------------------------------------------------------
def test_argument_errors():
    import image_lens
    from metrics import Kerr
    metric = Kerr(M=1.0, a=0.9, integrator="rk4", precision=32)
    fov = (np.radians(40.0), np.radians(40.0))
    movie = diskmod.DiskMovie(movie_table(2, (2, 3)))
    td = diskmod.TransparentDisk(max_images=3)
    with pytest.raises(ValueError, match="hot spot"):
        image_lens.render_sequence(None, metric, 50.0, fov, td, diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8), diskmap=movie)
    with pytest.raises(ValueError, match="not polarized"):
        image_lens.render_sequence(None, metric, 50.0, fov, td, None, [0.0, 10.0], shape=(8, 8), bfield=diskmod.BField(), diskmap=movie)
    hits, n_hits = synth(6, 9, 2, 5, 2.4, 20.0)
    met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
    dm, mv = movie.to_lt()
    for fn in (lambda t: ltrace.shade_diskmovie(hits, n_hits, met, d, dm, mv, t, 0.0),
               lambda t: ltrace.shade_diskmovie_aa(hits, n_hits, 3, met, d, dm, mv, t, 0.0),
               lambda t: ltrace.diskmovie_lightcurve(hits, n_hits, met, d, dm, mv, t, 0.0, 1.0, 2),
               lambda t: ltrace.diskmovie_spectrum(hits, n_hits, met, d, dm, mv, t, ltrace.default_spectrum(), 0.0, 1.0, 2),
               lambda t: ltrace.diskmovie_visibility(hits, n_hits, met, d, dm, mv, t, [[0.1, 0.2]], False, 0.0, 1.0, 2)):
        for bad in (np.zeros((2, 3), np.float32), np.zeros((3, 2, 3), np.float32), np.zeros((2, 3, 2), np.float32)):
            with pytest.raises(ValueError, match="texels"):   # tables that are not the structs' (n_frames, n_r, n_phi) never reach the library
                fn(bad)
    for bad in (dict(texels=np.zeros((2, 3))), dict(texels=np.zeros((0, 2, 3))), dict(texels=np.zeros((1, 2, 3)), rotation="solid"),
                dict(texels=np.zeros((1, 2, 3)), boundary="bounce"), dict(texels=np.zeros((1, 2, 3)), dt_frame=0.0),
                dict(texels=np.zeros((1, 2, 3)), dt_frame=-1.0), dict(texels=np.zeros((1, 2, 3)), t0=np.nan),
                dict(texels=np.zeros((1, 2, 3)), dt_frame=np.inf)):
        with pytest.raises(ValueError):
            diskmod.DiskMovie(**bad)


def _parse(extra):
    import image_lens
    return image_lens.build_parser().parse_args(["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"] + extra)


def test_cli_refusals(tmp_path):
    import image_lens
    td = diskmod.TransparentDisk(max_images=3, r_out=18.0)
    np.save(tmp_path / "movie.npy", movie_table(3, (4, 8)))
    np.save(tmp_path / "map.npy", table((4, 8)))
    movie, flat = str(tmp_path / "movie.npy"), str(tmp_path / "map.npy")
    for extra, match in ((["--disk-map", movie], "needs its clock"),                                 # a 3-D array is not guessed at
                         (["--disk-map", "flare"], "needs its clock"),
                         (["--disk-map", flat, "--disk-map-frames", "0", "10"], "clock of a movie"),
                         (["--disk-map", "spiral", "--disk-map-frames", "0", "10"], "clock of a movie"),
                         (["--disk-map", movie, "--disk-map-frames", "0"], "T0 DT"),
                         (["--disk-map", movie, "--disk-map-frames", "0", "10", "bounce"], "T0 DT"),
                         (["--disk-map", movie, "--disk-map-frames", "0", "10", "hold", "1"], "T0 DT"),
                         (["--disk-map", movie, "--disk-map-frames", "zero", "10"], "numbers"),
                         (["--disk-map", movie, "--disk-map-frames", "0", "0"], "DT > 0"),
                         (["--disk-map", movie, "--disk-map-frames", "0", "-5"], "DT > 0"),
                         (["--disk-map", movie, "--disk-map-frames", "nan", "5"], "finite")):
        with pytest.raises(ValueError, match=match):
            image_lens.diskmap_from_args(_parse(extra), td, 1.0, 0.9)
    for extra, match in ((["--hotspot", "8", "0", "1.5"], "--hotspot"), (["--bfield", "0", "0", "1"], "--bfield"),
                         (["--samples", "4", "--adaptive", "2"], "not adaptively sampled")):
        with pytest.raises(ValueError, match=match):                     # a movie with a spot or a field is refused as the map is
            image_lens.main_sequence(_parse(["--disk-map", "flare", "--disk-map-frames", "0", "10"] + extra), td)


def test_cli_builds_the_movie(tmp_path):
    import image_lens
    td = diskmod.TransparentDisk(max_images=3, r_out=18.0)
    tex = movie_table(3, (4, 8))
    np.save(tmp_path / "movie.npy", tex)
    mv = image_lens.diskmap_from_args(_parse(["--disk-map", str(tmp_path / "movie.npy"), "--disk-map-frames", "-4", "2.5", "loop", "--disk-map-range",
                                              "5", "15", "--disk-map-rotation", "rigid", "--disk-map-omega", "0.02", "--disk-map-exposure", "0.5"]),
                                      td, 1.0, 0.9)
    assert isinstance(mv, diskmod.DiskMovie) and np.array_equal(mv.texels, tex)
    assert (mv.t0, mv.dt_frame, mv.boundary, mv.r_min, mv.r_max, mv.rotation, mv.omega_p, mv.exposure) == (-4.0, 2.5, "loop", 5.0, 15.0, "rigid",
                                                                                                         0.02, 0.5)
    fl = image_lens.diskmap_from_args(_parse(["--disk-map", "flare", "--disk-map-frames", "100", "10"]), td, 1.0, 0.9)
    assert isinstance(fl, diskmod.DiskMovie) and fl.texels.shape == (32, 256, 1024) and fl.boundary == "hold"
    assert (fl.t0, fl.dt_frame, fl.r_min, fl.r_max) == (100.0, 10.0, td.inner_edge(1.0, 0.9), 18.0)
    assert np.argmax(fl.texels.astype(np.float64).sum(axis=(1, 2))) == 12
    flat = image_lens.diskmap_from_args(_parse(["--disk-map", "spiral"]), td, 1.0, 0.9)
    assert isinstance(flat, diskmod.DiskMap)
