"""The disk movie's kernels (lt_diskmovie.hpp) through the ten lt_*diskmovie* entry points.  Cases, movies, variants, the
longdouble reference and the bounds are tests/test_diskmovie_host.py's (its header derives the bounds); the records are the
map's synthetic ones at the sizes that reach the kernels' edges -- 257 x 331 x 8, 260 x 300 x 3, 3 x 70 x 5, 1 x 1 x 1,
counts above max_images -- and the 96 x 80 trace of test_gpu_diskmap.py for render_sequence.

Rolled tables (test_rolled_tables_are_the_rigid_map), derived.  Under rigid rotation with omega_p dt_frame = j 2 pi / n_phi,
frame k = roll(table, j k) along phi and t0 = 0, frame k looked up at psi_k = phi - omega_p (t_em - k dt_frame) is the table
looked up at phi - omega_p t_em: both frames of a pair give the rigid map's m, and so does their blend.  What is left is
rounding.  (a) The blend (1 - f_t) m + f_t m: three roundings, 4 2^-53 relative.  (b) The azimuth: the float64 omega_p
dt_frame differs from j 2 pi / n_phi by at most 2 2^-53 of it, q <= n_frames times over; both sides round their phases, each
within 8 2^-53 omega_p (|t_em| + n_frames dt_frame) (test_diskmovie_host.py, (a)):
    d_psi <= 8 2^-53 (2 omega_p (max|t_em| + n_frames dt_frame) + 2 pi j n_frames / n_phi),
and a step d_psi moves a bilinear value by at most d_psi (n_phi / 2 pi) (T_max - T_min).  Per pixel and channel, ramp <= 1:
    |d rgb| <= sum_j exposure g_j^4 [d_psi (n_phi / 2 pi) (T_max - T_min) + 4 2^-53 T_max]  +  2 ulp of float32
-- some 1e-14 next to 2 ulp.  The light curves agree within the sum of the map's and the movie's bounds.  The control rolls
the frames the other way: the brightest pixel must then miss its bound by a factor of at least 100.

MEASURED on an MI355X (gfx950), the figures the tests print:
    frames against longdouble: no float32 differs (0.00 ulp) on big and mid (6 frames each), strip and one (16 each); bound 2;
        433 380, 375 332, 1 011 and 12 lit, unsaturated values;
    light curves against longdouble, nearest to the bound: big 1.8e-16 relative (bound 1.7e-12, rigid loop, t = 600), mid
        2.9e-15 (2.6e-11, Keplerian hold, t = -3e4), strip 1.1e-13 (2.9e-11, one rigid held frame, t = 1e5), one 6.2e-13 (1.8e-11,
        one rigid held frame, t = -3e4); never above 3.5 % of a bound;
    sum of a frame against the light curve: big 2.5e-10, mid 3.1e-10, strip 1.9e-9, one 9.4e-9 (bound 2^-23 = 1.19e-7); brightest
        pixel 0.41, 0.25, 0.21, 0.007;
    rolled tables against lt_shade_diskmap: no float32 differs on mid and strip; the light curves 1.4e-16 and 2.9e-16 relative
        (bound 2.1e-12); rolled the other way the brightest pixel (0.27, 0.20) misses its bound 1 184 732 and 1 593 834 times;
    spectrum against disk.diskmovie_spectrum: mid 5.7e-15 relative, 0.2 % of its bound, strip 1.0e-15; rows against the light
        curve's column 0: 4.5e-16 (bound 1.1e-11) and 2.6e-16 (4.3e-14); visibilities: 0.1 % of the bound on mid, less on strip;
    render_sequence with flare_movie: the light peaks at t = 268; per image order at 268, 316, 300 (excess light's centre
        267.0, 314.6, 303.9), with samples = 2 at 268, 308, 324 (267.0, 311.5, 313.3).
"""
import ctypes as C

import numpy as np
import pytest

import aa
import disk as diskmod
import ltrace
from test_diskmap_host import CASES, DISK_EXPOSURE, LC_GRIDS, MAP_EXPOSURE, base_of, grid_times, make_map, map_lc_bound, records, table
from test_diskmap_host import VARIANTS as MAP_VARIANTS
from test_diskmovie_host import (BIG_LC_GRIDS, DT_FRAME, MOVIE_LC_GRIDS, T0, TABLES, VARIANTS, make_movie, movie_lc_bound, movie_records, movie_table,
                                 observer_time)
from test_gpu_diskmap import SEQ, check_rgba, replicate, upload
from test_hotspot_records_host import isco_ref, lc_excess, synth, ulps
from test_spectrum_host import GRIDS, SpectrumReference, U, check_spectrum
from test_visibility_host import BASELINES, check_visibility, phase_bound

pytestmark = pytest.mark.gpu
LD = np.longdouble


def setup(name):
    c = CASES[name]
    hits, n_hits, ref = movie_records(name)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a)
    dk = ltrace.default_disk(r_out=c.r_out, exposure=DISK_EXPOSURE)      # r_in 0: the ISCO, resolved by the library
    return c, hits, n_hits, ref, met, dk


def lt(movie):
    """(lt_diskmap, lt_diskmovie, texels): the movie as the bindings take it."""
    dm, mv = movie.to_lt()
    return dm, mv, movie.texels


def one_frame(movie, k, **kw):
    """The one-frame movie that holds frame k of `movie`."""
    return diskmod.DiskMovie(movie.texels[k:k + 1], **{**dict(t0=movie.t0, dt_frame=movie.dt_frame, r_min=movie.r_min, r_max=movie.r_max,
                                                               rotation=movie.rotation, omega_p=movie.omega_p, exposure=movie.exposure,
                                                               with_disk=movie.with_disk), **kw})


def same(a, b):
    return a["rgb"].tobytes() == b["rgb"].tobytes() and a["rgba"].tobytes() == b["rgba"].tobytes()


# ---- 1. frames against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_frames_against_the_reference(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(isco_ref(c.M, c.a))
    worst, inside, frames = 0.0, 0, 0
    for v in VARIANTS:
        movie, base = make_movie(c, v), base_of(c, v)
        for t in v.t_obs[:1] if c.R * c.W > 1000 else v.t_obs:
            t_obs = observer_time(t, ref, movie)
            got = ltrace.shade_diskmovie(hits, n_hits if v.counts else None, met, dk, *lt(movie), t_obs, base=base, channels=v.channels)
            want = ref.frame(c.M, c.a, movie, t_obs, r_in, 3.0, DISK_EXPOSURE, base=base, channels=v.channels).astype(np.float32)
            assert got["rgb"].shape == want.shape and got["rgb"].dtype == np.float32
            worst = max(worst, float(np.max(ulps(got["rgb"], want))))
            check_rgba(got["rgba"], want)
            if t == v.t_obs[0]:
                inside += int(((want > (0 if base is None else base)) & (want < 1)).sum())
            frames += 1
    print(f"{name}: {frames} frames against longdouble, largest difference {worst:.2f} ulp of float32; {inside} lit, unsaturated values")
    assert worst <= 2
    assert inside >= (1 if c.R * c.W == 1 else 0.2 * c.R * c.W)


# ---- 2. light curves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lightcurve_against_the_reference(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(diskmod.isco(c.M, c.a))
    big = c.R * c.W > 1000
    top = (0.0, 0.0, "")
    for v in VARIANTS[:2] if big else VARIANTS:
        movie = make_movie(c, v)
        for grid in BIG_LC_GRIDS if big else MOVIE_LC_GRIDS:
            times = grid_times(grid)
            lc = ltrace.diskmovie_lightcurve(hits, n_hits if v.counts else None, met, dk, *lt(movie), *grid)
            assert lc.shape == (grid[2], 3)
            again = ltrace.diskmovie_lightcurve(hits, n_hits if v.counts else None, met, dk, *lt(movie), *grid)
            assert again.tobytes() == lc.tobytes()                       # a second run differs in no bit
            want = ref.lightcurve(c.M, c.a, movie, times)
            bound = movie_lc_bound(c.M, c.a, movie, times, r_in)
            excess, rel = lc_excess(lc, want, bound)
            top = max(top, (excess, rel, f"{v.rotation} {v.boundary} {v.n_frames} x {TABLES[v.table]} t = {grid[0]:g} (bound {bound:.2e})"))
            assert np.all(want[:, 0] > 0)
            assert excess <= 1
    print(f"{name}: light curve against longdouble, nearest to its bound: {top[1]:.2e} relative, {top[0]:.3f} of the bound, at {top[2]}")


@pytest.mark.parametrize("name", list(CASES))
def test_frame_sums_to_the_lightcurve(name):
    """The set-up of test_gpu_diskmap's test of this name: without disk and base, one channel, unclamped (the reference's
    brightest pixel is below 1), a frame's pixels are the light curve's terms rounded to float32: sums agree to 2^-23."""
    c, hits, n_hits, ref, met, dk = setup(name)
    ix, iy = np.meshgrid(np.arange(c.W), np.arange(c.R))
    worst = 0.0
    for v in (VARIANTS[1], VARIANTS[4]):                                  # rigid loop and Keplerian hold, both without the disk
        movie = make_movie(c, v, exposure=0.02)
        brightest = float(ref.frame(c.M, c.a, movie, 600.0, 0.0, channels=1, clamp=False).max())
        assert brightest < 1
        rgb = ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(movie), 600.0, channels=1, want=("rgb",))["rgb"].astype(LD)
        lc = ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(movie), 600.0, 1.0, 1)[0].astype(LD)
        assert lc[0] > 0
        for col, wgt in enumerate((1, ix, iy)):
            s = (rgb * wgt).sum()
            assert abs(s - lc[col]) <= LD(2.0 ** -23) * lc[col]
            if lc[col] > 0:
                worst = max(worst, float(abs(s - lc[col]) / lc[col]))
    print(f"{name}: brightest pixel {brightest:.3f}; sum of the frame against the light curve, largest relative difference {worst:.2e}")


# ---- 3. one held frame is the map ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip", "one"))
def test_one_held_frame_is_the_map(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    sp = ltrace.default_spectrum(g_min=0.3, g_max=1.2, n_bins=7, split_orders=1)
    lit = 0
    for v, dt_frame in zip(MAP_VARIANTS[:4], (3.7, 128.0, 1e-3, 1e9)):   # both rotations, with and without base, counts and disk
        dmap, base, nh = make_map(c, v), base_of(c, v), n_hits if v.counts else None
        movie = diskmod.DiskMovie(dmap.texels[None], t0=0.0, dt_frame=dt_frame, boundary="hold", r_min=dmap.r_min, r_max=dmap.r_max,
                                  rotation=dmap.rotation, omega_p=dmap.omega_p, exposure=dmap.exposure, with_disk=dmap.with_disk)
        m_args, mv_args = (dmap.to_lt(), dmap.texels), lt(movie)
        want = ltrace.shade_diskmap(hits, nh, met, dk, *m_args, v.t_obs, base=base, channels=v.channels)
        assert same(ltrace.shade_diskmovie(hits, nh, met, dk, *mv_args, v.t_obs, base=base, channels=v.channels), want)
        lit += int((want["rgb"] > (0 if base is None else base)).sum())
        if c.R % 2 == 0 and c.W % 2 == 0:
            fb = None if base is None else base
            assert same(ltrace.shade_diskmovie_aa(hits, nh, 2, met, dk, *mv_args, v.t_obs, base=fb, channels=v.channels),
                        ltrace.shade_diskmap_aa(hits, nh, 2, met, dk, *m_args, v.t_obs, base=fb, channels=v.channels))
        else:
            assert same(ltrace.shade_diskmovie_aa(replicate(hits, 2), None if nh is None else replicate(nh, 2), 2, met, dk, *mv_args, v.t_obs),
                        ltrace.shade_diskmap_aa(replicate(hits, 2), None if nh is None else replicate(nh, 2), 2, met, dk, *m_args, v.t_obs))
        for grid in LC_GRIDS[:3]:
            assert (ltrace.diskmovie_lightcurve(hits, nh, met, dk, *mv_args, *grid).tobytes()
                    == ltrace.diskmap_lightcurve(hits, nh, met, dk, *m_args, *grid).tobytes())
        grid = (LC_GRIDS[0][0], LC_GRIDS[0][1], 3)
        assert (ltrace.diskmovie_spectrum(hits, nh, met, dk, *mv_args, sp, *grid).tobytes()
                == ltrace.diskmap_spectrum(hits, nh, met, dk, *m_args, sp, *grid).tobytes())
        for split in (False, True):
            assert (ltrace.diskmovie_visibility(hits, nh, met, dk, *mv_args, BASELINES, split, *grid).tobytes()
                    == ltrace.diskmap_visibility(hits, nh, met, dk, *m_args, BASELINES, split, *grid).tobytes())
    assert lit > 0


# ---- 4. rolled tables are the rigid map, and the sign is pinned -------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip"))
def test_rolled_tables_are_the_rigid_map(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    n_frames, j, dt_frame, t_obs, exposure = 5, 3, 128.0, 470.0, 0.02       # emission times 70 ... 440 inside the movie's 0 ... 512
    T = table((37, 64))
    n_phi = T.shape[1]
    omega_p = j * 2 * np.pi / n_phi / dt_frame
    r_in = float(diskmod.isco(c.M, c.a))
    common = dict(r_min=0.5 * r_in, r_max=c.r_out + c.M, rotation="rigid", omega_p=omega_p, exposure=exposure, with_disk=False)
    dmap = diskmod.DiskMap(T, **common)
    movie = diskmod.DiskMovie(np.stack([np.roll(T, j * k, axis=1) for k in range(n_frames)]), t0=0.0, dt_frame=dt_frame, **common)
    wrong = diskmod.DiskMovie(np.stack([np.roll(T, -j * k, axis=1) for k in range(n_frames)]), t0=0.0, dt_frame=dt_frame, **common)
    t_em = t_obs - ref.dt.astype(np.float64)
    assert t_em.min() > 0 and t_em.max() < (n_frames - 1) * dt_frame
    want = ltrace.shade_diskmap(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, t_obs, channels=1, want=("rgb",))["rgb"]
    got = ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(movie), t_obs, channels=1, want=("rgb",))["rgb"]
    bad = ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(wrong), t_obs, channels=1, want=("rgb",))["rgb"]
    assert 0 < want.max() < 1
    d_psi = 8 * U * (2 * omega_p * (np.abs(t_em).max() + n_frames * dt_frame) + 2 * np.pi * j * n_frames / n_phi)
    per_g4 = exposure * (d_psi * n_phi / (2 * np.pi) * float(T.max() - T.min()) + 4 * U * float(T.max()))
    stored = np.arange(c.m) < np.minimum(n_hits, c.m)[..., None]
    g4 = (np.where(stored, hits[..., 2].astype(np.float64), 0.0) ** 4).sum(axis=-1)
    bound = g4 * per_g4 + 2 * np.spacing(np.maximum(np.abs(want), np.float32(1e-30))).astype(np.float64)
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    worst = float(np.max(diff / bound))
    at = np.unravel_index(np.argmax(want), want.shape)
    control = float(abs(float(bad[at]) - float(want[at])) / bound[at])
    print(f"{name}: rolled frames against lt_shade_diskmap, largest difference {worst:.2f} of the pixel's bound ({float(np.max(ulps(got, want))):.2f} "
          f"ulp); rolled the other way the brightest pixel ({float(want[at]):.3f}) misses its bound {control:.0f} times")
    assert np.all(diff <= bound)
    assert control >= 100                                                  # otherwise the comparison says nothing
    grid = (t_obs, 0.25, 4)
    times = grid_times(grid)
    lc_map = ltrace.diskmap_lightcurve(hits, n_hits, met, dk, dmap.to_lt(), dmap.texels, *grid)
    lc = ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(movie), *grid)
    both = map_lc_bound(c.M, c.a, dmap, times, r_in) + movie_lc_bound(c.M, c.a, movie, times, r_in)
    rel = float(np.max(np.abs(lc - lc_map) / np.where(lc_map == 0, 1.0, np.abs(lc_map))))
    print(f"{name}: rolled frames' light curve against lt_diskmap_lightcurve, largest relative difference {rel:.2e}, bound {both:.2e}")
    assert np.all(lc_map[:, 0] > 0) and rel <= both
    lc_bad = ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(wrong), *grid)
    assert np.max(np.abs(lc_bad - lc_map) / np.abs(lc_map)) >= 100 * both


# ---- 5., 6. loop and hold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("mid", "strip"))
def test_loop_repeats_after_one_period(name):
    """Dyadic t0, dt_frame and t_obs and omega_p = 0: t_em and t_em + n_frames dt_frame are exact and give one s - floor(s)."""
    c, hits, n_hits, ref, met, dk = setup(name)
    v = VARIANTS[1]._replace(counts=True)                                  # rigid, loop, five frames of 37 x 64
    movie = make_movie(c, v)
    movie.omega_p = 0.0
    period = movie.n_frames * movie.dt_frame
    base = base_of(c, v._replace(base=True, channels=3))
    frame = lambda t: ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(movie), t, base=base)
    curve = lambda t: ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(movie), t, 0.5, 3)
    for t_obs in (600.0, 80.0):
        assert same(frame(t_obs), frame(t_obs + period)) and same(frame(t_obs), frame(t_obs - 3 * period))
        assert curve(t_obs).tobytes() == curve(t_obs + period).tobytes()
        assert not same(frame(t_obs), frame(t_obs + movie.dt_frame)) and curve(t_obs).tobytes() != curve(t_obs + movie.dt_frame).tobytes()


@pytest.mark.parametrize("name", ("mid", "strip"))
def test_hold_keeps_the_end_frames(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    v = VARIANTS[0]                                                       # hold, five frames of 37 x 64, with disk and base
    movie = make_movie(c, v._replace(rotation="rigid"))
    movie.omega_p = 0.0
    base = base_of(c, v)
    for t_obs, k in ((80.0, 0), (20.0, 0), (2000.0, movie.n_frames - 1), (T0 + 4 * DT_FRAME + 400.0, movie.n_frames - 1)):
        t_em = t_obs - ref.dt.astype(np.float64)
        assert np.all(t_em < movie.t0) if k == 0 else np.all(t_em >= movie.t0 + k * movie.dt_frame)
        held = one_frame(movie, k)
        assert same(ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(movie), t_obs, base=base),
                    ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(held), t_obs, base=base))
        assert (ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(movie), t_obs, 0.0, 1).tobytes()
                == ltrace.diskmovie_lightcurve(hits, n_hits, met, dk, *lt(held), t_obs, 0.0, 1).tobytes())
    other = one_frame(movie, 1)
    assert not same(ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(movie), 80.0, base=base),
                    ltrace.shade_diskmovie(hits, n_hits, met, dk, *lt(other), 80.0, base=base))


# ---- 7. supersampled frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,R,W,m", [(2, 37, 51, 3), (3, 19, 29, 8), (4, 13, 21, 5)])
def test_aa_is_the_resolve_of_the_fine_frame(S, R, W, m):
    """R W is no multiple of 256 / S^2 (64, 28, 16), so the last workgroup is partial and slots straddle output rows."""
    assert (R * W) % (256 // (S * S)) != 0
    import hipmini
    M, a, r_out = 1.0, 0.9, 20.0
    hits, n_hits = synth(R * S, W * S, m, 80 + S, float(diskmod.isco(M, a)), r_out)
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), ltrace.default_disk(r_out=r_out, exposure=DISK_EXPOSURE)
    rng = np.random.default_rng(S)
    differs = 0
    for v in VARIANTS[:4]:
        movie, t_obs = make_movie(CASES["big"], v), 600.0
        base = rng.uniform(0.0, 0.5, (R * S, W * S) + ((3,) if v.channels == 3 else ())).astype(np.float32) if v.base else None
        nh = n_hits if v.counts else None
        fine = ltrace.shade_diskmovie(hits, nh, met, dk, *lt(movie), t_obs, base=base, channels=v.channels)
        got = ltrace.shade_diskmovie_aa(hits, nh, S, met, dk, *lt(movie), t_obs, base=base, channels=v.channels)
        want = aa.resolve(fine["rgb"], S)
        assert got["rgb"].shape == want.shape == ((R, W, 3) if v.channels == 3 else (R, W)) and got["rgb"].dtype == np.float32
        assert np.array_equal(got["rgb"], want)
        check_rgba(got["rgba"], want)
        differs += int(not np.array_equal(want, fine["rgb"][::S, ::S]))
        # device pointers give the host form's bytes
        d_hits, d_n, d_tex = upload(hits), upload(n_hits), upload(movie.texels)
        d_base = upload(base) if base is not None else None
        d_rgb, d_rgba = hipmini.DeviceArray(want.shape, np.float32), hipmini.DeviceArray((R, W, 4), np.uint8)
        dm, mv, _ = lt(movie)
        ltrace.shade_diskmovie_aa_dev(d_hits.ptr, d_n.ptr if v.counts else 0, R, W, S, m, met, dk, dm, mv, d_tex.ptr, t_obs,
                                      d_base=d_base.ptr if d_base else 0, channels=v.channels, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
        assert d_rgb.get().tobytes() == got["rgb"].tobytes() and d_rgba.get().tobytes() == got["rgba"].tobytes()
    assert differs == 4                                                   # a mean, not a pick


@pytest.mark.parametrize("name", ("strip", "one"))
def test_aa_of_one_sample_and_of_repeated_records(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    for v in VARIANTS[:4]:
        movie, base, nh, t_obs = make_movie(c, v), base_of(c, v), n_hits if v.counts else None, 600.0
        one = ltrace.shade_diskmovie(hits, nh, met, dk, *lt(movie), t_obs, base=base, channels=v.channels)
        assert same(ltrace.shade_diskmovie_aa(hits, nh, 1, met, dk, *lt(movie), t_obs, base=base, channels=v.channels), one)
        for S in (2, 3, 8):
            # every sub-sample is the same float32 x; k x is exact in float64 for k <= 64, so the mean is x
            rep = ltrace.shade_diskmovie_aa(replicate(hits, S), None if nh is None else replicate(nh, S), S, met, dk, *lt(movie), t_obs,
                                            base=None if base is None else replicate(base, S), channels=v.channels)
            assert same(rep, one)


# ---- 8. spectrum and visibilities ---------------------------------------------------------------------------------------------------
_SREF = {}


def spectrum_ref(name):
    if name not in _SREF:
        hits, n_hits, _ = records(name)
        _SREF[name] = SpectrumReference(hits, n_hits)
    return _SREF[name]


@pytest.mark.parametrize("name", ("mid", "strip"))
def test_spectrum_against_the_numpy_statement(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(diskmod.isco(c.M, c.a))
    sref = spectrum_ref(name)
    worst = (0.0, 0.0)
    for v, lcg in ((VARIANTS[0], (600.0, 9.0, 3)), (VARIANTS[1], (1e5, 11.0, 2))):
        movie, times = make_movie(c, v), grid_times(lcg)
        bound = movie_lc_bound(c.M, c.a, movie, times, r_in)
        for grid, split in ((GRIDS[0], True), (GRIDS[1], False)):
            spec = diskmod.Spectrum(*grid, split_orders=split)
            nh = n_hits if split else None                       # with the counts and with the NaN padding
            got = ltrace.diskmovie_spectrum(hits, nh, met, dk, *lt(movie), spec.to_lt(), *lcg)
            want = diskmod.diskmovie_spectrum(c.M, c.a, hits, nh, movie, spec, times).astype(LD)
            worst = max(worst, check_spectrum(got, want, sref.keys(grid, split)[3], bound))
            assert np.all(got.sum(axis=(1, 2)) > 0)
            # the same bits run after run and whatever batch of times a row is computed in
            assert ltrace.diskmovie_spectrum(hits, nh, met, dk, *lt(movie), spec.to_lt(), *lcg).tobytes() == got.tobytes()
            for i in range(lcg[2]):
                row = ltrace.diskmovie_spectrum(hits, nh, met, dk, *lt(movie), spec.to_lt(), float(times[i]), lcg[1], 1)
                assert row.tobytes() == got[i:i + 1].tobytes()
    print(f"{name}: spectrum against disk.diskmovie_spectrum, largest relative difference {worst[1]:.2e}, {worst[0]:.3f} of its bound")
    assert worst[0] <= 1


@pytest.mark.parametrize("name", ("mid", "strip"))
def test_spectrum_rows_sum_to_the_light_curve(name):
    """test_gpu_spectrum's set-up: with every g in [1, 1.4] the ramp is (1, 1, 1) and a row adds the light curve's terms:
    within (4 + n_terms) 2^-53 relative of column 0."""
    c, hits, n_hits, ref, met, dk = setup(name)
    bright = hits.copy()
    bright[..., 2] = (1.0 + 0.4 * (hits[..., 2].astype(np.float64) - 0.15) / 1.25).astype(np.float32)     # g into [1, 1.4]
    stored = np.arange(c.m) < np.minimum(n_hits, c.m)[..., None]
    n_terms = int(stored.sum())
    worst = 0.0
    for v in VARIANTS[:2]:
        movie = make_movie(c, v)
        for lcg in ((600.0, 8.0, 3), LC_GRIDS[1]):                        # (times whose i dt is exact: the light curve may use an fma)
            for grid, split in ((GRIDS[1], False), (GRIDS[0], True)):
                sp = diskmod.Spectrum(*grid, split_orders=split).to_lt()
                spectrum = ltrace.diskmovie_spectrum(bright, n_hits, met, dk, *lt(movie), sp, *lcg)
                lc = ltrace.diskmovie_lightcurve(bright, n_hits, met, dk, *lt(movie), *lcg)
                rows = spectrum.astype(LD).sum(axis=(1, 2))
                assert np.all(lc[:, 0] > 0)
                rel = np.abs(rows - lc[:, 0].astype(LD)) / lc[:, 0].astype(LD)
                worst = max(worst, float(rel.max()))
                assert np.all(rel <= (4 + n_terms) * U)
    print(f"{name}: spectrum rows against the light curve's column 0, largest relative difference {worst:.2e}, bound {(4 + n_terms) * U:.2e}")


@pytest.mark.parametrize("name", ("mid", "strip"))
def test_visibility_against_the_numpy_statement(name):
    c, hits, n_hits, ref, met, dk = setup(name)
    r_in = float(diskmod.isco(c.M, c.a))
    sref = spectrum_ref(name)
    pb = phase_bound(c.R, c.W)
    worst = 0.0
    for v, lcg in ((VARIANTS[0], (600.0, 9.0, 3)), (VARIANTS[1], (1e5, 11.0, 2))):
        movie, times = make_movie(c, v), grid_times(lcg)
        bound = movie_lc_bound(c.M, c.a, movie, times, r_in)
        for split in (False, True):
            nh = n_hits if split else None
            counts = np.bincount(sref.slot, minlength=c.m) if split else np.array([sref.slot.size])
            got = ltrace.diskmovie_visibility(hits, nh, met, dk, *lt(movie), BASELINES, split, *lcg)
            want = diskmod.diskmovie_visibility(c.M, c.a, hits, nh, movie, BASELINES, split, times)
            assert np.all(BASELINES[0] == 0)
            flux = want[..., 0].real.astype(LD)                            # the zero baseline is the plane's flux
            worst = max(worst, check_visibility(got, (want.real.astype(LD), want.imag.astype(LD), flux), counts, bound, pb))
            assert np.all(flux[..., counts > 0] > 0)
            # the same bits run after run, whatever batch of times a row is computed in; V(-u, -v) is the conjugate to the bit
            assert ltrace.diskmovie_visibility(hits, nh, met, dk, *lt(movie), BASELINES, split, *lcg).tobytes() == got.tobytes()
            for i in range(lcg[2]):
                row = ltrace.diskmovie_visibility(hits, nh, met, dk, *lt(movie), BASELINES, split, float(times[i]), lcg[1], 1)
                assert row.tobytes() == got[i:i + 1].tobytes()
            mirror = ltrace.diskmovie_visibility(hits, nh, met, dk, *lt(movie), -BASELINES, split, *lcg)
            assert np.array_equal(mirror.real, got.real) and np.array_equal(mirror.imag, -got.imag)
    print(f"{name}: visibilities against disk.diskmovie_visibility, {worst:.3f} of the bound")
    assert worst <= 1


def test_visibility_batches_of_times():
    """More times than a workgroup holds at once (16 without split_orders, 3 with five planes): a row does not depend on its batch."""
    c, hits, n_hits, ref, met, dk = setup("strip")
    movie = make_movie(c, VARIANTS[0])
    for split, n in ((False, 19), (True, 7)):
        assert n > ltrace.visibility_batch_times(split, c.m)
        got = ltrace.diskmovie_visibility(hits, n_hits, met, dk, *lt(movie), BASELINES, split, 500.0, 16.0, n)
        for i in (0, n // 2, n - 1):
            row = ltrace.diskmovie_visibility(hits, n_hits, met, dk, *lt(movie), BASELINES, split, 500.0 + 16.0 * i, 16.0, 1)
            assert row.tobytes() == got[i:i + 1].tobytes()
        assert len({got[i].tobytes() for i in range(n)}) == n             # the movie moves


# ---- 9. device pointers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("big", "one"))
def test_dev_entry_points_give_the_host_bytes(name):
    import hipmini
    c, hits, n_hits, ref, met, dk = setup(name)
    d_hits, d_n = upload(hits), upload(n_hits)
    for v in VARIANTS[:4]:
        movie, base = make_movie(c, v), base_of(c, v)
        dm, mv, tex = lt(movie)
        d_tex = upload(tex)
        nh, d_nh = (n_hits, d_n.ptr) if v.counts else (None, 0)
        grid = (600.0, 7.5, 3)
        lc = ltrace.diskmovie_lightcurve(hits, nh, met, dk, dm, mv, tex, *grid)
        d_out = hipmini.DeviceArray((grid[2], 3), np.float64)
        ltrace.diskmovie_lightcurve_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm, mv, d_tex.ptr, *grid, d_out.ptr)
        assert d_out.get().tobytes() == lc.tobytes()      # (the blocking copy orders behind the default stream's kernels)
        host = ltrace.shade_diskmovie(hits, nh, met, dk, dm, mv, tex, 600.0, base=base, channels=v.channels)
        d_base = upload(base) if base is not None else None
        d_rgb, d_rgba = hipmini.DeviceArray(host["rgb"].shape, np.float32), hipmini.DeviceArray((c.R, c.W, 4), np.uint8)
        ltrace.shade_diskmovie_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm, mv, d_tex.ptr, 600.0, d_base=d_base.ptr if d_base else 0,
                                   channels=v.channels, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
        assert d_rgb.get().tobytes() == host["rgb"].tobytes() and d_rgba.get().tobytes() == host["rgba"].tobytes()
        split = v.counts
        sp = diskmod.Spectrum(*GRIDS[0], split_orders=split).to_lt()
        spectrum = ltrace.diskmovie_spectrum(hits, nh, met, dk, dm, mv, tex, sp, *grid)
        d_sp = hipmini.DeviceArray(spectrum.shape, np.float64)
        ltrace.diskmovie_spectrum_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm, mv, d_tex.ptr, sp, *grid, d_sp.ptr)
        assert d_sp.get().tobytes() == spectrum.tobytes()
        vis = ltrace.diskmovie_visibility(hits, nh, met, dk, dm, mv, tex, BASELINES, split, *grid)
        d_vis = hipmini.DeviceArray(vis.shape + (2,), np.float64)
        ltrace.diskmovie_visibility_dev(d_hits.ptr, d_nh, c.R, c.W, c.m, met, dk, dm, mv, d_tex.ptr, BASELINES, split, *grid, d_vis.ptr)
        assert d_vis.get().tobytes() == vis.tobytes()


# ---- 10. render_sequence with a DiskMovie -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [None, 2])
def test_render_sequence_with_a_flare(S):
    import image_lens
    from metrics import Kerr
    M, a = SEQ["M"], SEQ["a"]
    r_in = float(diskmod.isco(M, a))
    # a clump far out, where the orbit (332 M) is long against the flare (15 M wide): the beaming changes little while it lasts
    movie = diskmod.flare_movie(48, 32, 128, r_in, SEQ["r_out"], r_s=14.0, phi_s=1.0, sigma=2.0, t_peak=220.0, t_width=15.0, dt_frame=10.0, t0=0.0,
                                floor=0.05, amplitude=6.0, M=M, a=a, exposure=0.5)
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    times = 100.0 + 8.0 * np.arange(48)
    spec = diskmod.Spectrum(0.0625, 1.5625, 8, split_orders=True)
    out = image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk, None, times,
                                     shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], samples=S, diskmap=movie, spectrum=spec,
                                     baselines=diskmod.Baselines.radial(4, 0.2, 30.0, split_orders=True))
    k = 1 if S is None else S
    n = times.size
    assert out["hits"].shape == (SEQ["shape"][0] * k, SEQ["shape"][1] * k, SEQ["max_images"], 4)
    assert out["frames"].shape == (n,) + SEQ["shape"] + (3,) and out["rgba"].shape == (n,) + SEQ["shape"] + (4,)
    assert out.get("samples") == S and out["spectrum"].shape == (n, 3, 10) and out["visibility"].shape == (n, 3, 4)
    assert out["disk_spectrum"].shape == (3, 10) and out["disk_visibility"].shape == (3, 4)
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
    rec = (out["hits"], out["n_hits"])
    for i in range(0, n, 5):
        if S is None:
            f = ltrace.shade_diskmovie(*rec, met, dk, *lt(movie), float(times[i]))
        else:
            f = ltrace.shade_diskmovie_aa(*rec, S, met, dk, *lt(movie), float(times[i]))
        assert np.array_equal(out["frames"][i], f["rgb"]) and np.array_equal(out["rgba"][i], f["rgba"])
    lc = ltrace.diskmovie_lightcurve(*rec, met, dk, *lt(movie), 100.0, 8.0, n)
    assert np.array_equal(out["lightcurve"], lc / np.array([k * k, k ** 3, k ** 3], dtype=np.float64))
    dyn = ltrace.diskmovie_spectrum(*rec, met, dk, *lt(movie), spec.to_lt(), 100.0, 8.0, n)
    assert np.array_equal(out["spectrum"], dyn / np.float64(k * k))
    # the light curve rises and falls
    flux = out["lightcurve"][:, 0]
    peak = int(np.argmax(flux))
    assert 5 < peak < n - 5 and flux[peak] > 1.5 * flux[0] and flux[peak] > 1.5 * flux[-1]
    assert flux[peak - 6] < flux[peak - 3] < flux[peak] > flux[peak + 3] > flux[peak + 6]
    # the echo: every image order sees the flare at its own emission time, so the first-order image peaks later
    orders = out["spectrum"].sum(axis=2)                                  # (n, planes): the light of every image order
    excess = orders - orders.min(axis=0)
    t_c = (excess * times[:, None]).sum(axis=0) / excess.sum(axis=0)
    t_pk = times[np.argmax(orders, axis=0)]
    vis0 = np.abs(out["visibility"][:, :, 0])                             # the zero baseline of the per-order visibilities: the same light
    print(f"samples {S}: the flare's light peaks at t = {times[peak]:g}; per image order the peak is at {t_pk.tolist()} and the excess light's "
          f"centre at {np.round(t_c, 1).tolist()}")
    assert t_pk[1] > t_pk[0] and t_c[1] > t_c[0]
    assert np.argmax(vis0[:, 1]) > np.argmax(vis0[:, 0])
    stored = np.arange(3) < np.minimum(out["n_hits"], 3)[..., None]
    assert np.nanmean(np.where(stored[..., 1], out["hits"][..., 1, 3], np.nan)) > np.nanmean(np.where(stored[..., 0], out["hits"][..., 0, 3], np.nan))


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, ref, met, dk = setup("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    good = make_movie(c, VARIANTS[0])
    uv = np.ascontiguousarray(BASELINES[:3])
    spec = ltrace.default_spectrum(g_min=0.3, g_max=1.2, n_bins=7)
    FORMS = ("frame", "aa", "curve", "spectrum", "visibility")

    def call(form="frame", hits_=hits, met_=met, disk_=dk, lt_=None, mv=None, tex=good.texels, R=c.R, W=c.W, m=c.m, S_=1, channels=3, t_obs=333.25,
             t_start=0.0, dt=1.0, n_times=2):
        """-> (code, message); the outputs of a refused call are untouched."""
        lt_ = lt_ or good.to_lt()[0]
        mv = mv or good.to_lt()[1]
        rgb, rgba, out = np.full((c.R, c.W, 3), -7.0, np.float32), np.full((c.R, c.W, 4), 77, np.uint8), np.full((4, 3), -7.0)
        sp_out, vis_out = np.full((4, 1, 9), -7.0), np.full((4, 1, 3, 2), -7.0)
        head = (ptr(hits_), ptr(n_hits), R, W)
        mid = (m, C.byref(met_) if met_ is not None else None, C.byref(disk_) if disk_ is not None else None,
               C.byref(lt_) if lt_ != "null" else None, C.byref(mv) if mv != "null" else None, ptr(tex))
        if form == "frame":
            rc = lib.lt_shade_diskmovie(*head, *mid, t_obs, None, channels, ptr(rgb), ptr(rgba))
        elif form == "aa":
            rc = lib.lt_shade_diskmovie_aa(*head, S_, *mid, t_obs, None, channels, ptr(rgb), ptr(rgba))
        elif form == "curve":
            rc = lib.lt_diskmovie_lightcurve(*head, *mid, t_start, dt, n_times, ptr(out))
        elif form == "spectrum":
            rc = lib.lt_diskmovie_spectrum(*head, *mid, C.byref(spec), t_start, dt, n_times, ptr(sp_out))
        else:
            rc = lib.lt_diskmovie_visibility(*head, *mid, ptr(uv), 3, 0, t_start, dt, n_times, ptr(vis_out))
        if rc != ltrace.OK:
            assert np.all(rgb == -7.0) and np.all(rgba == 77) and np.all(out == -7.0) and np.all(sp_out == -7.0) and np.all(vis_out == -7.0)
        return rc, lib.lt_last_error().decode()

    for form in FORMS:
        assert call(form)[0] == ltrace.OK, call(form)

    def bad_map(**kw):
        m_ = good.frame(0)
        for k, x in kw.items():
            setattr(m_, k, x)
        return m_.to_lt()

    def bad_movie(**kw):
        mv = good.to_lt()[1]
        for k, x in kw.items():
            setattr(mv, k, x)
        return mv

    nan, inf = float("nan"), float("inf")
    rot7 = good.to_lt()[0]
    rot7.rotation = 7
    sizes = good.to_lt()[0]
    sizes.n_r, sizes.n_phi = 1 << 14, 1 << 13                             # 2^27 texels: the map's limit
    zero = good.to_lt()[0]
    zero.n_phi = 0
    too_many = ((1 << 28) // (37 * 64)) + 1                               # n_frames n_r n_phi just above 2^28: refused before the table is read
    assert too_many * 37 * 64 > 1 << 28 >= (too_many - 1) * 37 * 64
    # (keywords, code, a word of the message), in the header's order; every later fault is also present in `worse`
    steps = [(dict(hits_=None), ltrace.ERR_INVALID_ARG, "null"), (dict(met_=None), ltrace.ERR_INVALID_ARG, "null"),
             (dict(disk_=None), ltrace.ERR_INVALID_ARG, "null"), (dict(lt_="null"), ltrace.ERR_INVALID_ARG, "null"),
             (dict(mv="null"), ltrace.ERR_INVALID_ARG, "null"), (dict(tex=None), ltrace.ERR_INVALID_ARG, "null"),
             (dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"),
             (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), ltrace.ERR_INVALID_ARG, "bad metric"),
             (dict(R=0), ltrace.ERR_INVALID_ARG, "empty frame"), (dict(W=-3), ltrace.ERR_INVALID_ARG, "empty frame"),
             (dict(m=0), ltrace.ERR_INVALID_ARG, "max_images"), (dict(m=9), ltrace.ERR_INVALID_ARG, "max_images"),
             (dict(lt_=bad_map(r_min=0.0)), ltrace.ERR_INVALID_ARG, "r_min"), (dict(lt_=bad_map(r_max=inf)), ltrace.ERR_INVALID_ARG, "r_min"),
             (dict(lt_=bad_map(rotation="rigid", omega_p=nan)), ltrace.ERR_INVALID_ARG, "omega_p"),
             (dict(lt_=bad_map(exposure=-1.0)), ltrace.ERR_INVALID_ARG, "map exposure"),
             (dict(lt_=zero), ltrace.ERR_INVALID_ARG, "disk map of"), (dict(lt_=sizes), ltrace.ERR_INVALID_ARG, "disk map of"),
             (dict(lt_=rot7), ltrace.ERR_INVALID_ARG, "rotation"),
             (dict(mv=bad_movie(t0=nan)), ltrace.ERR_INVALID_ARG, "t0"), (dict(mv=bad_movie(t0=-inf)), ltrace.ERR_INVALID_ARG, "t0"),
             (dict(mv=bad_movie(dt_frame=0.0)), ltrace.ERR_INVALID_ARG, "dt_frame"), (dict(mv=bad_movie(dt_frame=-1.0)), ltrace.ERR_INVALID_ARG, "dt_frame"),
             (dict(mv=bad_movie(dt_frame=nan)), ltrace.ERR_INVALID_ARG, "dt_frame"), (dict(mv=bad_movie(dt_frame=inf)), ltrace.ERR_INVALID_ARG, "dt_frame"),
             (dict(mv=bad_movie(n_frames=0)), ltrace.ERR_INVALID_ARG, "n_frames"), (dict(mv=bad_movie(n_frames=-2)), ltrace.ERR_INVALID_ARG, "n_frames"),
             (dict(mv=bad_movie(n_frames=too_many)), ltrace.ERR_INVALID_ARG, "n_frames"),
             (dict(mv=bad_movie(boundary=7)), ltrace.ERR_INVALID_ARG, "boundary"),
             (dict(disk_=ltrace.default_disk(q=nan)), ltrace.ERR_INVALID_ARG, "disk q"),
             (dict(disk_=ltrace.default_disk(exposure=-1.0)), ltrace.ERR_INVALID_ARG, "disk q")]
    times = [(dict(n_times=-1), "n_times"), (dict(n_times=65536), "n_times"), (dict(t_start=nan), "t_start"), (dict(dt=inf), "t_start")]
    last = dict(frame=[(dict(channels=2), "channels"), (dict(t_obs=nan), "t_obs"), (dict(t_obs=inf), "t_obs")], curve=times, spectrum=times,
                visibility=times)
    last["aa"] = last["frame"]
    for form in FORMS:
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
        # within the movie's struct, in the struct's order
        for kw, word in ((dict(t0=nan, dt_frame=0.0, n_frames=0, boundary=7), "t0"), (dict(dt_frame=-1.0, n_frames=too_many, boundary=7), "dt_frame"),
                         (dict(n_frames=0, boundary=7), "n_frames"), (dict(n_frames=too_many, boundary=-1), "n_frames")):
            rc, msg = call(form, mv=bad_movie(**kw))
            assert rc == ltrace.ERR_INVALID_ARG and word in msg, (form, kw, rc, msg)
    # both boundaries are accepted
    assert call(mv=bad_movie(boundary=ltrace.MOVIE_LOOP))[0] == ltrace.OK
    # the aa forms look at samples right after the device, before everything else
    for S_ in (0, -1, 9):
        rc, msg = call("aa", S_=S_, met_=schw, hits_=None)
        assert rc == ltrace.ERR_INVALID_ARG and "samples" in msg
    # no times: nothing to do, nothing written; a null out with times is refused last
    for form in ("curve", "spectrum", "visibility"):
        assert call(form, n_times=0)[0] == ltrace.OK
    d_hits, d_tex = upload(hits), upload(good.texels)
    dm, mv, _ = lt(good)
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.diskmovie_lightcurve_dev(d_hits.ptr, 0, c.R, c.W, c.m, met, dk, dm, mv, d_tex.ptr, 0.0, 1.0, 2, 0)
    assert ei.value.code == ltrace.ERR_INVALID_ARG and "null out" in str(ei.value)
