"""The polarized thermal continuum's kernels (lt_thermal_stokes.hpp) through lt_disk_thermal_spectrum_stokes[_dev] and
lt_shade_thermal_stokes[_dev].  Cases, records, emitters and frequencies are tests/test_thermal_host.py's, the polarization
records, the atmosphere, the longdouble reference and its bound tests/test_thermal_stokes_host.py's (its header derives the
bound): the records of test_diskmap_host -- 257 x 331 x 8 (its lists are walked in two halves), 260 x 300 x 3, 3 x 70 x 5,
1 x 1 x 1 -- with slots that the thermal rule darkens and slots whose mu is NaN, -0.1 or 1.5 mixed in.

The reference takes c and the weights from the numpy statements and rounds nu c to float64 before anything else, so the
bound of (E + 2) ulp per term holds the kernel's steps 1 to 4, 6 and 7 to the bit (a one-ulp difference in a weight moves
a term by one ulp, and in c by hundreds).  Both numpy statements are themselves held to independent longdouble
restatements on the CPU (coefficients_ref, weights_ref).

The weak-field limit (test 6) is the one claim that rests on no arithmetic: that the records of the field (0, 0, 1) are the
scattering atmosphere's.  A 48 x 48 frame, DP45 float64, of a disk from r = 200 M to 400 M seen from r = 2000 M at 60
degrees.  In flat space every direct hit would have q = 1, u = 0 (the electric vector along the disk's projected major axis,
which is e_1) and mu = cos 60 deg, and the spectrum's degree would be delta(1/2) at angle 0.  The departures are first
order in v = sqrt(M / r_in) = 0.07 (aberration) and 4 M / r (bending).  MEASURED on an MI355X, over the 651 first-order hits:
    max |q - 1| = 0.0272, max |u| = 0.2315, max |mu - 1/2| = 0.1004 (means: q 0.9909, u -0.0126, mu 0.5165); q is positive:
    the convention holds;  the degree at nu = 0.1 ... 8 t_max lies 5.85 ... 6.05 % below delta(1/2) = 0.02098 (the spread of
    the angles and of mu depolarizes), the angle between -0.0041 and +0.0117 rad;
and asserted with a margin of twice the measured value where that is no looser than the caps |q - 1| < 0.1, |u| < 0.35,
|mu - 1/2| < 0.15 and the degree within 15 % of delta(1/2), and with the cap elsewhere: 0.055, 0.35 (twice would be 0.46),
0.15 (0.20), 12.2 % and 0.024 rad.

MEASURED on an MI355X (gfx950), the figures the tests print:
    spectra against longdouble, largest difference in units of its bound, (I, Q, U): strip 0.006 ... 0.168, 0.005 ... 0.148,
        0.003 ... 0.099 (1 ... 1024 frequencies; the same with and without counts), one 0.054 ... 0.484, 0.100 ... 0.377,
        0.140 ... 0.458, mid and big 0.001 at the most (the sums' n 2^-53 dominates those bounds);
    band images: 0.997 (mid, 3 bands) and 0.999 (big, 16 bands) of the bound, nearly all of which is the one rounding to
        float32; 47 420 of 78 000 and 48 822 of 85 067 pixels dark, all exactly +0.0;
    one degree, aligned vectors: sqrt(Q^2 + U^2) / (0.1 I) - 1 within [-1.9e-15, 1.8e-15] on big (n 2^-52 >= 2.2e-12) and
        [-1.0e-15, 6.7e-16] on strip (n 2^-52 >= 6.0e-15);
    the traced frame: degree 0.03493 at -0.34 deg at nu = 7.5e-06 and 0.03102 at -8.89 deg at nu = 255; per image order at
        nu = 0.0447: 0.03686, 0.02045, 0.00138;
    every byte-for-byte comparison holds; the whole file runs in 2.7 s, its slowest case (big, 16 bands) in 1.0 s.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES
from test_gpu_thermal import setup, upload
from test_thermal_host import EXPOSURE, F_COL, LD, T_MAX, closure_grid, excess, frequencies, make_thermal
from test_thermal_stokes_host import make_atmosphere, stokes_pol, stokes_reference

pytestmark = pytest.mark.gpu

# test 6's margins: twice what was measured (header above) where that is within the check's own caps, the caps elsewhere
WEAK_Q, WEAK_U, WEAK_MU, WEAK_DEGREE, WEAK_ANGLE = 0.055, 0.35, 0.15, 0.122, 0.024
assert WEAK_Q <= 0.1 and WEAK_U <= 0.35 and WEAK_MU <= 0.15 and WEAK_DEGREE <= 0.15


def spectrum(hits, n_hits, pol, met, dk, td, atm, nu):
    return ltrace.thermal_spectrum_stokes(hits, n_hits, pol, met, dk, td.to_lt(), td.flux, atm.limb, atm.poldeg, nu)


def bands(hits, n_hits, pol, met, dk, td, atm, nu):
    return ltrace.shade_thermal_stokes(hits, n_hits, pol, met, dk, td.to_lt(), td.flux, atm.limb, atm.poldeg, nu)


def clean(out):
    return not np.any(np.isnan(out)) and not np.any(np.signbit(out) & (out == 0))


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
SMALL = [(name, n, split, counts) for name in ("strip", "one") for n in (1, 257, 1024) for split in (False, True) for counts in (True, False)]


@pytest.mark.parametrize("name,n_freq,split,counts", SMALL + [("mid", 16, False, True), ("mid", 16, True, False), ("big", 5, True, True),
                                                              ("big", 5, False, True)])
def test_spectrum_against_the_reference(name, n_freq, split, counts):
    c, hits, n_hits, met, dk, td = setup(name, split)
    nu = frequencies(n_freq)
    got = spectrum(hits, n_hits if counts else None, stokes_pol(name), met, dk, td, make_atmosphere(), nu)
    want, bound = stokes_reference(name, counts).spectrum(nu, split)
    assert got.shape == want.shape == (c.m if split else 1, 3, n_freq) and got.dtype == np.float64
    q = [excess(got[:, s], want[:, s], bound[:, s]) for s in range(3)]
    print(f"{name} {n_freq} frequencies, split {split}, counts {counts}: against longdouble, largest difference {q[0]:.3f} (I), {q[1]:.3f} (Q), "
          f"{q[2]:.3f} (U) of its bound")
    assert clean(got) and not np.any(np.signbit(got[:, 0]))
    assert max(q) <= 1
    assert np.all(got[:, 0][:, np.argsort(nu)[:n_freq // 2 + 1]].sum(axis=0) > 0)    # there is light to compare
    if name != "one":
        assert np.count_nonzero(got[:, 1:]) > n_freq


@pytest.mark.parametrize("name,n_bands", [("mid", 3), ("big", 16)])
def test_bands_against_the_reference(name, n_bands):
    c, hits, n_hits, met, dk, td = setup(name)
    nu = frequencies(n_bands, seed=5)
    got = bands(hits, n_hits, stokes_pol(name), met, dk, td, make_atmosphere(), nu)
    ref = stokes_reference(name)
    want, bound = ref.bands(nu)
    assert got.shape == (n_bands, 3, c.R, c.W) and got.dtype == np.float32
    q = excess(got, want, bound + LD(2.0) ** -24 * np.abs(want) + LD(1e-45))          # (one rounding to float32; its subnormal step)
    dark = ~ref.emits.any(axis=-1)
    print(f"{name} {n_bands} bands: against longdouble, largest difference {q:.3f} of its bound; {int(dark.sum())} of {dark.size} pixels dark")
    assert q <= 1 and 0 < dark.sum() < dark.size
    assert np.all(got[:, :, dark] == 0.0) and not np.any(np.signbit(got[:, :, dark])) and not np.any(np.isnan(got))
    assert np.count_nonzero(got[:, 1:]) > dark.size // 4


# ---- 2. bit identities -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,split", [("big", True), ("strip", False), ("strip", True)])
def test_isotropic_has_the_unpolarized_bits(name, split):
    c, hits, n_hits, met, dk, td = setup(name, split)
    pol = stokes_pol(name, clean=True)                                    # (every mu in [0, 1]: no slot is darkened)
    nu = frequencies(257)
    iso = diskmod.Atmosphere.isotropic()
    got = spectrum(hits, n_hits, pol, met, dk, td, iso, nu)
    plain = ltrace.thermal_spectrum(hits, n_hits, met, dk, td.to_lt(), td.flux, nu)
    assert np.ascontiguousarray(got[:, 0]).tobytes() == plain.tobytes() and np.count_nonzero(plain) > 100
    assert np.all(got[:, 1:] == 0.0) and not np.any(np.signbit(got))      # poldeg = 0: exactly +0.0
    flat = make_thermal(name)
    nb = frequencies(16, seed=5)
    img = bands(hits, n_hits, pol, met, dk, flat, iso, nb)
    assert np.ascontiguousarray(img[:, 0]).tobytes() == ltrace.shade_thermal(hits, n_hits, met, dk, flat.to_lt(), flat.flux, nb).tobytes()
    assert np.all(img[:, 1:] == 0.0) and not np.any(np.signbit(img))
    # poldeg = 0 under a limb-darkening law that is not flat: Q and U are still exactly +0.0, whatever the sign of q and u
    dark = diskmod.Atmosphere(make_atmosphere().limb, np.zeros(make_atmosphere().n_mu))
    for out in (spectrum(hits, n_hits, stokes_pol(name), met, dk, td, dark, nu)[:, 1:], bands(hits, n_hits, stokes_pol(name), met, dk, flat, dark, nb)[:, 1:]):
        assert np.all(out == 0.0) and not np.any(np.signbit(out))


@pytest.mark.parametrize("name", ["big", "strip"])
def test_a_frequency_does_not_depend_on_the_others(name):
    c, hits, n_hits, met, dk, td = setup(name, True)
    pol, atm = stokes_pol(name), make_atmosphere()
    nu = frequencies(257)
    row = spectrum(hits, n_hits, pol, met, dk, td, atm, nu)
    assert row.shape == (c.m, 3, 257) and np.count_nonzero(row) > 3 * 257
    assert spectrum(hits, n_hits, pol, met, dk, td, atm, nu).tobytes() == row.tobytes()      # a second run differs in no bit
    for k in (0, 128, 255, 256):                               # (256: the second pass's first owner, alone in it at 257)
        assert spectrum(hits, n_hits, pol, met, dk, td, atm, nu[k:k + 1]).tobytes() == np.ascontiguousarray(row[:, :, k:k + 1]).tobytes(), k
    assert spectrum(hits, n_hits, pol, met, dk, td, atm, nu[::-1]).tobytes() == np.ascontiguousarray(row[:, :, ::-1]).tobytes()
    img = bands(hits, n_hits, pol, met, dk, make_thermal(name), atm, nu[:5])
    assert bands(hits, n_hits, pol, met, dk, make_thermal(name), atm, nu[:5]).tobytes() == img.tobytes()


def test_dev_forms_equal_the_host_forms():
    import hipmini
    c, hits, n_hits, met, dk, td = setup("strip", True)
    pol, atm = stokes_pol("strip"), make_atmosphere()
    d_hits, d_nh, d_pol, d_flux, d_limb, d_deg = (upload(a) for a in (hits, n_hits, pol, td.flux, atm.limb, atm.poldeg))
    for n_freq in (1, 257):
        nu = frequencies(n_freq)
        d_nu = upload(nu)
        for counts, d_counts in ((n_hits, d_nh.ptr), (None, 0)):
            d_out = hipmini.DeviceArray((c.m, 3, n_freq), np.float64)
            ltrace.thermal_spectrum_stokes_dev(d_hits.ptr, d_counts, d_pol.ptr, c.R, c.W, c.m, met, dk, td.to_lt(), d_flux.ptr, atm.n_mu,
                                               d_limb.ptr, d_deg.ptr, d_nu.ptr, n_freq, d_out.ptr)
            hipmini.device_synchronize()
            assert d_out.get().tobytes() == spectrum(hits, counts, pol, met, dk, td, atm, nu).tobytes()
    nu = frequencies(16, seed=5)
    d_nu, d_img = upload(nu), hipmini.DeviceArray((16, 3, c.R, c.W), np.float32)
    flat = make_thermal("strip")
    ltrace.shade_thermal_stokes_dev(d_hits.ptr, d_nh.ptr, d_pol.ptr, c.R, c.W, c.m, met, dk, flat.to_lt(), d_flux.ptr, atm.n_mu, d_limb.ptr,
                                    d_deg.ptr, d_nu.ptr, 16, d_img.ptr)
    hipmini.device_synchronize()
    assert d_img.get().tobytes() == bands(hits, n_hits, pol, met, dk, flat, atm, nu).tobytes()


def test_whole_and_halved_walks_give_the_same_bits():
    """Four images are the most whose lists the polarized first stage holds in LDS at once, five the fewest it walks in
    halves, and no case has four.  A: the strip's first four slots.  B: A behind a fifth slot of NaN, which stores and emits
    nothing.  The two are the same records, so the spectra must agree in every bit -- 257 frequencies: two passes, the second
    with one owner -- and B's fifth plane is exactly +0.0.  The unpolarized spectrum, one path for both, says the same."""
    c, hits, n_hits, met, dk, _ = setup("strip")
    a_hits, a_pol = np.ascontiguousarray(hits[:, :, :4]), np.ascontiguousarray(stokes_pol("strip")[:, :, :4])
    pad = np.full((c.R, c.W, 1, 4), np.nan, dtype=np.float32)
    b_hits, b_pol = np.concatenate([a_hits, pad], axis=2), np.concatenate([a_pol, pad], axis=2)
    assert a_hits.shape[2] == 4 and b_hits.shape[2] == 5
    atm, nu = make_atmosphere(), frequencies(257)
    for split in (False, True):
        td = make_thermal("strip", split)
        for counts in (np.minimum(n_hits, 4).astype(np.uint8), None):
            stokes = [spectrum(h, counts, p, met, dk, td, atm, nu) for h, p in ((a_hits, a_pol), (b_hits, b_pol))]
            plain = [ltrace.thermal_spectrum(h, counts, met, dk, td.to_lt(), td.flux, nu) for h in (a_hits, b_hits)]
            for a, b in (stokes, plain):
                assert a.shape[0] == (4 if split else 1) and b.shape[0] == (5 if split else 1)
                assert b[:a.shape[0]].tobytes() == a.tobytes(), (split, counts is None, a.ndim)
                assert not split or (np.all(b[4] == 0.0) and not np.any(np.signbit(b[4])))
            assert np.count_nonzero(stokes[0][:, 0]) > 0 and np.count_nonzero(stokes[0][:, 1:]) > 0 and np.count_nonzero(plain[0]) > 0


# ---- 3. exact zeros -----------------------------------------------------------------------------------------------------------------
def test_records_that_emit_nothing_give_exact_zeros():
    c, hits, n_hits, met, dk, td = setup("mid", True)
    pol, atm = stokes_pol("mid", clean=True), make_atmosphere()
    flat = make_thermal("mid")
    nu = frequencies(70)
    r_dark = 0.5 * (td.nodes()[10] + td.nodes()[12])                      # inside the table's zero stretch, its negative node beside it
    f32 = np.float32
    changes = dict(g_nan=("hits", 2, np.nan), g_zero=("hits", 2, 0.0), g_negative=("hits", 2, -0.7),
                   r_below=("hits", 0, np.nextafter(f32(td.r_min), f32(0))), r_above=("hits", 0, np.nextafter(f32(td.r_max), f32(1e9))),
                   r_nan=("hits", 0, np.nan), dark_stretch=("hits", 0, r_dark),
                   mu_nan=("pol", 3, np.nan), mu_negative=("pol", 3, -0.1), mu_above=("pol", 3, 1.5),
                   mu_just_below=("pol", 3, np.nextafter(f32(0), f32(-1))), mu_just_above=("pol", 3, np.nextafter(f32(1), f32(2))),
                   mu_infinite=("pol", 3, -np.inf))

    def all_zero(h, p, counts, what):
        for out in (spectrum(h, counts, p, met, dk, td, atm, nu), bands(h, counts, p, met, dk, flat, atm, nu[:5])):
            assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out)), what

    for what, (which, column, value) in changes.items():
        h, p = hits.copy(), pol.copy()
        (h if which == "hits" else p)[..., column] = f32(value)
        for counts in (n_hits, None):
            if counts is None and what == "r_nan":
                continue                                                  # (without counts a NaN r ends the slots: covered below)
            all_zero(h, p, counts, what)
    empty = np.full_like(hits, np.nan)                                    # an empty frame's worth of records
    for counts in (np.zeros_like(n_hits), None, n_hits):
        all_zero(empty, np.full_like(pol, np.nan), counts, "empty")
    assert np.all(spectrum(hits, n_hits, pol, met, dk, td, atm, nu)[:, 0, nu < 10 * T_MAX] > 0)       # (and the unchanged records shine)


# ---- 4. an inequality that needs no reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big", "mid", "strip", "one"])
def test_polarized_flux_is_bounded_by_the_largest_degree(name):
    c, hits, n_hits, met, dk, td = setup(name, True)
    nu = frequencies(64)
    n = np.array([int(stokes_reference(name).emits[..., j].sum()) for j in range(c.m)], dtype=np.float64)[:, None]
    atm = make_atmosphere()
    got = spectrum(hits, n_hits, stokes_pol(name), met, dk, td, atm, nu)
    i, p = got[:, 0], np.hypot(got[:, 1], got[:, 2])
    assert np.all(p <= np.abs(atm.poldeg).max() * i * (1 + n * 2.0 ** -52))
    if name in ("big", "strip"):
        # the bound met: one degree at every mu and every electric vector along e_1, so that sqrt(Q^2 + U^2) = 0.1 I but for rounding
        level = diskmod.Atmosphere(atm.limb, np.full(atm.n_mu, 0.1))
        pol = stokes_pol(name).copy()
        pol[..., 0], pol[..., 1] = 1.0, 0.0
        got = spectrum(hits, n_hits, pol, met, dk, td, level, nu)
        i, p = got[:, 0], np.hypot(got[:, 1], got[:, 2])
        lit = i > 0
        print(f"{name}: sqrt(Q^2 + U^2) / (0.1 I) - 1 within [{float((p[lit] / (0.1 * i[lit]) - 1).min()):.1e}, {float((p[lit] / (0.1 * i[lit]) - 1).max()):.1e}]; "
              f"n 2^-52 is {float(n.min() * 2.0 ** -52):.1e} at the least")
        assert lit.sum() > 16 * c.m and np.all(p <= 0.1 * i * (1 + n * 2.0 ** -52))
        assert np.all(p >= 0.1 * i * (1 - (n + 1) * 2.0 ** -52)) and np.all(got[:, 2] == 0.0)      # (and from below: it is an equality)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, met, dk, td = setup("strip")
    pol, atm = stokes_pol("strip"), make_atmosphere()
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    nu = frequencies(5)

    def call(form, hits_=hits, pol_=pol, met_=met, disk_=dk, th=td.to_lt(), flux=td.flux, at=atm.to_lt(), limb=atm.limb, deg=atm.poldeg, nu_=nu,
             R=c.R, W=c.W, m=c.m, n_freq=5, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full((8, 48, c.R * c.W), -7.0, dtype=np.float64 if form == "spectrum" else np.float32)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        fn = lib.lt_disk_thermal_spectrum_stokes if form == "spectrum" else lib.lt_shade_thermal_stokes
        rc = fn(ptr(hits_), ptr(n_hits), ptr(pol_), R, W, m, ref_(met_), ref_(disk_), ref_(th), ptr(flux), ref_(at), ptr(limb), ptr(deg), ptr(nu_),
                n_freq, None if null_out else ptr(out))
        if rc != ltrace.OK or n_freq == 0:
            assert np.all(out == -7.0)
        return rc, lib.lt_last_error().decode()

    nan, inf = float("nan"), float("inf")
    INV = ltrace.ERR_INVALID_ARG
    th = lambda **kw: ltrace.default_thermal(**{**dict(r_min=td.r_min, r_max=td.r_max, t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE, n_r=td.n_r), **kw})
    steps = [(dict(hits_=None), INV, "null"), (dict(met_=None), INV, "null"), (dict(disk_=None), INV, "null"),
             (dict(met_=schw), ltrace.ERR_UNSUPPORTED, "LT_METRIC_KERR"), (dict(met_=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), INV, "bad metric"),
             (dict(R=0), INV, "empty frame"), (dict(W=-3), INV, "empty frame"), (dict(m=0), INV, "max_images"), (dict(m=9), INV, "max_images"),
             (dict(disk_=ltrace.default_disk(q=nan)), INV, "disk q"), (dict(disk_=ltrace.default_disk(exposure=-1.0)), INV, "disk q"),
             (dict(th="null"), INV, "null thermal"), (dict(flux=None), INV, "null thermal"), (dict(nu_=None), INV, "null thermal"),
             (dict(th=th(r_min=0.0)), INV, "r_min"), (dict(th=th(r_min=nan)), INV, "r_min"), (dict(th=th(r_max=td.r_min)), INV, "r_min"),
             (dict(th=th(r_max=inf)), INV, "r_min"), (dict(th=th(t_max=0.0)), INV, "t_max"), (dict(th=th(t_max=inf)), INV, "t_max"),
             (dict(th=th(f_col=-1.0)), INV, "f_col"), (dict(th=th(f_col=nan)), INV, "f_col"), (dict(th=th(exposure=-1.0)), INV, "thermal exposure"),
             (dict(th=th(exposure=inf)), INV, "thermal exposure"), (dict(th=th(n_r=1)), INV, "n_r"), (dict(th=th(n_r=65537)), INV, "n_r")]
    atmos = [(dict(pol_=None), INV, "null pol"), (dict(at="null"), INV, "null pol"), (dict(limb=None), INV, "null pol"), (dict(deg=None), INV, "null pol"),
             (dict(at=ltrace.Atmosphere(1, 0)), INV, "n_mu"), (dict(at=ltrace.Atmosphere(4097, 0)), INV, "n_mu"), (dict(at=ltrace.Atmosphere(-5, 0)), INV, "n_mu")]
    tail = {"spectrum": atmos + [(dict(n_freq=-1), INV, "n_freq"), (dict(n_freq=1025), INV, "n_freq"), (dict(null_out=True), INV, "null out")],
            "bands": [(dict(th=th(split_orders=1)), INV, "split_orders")] + atmos
                     + [(dict(n_freq=-1), INV, "n_freq"), (dict(n_freq=17), INV, "n_freq"), (dict(null_out=True), INV, "null out")]}
    for form in ("spectrum", "bands"):
        assert call(form)[0] == ltrace.OK
        assert call(form, at=ltrace.Atmosphere(atm.n_mu, 12345))[0] == ltrace.OK                                  # `reserved` is not looked at
        assert call(form, n_freq=0)[0] == ltrace.OK and call(form, n_freq=0, null_out=True)[0] == ltrace.OK      # no frequency: no work
        if form == "spectrum":
            assert call(form, th=th(split_orders=1))[0] == ltrace.OK
        order = steps + tail[form]
        for i, (kw, code, text) in enumerate(order):
            rc, msg = call(form, **kw)
            assert rc == code and text in msg, (form, kw, rc, msg)
            for later, _, _ in order[i + 1:]:                             # an earlier fault wins over every later one
                if set(later) & set(kw):
                    continue
                rc2, msg2 = call(form, **{**later, **kw})
                assert rc2 == code and text in msg2, (form, kw, later, rc2, msg2)


# ---- 6. the weak-field limit ----------------------------------------------------------------------------------------------------------
def test_the_weak_field_limit_is_the_flat_atmosphere():
    M, a, n = 1.0, 0.5, 48
    r_in, r_out, r_obs, theta = 200.0, 400.0, 2000.0, np.radians(60.0)
    fov = 2 * np.arctan(1.05 * r_out / r_obs)                             # the disk's major axis and a twentieth more
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    dk = ltrace.default_disk(r_in=r_in, r_out=r_out)
    opts = ltrace.default_opts(integrator="dp45", precision=64, tb_symmetry=0)
    cam = ltrace.Camera(n, n, fov, fov, 0.0, 0.0, r_obs, theta)
    tr = ltrace.trace_disk_pol(cam, met, opts, dk, ltrace.default_bfield(b_r=0.0, b_phi=0.0, b_z=1.0), max_images=2, want=("hits", "n_hits", "pol"))
    hits, n_hits, pol = tr["hits"], tr["n_hits"], tr["pol"]
    first = n_hits > 0
    q, u, mu = (pol[..., 0, k][first].astype(np.float64) for k in (0, 1, 3))
    r = hits[..., 0, 0][first]
    assert first.sum() > 0.2 * n * n and r.min() >= r_in * (1 - 1e-6) and r.max() <= r_out * (1 + 1e-6)
    assert np.all(np.abs(np.hypot(q, u) - 1) < 1e-5)
    dq, du, dmu = np.abs(q - 1).max(), np.abs(u).max(), np.abs(mu - np.cos(theta)).max()
    print(f"weak field, {int(first.sum())} first-order hits: max |q - 1| = {dq:.4f}, max |u| = {du:.4f}, max |mu - cos theta_obs| = {dmu:.4f}; "
          f"mean q {q.mean():.4f}, mean u {u.mean():+.4f}, mean mu {mu.mean():.4f}")
    assert dq < WEAK_Q and du < WEAK_U and dmu < WEAK_MU
    nodes = r_in + np.arange(65) * (r_out - r_in) / 64
    td = diskmod.ThermalDisk((r_in / nodes) ** 3, r_in, r_out, t_max=1.0)
    atm = diskmod.Atmosphere.chandrasekhar()
    nu = np.array([0.1, 0.5, 1.0, 2.0, 4.0, 8.0])
    deg, ang = diskmod.polarization_degree_angle(spectrum(hits, n_hits, pol, met, dk, td, atm, nu))
    want = 0.1171 * 0.5 / (1 + 3.582 * 0.5)
    print(f"weak field: degree / delta(cos theta_obs) - 1 = {np.array2string(deg[0] / want - 1, precision=4)}, angle = {np.array2string(ang[0], precision=4)} rad")
    assert np.all(np.abs(deg[0] / want - 1) < WEAK_DEGREE) and np.all(np.abs(ang[0]) < WEAK_ANGLE)


# ---- 7. the traced frame --------------------------------------------------------------------------------------------------------------
def test_the_traced_frame_through_render_sequence():
    import image_lens
    from metrics import Kerr
    from test_gpu_diskmap import SEQ
    M, a = SEQ["M"], SEQ["a"]
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
    td = diskmod.ThermalDisk.novikov_thorne(M, a, SEQ["r_out"], t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE, split_orders=True)
    flat = diskmod.ThermalDisk(td.flux, td.r_min, td.r_max, t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE)
    atm = diskmod.Atmosphere.chandrasekhar()
    nu = closure_grid(td, 2.0)
    nb = np.array([0.3, 1.0, 3.0]) * T_MAX
    seq = lambda **kw: image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk,
                                                  diskmod.HotSpot(), [0.0], shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], thermal=td,
                                                  frequencies=nu, bands=nb, **kw)
    out, plain = seq(atmosphere=atm), seq()
    hits, n_hits, pol = out["hits"], out["n_hits"], out["pol"]
    assert "pol" not in plain and "thermal_spectrum_stokes" not in plain and "stokes" not in out
    for key in ("hits", "n_hits", "thermal_spectrum", "thermal_bands", "frames", "lightcurve"):     # what there was stays what it was
        assert np.asarray(out[key]).tobytes() == np.asarray(plain[key]).tobytes(), key
    assert pol.shape == hits.shape and int((n_hits > 0).sum()) > 1000
    direct = spectrum(hits, n_hits, pol, met, dk, td, atm, nu)
    assert out["thermal_spectrum_stokes"].shape == (SEQ["max_images"], 3, nu.size) and out["thermal_spectrum_stokes"].tobytes() == direct.tobytes()
    assert out["thermal_bands_stokes"].shape == (3, 3) + tuple(SEQ["shape"]) and out["thermal_bands_stokes"].tobytes() == bands(hits, n_hits, pol, met, dk, flat, atm, nb).tobytes()
    with_field = seq(atmosphere=atm, bfield=diskmod.BField(0.0, 0.0, -1.0))         # the normal the other way round: the same records
    assert with_field["pol"].tobytes() == pol.tobytes() and with_field["thermal_spectrum_stokes"].tobytes() == direct.tobytes() and "stokes" in with_field
    S = 2
    fine = seq(atmosphere=atm, samples=S)                                         # with samples: divided and resolved as the thermal entries are
    d_fine = spectrum(fine["hits"], fine["n_hits"], fine["pol"], met, dk, td, atm, nu)
    assert fine["thermal_spectrum_stokes"].tobytes() == (d_fine / np.float64(S * S)).tobytes()
    import aa
    b_fine = bands(fine["hits"], fine["n_hits"], fine["pol"], met, dk, flat, atm, nb)
    assert fine["thermal_bands_stokes"].shape == (3, 3) + tuple(SEQ["shape"])
    assert fine["thermal_bands_stokes"].tobytes() == np.stack([np.stack([aa.resolve(p, S) for p in band]) for band in b_fine]).tobytes()
    deg, ang = diskmod.polarization_degree_angle(direct.sum(axis=0))
    lit = direct[:, 0].sum(axis=0) > 0
    lo, hi = int(np.argmax(lit)), int(nu.size - 1 - np.argmax(lit[::-1]))
    print(f"traced frame: degree {deg[lo]:.5f} at angle {np.degrees(ang[lo]):+.2f} deg at nu = {nu[lo]:.3g}; degree {deg[hi]:.5f} at angle "
          f"{np.degrees(ang[hi]):+.2f} deg at nu = {nu[hi]:.3g}; per order at nu = {nu[nu.size // 2]:.3g}: "
          f"{np.array2string(diskmod.polarization_degree_angle(direct)[0][:, nu.size // 2], precision=5)}")
    assert np.all(deg[lit] <= 0.1171 * (1 + 1e-9))
