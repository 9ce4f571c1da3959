"""The thermal continuum's kernels (lt_thermal.hpp) through lt_disk_thermal_spectrum[_dev] and lt_shade_thermal[_dev].
Cases, records, emitters, frequencies, the longdouble reference and its bound are tests/test_thermal_host.py's (its header
derives the bound): the records of test_diskmap_host -- 257 x 331 x 8, 260 x 300 x 3, 3 x 70 x 5, 1 x 1 x 1 -- with slots
that emit nothing mixed in, an emitter whose table has a dark stretch and leaves slots off both ends, frequencies that take
nu c from 1e-3 to beyond 700, and the 96 x 80 traced frame of test_gpu_diskmap.

The reference takes c from the numpy statement and rounds nu c to float64 before anything else; at nu c of several hundred a
one-ulp difference in c from a contracted operation would move a term by hundreds of ulp, so the bound of (E + 2) ulp per
term holds the kernel's steps 1 to 4 to the bit.  That c is itself held to an independent longdouble restatement of the
steps in tests/test_thermal_host.py (coefficients_ref), and the traced frame's closure takes its temperatures from that
restatement, not from c: a misreading of the rule shared by the kernel and the numpy statement fails both.

MEASURED on an MI355X (gfx950), the figures the tests print:
    spectra against longdouble, largest difference in units of its bound: strip 0.03 ... 0.15 (1 ... 1024 frequencies; the
        same with and without counts), one 0.11 ... 0.38, mid 0.001, big 0.001 (the sums' n 2^-53 dominates those bounds);
    band images: 0.998 (mid, 3 bands) and 0.999 (big, 16 bands) of the bound, nearly all of which is the one rounding to
        float32; 46 620 of 78 000 and 48 514 of 85 067 pixels dark, all exactly +0.0;
    sum of a plane against the spectrum: 2.7e-10 and 4.7e-10 relative (bounds 4.7e-3 and 5.1e-3);
    the traced frame: closure 2.2e-16 relative; the spectrum peaks at nu = 2.234, at 4.478 with twice t_max or twice f_col;
    every byte-for-byte comparison holds; the whole file runs in 1.6 s, its slowest case (big, 16 bands) in 0.4 s.
"""
import ctypes as C

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES
from test_thermal_host import (EXPOSURE, F_COL, LD, T_MAX, closure, closure_grid, excess, frequencies, make_thermal, reference,
                               thermal_records)

pytestmark = pytest.mark.gpu


def setup(name, split=False, **kw):
    c = CASES[name]
    hits, n_hits = thermal_records(name)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, c.M, c.a)
    dk = ltrace.default_disk(r_out=c.r_out)
    return c, hits, n_hits, met, dk, make_thermal(name, split, **kw)


def spectrum(hits, n_hits, met, dk, td, nu):
    return ltrace.thermal_spectrum(hits, n_hits, met, dk, td.to_lt(), td.flux, nu)


def upload(a):
    import hipmini
    a = np.ascontiguousarray(a)
    d = hipmini.DeviceArray(a.shape, a.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(a.ctypes.data), a.nbytes, 1), "hipMemcpy H2D")
    return d


# ---- 1. against the reference ---------------------------------------------------------------------------------------------------
SMALL = [(name, n, split, counts) for name in ("strip", "one") for n in (1, 64, 257, 1024) for split in (False, True) for counts in (True, False)]


@pytest.mark.parametrize("name,n_freq,split,counts", SMALL + [("mid", 16, False, True), ("mid", 16, True, False), ("big", 5, True, True)])
def test_spectrum_against_the_reference(name, n_freq, split, counts):
    c, hits, n_hits, met, dk, td = setup(name, split)
    nu = frequencies(n_freq)
    got = spectrum(hits, n_hits if counts else None, met, dk, td, nu)
    want, bound = reference(name, counts).spectrum(nu, split)
    assert got.shape == want.shape == (c.m if split else 1, n_freq) and got.dtype == np.float64
    q = excess(got, want, bound)
    print(f"{name} {n_freq} frequencies, split {split}, counts {counts}: against longdouble, largest difference {q:.3f} of its bound")
    assert not np.any(np.isnan(got)) and not np.any(np.signbit(got))
    assert q <= 1
    assert np.all(got[:, np.argsort(nu)[:n_freq // 2 + 1]].sum(axis=0) > 0)          # there is light to compare


# ---- 2. independent of the company it keeps, and reproducible -----------------------------------------------------------------------
@pytest.mark.parametrize("n_freq", [257, 1024])
def test_a_frequency_does_not_depend_on_the_others(n_freq):
    c, hits, n_hits, met, dk, td = setup("big", True)
    nu = frequencies(n_freq)
    row = spectrum(hits, n_hits, met, dk, td, nu)
    assert row.shape == (8, n_freq) and np.count_nonzero(row) > 4 * n_freq
    assert spectrum(hits, n_hits, met, dk, td, nu).tobytes() == row.tobytes()       # a second run differs in no bit
    for k in (0, 255, 256, 128):                               # (256: the second pass's first owner, alone in it at 257)
        assert spectrum(hits, n_hits, met, dk, td, nu[k:k + 1]).tobytes() == np.ascontiguousarray(row[:, k:k + 1]).tobytes(), k
    assert spectrum(hits, n_hits, met, dk, td, nu[::-1]).tobytes() == np.ascontiguousarray(row[:, ::-1]).tobytes()


# ---- 3. exact zeros -----------------------------------------------------------------------------------------------------------------
def test_records_that_emit_nothing_give_exact_zeros():
    c, hits, n_hits, met, dk, td = setup("mid", True)
    nu = frequencies(70)
    r_dark = 0.5 * (td.nodes()[10] + td.nodes()[12])                      # inside the table's zero stretch, its negative node beside it
    changes = dict(g_nan=(2, np.nan), g_zero=(2, 0.0), g_negative=(2, -0.7), r_below=(0, np.nextafter(np.float32(td.r_min), np.float32(0))),
                   r_above=(0, np.nextafter(np.float32(td.r_max), np.float32(1e9))), r_nan=(0, np.nan), dark_stretch=(0, r_dark))
    for what, (column, value) in changes.items():
        h = hits.copy()
        h[..., column] = np.float32(value)
        for counts in (n_hits, None):
            if counts is None and what == "r_nan":
                continue                                                  # (without counts a NaN r ends the slots: covered below)
            sp = spectrum(h, counts, met, dk, td, nu)
            img = ltrace.shade_thermal(h, counts, met, dk, make_thermal("mid").to_lt(), td.flux, nu[:5])
            for out in (sp, img):
                assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out)), what
    empty = np.full_like(hits, np.nan)                                    # an empty frame's worth of records
    for counts in (np.zeros_like(n_hits), None, n_hits):
        sp = spectrum(empty, counts, met, dk, td, nu)
        img = ltrace.shade_thermal(empty, counts, met, dk, make_thermal("mid").to_lt(), td.flux, nu[:5])
        for out in (sp, img):
            assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out))


# ---- 4. band images ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_bands", [("mid", 3), ("big", 16)])
def test_bands_against_the_reference(name, n_bands):
    c, hits, n_hits, met, dk, td = setup(name)
    nu = frequencies(n_bands, seed=5)
    got = ltrace.shade_thermal(hits, n_hits, met, dk, td.to_lt(), td.flux, nu)
    ref = reference(name)
    want, bound = ref.bands(nu)
    assert got.shape == (n_bands, c.R, c.W) and got.dtype == np.float32
    q = excess(got, want, bound + LD(2.0) ** -24 * want + LD(1e-45))      # (one rounding to float32; its subnormal step)
    dark = ~ref.emits.any(axis=-1)
    print(f"{name} {n_bands} bands: against longdouble, largest difference {q:.3f} of its bound; {int(dark.sum())} of {dark.size} pixels dark")
    assert q <= 1 and 0 < dark.sum() < dark.size
    assert np.all(got[:, dark] == 0.0) and not np.any(np.signbit(got)) and not np.any(np.isnan(got))
    sp = spectrum(hits, n_hits, met, dk, td, nu)[0]
    total = got.astype(np.float64).reshape(n_bands, -1).sum(axis=1)
    lit = sp > 1e-290                                                     # (a sum of float32 pixels cannot follow the spectrum below their range)
    rel = np.abs(total[lit] - sp[lit]) / sp[lit]
    visible = want.max(axis=(1, 2))[lit] > 1e-30                          # planes whose pixels are normal float32 numbers
    print(f"{name}: sum of a plane against the spectrum, largest relative difference {float(rel[visible].max()):.2e} (bound {c.R * c.W * 2.0 ** -24:.2e})")
    assert visible.sum() >= 2 and np.all(rel[visible] <= c.R * c.W * 2.0 ** -24)


# ---- 5. the _dev forms ----------------------------------------------------------------------------------------------------------------
def test_dev_forms_equal_the_host_forms():
    import hipmini
    c, hits, n_hits, met, dk, td = setup("strip", True)
    d_hits, d_nh, d_flux = upload(hits), upload(n_hits), upload(td.flux)
    for n_freq in (1, 257):
        nu = frequencies(n_freq)
        d_nu = upload(nu)
        for counts, d_counts in ((n_hits, d_nh.ptr), (None, 0)):
            d_out = hipmini.DeviceArray((c.m, n_freq), np.float64)
            ltrace.thermal_spectrum_dev(d_hits.ptr, d_counts, c.R, c.W, c.m, met, dk, td.to_lt(), d_flux.ptr, d_nu.ptr, n_freq, d_out.ptr)
            hipmini.device_synchronize()
            assert d_out.get().tobytes() == spectrum(hits, counts, met, dk, td, nu).tobytes()
    nu = frequencies(16, seed=5)
    d_nu, d_img = upload(nu), hipmini.DeviceArray((16, c.R, c.W), np.float32)
    lt = make_thermal("strip").to_lt()
    ltrace.shade_thermal_dev(d_hits.ptr, d_nh.ptr, c.R, c.W, c.m, met, dk, lt, d_flux.ptr, d_nu.ptr, 16, d_img.ptr)
    hipmini.device_synchronize()
    assert d_img.get().tobytes() == ltrace.shade_thermal(hits, n_hits, met, dk, lt, td.flux, nu).tobytes()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order():
    c, hits, n_hits, met, dk, td = setup("strip")
    lib = ltrace.load()
    ptr = ltrace._np_ptr
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    nu = frequencies(5)

    def call(form, hits_=hits, met_=met, disk_=dk, th=td.to_lt(), flux=td.flux, nu_=nu, R=c.R, W=c.W, m=c.m, n_freq=5, null_out=False):
        """-> (code, message); the output of a refused call is untouched."""
        out = np.full((8, 16, c.R * c.W), -7.0, dtype=np.float64 if form == "spectrum" else np.float32)
        ref_ = lambda x: None if x is None or isinstance(x, str) else C.byref(x)
        fn = lib.lt_disk_thermal_spectrum if form == "spectrum" else lib.lt_shade_thermal
        rc = fn(ptr(hits_), ptr(n_hits), R, W, m, ref_(met_), ref_(disk_), ref_(th), ptr(flux), ptr(nu_), n_freq, None if null_out else ptr(out))
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
    tail = {"spectrum": [(dict(n_freq=-1), INV, "n_freq"), (dict(n_freq=1025), INV, "n_freq"), (dict(null_out=True), INV, "null out")],
            "bands": [(dict(th=th(split_orders=1)), INV, "split_orders"), (dict(n_freq=-1), INV, "n_freq"), (dict(n_freq=17), INV, "n_freq"),
                      (dict(null_out=True), INV, "null out")]}
    fields = [(th(r_min=0.0, t_max=0.0), "r_min"), (th(t_max=0.0, f_col=-1.0), "t_max"), (th(f_col=-1.0, exposure=-1.0), "f_col"),
              (th(exposure=-1.0, n_r=1), "thermal exposure"), (th(n_r=1, split_orders=1), "n_r")]     # the struct's fields in the struct's order
    for form in ("spectrum", "bands"):
        assert call(form)[0] == ltrace.OK
        for bad, text in fields:
            rc, msg = call(form, th=bad)
            assert rc == INV and text in msg, (form, text, rc, msg)
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


# ---- 7. the traced frame --------------------------------------------------------------------------------------------------------------
def test_the_traced_frame_through_render_sequence():
    import image_lens
    from metrics import Kerr
    from test_gpu_diskmap import SEQ
    M, a = SEQ["M"], SEQ["a"]
    tdisk = diskmod.TransparentDisk(r_out=SEQ["r_out"], max_images=SEQ["max_images"])
    met, dk = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), tdisk.to_lt()
    td = diskmod.ThermalDisk.novikov_thorne(M, a, SEQ["r_out"], t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE, split_orders=True)
    nu = closure_grid(td, 2.0)
    bands = np.array([0.3, 1.0, 3.0]) * T_MAX
    out = image_lens.render_sequence(None, Kerr(M=M, a=a, integrator="rk4", precision=32), SEQ["r_obs"], SEQ["fov"], tdisk, diskmod.HotSpot(),
                                     [0.0], shape=SEQ["shape"], theta_obs=SEQ["theta_obs"], thermal=td, frequencies=nu, bands=bands)
    hits, n_hits = out["hits"], out["n_hits"]
    assert float(np.nanmax(hits[..., 2])) < 2.0 and int((n_hits > 0).sum()) > 1000
    direct = ltrace.thermal_spectrum(hits, n_hits, met, dk, td.to_lt(), td.flux, nu)
    assert out["thermal_spectrum"].shape == (SEQ["max_images"], nu.size) and out["thermal_spectrum"].tobytes() == direct.tobytes()
    assert np.array_equal(out["thermal_frequencies"], nu)
    flat = diskmod.ThermalDisk(td.flux, td.r_min, td.r_max, t_max=T_MAX, f_col=F_COL, exposure=EXPOSURE)
    assert out["thermal_bands"].tobytes() == ltrace.shade_thermal(hits, n_hits, met, dk, flat.to_lt(), td.flux, bands).tobytes()
    got, want = closure(direct.sum(axis=0), nu, hits, n_hits, td)
    print(f"traced frame: Stefan-Boltzmann closure {got:.10e} against {want:.10e}, relative {abs(got / want - 1):.1e}")
    assert want > 0 and abs(got / want - 1) <= 1e-9
    peak = lambda t: float(nu[np.argmax(ltrace.thermal_spectrum(hits, n_hits, met, dk, t.to_lt(), t.flux, nu)[0])])
    base = peak(flat)
    hotter = peak(diskmod.ThermalDisk(td.flux, td.r_min, td.r_max, t_max=2 * T_MAX, f_col=F_COL, exposure=EXPOSURE))
    harder = peak(diskmod.ThermalDisk(td.flux, td.r_min, td.r_max, t_max=T_MAX, f_col=2 * F_COL, exposure=EXPOSURE))
    print(f"traced frame: the spectrum peaks at nu = {base:.3f}; twice t_max {hotter:.3f}; twice f_col {harder:.3f}")
    assert hotter > 1.5 * base and harder > 1.5 * base
