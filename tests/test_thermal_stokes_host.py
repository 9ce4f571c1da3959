"""The polarized thermal continuum on the CPU: the numpy statements of the rule (disk.atmosphere_weights /
thermal_spectrum_stokes / shade_thermal_stokes / polarization_degree_angle) against a longdouble reference, the atmosphere's
tables, the struct, the bindings, the command line and render_sequence's refusals that need no device.
tests/test_gpu_thermal_stokes.py holds the kernels to the same reference with the same bounds.  The cases, records, emitters,
frequencies and the reference's machinery are tests/test_thermal_host.py's; the polarization records are synth_pol's of
tests/test_polarization_host.py with about one slot in 16 given a mu that emits nothing -- NaN, -0.1, 1.5 in turn.

The sums' bound, derived (the GPU section's).  The reference takes c of every emitting slot from disk.thermal_coeffs and the
weights (w_I, w_Q, w_U) from disk.atmosphere_weights -- steps 1 to 4, 6 and 7 are IEEE-exact operations, held to the bit on
the GPU --, x = nu c rounded to float64, and computes t = A / expm1(x), the terms w t, their sums and nu^3 in longdouble.
It is test_thermal_host's bound with t replaced by |w t|: a float64 t differs from the reference's by expm1's E ulp, the
division's half and the rounding of A (E + 2 covers them), and the kernel's S = fma(w, t, S) rounds once per addition,
which the sum's own n 2^-53 already counts -- so the fma adds nothing, and the numpy statement, which rounds the product
w t before it adds, spends the half ulp that E + 2 leaves over E + 1.5.  Q and U are signed, so it is the sum of the
absolute values that bounds every rounding; nu^3 adds three roundings of at most that sum:
    |S - S_ref| <= nu^3 ((E + 2) 2^-53 sum_{x < 700} |w t| + sum_{x >= 700} |w t| + n 2^-53 sum |w t|) + 3 2^-53 nu^3 sum |w t|.

Steps 6 and 7 on their own (test_weights_against_an_independent_restatement).  weights_ref restates them in plain
longdouble from the header's words, not from disk.atmosphere_weights: node i sits at mu_i = i / (n_mu - 1), so the interval
is floor(mu (n_mu - 1)), clamped to the table, h and d are the chords' values there, and the weights are h, h d q, h d u.
The float64 statement rounds v = mu (n_mu - 1) once, so v and with it the interpolation weight (v - i0 is exact) is off by
at most u v <= u n_mu; where that rounding carries v onto a node the statement reads the next interval at weight 0, which
is the same chord's end.  The fma rounds once and its slope l1 - l0 once:  dh = u (2 n_mu |l1 - l0| + 2 (|l0| + |l1|)) with
room, and dd likewise.  h d is a rounded product of the two, and its products with q and u one more:
    |w_I - ref| <= dh;   |w_Q - ref| <= 1.01 |q| (|d| dh + |h| dd + 2 u |h d|), and w_U likewise.
Both statements must agree on which slots' mu lets them emit: the comparisons are exact on the float32 value.

MEASURED here, the figures the tests print:
    steps 6 and 7 against the independent restatement: w_I within 0.18 of its bound, w_Q and w_U within 0.17, on strip, mid,
        big and one, with the 257-node fit and a rough 5-node table (0.11 and 0.07 there); the same slots emit;
    numpy statements against longdouble: at most 0.42 of the bound (spectra: the single pixel; 0.12 on strip, below 0.001 on
        mid and big, whose sums' n 2^-53 dominates) and 0.997 (band images: the float32 rounding is most of that bound);
    Atmosphere.chandrasekhar: 2 int h mu dmu - 1 = 0.0 by Simpson's rule on the 257 nodes (exact for the cubic h mu, up to
        rounding; tolerance 4e-16).
"""
import ctypes

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES
from test_hotspot_records_host import synth
from test_polarization_host import synth_pol
from test_thermal_host import E_EXPM1, LD, SEQUENCE, SPOT, T_MAX, U, ThermalReference, excess, frequencies, make_thermal, thermal_records

_POL, _REFERENCES = {}, {}
N_MU = 33                       # the reference cases' atmosphere: the fit on 33 nodes, so that slots fall inside every interval


# ---- cases: the polarization records, the atmosphere, the reference -------------------------------------------------------------
def stokes_pol(name, clean=False):
    """The polarization records of a case: synth_pol's -- unit (q, u), mu in [0, 1] -- and, unless `clean`, about one slot in 16
    with a mu that emits nothing -- NaN, -0.1, 1.5, in turn -- so that every pixel walk meets them.  Made once."""
    if (name, clean) not in _POL:
        c = CASES[name]
        pol = synth_pol((c.R, c.W, c.m), c.seed + 100)
        if not clean:
            pick = np.random.default_rng(c.seed + 11).random(pol.shape[:3]) < (1 / 16 if pol.size > 4 else 0)
            mu = pol[..., 3]
            mu[pick] = np.choose(np.arange(pick.sum()) % 3, [np.nan, -0.1, 1.5]).astype(np.float32)
        _POL[name, clean] = pol
    return _POL[name, clean]


def make_atmosphere():
    return diskmod.Atmosphere.chandrasekhar(N_MU)


class StokesReference(ThermalReference):
    """ThermalReference with the weights of steps 6 and 7: the longdouble sums of w t and their bound (header above)."""

    def __init__(self, hits, n_hits, pol, thermal, atmosphere):
        super().__init__(hits, n_hits, thermal)
        self.w, ok = diskmod.atmosphere_weights(pol, atmosphere)
        self.emits = self.emits & ok

    @staticmethod
    def _sum_and_bound(nu, x, wt, axis=None):
        """nu^3 sum w t and its bound, over all entries or along `axis` (entries that do not emit carry w t = 0)."""
        n3 = LD(nu) ** 3
        total, mag = wt.sum(axis=axis), np.abs(wt)
        whole = mag.sum(axis=axis)
        n = wt.size if axis is None else wt.shape[axis]
        warm = np.where(x < 700.0, mag, LD(0)).sum(axis=axis)
        bound = n3 * ((E_EXPM1 + 2) * U * warm + (whole - warm) + n * U * whole) + 3 * U * n3 * whole
        return n3 * total, bound

    def spectrum(self, nu, split):
        """-> (value, bound), each (planes, 3, n_freq) longdouble."""
        planes = self.m if split else 1
        val, bnd = np.zeros((planes, 3, len(nu)), dtype=LD), np.zeros((planes, 3, len(nu)), dtype=LD)
        for p in range(planes):
            on = self.emits[..., p] if split else self.emits
            c, w = (self.c[..., p][on], self.w[..., p, :][on]) if split else (self.c[on], self.w[on])
            w = w.astype(LD)
            for k, f in enumerate(nu):
                x, t = self._terms(f, c)
                val[p, :, k], bnd[p, :, k] = self._sum_and_bound(f, x[:, None], w * t[:, None], axis=0)
        return val, bnd

    def bands(self, nu):
        """-> (value, bound), each (n_bands, 3, R, W) longdouble; the bound without the float32 rounding."""
        val, bnd = [], []
        for f in nu:
            x, t = self._terms(f, np.where(self.emits, self.c, 1.0))
            t = np.where(self.emits, t, LD(0))
            pairs = [self._sum_and_bound(f, x, self.w[..., s].astype(LD) * t, axis=-1) for s in range(3)]
            val.append(np.stack([p[0] for p in pairs]))
            bnd.append(np.stack([p[1] for p in pairs]))
        return np.stack(val), np.stack(bnd)


def stokes_reference(name, counts=True):
    """The StokesReference of a case's records, its unsplit emitter and make_atmosphere(), made once."""
    if (name, counts) not in _REFERENCES:
        hits, n_hits = thermal_records(name)
        _REFERENCES[name, counts] = StokesReference(hits, n_hits if counts else None, stokes_pol(name), make_thermal(name), make_atmosphere())
    return _REFERENCES[name, counts]


def weights_ref(pol, atm):
    """Steps 6 and 7 restated from the header in plain longdouble, independently of disk.atmosphere_weights -> (w, ok, dw): the
    weights (..., 3), which slots' mu lets them emit, and the float64 statement's error bound on each weight (header above)."""
    p = np.asarray(pol, dtype=np.float32).astype(LD)
    q, u, mu = p[..., 0], p[..., 1], p[..., 3]
    with np.errstate(invalid="ignore"):
        ok = (mu >= 0) & (mu <= 1)
    n = atm.n_mu
    at = np.where(ok, mu, LD(0)) * LD(n - 1)
    i0 = np.clip(np.floor(at).astype(np.int64), 0, n - 2)
    frac = at - i0
    l0, l1, p0, p1 = (t.astype(LD) for t in (atm.limb[i0], atm.limb[i0 + 1], atm.poldeg[i0], atm.poldeg[i0 + 1]))
    h, d = l0 + frac * (l1 - l0), p0 + frac * (p1 - p0)
    dh = U * (2 * n * np.abs(l1 - l0) + 2 * (np.abs(l0) + np.abs(l1)))
    dd = U * (2 * n * np.abs(p1 - p0) + 2 * (np.abs(p0) + np.abs(p1)))
    dhd = LD(1.01) * (np.abs(d) * dh + np.abs(h) * dd + 2 * U * np.abs(h * d))
    w = np.stack([h, h * d * q, h * d * u], axis=-1)
    dw = np.stack([dh, np.abs(q) * dhd, np.abs(u) * dhd], axis=-1)
    return np.where(ok[..., None], w, LD(0)), ok, dw


# ---- 1. the atmosphere's tables ------------------------------------------------------------------------------------------------
def test_chandrasekhar_fit_is_normalized():
    atm = diskmod.Atmosphere.chandrasekhar()
    assert atm.n_mu == 257 and atm.limb.dtype == atm.poldeg.dtype == np.float64
    mu = atm.nodes()
    assert mu[0] == 0.0 and mu[-1] == 1.0 and atm.poldeg[-1] == 0.0 and atm.poldeg[0] == 0.1171
    assert np.all(np.diff(atm.poldeg) < 0) and np.all(np.diff(atm.limb) > 0) and atm.limb[0] > 0
    y = atm.limb * mu                                                     # a cubic: Simpson's rule on the 257 nodes is exact
    simpson = (y[0] + y[-1] + 4 * y[1:-1:2].sum() + 2 * y[2:-1:2].sum()) / (3 * 256)
    print(f"Atmosphere.chandrasekhar: 2 int h mu dmu - 1 = {2 * simpson - 1:.1e}")
    assert abs(2 * simpson - 1) <= 4e-16
    assert abs(atm.limb[-1] / atm.limb[0] - 3.0) < 1e-15                  # 1 + 2.3 - 0.3 against 1
    for n in (2, 5, 4096):
        a = diskmod.Atmosphere.chandrasekhar(n)
        assert a.n_mu == n and a.poldeg[0] == 0.1171 and a.poldeg[-1] == 0.0
    iso = diskmod.Atmosphere.isotropic()
    assert iso.n_mu == 2 and iso.limb.tolist() == [1.0, 1.0] and iso.poldeg.tolist() == [0.0, 0.0]
    assert diskmod.Atmosphere.isotropic(7).limb.tolist() == [1.0] * 7
    lt = atm.to_lt()
    assert (lt.n_mu, lt.reserved) == (257, 0)
    for bad in (dict(limb=[1.0]), dict(limb=np.ones(4097), poldeg=np.zeros(4097)), dict(poldeg=[0.0, 0.0, 0.0]), dict(limb=np.ones((2, 2)))):
        with pytest.raises(ValueError):
            diskmod.Atmosphere(**{**dict(limb=[1.0, 1.0], poldeg=[0.0, 0.0]), **bad})


def rough_atmosphere():
    """Five nodes with slopes of both signs, a negative h and degrees beyond 1: the tables are not checked."""
    return diskmod.Atmosphere([0.3, 1.7, -0.2, 0.9, 2.5], [0.5, -0.25, 1.5, 0.0, 0.125])


@pytest.mark.parametrize("name", ["strip", "mid", "big", "one"])
def test_weights_against_an_independent_restatement(name):
    pol = stokes_pol(name)
    for atm in (diskmod.Atmosphere.chandrasekhar(), rough_atmosphere()):
        w, ok = diskmod.atmosphere_weights(pol, atm)
        w_ref, ok_ref, dw = weights_ref(pol, atm)
        assert w.shape == pol.shape[:3] + (3,) and np.array_equal(ok, ok_ref) and np.all(w[~ok] == 0.0)
        d = np.abs(w.astype(LD) - w_ref)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(d == 0, LD(0), d / dw)[ok]
        print(f"{name}, {atm.n_mu} nodes: weights of {int(ok.sum())} slots against the restatement, largest difference "
              f"{float(q[:, 0].max()):.3f} (w_I) and {float(q[:, 1:].max()):.3f} (w_Q, w_U) of the bound")
        assert ok.sum() >= (1 if pol.size == 4 else 0.9 * ok.size) and np.all(q <= 1)
    # the ends and the slots that emit nothing, on a table whose nodes are told apart
    atm = rough_atmosphere()
    ends = np.zeros((1, 6, 4), dtype=np.float32)
    ends[0, :, 0], ends[0, :, 1] = 0.6, -0.8
    ends[0, :, 3] = [0.0, 1.0, np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2)), np.nan, 0.5]
    w, ok = diskmod.atmosphere_weights(ends, atm)
    assert ok.tolist() == [[True, True, False, False, False, True]]
    assert w[0, 0].tolist() == [0.3, (0.3 * 0.5) * np.float64(np.float32(0.6)), (0.3 * 0.5) * np.float64(np.float32(-0.8))]
    assert w[0, 1, 0] == 2.5 and w[0, 5, 0] == -0.2 and np.all(w[0, 2:5] == 0.0)


# ---- 2. the numpy statements against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_freq,split,counts", [("big", 5, True, True), ("mid", 16, False, True), ("strip", 64, True, False),
                                                      ("strip", 257, False, True), ("one", 1, False, True), ("one", 64, True, False)])
def test_numpy_spectrum_against_the_reference(name, n_freq, split, counts):
    hits, n_hits = thermal_records(name)
    nu = frequencies(n_freq)
    got = diskmod.thermal_spectrum_stokes(hits, n_hits if counts else None, stokes_pol(name), make_thermal(name, split), make_atmosphere(), nu)
    want, bound = stokes_reference(name, counts).spectrum(nu, split)
    assert got.shape == want.shape == (CASES[name].m if split else 1, 3, n_freq)
    q = excess(got, want, bound)
    print(f"{name} {n_freq} frequencies, split {split}: numpy statement against longdouble, largest difference {q:.3f} of its bound")
    assert q <= 1 and np.all(want[:, 0][:, np.argsort(nu)[:n_freq // 2 + 1]].sum(axis=0) > 0)
    if name != "one":
        assert np.count_nonzero(want[:, 1:]) > n_freq                     # there is polarized light to compare


@pytest.mark.parametrize("name,n_bands", [("mid", 3), ("strip", 16), ("one", 2)])
def test_numpy_bands_against_the_reference(name, n_bands):
    hits, n_hits = thermal_records(name)
    nu = frequencies(n_bands, seed=5)
    got = diskmod.shade_thermal_stokes(hits, n_hits, stokes_pol(name), make_thermal(name), make_atmosphere(), nu)
    ref = stokes_reference(name)
    want, bound = ref.bands(nu)
    assert got.shape == (n_bands, 3, CASES[name].R, CASES[name].W) and got.dtype == np.float32
    q = excess(got, want, bound + LD(2.0) ** -24 * np.abs(want) + LD(1e-45))      # (one rounding to float32; its subnormal step)
    dark = ~ref.emits.any(axis=-1)
    print(f"{name} {n_bands} bands: numpy statement against longdouble, largest difference {q:.3f} of its bound; {int(dark.sum())} dark pixels")
    assert q <= 1
    assert np.all(got[:, :, dark] == 0.0) and not np.any(np.signbit(got[:, :, dark])) and not np.any(np.isnan(got))
    with pytest.raises(ValueError, match="split_orders"):
        diskmod.shade_thermal_stokes(hits, n_hits, stokes_pol(name), make_thermal(name, True), make_atmosphere(), nu)


def test_isotropic_is_the_unpolarized_continuum():
    name = "strip"
    hits, n_hits = thermal_records(name)
    pol = stokes_pol(name, clean=True)
    nu = frequencies(9)
    for split in (False, True):
        got = diskmod.thermal_spectrum_stokes(hits, n_hits, pol, make_thermal(name, split), diskmod.Atmosphere.isotropic(), nu)
        assert np.array_equal(got[:, 0], diskmod.thermal_spectrum(hits, n_hits, make_thermal(name, split), nu))
        assert np.all(got[:, 1:] == 0.0) and not np.any(np.signbit(got))
    img = diskmod.shade_thermal_stokes(hits, n_hits, pol, make_thermal(name), diskmod.Atmosphere.isotropic(), nu[:3])
    assert np.array_equal(img[:, 0], diskmod.shade_thermal(hits, n_hits, make_thermal(name), nu[:3]))
    assert np.all(img[:, 1:] == 0.0) and not np.any(np.signbit(img))
    # a slot that the atmosphere darkens leaves the I plane too
    dim = diskmod.thermal_spectrum_stokes(hits, n_hits, stokes_pol(name), make_thermal(name), diskmod.Atmosphere.isotropic(), nu)
    warm = nu < 10 * T_MAX
    assert np.all(dim[0, 0][warm] < diskmod.thermal_spectrum(hits, n_hits, make_thermal(name), nu)[0][warm])


def test_a_fifth_slot_of_nan_changes_no_bit():
    """The records of tests/test_gpu_thermal_stokes.py's whole-and-halved case are one set of records to the numpy
    statements too: the strip's first four slots, and the same behind a fifth slot of NaN."""
    hits, n_hits = thermal_records("strip")
    a_hits, a_pol = hits[:, :, :4], stokes_pol("strip")[:, :, :4]
    pad = np.full(a_hits.shape[:2] + (1, 4), np.nan, dtype=np.float32)
    b_hits, b_pol = np.concatenate([a_hits, pad], axis=2), np.concatenate([a_pol, pad], axis=2)
    nu = frequencies(9)
    for split in (False, True):
        td = make_thermal("strip", split)
        for counts in (np.minimum(n_hits, 4).astype(np.uint8), None):
            a = diskmod.thermal_spectrum_stokes(a_hits, counts, a_pol, td, make_atmosphere(), nu)
            b = diskmod.thermal_spectrum_stokes(b_hits, counts, b_pol, td, make_atmosphere(), nu)
            assert b[:a.shape[0]].tobytes() == a.tobytes() and a.shape[0] == (4 if split else 1) and b.shape[0] == (5 if split else 1)
            assert not split or (np.all(b[4] == 0.0) and not np.any(np.signbit(b[4])))
            assert np.count_nonzero(a[:, 0]) > 0 and np.count_nonzero(a[:, 1:]) > 0


def test_slots_that_emit_nothing_are_exact_zeros():
    hits, n_hits = synth(6, 9, 3, 5, 2.4, 20.0)
    n_hits[:] = 3
    hits[..., 0] = np.random.default_rng(1).uniform(4.0, 12.0, hits.shape[:3])
    hits[..., 2] = 0.8
    pol = synth_pol(hits.shape[:3], 4)
    td = diskmod.ThermalDisk([0.5, 1.0, 0.75, 0.5, 0.4, 0.25], 4.0, 12.0, t_max=T_MAX)
    atm, nu = make_atmosphere(), frequencies(7)
    warm = nu < 10 * T_MAX
    assert np.all(diskmod.thermal_spectrum_stokes(hits, n_hits, pol, td, atm, nu)[:, 0, warm] > 0)
    for value in (np.nan, -0.1, 1.5, np.nextafter(np.float32(0), np.float32(-1)), np.nextafter(np.float32(1), np.float32(2)), -np.inf, np.inf):
        p = pol.copy()
        p[..., 3] = value
        for out in (diskmod.thermal_spectrum_stokes(hits, n_hits, p, td, atm, nu), diskmod.shade_thermal_stokes(hits, n_hits, p, td, atm, nu[:3])):
            assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out)), value
    for value in (0.0, 1.0):                                              # the ends themselves emit
        p = pol.copy()
        p[..., 3] = value
        assert np.all(diskmod.thermal_spectrum_stokes(hits, n_hits, p, td, atm, nu)[:, 0, warm] > 0)
    h = hits.copy()
    h[..., 2] = np.nan                                                    # and the thermal rule's own zeros stay zeros in all three
    out = diskmod.thermal_spectrum_stokes(h, n_hits, pol, td, atm, nu)
    assert np.all(out == 0.0) and not np.any(np.signbit(out)) and not np.any(np.isnan(out))


def test_degree_and_angle():
    iqu = np.array([[[2.0, 4.0, 0.0, 1.0], [1.0, 0.0, 0.0, -0.5], [0.0, -2.0, 0.0, 0.0]]])
    deg, ang = diskmod.polarization_degree_angle(iqu)
    assert deg.shape == ang.shape == (1, 4)
    assert deg[0, :2].tolist() == [0.5, 0.5] and np.isnan(deg[0, 2]) and deg[0, 3] == 0.5
    assert ang[0].tolist() == [0.0, -np.pi / 4, 0.0, np.pi / 2]
    bands = np.moveaxis(np.broadcast_to(iqu[0][:, :, None, None], (3, 4, 2, 5)), 0, 1)       # (n_bands, 3, R, W)
    d2, a2 = diskmod.polarization_degree_angle(bands, axis=1)
    assert d2.shape == (4, 2, 5) and np.array_equal(d2[:, 0, 0], deg[0], equal_nan=True) and np.array_equal(a2[:, 1, 4], ang[0])
    # one pixel's light: the degree is the table's and the angle the record's
    hits, n_hits = thermal_records("one")
    pol = np.array([[[[np.cos(1.2), np.sin(1.2), 0.3, 0.25]]]], dtype=np.float32)
    atm = diskmod.Atmosphere.chandrasekhar()
    sp = diskmod.thermal_spectrum_stokes(hits, n_hits, pol, make_thermal("one"), atm, frequencies(4))
    deg, ang = diskmod.polarization_degree_angle(sp)
    want = 0.1171 * 0.75 / (1 + 3.582 * 0.25)
    assert np.all(np.abs(deg - want) <= 1e-6 * want) and np.all(np.abs(ang - 0.6) <= 1e-7)


# ---- 3. the struct, exports and bindings ---------------------------------------------------------------------------------------------
def test_struct_layout_and_constants(tmp_path):
    import os
    import subprocess
    assert ctypes.sizeof(ltrace.Atmosphere) == 8 and ltrace.Atmosphere.n_mu.offset == 0 and ltrace.Atmosphere.reserved.offset == 4
    assert ltrace.ATMOSPHERE_MAX_NODES == diskmod.ATMOSPHERE_MAX_NODES == 4096
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ltrace.h")).read()
    for text in ("#define LT_ATMOSPHERE_MAX_NODES 4096", "polarized thermal continuum", "#define LT_VERSION 200"):
        assert text in header
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ltrace.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(lt_atmosphere), offsetof(lt_atmosphere, n_mu), offsetof(lt_atmosphere, reserved));\n'
                   '  return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")])
    assert [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()] == [8, 0, 4]


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    th, atm = ctypes.POINTER(ltrace.Thermal), ctypes.POINTER(ltrace.Atmosphere)
    for suffix in ("", "_dev"):
        for plain, name in (("lt_disk_thermal_spectrum", "lt_disk_thermal_spectrum_stokes"), ("lt_shade_thermal", "lt_shade_thermal_stokes")):
            assert hasattr(lib, name + suffix) and name + suffix in ltrace.SIGNATURES, name + suffix
            res, args = ltrace.SIGNATURES[plain + suffix]
            at = args.index(th)
            # the unpolarized arguments with pol behind the counts and (atmosphere, limb, poldeg) behind the flux table
            want = args[:2] + [ctypes.c_void_p] + args[2:at + 2] + [atm, ctypes.c_void_p, ctypes.c_void_p] + args[at + 2:]
            assert ltrace.SIGNATURES[name + suffix] == (res, want)
    for fn in (ltrace.thermal_spectrum_stokes, ltrace.thermal_spectrum_stokes_dev, ltrace.shade_thermal_stokes, ltrace.shade_thermal_stokes_dev):
        assert callable(fn)
    hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
    pol = synth_pol((4, 4, 2), 3)
    met, d = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk()
    td, atm_ = diskmod.ThermalDisk([0.0, 1.0, 0.5], 3.0, 9.0), diskmod.Atmosphere.chandrasekhar(9)
    tables = (td.flux, atm_.limb, atm_.poldeg)
    for fn, limit in ((ltrace.thermal_spectrum_stokes, 1025), (ltrace.shade_thermal_stokes, 17)):
        with pytest.raises(ValueError, match="pol"):           # records, tables and frequencies of the wrong size never reach the library
            fn(hits, n_hits, pol[:, :, :1], met, d, td.to_lt(), *tables, [1.0])
        with pytest.raises(ValueError, match="flux"):
            fn(hits, n_hits, pol, met, d, td.to_lt(), [0.0, 1.0], atm_.limb, atm_.poldeg, [1.0])
        with pytest.raises(ValueError, match="limb and poldeg"):
            fn(hits, n_hits, pol, met, d, td.to_lt(), td.flux, atm_.limb, atm_.poldeg[:5], [1.0])
        with pytest.raises(ValueError, match="limb and poldeg"):
            fn(hits, n_hits, pol, met, d, td.to_lt(), td.flux, [1.0], [0.0], [1.0])
        with pytest.raises(ValueError, match="frequencies"):
            fn(hits, n_hits, pol, met, d, td.to_lt(), *tables, np.ones(limit))
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        calls = (lambda: ltrace.thermal_spectrum_stokes(hits, n_hits, pol, met, d, td.to_lt(), *tables, [1.0, 2.0]),
                 lambda: ltrace.shade_thermal_stokes(hits, n_hits, pol, met, d, td.to_lt(), *tables, [1.0, 2.0]),
                 lambda: ltrace.thermal_spectrum_stokes_dev(8, 0, 8, 4, 4, 2, met, d, td.to_lt(), 8, 9, 8, 8, 8, 2, 8),
                 lambda: ltrace.shade_thermal_stokes_dev(8, 0, 8, 4, 4, 2, met, d, td.to_lt(), 8, 9, 8, 8, 8, 2, 8),
                 lambda: ltrace.thermal_spectrum_stokes_dev(8, 0, 0, 4, 4, 2, met, d, td.to_lt(), 8, 1, 0, 0, 8, 2, 8))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE       # the first refusal of all, whatever else is wrong


# ---- 4. the command line and render_sequence ---------------------------------------------------------------------------------------
THERMAL = ["--thermal", "0.5", "--thermal-bands", "1.0"]


@pytest.mark.parametrize("argv,match", [(SEQUENCE + SPOT + ["--thermal-atmosphere", "chandrasekhar"], "needs --thermal"),
                                        (SEQUENCE + ["--disk-map", "spiral"] + THERMAL + ["--thermal-atmosphere", "isotropic"], "not polarized"),
                                        (SEQUENCE + SPOT + THERMAL + ["--bfield", "1", "0", "0", "--thermal-atmosphere", "chandrasekhar"], "--bfield 0 0 1"),
                                        (SEQUENCE + THERMAL + ["--bfield", "0", "0.5", "1", "--thermal-atmosphere", "chandrasekhar"], "--bfield 0 0 1"),
                                        (SEQUENCE + THERMAL + ["--bfield", "0", "0", "0", "--thermal-atmosphere", "isotropic"], "--bfield 0 0 1")])
def test_cli_refusals(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    thin = diskmod.TransparentDisk(max_images=3)
    with pytest.raises(ValueError, match=match):
        image_lens.atmosphere_from_args(args)
    with pytest.raises(ValueError, match=match):
        image_lens.main_sequence(args, thin)


def test_cli_builds_the_atmosphere():
    import image_lens
    parse = image_lens.build_parser().parse_args
    with pytest.raises(SystemExit):
        parse(SEQUENCE + SPOT + THERMAL + ["--thermal-atmosphere", "rayleigh"])
    assert image_lens.atmosphere_from_args(parse(SEQUENCE + SPOT + THERMAL)) is None
    atm = image_lens.atmosphere_from_args(parse(SEQUENCE + SPOT + THERMAL + ["--thermal-atmosphere", "chandrasekhar"]))
    assert atm.n_mu == 257 and atm.poldeg[0] == 0.1171
    for field in (["0", "0", "1"], ["0", "0", "-2.5"]):            # the normal, either way round, is the atmosphere's own field
        atm = image_lens.atmosphere_from_args(parse(SEQUENCE + THERMAL + ["--bfield"] + field + ["--thermal-atmosphere", "isotropic"]))
        assert atm.n_mu == 2 and atm.limb.tolist() == [1.0, 1.0]


def test_render_sequence_refusals():
    import image_lens
    td = diskmod.ThermalDisk([0.0, 1.0, 0.5], 3.0, 9.0)
    atm = diskmod.Atmosphere.chandrasekhar()
    seq = lambda **kw: image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), kw.pop("hotspot", diskmod.HotSpot()),
                                                  [0.0, 10.0], shape=(8, 8), **kw)
    with pytest.raises(ValueError, match="atmosphere= belongs to thermal"):
        seq(atmosphere=atm)
    with pytest.raises(ValueError, match="thermal"):               # (thermal's own refusals of its arguments come first)
        seq(atmosphere=atm, bands=[1.0])
    with pytest.raises(ValueError, match="not polarized"):
        seq(atmosphere=atm, thermal=td, bands=[1.0], hotspot=None, diskmap=object())
    for field in (diskmod.BField(1.0, 0.0, 0.0), diskmod.BField(0.0, 0.3, 1.0), diskmod.BField(0.0, 0.0, 0.0)):
        with pytest.raises(ValueError, match=r"\(0, 0, \+-1\)"):
            seq(atmosphere=atm, thermal=td, bands=[1.0], bfield=field)
