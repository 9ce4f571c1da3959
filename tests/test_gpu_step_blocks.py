"""The arithmetic the float32 fast path is made of, each block against float64: the math primitives over EVERY float32 of
their domain, the right-hand side and one RK4 step in every form on classes of states, in the unit of tests/step_blocks.py
with the bounds tests/test_step_blocks_host.py derives from the reference's own float32 arithmetic (K_REF = 13 u S for the
right-hand side, K_STEP = 4 units for a step; the device forms are held to twice that).  The float64 functions that serve as
yardsticks on the device are held to mpmath first.

Whole rays in float32 stay under statistical budgets (test_gpu_parity.py): rays near the critical curve amplify any rounding
without bound.  One step does not, so this is where the float32 arithmetic is pinned.

MEASURED on the MI355X (build 6e7d2b488dbd; profiles/step_blocks_6e7d2b488dbd.json, LT_STEP_BLOCKS_MEASURE=path writes it):
    M<float>::sincos, 2 352 513 026 values |x| <= 1e4: 1.560 u (sin), 1.559 u (cos) absolute, bound 2 u; |x| <= 13: 5.79 ulp
        of the result at 3 pi / 2 and 3 pi (recorded, not bounded);
    M<float>::rcp_pos, 1 677 721 601 values: 0.775 ulp, bound 1;
    M<float>::sincos_small, 2 097 152 002 values: cos 0.534 u, bound 1 u; sin 1.318 ulp, bound 2;
    sincos_shift / sincos_shift_pk, 14 680 064 014 (base, d): 0 differing; 1.17 u / 1.20 u against the rotation of the
        float32 base, bound 3 u; 1.44 u against the angle itself;
    sincos_f64 0.73 ulp beyond the reduction's error (1.52 before its evaluation order was changed for this test), bound 1;
        M<double>::sincos_small 0.58 ulp; M<double>::rcp_pos 0.50 ulp; pow_m02 0.93 ulp, bound 2;
    right-hand side, checked: float32 14.8 u S (dp_theta, pole class, a = 0.9), float64 11.0 2^-53 S, bound 26; per
        component over all classes  dr 2.4  dtheta 5.1  dphi 8.8  dp_r 14.7  dp_theta 14.8;
    forms: every bit equal (35 950 valid states checked = fast, 23 194 in the band q1 = fast, packed = fast on all);
        the checked step where fast is invalid (793 by radius, 2 239 by angle): 9.1 units, bound 52;
    one step, float32, checked and fast: 5.81 units (dp_theta, pole_approach, a = 0.998), bound 8; far / mid / eq_band 0.45 ... 1.1;
    one step, float64: 2.32 units (dp_theta, `band` at a = 0.998), bound 8 -- 12.92 there while the float64 right-hand side
        formed Delta as (r^2 + a^2) - 2 M r, see kerr_rhs_parts; and 13.31 at the one state of `pole_approach`, a = 0.9,
        whose step crosses the axis (held to 54: the float64 oracle is 26 off there).
"""
import json
import os

import numpy as np
import pytest

import ltrace
import step_blocks as sb
from oracle import oracle

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_STEP_BLOCKS_MEASURE")  # a path: the figures the tests print are also written there as JSON
U = sb.U32
N = 1501  # states per class: no multiple of 64
_RECORD = {}


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


def bits(x):
    return int(np.float32(x).view(np.uint32))


def same_bits(x, y):
    """Elementwise: the float32 values held in two float64 arrays have the same bit pattern (a NaN equals a NaN)."""
    x32, y32 = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    assert np.array_equal(x32.astype(np.float64), x, equal_nan=True) and np.array_equal(y32.astype(np.float64), y, equal_nan=True)
    return (x32.view(np.uint32) == y32.view(np.uint32)) | (np.isnan(x32) & np.isnan(y32))


# ---------------------------------------------------------------------------------------------------------------------------
# float64 yardsticks against mpmath
# ---------------------------------------------------------------------------------------------------------------------------
def _sincos_args():
    rng = np.random.default_rng(11)
    m = np.arange(1, 6367) * (np.pi / 2)  # every multiple of pi/2 below 1e4: the float64 next to it and its two neighbours
    near = np.concatenate([np.nextafter(m, -np.inf), m, np.nextafter(m, np.inf)])
    n = (200000 - 2 * near.size) // 2
    logs = np.exp(rng.uniform(np.log(1e-300), np.log(1e5), n)) * rng.choice([-1.0, 1.0], n)
    return np.concatenate([near, -near, logs, rng.uniform(-1e5, 1e5, n), [0.0, -0.0, 1e5, -1e5]])


def test_sincos_f64_against_mpmath():
    """`< 1 ulp` (lt_device.hpp) is the claim for the polynomials on an exact remainder; the remainder itself is `a
    double-double good to |x| ~ 1e5`: pi/2 is carried as P1 + P1T, short of it by at most half an ulp of P1T (2^-87) and
    multiplied by k with one rounding (2^-53 k P1T), so the reduced angle of x = k pi/2 + y is off by at most 1.4e-26 |k|.
    Next to a multiple of pi/2, where one of the two results is of the size of the argument's own rounding, that -- not an
    ulp of the result -- is what a two-word reduction can give.  So: error < 1 ulp of the true result + 1.4e-26 |k|."""
    x = _sincos_args()
    got = ltrace.math64_probe("sincos", x)
    hi, lo = sb.mp_sincos(x)
    err, ulps = sb.err64(got, hi, lo)
    k = np.abs(np.rint(x * (2 / np.pi)))[:, None]
    rest = np.maximum(err - 1.4e-26 * k, 0.0) / np.spacing(np.abs(hi))
    i = np.unravel_index(np.argmax(rest), rest.shape)
    print(f"sincos_f64, {x.size} arguments: max error beyond the reduction's {rest.max():.3f} ulp at x = {x[i[0]]!r} "
          f"({('sin', 'cos')[i[1]]}); max absolute error {err.max() / sb.U64:.3f} 2^-53; max error in ulps of the result {ulps.max():.3g}")
    record("sincos_f64", dict(n=x.size, max_ulp_beyond_reduction=rest.max(), max_abs_over_2m53=err.max() / sb.U64, max_ulp_raw=ulps.max(),
                              at=float(x[i[0]])))
    assert np.array_equal(ltrace.math64_probe("sincos", x[:1]), got[:1]) and np.array_equal(ltrace.math64_probe("sincos", x[:65]), got[:65])
    assert err.max() > 0
    assert rest.max() < 1.0


def test_sincos_small_f64_against_mpmath():
    """`error < 3e-18` is the truncation error of the Taylor polynomials; the result is then rounded.  The last operation of
    either value is one fma (half an ulp of the result); what it adds to d, or to 1, is at most 1/32 of the result and
    carries at most four roundings, under 1/8 ulp together.  So: |error| <= 3e-18 + 0.75 ulp of the true result."""
    rng = np.random.default_rng(12)
    d = np.concatenate([rng.uniform(-0.25, 0.25, 10000), np.exp(rng.uniform(np.log(1e-300), np.log(0.25), 10000)), [0.25, -0.25, 0.0]])
    got = ltrace.math64_probe("sincos_small", d)
    hi, lo = sb.mp_sincos(d)
    err, ulps = sb.err64(got, hi, lo)
    over = (err - 3e-18) / np.spacing(np.abs(hi))
    print(f"M<double>::sincos_small, {d.size} arguments: max error {ulps.max(axis=0)} ulp (sin, cos), {err.max():.3e} absolute")
    record("sincos_small_f64", dict(n=d.size, max_ulp_sin=ulps[:, 0].max(), max_ulp_cos=ulps[:, 1].max(), max_abs=err.max()))
    assert np.array_equal(ltrace.math64_probe("sincos_small", d[:65]), got[:65])
    assert err.max() > 0 and over.max() <= 0.75


def test_rcp_pos_f64_against_mpmath():
    rng = np.random.default_rng(13)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-300), np.log(1e300), 20000)), [1e-300, 1e300, 1.0, 3.0]])
    got = ltrace.math64_probe("rcp_pos", x)[:, 0]
    err, ulps = sb.err64(got, *sb.mp_rcp(x))
    print(f"M<double>::rcp_pos, {x.size} arguments: max error {ulps.max():.3f} ulp")
    record("rcp_pos_f64", dict(n=x.size, max_ulp=ulps.max()))
    assert np.array_equal(ltrace.math64_probe("rcp_pos", x[:1])[:, 0], got[:1])
    assert err.max() > 0 and ulps.max() <= 1.0  # "within an ulp"


def test_pow_m02_against_mpmath():
    rng = np.random.default_rng(14)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-6), np.log(1e4), 20000)), [1e-6, 1e4, 1.0, 32.0]])
    got = ltrace.math64_probe("pow_m02", x)[:, 0]
    err, ulps = sb.err64(got, *sb.mp_pow_m02(x))
    print(f"pow_m02, {x.size} arguments in [1e-6, 1e4]: max error {ulps.max():.3f} ulp")
    record("pow_m02", dict(n=x.size, max_ulp=ulps.max()))
    assert err.max() > 0 and ulps.max() <= 2.0  # "~1 ulp"
    # the clamps: the controllers cut the factor off there anyway
    lo, hi = np.array([9.999999e-7, 1e-9, 1e-300, 0.0]), np.array([1.0000001e4, 1e9, 1e300])
    assert (ltrace.math64_probe("pow_m02", lo)[:, 0] == 100.0).all() and (ltrace.math64_probe("pow_m02", hi)[:, 0] == 0.1).all()
    assert np.isnan(ltrace.math64_probe("pow_m02", [np.nan])[0, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# float32 primitives, every value of the domain
# ---------------------------------------------------------------------------------------------------------------------------
def sweep(which, lo, hi, bases=None, signs=(0, 0x80000000)):
    """math32_probe over every float32 with lo <= |x| <= hi (bit patterns), in calls of at most 2^30 values, merged."""
    total = None
    for sign in signs:
        b = lo
        while b <= hi:
            e = min(hi, b + (1 << 30) - 1)
            r = ltrace.math32_probe(which, sign | b, sign | e, bases)
            assert r["compared"] == (e - b + 1) * (1 if bases is None else len(bases))
            if total is None:
                total = r
            else:
                total["compared"] += r["compared"]
                total["differing"] += r["differing"]
                if total["first_differing"] is None:
                    total["first_differing"] = r["first_differing"]
                for key in ("abs_sin", "abs_cos", "ulp_sin", "ulp_cos", "abs_angle"):
                    total[key] = max(total[key], r[key], key=lambda t: t[0])
            b = e + 1
    return total


def _arg(r, key):
    v, a = r[key]
    return None if a is None else float(np.uint32(a & 0xFFFFFFFF).view(np.float32))


def test_sincos_f32_every_value():
    """M<float>::sincos on its stated domain |x| <= 1e4: absolute error <= 2 u for either value."""
    r = sweep("sincos", 0, bits(1e4))
    small = sweep("sincos", 0, bits(13.0))
    print(f"M<float>::sincos, {r['compared']} values |x| <= 1e4: max absolute error sin {r['abs_sin'][0] / U:.3f} u at {_arg(r, 'abs_sin')!r}, "
          f"cos {r['abs_cos'][0] / U:.3f} u at {_arg(r, 'abs_cos')!r}; |x| <= 13: max error in ulps of the result sin "
          f"{small['ulp_sin'][0]:.4g} at {_arg(small, 'ulp_sin')!r}, cos {small['ulp_cos'][0]:.4g} at {_arg(small, 'ulp_cos')!r}")
    record("sincos_f32", dict(compared=r["compared"], abs_sin_u=r["abs_sin"][0] / U, abs_cos_u=r["abs_cos"][0] / U,
                              at_sin=_arg(r, "abs_sin"), at_cos=_arg(r, "abs_cos"), ulp_sin_below_13=small["ulp_sin"][0],
                              ulp_cos_below_13=small["ulp_cos"][0], at_ulp_sin=_arg(small, "ulp_sin"), at_ulp_cos=_arg(small, "ulp_cos")))
    assert r["compared"] == 2 * (bits(1e4) + 1)
    assert 0 < r["abs_sin"][0] <= 2 * U and 0 < r["abs_cos"][0] <= 2 * U


def test_rcp_pos_f32_every_value():
    """M<float>::rcp_pos, every float32 in [2^-100, 2^100]: within 1 ulp."""
    r = sweep("rcp_pos", (127 - 100) << 23, (127 + 100) << 23, signs=(0,))
    print(f"M<float>::rcp_pos, {r['compared']} values: max error {r['ulp_sin'][0]:.4f} ulp at {_arg(r, 'ulp_sin')!r}")
    record("rcp_pos_f32", dict(compared=r["compared"], max_ulp=r["ulp_sin"][0], at=_arg(r, "ulp_sin")))
    assert r["compared"] == (200 << 23) + 1
    assert 0 < r["ulp_sin"][0] <= 1.0


def test_sincos_small_f32_every_value():
    """M<float>::sincos_small, every float32 |d| <= 0.25: cosine within 1 u absolute, sine within 2 ulp of the result."""
    r = sweep("sincos_small", 0, bits(0.25))
    print(f"M<float>::sincos_small, {r['compared']} values: max error cos {r['abs_cos'][0] / U:.3f} u at {_arg(r, 'abs_cos')!r}, "
          f"sin {r['ulp_sin'][0]:.3f} ulp at {_arg(r, 'ulp_sin')!r} ({r['abs_sin'][0] / U:.3f} u absolute)")
    record("sincos_small_f32", dict(compared=r["compared"], abs_cos_u=r["abs_cos"][0] / U, ulp_sin=r["ulp_sin"][0],
                                    abs_sin_u=r["abs_sin"][0] / U, at_cos=_arg(r, "abs_cos"), at_sin=_arg(r, "ulp_sin")))
    assert r["compared"] == 2 * (bits(0.25) + 1)
    assert 0 < r["abs_cos"][0] <= U and 0 < r["ulp_sin"][0] <= 2.0


SHIFT_BASES = (0.8, np.float32(np.pi / 2), 2.34, 1e-3, 3.1, 7.0, -2.0)


def test_sincos_shift_f32_every_value():
    """The stage rotation in its scalar and its packed form, every float32 |d| <= 0.25 at seven base angles: no bit differs,
    and against the float64 rotation of the same float32 (sin, cos) of the base: within 3 u (two rounded products and one
    sum of magnitudes <= 1, plus the small-angle errors)."""
    r = sweep("sincos_shift", 0, bits(0.25), bases=np.array(SHIFT_BASES, dtype=np.float32))
    worst = max(r["abs_sin"][0], r["abs_cos"][0])
    print(f"sincos_shift / sincos_shift_pk, {r['compared']} (base, d): differing {r['differing']}; max absolute error against the rotation "
          f"of the float32 base sin {r['abs_sin'][0] / U:.3f} u, cos {r['abs_cos'][0] / U:.3f} u; against the angle itself {r['abs_angle'][0] / U:.3f} u")
    record("sincos_shift_f32", dict(compared=r["compared"], differing=r["differing"], abs_sin_u=r["abs_sin"][0] / U,
                                    abs_cos_u=r["abs_cos"][0] / U, abs_angle_u=r["abs_angle"][0] / U,
                                    at_sin=r["abs_sin"][1], at_cos=r["abs_cos"][1]))
    assert r["compared"] == 2 * (bits(0.25) + 1) * len(SHIFT_BASES)
    assert r["differing"] == 0, f"first at (base << 32 | bits of d) = {r['first_differing']:#x}"
    assert 0 < worst <= 3 * U


def test_math32_probe_small_ranges():
    """One value and 65 values: counts, and maxima that the sweep of the whole domain contains."""
    one = ltrace.math32_probe("sincos", bits(1.0), bits(1.0))
    s, c = np.float32(np.sin(np.float64(np.float32(1.0)))), np.float32(np.cos(np.float64(np.float32(1.0))))
    assert one["compared"] == 1 and one["abs_sin"][0] <= 2 * U and one["abs_cos"][0] <= 2 * U
    got = ltrace.math64_probe("sincos_f32", [1.0])[0]
    assert abs(got[0] - float(s)) <= 2 * U and abs(got[1] - float(c)) <= 2 * U
    assert one["abs_sin"][0] == pytest.approx(abs(got[0] - np.sin(1.0)), abs=1e-15)
    for which, lo in (("sincos", bits(3.0)), ("sincos_small", bits(0.1)), ("rcp_pos", bits(3.0))):
        r = ltrace.math32_probe(which, lo, lo + 64)
        assert r["compared"] == 65 and r["ulp_sin"][0] > 0 and lo <= r["ulp_sin"][1] <= lo + 64
    r = ltrace.math32_probe("sincos_shift", bits(0.1), bits(0.1) + 64, bases=[0.8, 2.0])
    assert r["compared"] == 130 and r["differing"] == 0 and 0 < r["abs_sin"][0] <= 3 * U
    with pytest.raises(ltrace.LtraceError):
        ltrace.math32_probe("sincos", 5, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the right-hand side
# ---------------------------------------------------------------------------------------------------------------------------
COMPONENTS = ("dr", "dtheta", "dphi", "dp_r", "dp_theta")


@pytest.mark.parametrize("precision", [32, 64])
def test_rhs_checked_in_the_unit(precision):
    """The checked right-hand side on every class, pole and edge rows included, nothing left out: every component within
    2 K_REF u S of the float64 reference (float64: 2 K_REF 2^-53 S of the same statements in longdouble -- the float64
    oracle's own error is of that size)."""
    u = U if precision == 32 else sb.U64
    table = {}
    for a in sb.SPINS:
        for name in sb.RHS_CLASSES:
            st, L = sb.rhs_class(name, a, N)
            got = ltrace.kerr_rhs_form_probe(sb.M, a, st, L, precision=precision)
            assert np.isfinite(got).all()
            if precision == 32:
                assert np.array_equal(got.astype(np.float32).astype(np.float64), got)
                err = np.abs(got - oracle.kerr_rhs_n(st, L, sb.M, a))
            else:
                err = np.abs(got.astype(sb.LD) - sb.ref_rhs_longdouble(a, st, L)).astype(np.float64)
            # (edge rows: S with the floor as the float32 kernel applies it, sin^2 + 1e-15)
            S = sb.scales(a, st, L, floor_added=precision == 32 and name == "edge")
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(err == 0, 0.0, err / (u * S))
            worst = ratio.max(axis=0)
            table[f"a={a} {name}"] = worst
            print(f"rhs float{precision} a = {a} {name:8s}: max error / (u S) " + "  ".join(f"{c} {w:.2f}" for c, w in zip(COMPONENTS, worst)))
            assert st.shape[0] == N and worst.max() > 0
            assert (err <= 2 * sb.K_REF * u * S).all(), (a, name, worst)
    record(f"rhs_float{precision}", {k: v.tolist() for k, v in table.items()})
    record(f"rhs_float{precision}_max", max(v.max() for v in table.values()))


def test_rhs_forms_agree_in_every_bit():
    """Unchecked, packed and packed-last form against the checked one on every state outside r_cut; the checked form's zeros
    at and inside it."""
    for a in sb.SPINS:
        for name in sb.RHS_CLASSES:
            st, L = sb.rhs_class(name, a, N)
            assert (st[:, 0] > sb.r_cut(a) * (1 + 1e-6)).all()
            ref = ltrace.kerr_rhs_form_probe(sb.M, a, st, L, form="checked")
            assert np.array_equal(ltrace.kerr_rhs_probe(sb.M, a, st, L), ref)
            for form in ("unchecked", "packed", "packed_last"):
                got = ltrace.kerr_rhs_form_probe(sb.M, a, st, L, form=form)
                same = same_bits(got, ref)
                assert same.all(), (a, name, form, int((~same).sum()), st[np.argmin(same.all(axis=1))])
            ref64 = ltrace.kerr_rhs_form_probe(sb.M, a, st, L, precision=64)
            assert np.array_equal(ltrace.kerr_rhs_form_probe(sb.M, a, st, L, precision=64, form="unchecked"), ref64)
            for n in (1, 65):
                assert np.array_equal(ltrace.kerr_rhs_form_probe(sb.M, a, st[:n], L[:n], form="packed"), ref[:n])
        st, L = sb.inside_cut_class(a, N)
        assert (st[:, 0] <= np.float32(sb.r_cut(a))).all()
        for precision in (32, 64):
            assert (ltrace.kerr_rhs_form_probe(sb.M, a, st, L, precision=precision) == 0).all()
    with pytest.raises(ltrace.LtraceError):
        ltrace.kerr_rhs_form_probe(sb.M, 0.5, st, L, precision=64, form="packed")


# ---------------------------------------------------------------------------------------------------------------------------
# one step
# ---------------------------------------------------------------------------------------------------------------------------
def ref_step(a):
    return lambda st, L, h: oracle.rk4_step_kerr(st, L, h, sb.M, a)


_STEP_SETS = {}


def step_set(a, name):
    """(states, L, h (n,), refine (n,)) of a step class, and its float64 step, unit and exclusions: computed once."""
    key = (a, name)
    if key not in _STEP_SETS:
        if name == "fallback":
            st, L, h = sb.fallback_class(a, N)
            refine = np.zeros(N, dtype=np.uint8)
            y1, unit, keep = sb.fallback_unit(a, st, L, h, ref_step(a))
        else:
            c = sb.step_class(name, a, N)
            if c is None:
                return None
            st, L, h, rf = c
            h, refine = np.full(N, h), np.full(N, rf, dtype=np.uint8)
            y1, unit, keep = sb.step_unit(a, st, L, h, ref_step(a))
        _STEP_SETS[key] = dict(st=st, L=L, h=h, refine=refine, y1=y1, unit=unit, keep=keep)
    return _STEP_SETS[key]


def step(a, c, form, precision=32, n=None):
    n = N if n is None else n
    return ltrace.kerr_step_probe(sb.M, a, c["st"][:n], c["L"][:n], c["h"][:n], c["refine"][:n], precision=precision, form=form)


def valid(a, out):
    """The validity test of the branch-free step, with the r_cut the kernels use."""
    return sb.fast_step_valid(a, out)


STEP_SETS = sb.STEP_CLASSES + ("eq_band", "fallback")


def test_step_forms_agree_in_every_bit():
    fails_r = fails_d = in_band = checked_on_valid = 0
    worst_fallback = 0.0
    for a in sb.SPINS:
        for name in STEP_SETS:
            c = step_set(a, name)
            if c is None or (name == "fallback" and a > 0.9):
                continue
            chk, fast, q1, pk = (step(a, c, f) for f in ("checked", "fast", "fast_q1", "packed"))
            # fast and packed: everything, on every state
            for key in ("states", "min_r", "max_d"):
                same = same_bits(fast[key], pk[key])
                assert same.all(), (a, name, key, int((~same).sum()))
            assert np.isnan(chk["min_r"]).all() and np.isnan(fast["cs"]).all()
            # the packed step hands on [cos, sin] of its new polar angle
            sc = ltrace.math64_probe("sincos_f32", pk["states"][:, 1])
            fin = np.isfinite(pk["states"][:, 1])
            assert fin.sum() > (0.5 if name == "fallback" else 0.9) * N and same_bits(pk["cs"][fin], sc[fin][:, ::-1]).all(), (a, name)
            # the fixed-quadrant form inside the band
            band = (c["st"][:, 1] > 0.80) & (c["st"][:, 1] < 2.34)
            assert same_bits(q1["states"][band], fast["states"][band]).all() and same_bits(q1["min_r"][band], fast["min_r"][band]).all() \
                and same_bits(q1["max_d"][band], fast["max_d"][band]).all(), (a, name)
            in_band += int(band.sum())
            # checked against fast where fast says it is valid
            ok = valid(a, fast)
            same = same_bits(chk["states"][ok], fast["states"][ok])
            assert same.all(), (a, name, int((~same).sum()))
            checked_on_valid += int(ok.sum())
            if name == "fallback":
                bad_r = ~(fast["min_r"] > float(np.float32(sb.r_plus(a) * 1.001)))
                bad_d = ~(fast["max_d"] <= 0.25)
                fails_r += int((bad_r & c["keep"]).sum())
                fails_d += int((bad_d & c["keep"]).sum())
                # where the fast step is not valid the checked one has no twin: against the float64 step of the reference
                sel = ~ok & c["keep"]
                e = (np.abs(chk["states"] - c["y1"]) / c["unit"])[sel]
                print(f"checked step where the fast one is invalid, a = {a}: {sel.sum()} states ({int((bad_r & sel).sum())} by radius, "
                      f"{int((bad_d & sel).sum())} by angle), max error per component {np.round(e.max(axis=0), 2)} units")
                assert e.max() <= 2 * sb.K_FALLBACK
                worst_fallback = max(worst_fallback, e.max())
            else:
                assert ok.mean() > 0.9, (a, name, ok.mean())
            for n in (1, 65):
                for f, full in (("checked", chk), ("packed", pk)):
                    part = step(a, c, f, n=n)
                    assert all(same_bits(part[k], full[k][:n]).all() for k in ("states", "min_r", "max_d", "cs"))
    print(f"step forms: {checked_on_valid} valid states checked == fast, {in_band} in the band q1 == fast, "
          f"{fails_r} / {fails_d} kept states failing the radius / angle half of the validity test")
    record("step_forms", dict(valid=checked_on_valid, in_band=in_band, fails_radius=fails_r, fails_angle=fails_d, fallback_max_units=worst_fallback))
    assert fails_r > 100 and fails_d > 100 and in_band > 4 * N and worst_fallback > 0
    c = step_set(0.5, "far")
    for f in ("fast_q1", "packed"):
        with pytest.raises(ltrace.LtraceError):
            step(0.5, c, f, precision=64)


@pytest.mark.parametrize("precision", [32, 64])
def test_step_accuracy_in_the_unit(precision):
    """The checked and the branch-free step against the float64 step of the reference, in the unit A + h u S of
    tests/step_blocks.py, exclusions (at most 2 % of a class) from the float64 step alone: within 2 K_STEP units.

    Float64: 2^-53 for u; the values come from the same step in longdouble (the float64 oracle's own rounding is of the
    size of the bound), and a state at which the float64 oracle itself is more than K_STEP units from that is held to
    2 K_STEP64 instead (one state: step_blocks.py).

    What this test found: class `band` (r 1.3 ... 4 r_plus, h = 0.1) at a = 0.998 measured 12.92 units in dp_theta (5.49 in
    r, 4.09 in dp_r), worst at r = 1.42, theta = 1.555, p_r = -0.83, p_theta = 3.15, L = -5.42.  Delta = (r^2 + a^2) - 2 M r
    carried the rounding of r^2 + a^2, 34 ulps of Delta there, into every stage's P / Delta.  The float64 right-hand side
    now forms r (r - 2M) + a^2, rounded once (kerr_rhs_parts): 2.32 units, and `near` at a = 0.9 went from 4.23 to 2.15."""
    u = U if precision == 32 else sb.U64
    table, over = {}, []
    for a in sb.SPINS:
        for name in sb.STEP_CLASSES + ("eq_band",):
            c = step_set(a, name)
            if c is None:
                continue
            if precision == 32:
                y1, unit, keep = c["y1"], c["unit"], c["keep"]
            else:
                # unit and exclusions from the float64 oracle; the values from the same step in longdouble, because the
                # float64 oracle's own rounding is of the size of the bound (26 units in `pole_approach` at a = 0.9)
                y64, unit, keep = sb.step_unit(a, c["st"], c["L"], c["h"], ref_step(a), u=u)
                y1 = sb.ref_step_longdouble(a, c["st"], c["L"], c["h"])
                ref_ok = ((np.abs(y64.astype(sb.LD) - y1).astype(np.float64) / unit) <= sb.K_STEP).all(axis=1)
                assert ref_ok[keep].mean() > 0.99
            assert 1.0 - keep.mean() <= sb.EXCLUDED_CAP and keep.sum() > 0
            for form in ("checked", "fast"):
                out = step(a, c, form, precision=precision)
                sel = keep & (valid(a, out) if form == "fast" else True)
                assert sel.sum() > 0.9 * N
                e = (np.abs(out["states"].astype(y1.dtype) - y1).astype(np.float64) / unit)[sel]
                assert np.isfinite(e).all()
                worst = e.max(axis=0)
                table[f"a={a} {name} {form}"] = worst
                print(f"step float{precision} a = {a} {name:13s} {form:7s}: {sel.sum()} states, max error per component {np.round(worst, 2)} units")
                assert worst.max() > 0
                if precision == 32:
                    ok = worst.max() <= 2 * sb.K_STEP
                else:
                    ok = e[ref_ok[sel]].max() <= 2 * sb.K_STEP and worst.max() <= 2 * sb.K_STEP64
                if not ok:
                    over.append((a, name, form, np.round(worst, 2).tolist()))
    record(f"step_float{precision}", {k: v.tolist() for k, v in table.items()})
    record(f"step_float{precision}_max", max(v.max() for v in table.values()))
    assert not over, over
