"""Where the bounds of tests/test_gpu_disk_blocks.py come from, on the CPU, from the oracle, numpy and longdouble / mpmath
alone (tests/disk_blocks.py states the units, the classes, the tables and the exclusions).

    K_ROOT64 = K_ROOT32 = 2   the root of theta = pi/2 on the step's cubic, oracle (lto_disk_step) against longdouble
    K_HIT64  = K_HIT32  = 4   the crossing state, component by component
    K_G = 3, K_WRAP = 2, K_EMIT = 4   numpy's float64 disk.redshift, disk.wrap_2pi and the statements of disk.shade

Each is asserted from both sides: the measured maximum lies in (K - 1, K].  No class leaves out more than 2 % of its rows
(the rows +-1, +-2, +-8 ulp from an edge are a class of their own, exempt from that cap: every row of it is held to "a hit lies
in the annulus", its stable rows to everything else).  The oracle's
decisions are the longdouble's on every stable row.  The premises of the device's radius pre-filter and of its streak gate
are replayed in longdouble on every step of every class.  What the twin's terminal rule and the device's have in common and
where their statements part is recorded at the end.
"""
import math

import numpy as np
import pytest

import disk as diskmod
import disk_blocks as dk
from oracle import oracle

COMPONENTS = ("r", "theta", "phi", "p_r", "p_theta")


def oracle_step(c, precision, **kw):
    return oracle.disk_step(c["y0"], c["y1"], c["L"], c["h"], c["M"], c["a"], c["r_in"], c["r_out_t"], terminal=c["terminal"],
                            frac=c["t_end"], r_obs=c["r_obs"], f32=precision == 32, **kw)


def chord_crosses(c, precision):
    """The sign test of a step that also ended the ray (ltrace.h): between theta0 and the chord's theta at the cut.
    -> (crosses (n,) bool -- True on a row that did not end the ray --, clear (n,) bool: the chord's theta at the cut lies
    more than 8 roundings of its terms from the plane)."""
    hp = dk.LD(dk.as_t(np.pi / 2, precision))
    th0, th1, f = c["y0"][:, 1].astype(dk.LD), c["y1"][:, 1].astype(dk.LD), c["t_end"].astype(dk.LD)
    with np.errstate(invalid="ignore"):
        chord = th0 + f * (th1 - th0) - hp
        z0 = th0 - hp
        cross = ((z0 < 0) & (chord >= 0)) | ((z0 > 0) & (chord <= 0))
        clear = np.abs(chord) > 8 * dk.u_of(precision) * (np.abs(th0) + np.abs(th1) + hp)
    plain = c["terminal"] == 0
    return cross | plain, clear | plain


def all_classes(precision):
    for a in dk.SPINS:
        for name in dk.CROSSING_CLASSES:
            c = dk.crossing_class(name, a, precision)
            if c is not None:
                yield a, name, c


@pytest.mark.parametrize("precision", [64, 32])
def test_oracle_crossing_against_longdouble_in_the_units(precision):
    worst_t, worst_h, at_t, at_h = 0.0, 0.0, None, None
    checked = 0
    for a, name, c in all_classes(precision):
        ref, keep = c["ref"], c["keep"] & chord_crosses(c, precision)[1]
        o = oracle_step(c, precision)
        if name == "nan":
            # IEEE semantics and nothing else: a NaN polar angle never crosses, a NaN crossing radius is never a hit
            bad_th = np.isnan(c["y0"][:, 1]) | np.isnan(c["y1"][:, 1])
            assert not o["cross"][np.isnan(c["y0"][:, 1])].any() and not o["is_hit"][bad_th | np.isnan(o["state"][:, 0])].any()
            continue
        hits = o["is_hit"]
        assert ((o["state"][hits, 0] >= c["r_in"]) & (o["state"][hits, 0] <= c["r_out_t"])).all()
        left_out = 1.0 - keep.mean()
        if name in dk.UNSTABLE_CLASSES:
            assert 0.1 < left_out, (a, name, left_out)  # (what the class is for; its stable rows are held like any other's)
        else:
            assert left_out <= dk.EXCLUDED_CAP, (a, name, precision, left_out)  # (decided before any compared value is read)
        plain = keep & (c["terminal"] == 0)  # (a terminal row: the twin's `cross` is the chord's, test_terminal_rule_... below)
        assert np.array_equal(o["cross"][plain], ref["cross"][plain]), (a, name)
        want = ref["found"] & chord_crosses(c, precision)[0]
        assert np.array_equal(o["is_hit"][keep], want[keep]), (a, name, np.nonzero(keep & (o["is_hit"] != want))[0][:8])
        if name == "still":
            assert not o["cross"].any()
            continue
        # a terminal row's root lies on [0, 1] for the twin and on [0, t_end] here: the same root wherever it is on the path
        both = keep & o["cross"] & ref["cross"] & (o["on_path"] | (c["terminal"] == 0))
        assert both.sum() > 0.15 * dk.N, (a, name, both.sum())
        et = (np.abs(o["t"].astype(dk.LD) - ref["t"]).astype(np.float64) / ref["unit_t"])[both]
        eh = (np.abs(o["state"].astype(dk.LD) - ref["hit"]).astype(np.float64) / ref["unit"])[both]
        assert np.isfinite(et).all() and np.isfinite(eh).all()
        print(f"float{precision} oracle crossing, a = {a:6}, {name:12s}: left out {100 * left_out:.2f} %, crossings {int(ref['cross'].sum())}, "
              f"hits {int(ref['found'].sum())}; root {et.max():.2f} units, state {np.round(eh.max(axis=0), 2)} units")
        checked += int(keep.sum())
        if et.max() > worst_t:
            worst_t, at_t = et.max(), (a, name, int(np.nonzero(both)[0][np.argmax(et)]))
        if eh.max() > worst_h:
            i = np.unravel_index(np.argmax(eh), eh.shape)
            worst_h, at_h = eh.max(), (a, name, COMPONENTS[i[1]], int(np.nonzero(both)[0][i[0]]))
    print(f"K_root{precision}: measured {worst_t:.2f} -> {math.ceil(worst_t)} at {at_t}")
    print(f"K_hit{precision}: measured {worst_h:.2f} -> {math.ceil(worst_h)} at {at_h}")
    assert dk.k_root(precision) - 1 < worst_t <= dk.k_root(precision)
    assert dk.k_hit(precision) - 1 < worst_h <= dk.k_hit(precision)
    assert checked > 15000


@pytest.mark.parametrize("precision", [64, 32])
def test_a_state_on_the_plane_is_counted_once_over_two_steps(precision):
    """theta = pi/2 exactly (as T has it) and one ulp to either side, at the joint of two consecutive steps a -> b -> c: the
    strict-change rule counts the passage once wherever a and c lie on opposite sides -- in the oracle and in longdouble."""
    total = 0
    for a in dk.SPINS:
        c = dk.crossing_class("on_plane", a, precision)
        joint_end = (np.arange(dk.N) % 2) == 1            # rows whose END state was put on / beside the plane
        yb = c["y1"][joint_end]
        L, h = c["L"][joint_end], c["h"][joint_end]
        ya = c["y0"][joint_end]
        yc = dk.as_t(dk._step(c["M"], c["a"], yb, L, h, precision), precision)
        hp = float(dk.as_t(np.pi / 2, precision))
        first = oracle.disk_step(ya, yb, L, h, c["M"], c["a"], c["r_in"], c["r_out_t"], f32=precision == 32)["cross"]
        second = oracle.disk_step(yb, yc, L, h, c["M"], c["a"], c["r_in"], c["r_out_t"], f32=precision == 32)["cross"]
        r1 = dk.crossing_longdouble(c["M"], c["a"], ya, yb, L, h, 1.0, c["r_in"], c["r_out_t"], precision)["cross"]
        r2 = dk.crossing_longdouble(c["M"], c["a"], yb, yc, L, h, 1.0, c["r_in"], c["r_out_t"], precision)["cross"]
        assert np.array_equal(first, r1) and np.array_equal(second, r2)
        opposite = (ya[:, 1] - hp) * (yc[:, 1] - hp) < 0
        assert opposite.sum() > 100
        assert ((first.astype(int) + second.astype(int))[opposite] == 1).all()
        on = yb[:, 1] == hp
        assert on.sum() > 50 and first[on].all() and not second[on].any()  # landing counts, leaving does not
        total += int(opposite.sum())
    assert total > 500


@pytest.mark.parametrize("precision", [64, 32])
def test_premises_of_the_radius_prefilter_and_the_streak_gate(precision):
    """lt_disk.hpp: `near` widens the annulus by pad = (step bound) * vmax2 and the streak runs above r_out + 2 h vmax2 because
    (1) |r'| <= disk_vmax at both ends, (2) the step's Hermite cubic in r leaves the interval of its ends by at most
    0.15 h (|r'_0| + |r'_1|), hence (3) the cubic stays within h vmax2 / 2 of either end.  Replayed in longdouble on every
    step of every class whose ends lie outside r_cut (inside it the right-hand side is zero and no ray continues) and on the
    null shell to 1e-3 (disk_blocks.shell_defect; (1) is a statement about a null ray, and the kernels double vmax for the
    drift): the steps left out passed a stage through r_cut and carry momenta of 1e3 and more."""
    worst = np.zeros(3)
    rows = 0
    t = np.linspace(0.0, 1.0, 257).astype(dk.LD)
    for a, name, c in all_classes(precision):
        if name in ("nan", "still"):
            continue
        M, aa = c["M"], c["a"]
        outside = (c["y0"][:, 0] > 1.002 * 1.001 * dk.r_plus(M, aa)) & (c["y1"][:, 0] > 1.002 * 1.001 * dk.r_plus(M, aa))
        with np.errstate(invalid="ignore"):
            outside &= (dk.shell_defect(M, aa, c["y0"], c["L"]) < 1e-3) & (dk.shell_defect(M, aa, c["y1"], c["L"]) < 1e-3)
        y0, y1, L, h = c["y0"][outside], c["y1"][outside], c["L"][outside], c["h"][outside].astype(dk.LD)
        with dk.mass(M):
            v0 = dk.sb.ref_rhs_longdouble(aa, y0, L)[:, 0]
            v1 = dk.sb.ref_rhs_longdouble(aa, y1, L)[:, 0]
        vmax = (1.0 + (aa * aa + np.abs(aa * L)) / dk.r_plus(M, aa) ** 2).astype(dk.LD)
        d = (y0[:, 0].astype(dk.LD)[:, None], (h * v0)[:, None], y1[:, 0].astype(dk.LD)[:, None], (h * v1)[:, None])
        b = dk._basis(t[None, :])
        rc = b[0] * d[0] + b[1] * d[1] + b[2] * d[2] + b[3] * d[3]
        lo, hi = np.minimum(d[0], d[2]), np.maximum(d[0], d[2])
        speed = np.maximum(np.abs(v0), np.abs(v1)) / vmax
        excursion = np.maximum(rc - hi, lo - rc).max(axis=1) / (dk.LD(0.15) * h * (np.abs(v0) + np.abs(v1)))
        reach = np.maximum(np.abs(rc - d[0]), np.abs(rc - d[2])).max(axis=1) / (h * vmax)
        worst = np.maximum(worst, [float(speed.max()), float(excursion.max()), float(reach.max())])
        rows += int(outside.sum())
    print(f"float{precision}: {rows} steps; largest |r'| / vmax {worst[0]:.4f}, excursion / (0.15 h (|r'_0| + |r'_1|)) {worst[1]:.4f}, "
          f"reach / (h vmax2 / 2) {worst[2]:.4f}")
    assert rows > 15000
    assert worst[0] <= 1.0 and worst[1] <= 1.0 and worst[2] <= 1.0, worst


def test_redshift_in_its_unit():
    worst, at = 0.0, None
    for tb in dk.g_table():
        got = diskmod.redshift(tb["M"], tb["a"], tb["r"], tb["xi"])
        e = np.abs(got - tb["g"]) / tb["unit"]  # (g is the truth rounded to float64: half a unit of its own at most)
        i = int(np.argmax(e))
        rel = np.abs(got - tb["g"]) / tb["g"]
        print(f"g, M = {tb['M']}, a = {tb['a']:7.4f}: {tb['r'].size} rows, max {e[i]:.2f} units at r = {tb['r'][i]!r}, xi = {tb['xi'][i]!r}; "
              f"largest unit {np.max(tb['unit'] / tb['g']):.2e} relative, largest error {rel.max():.2e} relative")
        if e[i] > worst:
            worst, at = float(e[i]), (tb["M"], tb["a"], float(tb["r"][i]), float(tb["xi"][i]))
    print(f"K_g: measured {worst:.2f} -> {math.ceil(worst)} at {at}")
    assert dk.K_G - 1 < worst <= dk.K_G


def test_wrap_and_half_orbits_tables():
    tb = dk.phi_table()
    phi = tb["phi"]
    got = diskmod.wrap_2pi(phi)
    assert ((got >= 0) & (got < 2 * np.pi)).all()
    e = dk.circle_distance(got, tb["wrapped"]) / tb["unit"]
    i = int(np.argmax(e))
    print(f"wrap_2pi: {phi.size} rows, max {e[i]:.2f} units at phi = {phi[i]!r}")
    assert dk.K_WRAP - 1 < e[i] <= dk.K_WRAP
    # the guard: a tiny negative angle wraps to 0, which is its neighbour on the circle, never to 2 pi
    assert diskmod.wrap_2pi(np.array([-1e-17]))[0] == 0.0 and np.isnan(diskmod.wrap_2pi(np.array([np.nan]))[0])
    near = tb["near"]
    print(f"half_orbits: {int(near.sum())} of {phi.size} rows lie within the unit of a multiple of pi (either count is right there): "
          f"phi = 0, +-0, and the float64 neighbours of k pi from |k| = {int(np.abs(np.round(phi[near] / np.pi))[np.abs(phi[near]) > 1].min())} on")
    assert 0 < near.sum() < 0.7 * phi.size and (tb["half"] >= 0).all()


def test_emission_and_colour_statements():
    worst, at, unsure, n = 0.0, None, 0, 0
    M, a = 1.0, 0.9
    for q, ex in dk.SHADE_CASES:
        tb = dk.shade_table(M, a, q, ex)
        E, unit = dk.emission_longdouble(tb["r"], tb["g"], tb["r_in"], q, ex)
        got = dk.emission_numpy(tb["r"], tb["g"], tb["r_in"], q, ex)
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.where(unit > 0, np.abs(got.astype(dk.LD) - E).astype(np.float64) / unit, 0.0)
        assert (got[unit == 0] == 0).all()
        if e.max() > worst:
            i = np.unravel_index(np.argmax(e), e.shape)
            worst, at = float(e.max()), (q, ex, float(tb["r"][i[0]]), float(tb["g"][i[0]]), int(i[1]))
        rgb, sure3, mean, sure1 = dk.shade_expected(E, 2 * dk.K_EMIT * unit)
        s3 = diskmod.shade(tb["r"], tb["g"], tb["r_in"], q, ex, 3)
        s1 = diskmod.shade(tb["r"], tb["g"], tb["r_in"], q, ex, 1)
        assert np.array_equal(s3[sure3], rgb[sure3]) and np.array_equal(s1[sure1], mean[sure1])
        unsure += int((~sure3).sum()) + int((~sure1).sum())
        n += sure3.size + sure1.size
        # the knees are in the table: every channel is met below, on and above both of its clamps
        lin = 2.0 * tb["g"] * (tb["r_in"] / tb["r"]) ** 0.75
        for ch in range(3):
            for knee in (0.5 * ch, 0.5 * ch + 1.0):
                d = lin - knee
                beside = np.abs(d) < 1e-6
                # (s = 0 is g = 0: no redshift lies below it)
                assert beside.sum() >= 100 and (d[beside] > 0).any() and ((d[beside] < 0).any() or knee == 0)
        assert (np.abs(E.astype(np.float64) - 1.0) < 1e-6).sum() >= 50
    print(f"K_emit: measured {worst:.2f} -> {math.ceil(worst)} at (q, exposure, r, g, channel) = {at}; {unsure} of {n} colours lie "
          f"within the bound of a float32 rounding boundary")
    assert dk.K_EMIT - 1 < worst <= dk.K_EMIT
    assert unsure < 0.02 * n


def test_terminal_rule_of_the_twin_and_of_the_device_statement():
    """ltrace.h: on a step that also ends the ray, the sign change is looked for between the previous state and the terminal
    (chord) state, the root is the full step's cubic's, and the disk wins if the root lies at or before the cut.  The twin
    does exactly that (sign of the chord at frac, bisection on [0, 1], t <= frac).  The device takes the sign of the CUBIC at
    the cut and searches [0, t_end] (crossing_longdouble states that).  With one root on [0, 1] both say: a hit iff the root
    lies before the cut.  They part only where chord and cubic differ in sign at the cut -- then both say no hit, for
    different reasons -- or where the cubic has two roots on [0, 1], which no row of the table has."""
    for precision in (64, 32):
        c = dk.crossing_class("terminal", 0.998, precision)
        term = c["terminal"] != 0
        assert term.sum() > 100
        o = oracle_step(c, precision)
        ref = c["ref"]
        chord_cross, clear = chord_crosses(c, precision)
        differ = term & (chord_cross != ref["cross"])
        keep = c["keep"] & term & clear
        print(f"float{precision}: {int(term.sum())} terminal rows ({int((c['terminal'] < 0).sum())} captures, {int((c['terminal'] > 0).sum())} escapes), "
              f"{int(keep.sum())} stable; twin hits {int(o['is_hit'][keep].sum())}, chord crossed but root after the cut {int((o['cross'] & ~o['on_path'])[keep].sum())}; "
              f"chord and cubic differ in sign at the cut on {int(differ.sum())} rows, {int((differ & keep).sum())} of them stable")
        assert np.array_equal(o["is_hit"][keep], (ref["found"] & chord_cross)[keep])
        assert not o["is_hit"][differ & keep].any()
        hp = float(dk.as_t(np.pi / 2, precision))
        after = keep & ((c["y0"][:, 1] - hp) * (c["y1"][:, 1] - hp) < 0) & ~chord_cross  # the plane is crossed after the cut
        print(f"    {int(after.sum())} stable rows cross the plane after the cut")
        assert (o["is_hit"][keep]).sum() > 20 and after.sum() > 20 and not o["is_hit"][after].any()
        lost = differ & keep & ref["found"]
        print(f"    of those, {int(lost.sum())} cross the annulus on the cubic before the cut while the chord has not reached the plane: no hit, by the header's sign test")
