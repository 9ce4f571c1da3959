"""One crossing of the disk's plane on the device -- disk_crossing (lt_disk_crossing_probe), disk_advance with its pre-filter
and its wave-wide branch (lt_disk_advance_probe) -- and the closed forms a hit goes through (lt_disk_shade_probe), each by the
function the production kernels call, against the same statement in longdouble / mpmath and against the twin's disk_step on
the same step (oracle.disk_step).  tests/disk_blocks.py states the units, the classes and the tables;
tests/test_disk_blocks_host.py derives every K on the CPU.  A device block is held to 2 K against longdouble and to 3 K
where it meets the oracle directly.

With LT_DISK_BLOCKS_MEASURE=path the figures the tests print are also written there as JSON (profiles/disk_blocks_<build id>.json).
"""
import os

import numpy as np
import pytest

import disk_blocks as dk
import ltrace
import step_blocks as sb
from oracle import oracle

pytestmark = pytest.mark.gpu

MEASURE = os.environ.get("LT_DISK_BLOCKS_MEASURE")
_RECORD = {}
KERR = ltrace.METRIC_KERR
INTEGRATORS = {"rk4_f32": (ltrace.INTEGRATOR_RK4, 32, False), "rk4_f64": (ltrace.INTEGRATOR_RK4, 64, False),
               "dp45_exact": (ltrace.INTEGRATOR_DP45_EXACT, 64, True)}


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


def metric(c):
    return ltrace.Metric(KERR, 0, c["M"], c["a"])


def classes(precision, names=dk.CROSSING_CLASSES):
    for a in dk.SPINS:
        for name in names:
            c = dk.crossing_class(name, a, precision)
            if c is not None:
                yield a, name, c


def crossing(c, precision, y0=None, y1=None, sel=slice(None)):
    return ltrace.disk_crossing_probe(metric(c), (c["y0"] if y0 is None else y0)[sel], (c["y1"] if y1 is None else y1)[sel], c["L"][sel],
                                      c["h"][sel], c["t_end"][sel], r_in=c["r_in_arg"], r_out=c["r_out"], precision=precision)


# ---- 1. disk_crossing against longdouble ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_crossing_against_longdouble(precision):
    hp = float(dk.as_t(np.pi / 2, precision))
    worst_t = worst_h = 0.0
    per_class = {}
    for a, name, c in classes(precision):
        ref, keep = c["ref"], c["keep"]
        d = crossing(c, precision)
        crossed = ~np.isnan(d["tau"])
        assert not d["found"][~crossed].any()
        assert (d["hit"][crossed, 1] == hp).all()                                  # theta of a crossing state: pi/2 exactly, in T
        hits = d["found"]
        assert ((d["hit"][hits, 0] >= c["r_in"]) & (d["hit"][hits, 0] <= c["r_out_t"])).all()  # no hit outside [r_in, r_out]
        if name == "nan":
            # IEEE semantics and nothing else: a NaN polar angle never crosses, a NaN crossing radius is never a hit
            bad_th = np.isnan(c["y0"][:, 1]) | np.isnan(c["y1"][:, 1])
            assert not crossed[bad_th].any() and not d["found"][np.isnan(d["hit"][:, 0])].any()
            continue
        if name == "still":
            assert not crossed.any()
            continue
        # (the rows +-1, 2, 8 ulp from an edge: most are not stable -- what the class is for; those that are, are held like any)
        assert np.array_equal(crossed[keep], ref["cross"][keep]), (a, name, np.nonzero(keep & (crossed != ref["cross"]))[0][:8])
        assert np.array_equal(d["found"][keep], ref["found"][keep]), (a, name, np.nonzero(keep & (d["found"] != ref["found"]))[0][:8])
        both = keep & crossed & ref["cross"]
        et = (np.abs(d["tau"].astype(dk.LD) - ref["t"]).astype(np.float64) / ref["unit_t"])[both]
        eh = (np.abs(d["hit"].astype(dk.LD) - ref["hit"]).astype(np.float64) / ref["unit"])[both]
        print(f"float{precision} disk_crossing, a = {a:6}, {name:12s}: {int(both.sum())} crossings; root {et.max():.2f} units, "
              f"state {np.round(eh.max(axis=0), 2)} units")
        per_class[f"{a}/{name}"] = [float(et.max()), float(eh.max())]
        j = np.nonzero(both)[0][int(np.argmax(et))]
        assert et.max() <= 2 * dk.k_root(precision), (a, name, et.max(), int(j), d["tau"][j], float(ref["t"][j]), ref["unit_t"][j], c["y0"][j].tolist(),
                                                      c["y1"][j].tolist(), float(c["L"][j]), float(c["h"][j]), d["hit"][j].tolist())
        assert eh.max() <= 2 * dk.k_hit(precision), (a, name, eh.max(axis=0))
        worst_t, worst_h = max(worst_t, et.max()), max(worst_h, eh.max())
    print(f"float{precision} disk_crossing: root {worst_t:.2f} units (bound {2 * dk.k_root(precision)}), state {worst_h:.2f} units "
          f"(bound {2 * dk.k_hit(precision)})")
    record(f"crossing_f{precision}", dict(root=worst_t, state=worst_h, per_class=per_class))


@pytest.mark.parametrize("precision", [64, 32])
def test_a_state_on_the_plane_is_counted_once_over_two_steps(precision):
    """As tests/test_disk_blocks_host.py, by the device: a -> b -> c with theta_b on the plane or one ulp beside it."""
    hp = float(dk.as_t(np.pi / 2, precision))
    for a in dk.SPINS:
        c = dk.crossing_class("on_plane", a, precision)
        sel = (np.arange(dk.N) % 2) == 1
        ya, yb = c["y0"], c["y1"]
        yc = dk.as_t(dk._step(c["M"], c["a"], yb, c["L"], c["h"], precision), precision)
        first = ~np.isnan(crossing(c, precision, ya, yb, sel)["tau"])
        second = ~np.isnan(crossing(c, precision, yb, yc, sel)["tau"])
        r1 = dk.crossing_longdouble(c["M"], c["a"], ya[sel], yb[sel], c["L"][sel], c["h"][sel], 1.0, c["r_in"], c["r_out_t"], precision)["cross"]
        r2 = dk.crossing_longdouble(c["M"], c["a"], yb[sel], yc[sel], c["L"][sel], c["h"][sel], 1.0, c["r_in"], c["r_out_t"], precision)["cross"]
        assert np.array_equal(first, r1) and np.array_equal(second, r2)
        opposite = (ya[sel, 1] - hp) * (yc[sel, 1] - hp) < 0
        assert ((first.astype(int) + second.astype(int))[opposite] == 1).all()
        on = yb[sel, 1] == hp
        assert first[on].all() and not second[on].any()
        # ... and a START on the plane (the other half of the class) never crosses, whatever the end
        start_on = ~sel & (c["y0"][:, 1] == hp)
        assert start_on.sum() > 50 and np.isnan(crossing(c, precision, sel=start_on)["tau"]).all()


@pytest.mark.parametrize("precision", [64, 32])
def test_both_edges_belong_to_the_annulus(precision):
    """r_in <= r <= r_out (ltrace.h).  A step that stays at one radius with p_r = 0 at both ends has a cubic in r that is that
    radius in every bit (the three other terms are exact zeros), so the crossing radius can be put ON an edge: found there, not
    found one ulp outside."""
    t = np.float32 if precision == 32 else np.float64
    for a in (0.0, 0.9, -0.7):
        r_in, r_out = t(dk.isco(1.0, a)), t(20.0)
        radii = np.array([np.nextafter(r_in, t(0)), r_in, np.nextafter(r_in, t(99)), np.nextafter(r_out, t(0)), r_out,
                          np.nextafter(r_out, t(99))], dtype=np.float64)
        want = np.array([False, True, True, True, True, False])
        n = radii.size
        y0 = np.stack([radii, np.full(n, 1.5), np.zeros(n), np.zeros(n), np.full(n, 3.0)], axis=1)
        y1 = y0.copy()
        y1[:, 1] = 1.64
        for flip in (False, True):
            d = ltrace.disk_crossing_probe(ltrace.Metric(KERR, 0, 1.0, a), y1 if flip else y0, y0 if flip else y1, 2.0, 0.5, 1.0,
                                           r_in=0.0, r_out=20.0, precision=precision)
            assert np.array_equal(d["hit"][:, 0], radii) and np.array_equal(d["found"], want), (a, flip, d["found"], d["hit"][:, 0])


def test_hermite_at_the_end_of_the_step_is_the_end_state():
    """hermite() forms y0 + (y1 - y0) at t = 1.  For theta0 >= theta1 / 2 the difference is exact (Sterbenz) and the sum is
    y1, so the cubic's sign at t_end = 1 is that of the sign test which made the lane a candidate: an end state ON the plane is
    found as a crossing with root 1, on every row of the class.  Outside that premise -- a step that more than doubles theta,
    0.79 rad and more in one step -- the sum can miss y1 by an ulp; the step-size rule keeps every step of a tracer far from that
    (the rows of every class here turn theta by less than 0.5 rad)."""
    for precision in (64, 32):
        hp = float(dk.as_t(np.pi / 2, precision))
        for a in dk.SPINS:
            c = dk.crossing_class("on_plane", a, precision)
            sel = (c["y1"][:, 1] == hp) & (c["y0"][:, 1] != hp)
            assert sel.sum() > 50 and (c["y0"][sel, 1] >= hp / 2).all()
            d = crossing(c, precision, sel=sel)
            assert (d["tau"] == 1.0).all(), d["tau"][d["tau"] != 1.0][:8]
            assert np.array_equal(d["hit"][:, 0], c["y1"][sel, 0])


# ---- 2. disk_advance against the twin's disk_step on the same step --------------------------------------------------------------
_ADV = {}


def advance(kind, a, name):
    """(class, oracle side, device disk_advance, device Integ::advance alone) of one class -- computed once, never changed."""
    key = (kind, a, name)
    if key not in _ADV:
        integ, precision, dp45 = INTEGRATORS[kind]
        c = dk.dp45_capture_class() if name == "dp45_capture" else dk.crossing_class(name, a, precision)
        if c is None:
            _ADV[key] = None
            return None
        o = dk.advance_oracle(c, precision, dp45)
        kw = dict(r_obs=c["r_obs"], lambda_max=dk.LAMBDA_MAX)
        d = ltrace.disk_advance_probe(metric(c), c["y0"], c["L"], integ, precision, h=o["h"] if dp45 else 0.0, r_in=c["r_in_arg"],
                                      r_out=c["r_out"], h_max=1.0, **kw)
        if dp45:
            p = ltrace.dp45_advance_probe(c["M"], c["a"], c["y0"], c["L"], o["h"], exact=True, **kw)
        else:
            p = ltrace.rk4_advance_probe(c["M"], c["a"], c["y0"], c["L"], precision=precision, h_max=1.0, **kw)
        _ADV[key] = (c, o, d, p)
    return _ADV[key]


def advance_sets(kind):
    for a in dk.SPINS:
        for name in dk.ADVANCE_CLASSES:
            s = advance(kind, a, name)
            if s is not None:
                yield a, name, s
    if kind == "dp45_exact":  # the capture steps of DP45 that are candidates of the disk test exist at a = M only (disk_blocks.py)
        yield dk.DP45_CAPTURE_SPIN, "dp45_capture", advance(kind, dk.DP45_CAPTURE_SPIN, "dp45_capture")


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_advance_against_the_twin_on_the_same_step(kind):
    _, precision, dp45 = INTEGRATORS[kind]
    worst = np.zeros(3)
    hits = misses = terminal_rows = term_hits = 0
    for a, name, (c, o, d, p) in advance_sets(kind):
        st, ref, ok = o["step"], o["ref"], o["stable"]
        assert ok.mean() > 0.94, (a, name, ok.mean())  # (what is left out: RK4 iterations that retried or failed, beside r_cut)
        # the event; a hit iff the twin's is_hit (the twin has no pre-filter: this pins `near`)
        want_ev = np.where(st["is_hit"], ltrace.EV_DISK, o["event"])
        bad = np.nonzero(ok & ((d["is_hit"] != st["is_hit"]) | (d["event"] != want_ev)))[0]
        assert bad.size == 0, (kind, a, name, bad[:8], d["event"][bad[:8]], want_ev[bad[:8]], c["y0"][bad[:1]], c["L"][bad[:1]])
        both = ok & d["is_hit"] & st["is_hit"]
        hits += int(both.sum())
        misses += int((ok & ~st["is_hit"] & st["cross"]).sum())
        terminal_rows += int((ok & (o["terminal"] != 0)).sum())
        if not both.any():
            continue
        # the hit and the root against the twin on THE SAME step: the one the device reports (on.y1, on.h; for a step that
        # ended a DP45 ray the retaken RK4 step), cut where that step's chord in r meets the terminal radius
        t = np.float32 if precision == 32 else np.float64
        r0, r1 = c["y0"][:, 0].astype(t), d["on_y1"][:, 0].astype(t)
        target = np.where(o["terminal"] < 0, t(t(dk.r_plus(c["M"], c["a"])) * t(1.01)) if precision == 32 else 1.01 * dk.r_plus(c["M"], c["a"]),
                          t(2.0 * c["r_obs"])).astype(t)
        with np.errstate(all="ignore"):
            cut = np.where(o["terminal"] == 0, 1.0, np.clip((target - r0) / (r1 - r0), 0, 1).astype(np.float64))
        own = oracle.disk_step(c["y0"][both], d["on_y1"][both], c["L"][both], d["on_h"][both], c["M"], c["a"], c["r_in"], c["r_out_t"],
                               terminal=o["terminal"][both], frac=cut[both], r_obs=c["r_obs"], f32=precision == 32)
        lng = dk.crossing_longdouble(c["M"], c["a"], c["y0"][both], d["on_y1"][both], c["L"][both], d["on_h"][both], cut[both],
                                     c["r_in"], c["r_out_t"], precision)  # (for the units)
        assert own["is_hit"].all(), (kind, a, name, np.nonzero(~own["is_hit"])[0][:8])
        e = np.abs(d["hit"][both] - own["state"]) / lng["unit"] / (3 * dk.k_hit(precision))
        et = np.abs(d["on_tau"][both] - own["t"]) / lng["unit_t"] / (3 * dk.k_root(precision))
        assert e.max() <= 1.0 and et.max() <= 1.0, (kind, a, name, e.max(axis=0), et.max())
        # the step the hit lies on: its length is the twin's; its end is the device's own step in every bit, which lies
        # within 2 K_STEP units of the twin's step -- outside 1.3 r_plus, inside which the reference's
        # right-hand side loses the digits the kernel's keeps (step_blocks.py: 176 units at a = 0.998)
        assert np.array_equal(d["on_h"][both], dk.as_t(o["h"], precision)[both])
        plain = both & (o["terminal"] == 0)
        assert np.array_equal(d["on_y1"][plain], p["state"][plain])
        # ... and on a step that ended the ray it is the checked RK4 step of that length from the state before (for DP45 the
        # stand-in for its own end state, which is gone), in every bit
        ended = both & (o["terminal"] != 0)
        if ended.any():
            retaken = ltrace.kerr_step_probe(c["M"], c["a"], c["y0"][ended], c["L"][ended], d["on_h"][ended], precision=precision, form="checked")
            assert np.array_equal(d["on_y1"][ended], retaken["states"]), (kind, a, name)
        far = both & (np.minimum(c["y0"][:, 0], o["y1"][:, 0]) >= 1.3 * dk.r_plus(c["M"], c["a"]))
        slack = 2 * sb.K_STEP * o["unit_step"]
        ey = (np.abs(d["on_y1"] - st["y1"]) / np.where(slack > 0, slack, np.inf))[far]
        assert ey.size == 0 or ey.max() <= 1.0, (kind, a, name, ey.max(axis=0))
        term_hits += int((both & (o["terminal"] != 0)).sum())
        worst = np.maximum(worst, [e.max(), et.max(), ey.max() if ey.size else 0.0])
    print(f"{kind}: {hits} hits and {misses} crossings outside the annulus or after the cut on stable rows, {terminal_rows} of them on steps "
          f"that ended the ray, {term_hits} of the hits on such steps; hit state {worst[0]:.3f} of 3 K_hit, root {worst[1]:.3f} of 3 K_root, step end {worst[2]:.3f} of 2 K_step")
    record(f"advance_{kind}", dict(hits=hits, misses=misses, terminal_rows=terminal_rows, terminal_hits=term_hits, hit=worst[0], root=worst[1], step_end=worst[2]))
    assert hits > 4000 and misses > 500 and terminal_rows > 100 and term_hits >= 30


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_the_disk_test_changes_no_bit_of_a_step(kind):
    """"Nothing here changes a step": every row, hit or not, ends with the bits of Integ::advance alone -- state, lam, h /
    h_retry, steps -- and a row that did not hit with its event as well."""
    rows = 0
    for a, name, (c, o, d, p) in advance_sets(kind):
        for k in ("state", "lam", "steps"):
            assert np.array_equal(d[k], p[k], equal_nan=True), (kind, a, name, k)
        assert np.array_equal(d["h"], p["h" if kind == "dp45_exact" else "h_retry"], equal_nan=True)
        assert np.array_equal(d["event"][~d["is_hit"]], p["event"][~d["is_hit"]])
        assert (d["event"][d["is_hit"]] == ltrace.EV_DISK).all()
        assert np.isnan(d["hit"][~d["is_hit"]]).all() and np.isnan(d["on_h"][~d["is_hit"]]).all()
        rows += d["event"].size
    assert rows > 10000


@pytest.mark.parametrize("kind", list(INTEGRATORS))
def test_a_lane_does_not_depend_on_its_wavefront(kind):
    """The same row alone, as lane 37 among 63 lanes that are no candidates, and among 63 candidates: every bit equal.  Also a
    row that is no candidate, among candidates; and `act` = 0, which only keeps on_hit from running."""
    integ, precision, dp45 = INTEGRATORS[kind]
    c, o, d, p = advance(kind, 0.9, "ordinary")
    hit_rows = np.nonzero(d["is_hit"])[0]
    miss_rows = np.nonzero(~o["step"]["cross"] | ~d["is_hit"])[0]
    # lanes that are no candidates: the class's own states moved far above the plane (theta = 1, no sign change in a step)
    quiet = c["y0"].copy()
    quiet[:, 1] = 1.0
    assert hit_rows.size > 64

    hs = o["h"] if dp45 else c["h"]

    def run(y0, L, h, act=True):
        return ltrace.disk_advance_probe(metric(c), y0, L, integ, precision, h=h if dp45 else 0.0, act=act, r_in=c["r_in_arg"],
                                         r_out=c["r_out"], h_max=1.0, r_obs=c["r_obs"], lambda_max=dk.LAMBDA_MAX)

    keys = ("event", "steps", "is_hit", "state", "lam", "h", "hit", "on_y1", "on_h", "on_tau")
    for row in (int(hit_rows[3]), int(hit_rows[-1]), int(miss_rows[0])):
        alone = run(c["y0"][row:row + 1], c["L"][row:row + 1], hs[row:row + 1])
        for others, oL, oh in ((quiet[:63], c["L"][:63], hs[:63]), (c["y0"][hit_rows[5:68]], c["L"][hit_rows[5:68]], hs[hit_rows[5:68]])):
            y0 = np.insert(others, 37, c["y0"][row], axis=0)
            L = np.insert(oL, 37, c["L"][row])
            h = np.insert(oh, 37, hs[row])
            got = run(y0, L, h)
            for k in keys:
                assert np.array_equal(got[k][37:38], alone[k], equal_nan=True), (kind, row, k)
                assert np.array_equal(alone[k][0], d[k][row], equal_nan=True), (kind, row, k)
    quiet_run = run(quiet[:64], c["L"][:64], hs[:64])
    assert not quiet_run["is_hit"].any() and np.isnan(quiet_run["on_tau"]).all()  # no candidate in the wave: the branch is not taken
    off = run(c["y0"], c["L"], hs, act=np.arange(dk.N) % 2 == 0)
    odd = np.arange(dk.N) % 2 == 1
    assert not off["is_hit"][odd].any() and np.array_equal(off["event"][odd], p["event"][odd]) and np.isnan(off["hit"][odd]).all()
    for k in keys:
        assert np.array_equal(off[k][~odd], d[k][~odd], equal_nan=True), k
    assert np.array_equal(off["on_tau"], d["on_tau"], equal_nan=True)  # (the root is written wherever the search ran)


# ---- 3. the closed forms ------------------------------------------------------------------------------------------------------------
def test_redshift_wrap_and_half_orbits_tables():
    worst = 0.0
    for tb in dk.g_table():
        got = ltrace.disk_shade_probe(ltrace.Metric(KERR, 0, tb["M"], tb["a"]), tb["r"], 0.0, tb["xi"])["g"]
        e = np.abs(got - tb["g"]) / tb["unit"]
        i = int(np.argmax(e))
        print(f"g, M = {tb['M']}, a = {tb['a']:7.4f}: max {e[i]:.2f} units at r = {tb['r'][i]!r}, xi = {tb['xi'][i]!r} (relative {abs(got[i] - tb['g'][i]) / tb['g'][i]:.2e})")
        assert e[i] <= 2 * dk.K_G, (tb["M"], tb["a"], tb["r"][i], tb["xi"][i], e[i])
        worst = max(worst, float(e[i]))
    tb = dk.phi_table()
    phi = np.concatenate([tb["phi"], [np.nan]])
    d = ltrace.disk_shade_probe(ltrace.Metric(KERR, 0, 1.0, 0.9), np.full(phi.size, 10.0), phi, 0.0)
    w, half = d["phi"][:-1], d["half_orbits"][:-1]
    assert ((w >= 0) & (w < 2 * np.pi)).all()                # [0, 2 pi) on every row
    ew = dk.circle_distance(w, tb["wrapped"]) / tb["unit"]
    assert ew.max() <= 2 * dk.K_WRAP, (tb["phi"][np.argmax(ew)], ew.max())
    # the contract of the guard: an angle a rounding below 0 is returned as 0 (its neighbour on the circle), never as 2 pi
    assert w[tb["phi"] == -1e-17][0] == 0.0 and w[tb["phi"] == 1e-17][0] == 1e-17 and not np.signbit(w[tb["phi"] == 0.0]).any()
    assert np.isnan(d["phi"][-1]) and d["half_orbits"][-1] == 0      # NaN: never a hit's angle; it stays NaN, and counts no orbit
    exact = ~tb["near"]
    assert np.array_equal(half[exact], tb["half"][exact])
    off = half[tb["near"]] - tb["half"][tb["near"]]
    print(f"wrap_2pi: max {ew.max():.2f} units; half_orbits: exact on {int(exact.sum())} rows; {int(tb['near'].sum())} rows within the unit of "
          f"a multiple of pi, where the device counts {int((off == 0).sum())} as mpmath, {int((off == -1).sum())} one less, {int((off == 1).sum())} one more")
    # the device counts in multiples of the float64 pi, which lies 1.2e-16 BELOW pi: where |phi| reaches k pi it has reached
    # k times that value too, so beside a multiple of pi the device's count is mpmath's or one more, never one less
    assert np.isin(off, (0, 1)).all()
    record("closed_forms", dict(g=worst, wrap=float(ew.max()), half_near=int(tb["near"].sum()), half_off=int((off != 0).sum())))


def test_emission_and_colour_tables():
    worst, unsure, n = 0.0, 0, 0
    for M, a in ((1.0, 0.9), (2.5, -1.75)):
        for q, ex in dk.SHADE_CASES:
            tb = dk.shade_table(M, a, q, ex)
            E, unit = dk.emission_longdouble(tb["r"], tb["g"], tb["r_in"], q, ex)
            d = ltrace.disk_shade_probe(ltrace.Metric(KERR, 0, M, a), tb["r"], 0.0, 0.0, g=tb["g"], q=q, exposure=ex)
            with np.errstate(invalid="ignore", divide="ignore"):
                e = np.where(unit > 0, np.abs(d["emission"].astype(dk.LD) - E).astype(np.float64) / unit, 0.0)
            assert (d["emission"][unit == 0] == 0).all()
            flat = (E == E[:, 2:3]) & (unit > 0)  # the ramp is 1 in every channel: the emission is I alone
            i = np.unravel_index(np.argmax(e), e.shape)
            print(f"emission, M = {M}, a = {a}, q = {q}, exposure = {ex}: max {e.max():.2f} units at r = {tb['r'][i[0]]!r}, g = {tb['g'][i[0]]!r}, channel {i[1]} "
                  f"(device {d['emission'][i]!r}, longdouble {float(E[i])!r}); where the ramp is 1: {e[flat].max() if flat.any() else 0:.2f}")
            assert e.max() <= dk.emission_bound(q), (M, a, q, ex, e.max(axis=0))
            worst = max(worst, float(e.max()))
            rgb, sure3, mean, sure1 = dk.shade_expected(E, dk.emission_bound(q) * unit)
            assert np.array_equal(d["shade3"][sure3], rgb[sure3]) and np.array_equal(d["shade1"][sure1], mean[sure1])
            assert ((d["shade3"] >= 0) & (d["shade3"] <= 1)).all() and ((d["shade1"] >= 0) & (d["shade1"] <= 1)).all()
            unsure += int((~sure3).sum()) + int((~sure1).sum())
            n += sure3.size + sure1.size
    print(f"emission: max {worst:.2f} units; colour: bit-equal to the rounded longdouble value on {n - unsure} of {n}")
    assert unsure < 0.04 * n  # (a third of the table sits on a knee, where a ramp of 0 +- the bound is 0 or a denormal-sized colour)
    record("emission", dict(emission=worst, colours=n, unsure=unsure))
