"""The reverberation response on the CPU: the delay grid's bin rule, the numpy statement of the rule (disk.disk_transfer)
against a restatement written from the header's words, the exact cases, the closures, the lamp-post tables, the struct, the
bindings and the command line.  tests/test_gpu_transfer.py holds the kernel to the same restatement with the same bound; the
cases, records, tables, grids and the restatement are here.

The restatement (restate_slots, restate).  Steps 1 to 4 decide a slot's bins and are IEEE-exact float64 operations, so the
restatement takes them in float64 too, written again from the header: the comparisons, v as a subtraction and a product,
the index, w, and the two interpolations by fma_ref -- an fma of its own, the product and the sum in longdouble (64-bit
significand) rounded to float64, and wherever that double rounding could differ from a single one (the longdouble sum
within its own error of a midpoint between two doubles) the exact value by rational arithmetic.  The bins must therefore
agree exactly.  The weight and every sum are longdouble: exposure g^4 eps with one rounding each.

The bound, derived.  A float64 weight carries four roundings (g g, its square, the product with exposure, the product with
eps), each half an ulp: 2 2^-53 of itself, taken as 4; the restatement's own longdouble roundings are below 2^-62.  A sum of
n non-negative terms in any order adds at most (n - 1) 2^-53 of itself; the final stage's order is covered by the same
count.  Per key:  |S - S_ref| <= (n + 6) 2^-53 sum|w|.

The lamp-post tables' flat limit.  At h = 1000 M and r from 1000 to 3000 M space is flat to M / h: the delay is the
straight-line distance sqrt(r^2 + h^2) and eps (r^2 + h^2)^(3/2) is constant (the inverse-square law times the cosine of
incidence), each to the leading relativistic correction's order, a relative 10 M / h = 1e-2.
MEASURED here: delay within 1.4e-3 of the straight line (the Shapiro delay), eps (r^2 + h^2)^(3/2) constant to 2.3e-3, t_ref
within 7.1e-4 of the straight line; between theta0 = 1e-3 and 1e-4 the delays at h = 6, a = 0.9 move by 6.7e-3 -- the source
sits h theta0 off the axis -- against an interpolation error of 2.3e-2 on 64 nodes, the emissivities by 2.4e-5 against 6.7e-4.
The rays hold the Carter constant to 3e-12 of its scale and the null condition to 8e-11 of its largest term at rtol 1e-10.
The numpy statement lies within 0.31 of the restatement's bound on every case (0.009 on the single pixel).
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import disk as diskmod
import ltrace
from test_diskmap_host import CASES
from test_hotspot_records_host import synth
from test_thermal_host import thermal_records

LD = np.longdouble
U = LD(2.0) ** -53
EXPOSURE, T_REF, H_SRC = 0.25, 60.0, 6.0
G_LO, G_HI = 0.3, 1.2                  # inside the records' g of 0.15 ... 1.4: both of g's outer columns hold light
TAU_LO, TAU_HI = -16.0, 240.0          # inside the records' delays of about -27 ... 360: so do both outer rows
_RECORDS, _SLOTS = {}, {}


# ---- cases: records, tables, grids ------------------------------------------------------------------------------------------------
def transfer_records(name):
    """(hits, n_hits) of a case of test_diskmap_host: test_thermal_host's copy, in which about one stored slot in 16 has a g
    that contributes nothing (0, negative, NaN), with the dt of another one in 16 set to NaN.  Made once."""
    if name not in _RECORDS:
        hits, n_hits = thermal_records(name)
        hits = hits.copy()
        pick = np.random.default_rng(CASES[name].seed + 11).random(hits.shape[:3]) < (1 / 16 if hits.size > 4 else 0)
        hits[..., 3][pick] = np.nan
        _RECORDS[name] = (hits, n_hits)
    return _RECORDS[name]


def make_tables(name, n_r=37):
    """(r_min, r_max, delay, emis) of a case: a flat-space lamp post at H_SRC on n_r nodes over a range strictly inside the
    records' [r_isco, r_out], so that slots fall off both ends; the emissivity's nodes 9 ... 13 are 0 with one negative among
    them -- a stretch that re-emits nothing -- and one node of the delay is NaN."""
    c = CASES[name]
    lo, hi = float(diskmod.isco(c.M, c.a)) + 0.5 * c.M, c.r_out - 3.0 * c.M
    nodes = lo + np.arange(n_r) * (hi - lo) / (n_r - 1)
    delay = np.sqrt(nodes * nodes + H_SRC * H_SRC)
    emis = 100.0 * H_SRC / (nodes * nodes + H_SRC * H_SRC) ** 1.5
    emis[9:14] = 0.0
    emis[10] = -0.25
    delay[30] = np.nan
    return lo, hi, delay, emis


def grids(n_tau, n_bins, split=False):
    return diskmod.Spectrum(G_LO, G_HI, n_bins, split_orders=split), diskmod.TransferGrid(TAU_LO, TAU_HI, n_tau)


def statement(name, spec, grid, counts=True, **kw):
    hits, n_hits = transfer_records(name)
    r_min, r_max, delay, emis = make_tables(name)
    args = dict(hits=hits, n_hits=n_hits if counts else None, exposure=EXPOSURE, spec=spec, grid=grid, r_min=r_min, r_max=r_max, delay=delay,
                emis=emis, t_ref=T_REF)
    args.update(kw)
    return diskmod.disk_transfer(**args)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def fma_ref(a, b, c):
    """round(a b + c), one rounding, float64 (header above): longdouble, and exact rationals where that could differ."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(LD) * b.astype(LD)
        s = p + c.astype(LD)
        r = s.astype(np.float64)
        if np.finfo(LD).nmant >= 63:
            err = LD(2.0) ** -62 * (np.abs(p) + np.abs(s))
            doubt = np.zeros(r.shape, dtype=bool)
            for side in (np.inf, -np.inf):
                mid = (r.astype(LD) + np.nextafter(r, side).astype(LD)) / 2
                doubt |= np.abs(s - mid) <= err
            doubt &= np.isfinite(r)
        else:
            doubt = np.isfinite(r)
    r = r.copy()
    for i in np.flatnonzero(doubt):
        r.flat[i] = float(Fraction(float(a.flat[i])) * Fraction(float(b.flat[i])) + Fraction(float(c.flat[i])))
    return r


def bin_ref(x, lo, hi, n):
    """The header's bin rule on a float64 array without NaN: 0 below lo, n + 1 from hi on, else 1 + min(floor((x - lo) n / (hi - lo)), n - 1)."""
    inv = n / (hi - lo)
    inside = np.clip(x, lo, hi)
    k = 1 + np.minimum(np.floor((inside - lo) * inv).astype(np.int64), n - 1)
    return np.where(x < lo, 0, np.where(x >= hi, n + 1, k))


def restate_slots(hits, n_hits, exposure, r_min, r_max, delay, emis, t_ref):
    """Steps 1 to 5 from the header's words -> (on, tau float64, g float64, weight longdouble), each (..., max_images)."""
    h32 = np.asarray(hits, dtype=np.float32)
    m = h32.shape[-2]
    r, g, dt = (h32[..., i].astype(np.float64) for i in (0, 2, 3))
    stored = np.cumprod(~np.isnan(h32[..., 0]), axis=-1).sum(axis=-1) if n_hits is None else np.minimum(np.asarray(n_hits, dtype=np.int64), m)
    n_r = len(delay)
    with np.errstate(invalid="ignore"):
        on = (stored[..., None] > np.arange(m)) & (g > 0) & ~np.isnan(dt) & (r >= r_min) & (r <= r_max)
        inv_dr = (n_r - 1) / (r_max - r_min)
        v = (np.where(on, r, r_min) - r_min) * inv_dr
        i0 = np.minimum(v.astype(np.int64), n_r - 2)
        w = v - i0
        eps = fma_ref(w, emis[i0 + 1] - emis[i0], emis[i0])
        on = on & (eps > 0)
        t_ld = fma_ref(w, delay[i0 + 1] - delay[i0], delay[i0])
        tau = (t_ld + np.where(on, dt, 0.0)) - t_ref
        on = on & ~np.isnan(tau)
        weight = LD(exposure) * np.where(on, g, 0.0).astype(LD) ** 4 * np.where(on, eps, 0.0).astype(LD)
    return on, tau, g, weight


def slots_of(name, counts=True):
    """restate_slots of a case's records and tables, made once."""
    if (name, counts) not in _SLOTS:
        hits, n_hits = transfer_records(name)
        _SLOTS[name, counts] = restate_slots(hits, n_hits if counts else None, EXPOSURE, *make_tables(name), T_REF)
    return _SLOTS[name, counts]


def restate(slots, spec, grid):
    """-> (value, bound, terms), each (planes, n_tau + 2, n_bins + 2): the longdouble sums, (n + 6) 2^-53 sum|w| and n."""
    on, tau, g, weight = slots
    m = on.shape[-1]
    rows, cols, planes = grid.n_tau + 2, spec.n_bins + 2, m if spec.split_orders else 1
    plane = np.broadcast_to(np.arange(m), on.shape) if spec.split_orders else np.zeros(on.shape, dtype=np.int64)
    k_tau = bin_ref(np.where(on, tau, 0.0), grid.tau_min, grid.tau_max, grid.n_tau)
    k_g = bin_ref(np.where(on, g, 1.0), spec.g_min, spec.g_max, spec.n_bins)
    key = ((plane * rows + k_tau) * cols + k_g)[on]
    value = np.zeros(planes * rows * cols, dtype=LD)
    np.add.at(value, key, weight[on])
    terms = np.bincount(key, minlength=value.size)
    shape = (planes, rows, cols)
    return value.reshape(shape), ((terms + 6) * U * value).reshape(shape), terms.reshape(shape)


def check(got, slots, spec, grid, what=""):
    """got against the restatement: the same keys hold light, every key within its bound -> the largest difference in units
    of its bound."""
    want, bound, terms = restate(slots, spec, grid)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert not np.any(np.isnan(got)) and not np.any(np.signbit(got)), what
    assert np.array_equal(got != 0.0, terms > 0), what                    # the bins agree exactly: no light in a key without a term
    d = np.abs(got.astype(LD) - want)
    q = float(np.max(np.where(terms > 0, d / np.where(terms > 0, bound, LD(1)), LD(0))))
    print(f"{what}: {int((terms > 0).sum())} of {terms.size} keys hold light, {int(terms.sum())} terms; largest difference {q:.3f} of its bound")
    assert q <= 1, what
    return q


# ---- 1. the bin rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi,n", [(0.0, 256.0, 64), (-16.0, 240.0, 126), (-7.3, 11.9, 13), (3.0, 3.5, 1), (-1e3, -10.0, 1024)])
def test_bin_rule_at_every_edge(lo, hi, n):
    grid = diskmod.TransferGrid(lo, hi, n)
    e = grid.edges()
    assert e.shape == (n + 1,) and e[0] == lo and e[-1] == hi and np.all(np.diff(e) > 0)
    assert np.array_equal(diskmod.transfer_bin([lo, np.nextafter(lo, -np.inf), hi, np.nextafter(hi, -np.inf), -np.inf, np.inf, np.nan, -1e300, 1e300], grid),
                          [1, 0, n + 1, n, 0, n + 1, -1, 0, n + 1])
    inv = n / (hi - lo)
    for x in (e[1:-1], np.nextafter(e[1:-1], -np.inf), np.nextafter(e[1:-1], np.inf), 0.5 * (e[:-1] + e[1:])):
        k = diskmod.transfer_bin(x, grid)
        assert np.array_equal(k, 1 + np.minimum(np.floor((x - lo) * inv), n - 1))    # the rule itself, whatever the edge's rounding
        assert np.all((k >= 1) & (k <= n))
    mid = diskmod.transfer_bin(0.5 * (e[:-1] + e[1:]), grid)
    assert np.array_equal(mid, np.arange(1, n + 1))
    if (hi - lo) / n == 2.0 ** round(np.log2((hi - lo) / n)):             # exact edges: on, just below and just above each
        assert np.array_equal(diskmod.transfer_bin(e[:-1], grid), np.arange(1, n + 1))
        assert np.array_equal(diskmod.transfer_bin(np.nextafter(e[1:], -np.inf), grid), np.arange(1, n + 1))
        assert np.array_equal(diskmod.transfer_bin(np.nextafter(e[:-1], np.inf), grid), np.arange(1, n + 1))
    for bad in (dict(tau_min=1.0, tau_max=1.0), dict(tau_max=np.inf), dict(tau_min=np.nan), dict(n_tau=0), dict(n_tau=1025), dict(n_tau=2.5)):
        with pytest.raises(ValueError):
            diskmod.TransferGrid(**{**dict(tau_min=0.0, tau_max=8.0, n_tau=4), **bad})


@pytest.mark.parametrize("lo,below", [(0.0, True), (-16.0, False)])
def test_adjacent_grids_tile_the_spanning_grid(lo, below):
    """Two parts that share inv_dtau = 1 / 4 give every tau the bin the whole gives it, wherever tau - tau_min is exact: always
    with tau_min = 0 (and the right part's tau - 32 for tau >= 32), so there the delays one ulp below every edge are tried
    too.  With tau_min = -16 the sum tau + 16 of a tau one ulp below an interior edge rounds up to the edge, and the whole
    grid, which has no clamp there, puts it one bin up: the header says so, and that one delay per edge is left out."""
    mid, hi = lo + 32.0, lo + 64.0
    whole, left, right = diskmod.TransferGrid(lo, hi, 16), diskmod.TransferGrid(lo, mid, 8), diskmod.TransferGrid(mid, hi, 8)
    assert whole.n_tau / (whole.tau_max - whole.tau_min) == left.n_tau / (left.tau_max - left.tau_min) == right.n_tau / (right.tau_max - right.tau_min) == 0.25
    rng = np.random.default_rng(5)
    e = whole.edges()
    tau = np.concatenate([rng.uniform(lo - 24.0, hi + 22.0, 20000), e, np.nextafter(e, np.inf)] + ([np.nextafter(e, -np.inf)] if below else []))
    k, kl, kr = (diskmod.transfer_bin(tau, g) for g in (whole, left, right))
    in_left, in_right = (tau >= lo) & (tau < mid), (tau >= mid) & (tau < hi)
    assert np.array_equal(kl[in_left], k[in_left]) and np.array_equal(kr[in_right] + 8, k[in_right])
    assert np.all(kl[tau >= mid] == 9) and np.all(kr[tau < mid] == 0) and in_left.sum() > 1000 < in_right.sum()
    if not below:
        x = np.nextafter(e[1:-1], -np.inf)
        assert np.all(diskmod.transfer_bin(x, whole) - np.arange(1, 16) == (x - lo == e[1:-1] - lo))    # one bin up exactly where the sum rounds up


# ---- 2. the numpy statement against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_tau,n_bins,split,counts", [("strip", 1, 1, False, True), ("strip", 64, 96, True, False), ("mid", 64, 96, False, True),
                                                            ("mid", 126, 254, False, False), ("big", 62, 62, True, True), ("one", 64, 96, False, True),
                                                            ("one", 1, 1, True, False)])
def test_numpy_statement_against_the_restatement(name, n_tau, n_bins, split, counts):
    spec, grid = grids(n_tau, n_bins, split)
    got = statement(name, spec, grid, counts)
    assert got.shape == (CASES[name].m if split else 1, n_tau + 2, n_bins + 2)
    check(got, slots_of(name, counts), spec, grid, f"{name} {n_tau} x {n_bins}, split {split}, counts {counts}")
    # slot by slot: the same slots contribute, in the same row and column
    hits, n_hits = transfer_records(name)
    on, k_tau, k_g, weight = diskmod.transfer_slots(hits, n_hits if counts else None, EXPOSURE, spec, grid, *make_tables(name), T_REF)
    ron, tau, g, w_ref = slots_of(name, counts)
    assert np.array_equal(on, ron)
    assert np.array_equal(k_tau[on], bin_ref(tau[on], TAU_LO, TAU_HI, n_tau)) and np.array_equal(k_g[on], bin_ref(g[on], G_LO, G_HI, n_bins))
    assert np.all(np.abs(weight[on].astype(LD) - w_ref[on]) <= 4 * U * w_ref[on]) and np.all(weight[~on] == 0.0)


def test_the_records_exercise_every_way_of_contributing_nothing():
    hits, n_hits = transfer_records("mid")
    r_min, r_max, delay, emis = make_tables("mid")
    on, tau, g, _ = slots_of("mid")
    h = hits.astype(np.float64)
    stored = n_hits[..., None] > np.arange(hits.shape[2])
    with np.errstate(invalid="ignore"):
        assert (stored & np.isnan(h[..., 2])).sum() > 100 and (stored & (h[..., 2] <= 0)).sum() > 100 and (stored & np.isnan(h[..., 3])).sum() > 100
        assert (stored & (h[..., 0] < r_min)).sum() > 100 and (stored & (h[..., 0] > r_max)).sum() > 100
        nodes = r_min + np.arange(37) * (r_max - r_min) / 36
        dark = stored & (h[..., 0] > nodes[10]) & (h[..., 0] < nodes[12]) & (h[..., 2] > 0) & ~np.isnan(h[..., 3])
        lost = stored & (h[..., 0] > nodes[29]) & (h[..., 0] < nodes[31]) & (h[..., 2] > 0) & ~np.isnan(h[..., 3])
    assert dark.sum() > 100 and not on[dark].any() and lost.sum() > 100 and not on[lost].any()    # steps 3 and 4
    assert on.sum() > 0.3 * stored.sum() and np.ptp(g[on]) > 1.0 and (tau[on] < TAU_LO).any() and (tau[on] >= TAU_HI).any()
    assert len({j for j in range(hits.shape[2]) if on[..., j].any()}) == hits.shape[2]             # several image orders


def test_fma_ref_is_one_rounding():
    rng = np.random.default_rng(11)
    a, b, c = rng.uniform(-1, 1, (3, 4000))
    c[:2000] = -(a * b)[:2000] * (1 + rng.uniform(-4e-16, 4e-16, 2000))
    c[2000:2400] = (a * b)[2000:2400] * 2.0 ** 53                         # the product decides a tie
    want = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(fma_ref(a, b, c), want) and np.array_equal(diskmod.fma(a, b, c), want)


# ---- 3. exact cases --------------------------------------------------------------------------------------------------------------------
def exact_case(R=23, W=41, m=3, seed=3):
    """Records and tables on which every operation of the rule is exact: nodes at the integers 4 ... 20, delay = 2 r, emis = 1,
    r in eighths, g in {0.5, 1, 2}, dt in quarters, exposure and t_ref powers of two -> (hits, n_hits, tables, tau, exposure, t_ref);
    a slot's weight is exposure g^4 and its delay 2 r + dt - t_ref, both without rounding."""
    rng = np.random.default_rng(seed)
    hits, n_hits = synth(R, W, m, seed, 4.0, 20.0)
    hits[..., 0] = rng.integers(24, 168, hits.shape[:3]) / 8.0            # 3 ... 20.875: some off both ends of the table
    hits[..., 2] = np.choose(rng.integers(0, 3, hits.shape[:3]), [0.5, 1.0, 2.0])
    hits[..., 3] = rng.integers(0, 400, hits.shape[:3]) / 4.0
    hits[np.arange(m)[None, None, :] >= n_hits[..., None]] = np.nan
    nodes = np.arange(4.0, 21.0)
    h = hits.astype(np.float64)
    return hits, n_hits, (4.0, 20.0, 2.0 * nodes, np.ones(17)), 2.0 * h[..., 0] + h[..., 3] - 8.0, 0.5, 8.0


def exact_histogram(hits, n_hits, tau, spec, grid, plane=None):
    """16 / exposure times the transfer function as an integer-weighted np.histogram2d over (tau, g), outer rows and columns
    from infinite outer edges."""
    m = hits.shape[2]
    h = hits.astype(np.float64)
    on = (n_hits[..., None] > np.arange(m)) & (h[..., 0] >= 4.0) & (h[..., 0] <= 20.0)
    if plane is not None:
        on = on & (np.arange(m) == plane)
    weights = np.round(16.0 * h[..., 2][on] ** 4)
    assert set(weights.tolist()) <= {1.0, 16.0, 256.0}
    edges = lambda e: np.concatenate([[-np.inf], e, [np.inf]])
    return np.histogram2d(tau[on], h[..., 2][on], bins=(edges(grid.edges()), edges(spec.edges())), weights=weights)[0]


@pytest.mark.parametrize("split", [False, True])
def test_powers_of_two_equal_an_integer_histogram(split):
    hits, n_hits, tables, tau, exposure, t_ref = exact_case()
    spec, grid = diskmod.Spectrum(0.25, 2.25, 8, split_orders=split), diskmod.TransferGrid(8.0, 120.0, 28)
    got = diskmod.disk_transfer(hits, n_hits, exposure, spec, grid, *tables, t_ref)
    want = np.stack([exact_histogram(hits, n_hits, tau, spec, grid, j) for j in range(3)]) if split else exact_histogram(hits, n_hits, tau, spec, grid)[None]
    assert np.array_equal(got * (16.0 / exposure), want) and want.sum() > 1000 and np.count_nonzero(want) > 60
    assert want[:, 0].sum() > 0 and want[:, -1].sum() > 0 and np.all(want[:, :, 0] == 0) and np.all(want[:, :, -1] == 0)


# ---- 4. closures -----------------------------------------------------------------------------------------------------------------------
def test_the_line_the_bolometric_light_and_the_planes():
    name = "mid"
    spec, grid = grids(64, 96)
    tf = statement(name, spec, grid)
    on, tau, g, w_ref = slots_of(name)
    n = int(on.sum())
    hits, n_hits = transfer_records(name)
    # summed over tau it is the line: disk_spectrum's own bin sums given the same weights
    weights = diskmod.transfer_slots(hits, n_hits, EXPOSURE, spec, grid, *make_tables(name), T_REF)[3]
    line = diskmod._bin_weights(hits, n_hits, spec, weights)
    got = diskmod.reverberation_line(tf)
    assert got.shape == line.shape == (1, 98)
    assert np.all(np.abs(got.astype(LD) - line) <= 2 * n * U * line) and np.array_equal(got != 0, line != 0) and np.count_nonzero(line) == 98
    # summed over everything it is the disk's bolometric light under eps(r)
    total = w_ref[on].sum()
    assert abs(LD(tf.sum()) - total) <= (n + 6) * U * total and total > 0
    assert np.all(np.abs(diskmod.impulse_response(tf).astype(LD).sum() - total) <= 2 * (n + 6) * U * total)
    assert diskmod.impulse_response(tf).shape == (1, 66)
    # the planes of split_orders add up to the unsplit result
    planes = statement(name, grids(64, 96, True)[0], grid)
    assert planes.shape == (3, 66, 98) and np.all(np.abs(planes.astype(LD).sum(axis=0) - tf[0]) <= 2 * n * U * tf[0])
    for j in range(3):
        only = hits.copy()
        only[:, :, np.arange(3) != j, 2] = np.nan
        assert np.array_equal(diskmod.disk_transfer(only, n_hits, EXPOSURE, spec, grid, *make_tables(name), T_REF)[0], planes[j])
    with pytest.raises(ValueError, match="keys"):
        statement(name, *grids(126, 255))


def test_lag_of_a_single_bin():
    grid = diskmod.TransferGrid(0.0, 64.0, 16)
    tf = np.zeros((2, 18, 10))
    tf[1, 6, 3:5] = (0.25, 1.5)                                           # one delay bin: tau_0 = 22
    tau_0 = grid.centres()[5]
    for R in (1.0, 0.3, 2.5):
        lag = diskmod.lag_frequency(tf, grid, [1e-7, 1e-6], 3, 5, reflection_fraction=R)
        assert lag.shape == (2,) and np.all(np.abs(lag - tau_0 * R / (1 + R)) <= 1e-9 * tau_0)
    assert tau_0 == 22.0 and abs(diskmod.lag_frequency(tf, grid, [0.5 / 22.0], 0, 10, reflection_fraction=0.5)[0]) < 1e-9    # half a turn: no lag
    with pytest.raises(ValueError):
        diskmod.lag_frequency(tf, grid, [1e-3], 6, 9)


# ---- 5. the lamp-post tables --------------------------------------------------------------------------------------------------------------
def test_rays_conserve_the_carter_constant_and_stay_null():
    for a in (0.0, 0.9):
        lp = diskmod.Lamppost(1.0, a, 6.0)
        for c in (-0.9, -0.3, 0.2, 0.6):
            sol = lp.ray(c, 500.0)
            _, r, th, _, p_t, p_r, p_th, L = sol.y
            assert sol.y.shape[1] > 5 and np.all(L == 0.0) and np.all(p_t == -1.0)
            carter = p_th ** 2 - a * a * np.cos(th) ** 2                  # Q = p_th^2 + cos^2 th (L^2 / sin^2 th - a^2 E^2) at L = 0, E = 1
            Delta, Sigma = r * r - 2 * r + a * a, r * r + a * a * np.cos(th) ** 2
            two_h = (Delta * p_r ** 2 + p_th ** 2 + a * a * np.sin(th) ** 2 - (r * r + a * a) ** 2 / Delta) / Sigma
            scale = p_th[0] ** 2 + a * a + 1.0
            size = (r * r + a * a) ** 2 / (Delta * Sigma)                 # the null condition's largest term, point by point
            print(f"a {a}, cos delta {c}: {sol.y.shape[1]} points, Carter constant moves by {np.max(np.abs(carter - carter[0])) / scale:.1e} of its "
                  f"scale, 2 H at most {np.max(np.abs(two_h) / size):.1e} of its largest term (rtol {lp.rtol:.0e})")
            assert np.max(np.abs(carter - carter[0])) <= 1e3 * lp.rtol * scale, (a, c)
            assert np.max(np.abs(two_h) / size) <= 1e3 * lp.rtol, (a, c)


def test_tables_are_continuous_in_the_spin_at_zero():
    zero = diskmod.lamppost_tables(1.0, 0.0, 6.0, 6.0, 20.0, 17, n_rays=24)
    tiny = diskmod.lamppost_tables(1.0, 1e-12, 6.0, 6.0, 20.0, 17, n_rays=24)
    for x, y in zip(zero, tiny):
        assert np.all(np.isfinite(x)) and np.all(x > 0) and np.all(np.abs(x - y) <= 1e-8 * np.abs(x))
    assert np.all(np.diff(zero[0]) > 0) and np.all(np.diff(zero[1]) < 0)  # farther is later and dimmer


def test_tables_in_the_flat_limit():
    """h = 1000 M, r = 1000 ... 3000 M (header above): the largest deviations found are 1.4e-3 (delay), 2.3e-3 (emissivity)
    and 7.1e-4 (t_ref) against the margin of 10 M / h = 1e-2."""
    h = 1000.0
    lp = diskmod.Lamppost(1.0, 0.0, h, n_rays=48)
    delay, emis = lp.tables(1000.0, 3000.0, 33)
    r = 1000.0 + np.arange(33) * 2000.0 / 32
    flat = emis * (r * r + h * h) ** 1.5
    dev_t, dev_e = np.max(np.abs(delay / np.sqrt(r * r + h * h) - 1)), np.max(np.abs(flat / flat.mean() - 1))
    t_ref = lp.t_ref(5000.0, np.radians(60.0))
    straight = np.sqrt(5000.0 ** 2 + h * h - 2 * 5000.0 * h * np.cos(np.radians(60.0)))
    print(f"flat limit: delay within {dev_t:.1e}, eps (r^2 + h^2)^1.5 within {dev_e:.1e}, t_ref within {abs(t_ref / straight - 1):.1e} (margin {10 / h:.0e})")
    assert dev_t <= 10.0 / h and dev_e <= 10.0 / h and abs(t_ref / straight - 1) <= 10.0 / h
    assert lp.t_ref(5000.0, 0.0) > 0 and abs(lp.t_ref(5000.0, 0.0) / 4000.0 - 1) <= 10.0 / h      # a camera on the axis


def test_tables_do_not_depend_on_the_launch_angle():
    """theta0 = 1e-3 against 1e-4: each table moves by less than its own interpolation error, an eighth of its largest second
    difference (linear interpolation between the nodes)."""
    r_in = float(diskmod.isco(1.0, 0.9))
    coarse, fine = (diskmod.Lamppost(1.0, 0.9, 6.0, theta0=th0).tables(r_in, 20.0, 64, n_rays=48) for th0 in (1e-3, 1e-4))
    for what, x, y in zip(("delay", "emis"), coarse, fine):
        moved, interp = float(np.max(np.abs(x - y))), float(np.max(np.abs(np.diff(y, 2)))) / 8
        print(f"theta0 1e-3 against 1e-4: {what} moves by {moved:.1e}, interpolation error {interp:.1e}")
        assert moved <= interp
    with pytest.raises(ValueError):
        diskmod.Lamppost(1.0, 0.9, 1.2)


# ---- 6. the struct, exports and bindings, the command line -----------------------------------------------------------------------------
def test_struct_layout_defaults_and_constants():
    T = ltrace.Transfer
    assert ctypes.sizeof(T) == 2 * 8 + 2 * 4 + 3 * 8 == 48
    assert [getattr(T, f).offset for f in ("tau_min", "tau_max", "n_tau", "n_r", "r_min", "r_max", "t_ref")] == [0, 8, 16, 20, 24, 32, 40]
    d = ltrace.default_transfer()
    assert (d.tau_min, d.tau_max, d.n_tau, d.n_r, d.r_min, d.r_max, d.t_ref) == (0.0, 256.0, 64, 2, 6.0, 20.0, 0.0)
    lt = diskmod.TransferGrid(-4.0, 60.0, 32).to_lt(2.5, 18.0, 37, 61.5)
    assert (lt.tau_min, lt.tau_max, lt.n_tau, lt.n_r, lt.r_min, lt.r_max, lt.t_ref) == (-4.0, 60.0, 32, 37, 2.5, 18.0, 61.5)
    assert (ltrace.TRANSFER_MAX_TAU, ltrace.TRANSFER_MAX_KEYS) == (diskmod.TRANSFER_MAX_TAU, diskmod.TRANSFER_MAX_KEYS) == (1024, 32768)
    assert ltrace.SPECTRUM_BLOCKS * ltrace.TRANSFER_MAX_KEYS * 8 == ltrace.SPECTRUM_WORKSPACE_BYTES
    import os
    header = open(os.path.join(os.path.dirname(os.path.abspath(ltrace.__file__)), "..", "include", "ltrace.h")).read()
    for text in ("#define LT_TRANSFER_MAX_TAU 1024", "#define LT_TRANSFER_MAX_KEYS 32768", "reverberation"):
        assert text in header


def test_the_c_compiler_gives_the_struct_the_same_layout(tmp_path):
    import os
    import subprocess
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ltrace.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(lt_transfer), offsetof(lt_transfer, n_tau), offsetof(lt_transfer, n_r),\n'
                   '  offsetof(lt_transfer, r_min), offsetof(lt_transfer, r_max), offsetof(lt_transfer, t_ref)); return 0; }\n')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(root, "include"), str(src), "-o", str(tmp_path / "probe")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).split()]
    T = ltrace.Transfer
    assert got == [ctypes.sizeof(T), T.n_tau.offset, T.n_r.offset, T.r_min.offset, T.r_max.offset, T.t_ref.offset]


def test_exports_and_bindings():
    lib = ctypes.CDLL(ltrace.LIB_PATH)
    tr, spec = ctypes.POINTER(ltrace.Transfer), ctypes.POINTER(ltrace.Spectrum)
    for suffix in ("", "_dev"):
        res, args = ltrace.SIGNATURES["lt_disk_spectrum" + suffix]
        at = args.index(spec)
        assert hasattr(lib, "lt_disk_transfer" + suffix)
        # the disk spectrum's arguments with (transfer, delay, emis) behind the grid
        assert ltrace.SIGNATURES["lt_disk_transfer" + suffix] == (res, args[:at + 1] + [tr, ctypes.c_void_p, ctypes.c_void_p] + args[at + 1:])
    assert hasattr(lib, "lt_default_transfer") and ltrace.SIGNATURES["lt_default_transfer"] == (None, [tr])
    for fn in (ltrace.disk_transfer, ltrace.disk_transfer_dev, ltrace.default_transfer, diskmod.disk_transfer, diskmod.transfer_bin,
               diskmod.lamppost_tables, diskmod.impulse_response, diskmod.reverberation_line, diskmod.lag_frequency):
        assert callable(fn)
    hits, n_hits = synth(4, 4, 2, 5, 2.4, 20.0)
    met, d, sp = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9), ltrace.default_disk(), ltrace.default_spectrum()
    lt = ltrace.default_transfer(n_r=3)
    with pytest.raises(ValueError, match="delay"):             # a table that is not the struct's n_r never reaches the library
        ltrace.disk_transfer(hits, n_hits, met, d, sp, lt, [0.0, 1.0], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="emis"):
        ltrace.disk_transfer(hits, n_hits, met, d, sp, lt, [0.0, 1.0, 2.0], np.ones((3, 1)))
    if ltrace.device_count() == 0:                             # the entry points' answer on a machine without a GPU
        calls = (lambda: ltrace.disk_transfer(hits, n_hits, met, d, sp, lt, [0.0, 1.0, 2.0], [1.0, 1.0, 1.0]),
                 lambda: ltrace.disk_transfer_dev(8, 0, 4, 4, 2, met, d, sp, lt, 8, 8, 8),
                 lambda: ltrace.disk_transfer(hits, n_hits, met, d, sp, ltrace.default_transfer(n_r=3, n_tau=-1), [0.0, 1.0, 2.0], [1.0, 1.0, 1.0]))
        for call in calls:
            with pytest.raises(ltrace.LtraceError) as ei:
                call()
            assert ei.value.code == ltrace.ERR_NO_DEVICE       # the first refusal of all, whatever else is wrong


SEQUENCE = ["--a", "0.9", "--disk-images", "3", "--synthetic", "16", "12"]
SPOT = ["--hotspot", "8", "0", "1.5"]
SPEC = ["--spectrum", "0.1", "1.5", "32"]
FLASH = ["--lamppost", "6", "--transfer", "0", "128", "32"]


@pytest.mark.parametrize("argv,match", [(FLASH + SPEC, "sequence"),
                                        (SEQUENCE + FLASH + SPEC, "sequence"),
                                        (SEQUENCE + SPOT + FLASH, "--spectrum"),
                                        (SEQUENCE + SPOT + SPEC + ["--lamppost", "6"], "go together"),
                                        (SEQUENCE + SPOT + SPEC + ["--transfer", "0", "128", "32"], "go together"),
                                        (SEQUENCE + SPOT + SPEC + ["--lamppost", "6", "--transfer", "0", "128", "32.5"], "whole number"),
                                        (SEQUENCE + SPOT + SPEC + ["--lamppost", "6", "--transfer", "0", "128", "1025"], "n_tau"),
                                        (SEQUENCE + SPOT + SPEC + ["--lamppost", "6", "--transfer", "128", "0", "32"], "tau_min"),
                                        (SEQUENCE + ["--disk-map", "spiral"] + SPEC + ["--lamppost", "1.2", "--transfer", "0", "128", "32"], "horizon")])
def test_cli_refusals(argv, match):
    import image_lens
    args = image_lens.build_parser().parse_args(argv)
    thin = diskmod.TransparentDisk(max_images=3)
    with pytest.raises(ValueError, match=match):
        image_lens.transfer_from_args(args, thin, 1.0, 0.9)
    if args.hotspot is not None or args.disk_map is not None:
        with pytest.raises(ValueError, match=match):
            image_lens.main_sequence(args, thin)


def test_cli_needs_the_optically_thin_disk_and_builds_the_source():
    import image_lens
    args = image_lens.build_parser().parse_args(["--a", "0.9", "--disk", "--synthetic", "16", "12"] + SPOT + SPEC + FLASH)
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.transfer_from_args(args, diskmod.ThinDisk(), 1.0, 0.9)
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.main_sequence(args, diskmod.ThinDisk())
    with pytest.raises(ValueError, match="--disk-images"):
        image_lens.main_sequence(args, None)
    args = image_lens.build_parser().parse_args(SEQUENCE + SPOT + SPEC + FLASH)
    lamp, grid = image_lens.transfer_from_args(args, diskmod.TransparentDisk(max_images=3), 2.0, 0.9)
    assert (lamp.M, lamp.a, lamp.h) == (2.0, 0.9, 12.0) and (grid.tau_min, grid.tau_max, grid.n_tau) == (0.0, 128.0, 32)
    assert image_lens.transfer_from_args(image_lens.build_parser().parse_args(SEQUENCE + SPOT + SPEC)) is None
    for kw in (dict(lamppost=lamp), dict(transfer=grid), dict(lamppost=lamp, transfer=grid)):
        with pytest.raises(ValueError, match="transfer"):      # render_sequence's own refusals of the arguments come first
            image_lens.render_sequence(None, None, 50.0, (0.7, 0.7), diskmod.TransparentDisk(), diskmod.HotSpot(), [0.0, 10.0], shape=(8, 8), **kw)
