"""GPU tests of the linear polarization (lt_trace_disk_pol, lt_trace_batch_kerr_disk_pol, lt_polarization_probe,
lt_shade_stokes, lt_hotspot_lightcurve_stokes).

Identity: the polarized trace takes lt_trace_disk_hits' steps, so everything the two share is equal bit for bit.  The
device's rule is held to disk.polarization; the stored records to the transported truth of tests/test_polarization_host.py
within a budget in the model of tests/test_gpu_hit_time.py: a hit whose position along the track is off by the
integrator's r budget is off in (q, u) by |d(q, u)/dr| times that, times e^(pi k) behind k plane crossings, d(q, u)/dr taken
from the closed form at the two track points around the hit.  The Stokes kernels are held to a longdouble reference on
the synthetic records of tests/test_hotspot_records_host.py.

MEASURED on the MI355X (build a0525ed44419; profiles/polarization_a0525ed44419.json, written with LT_POL_MEASURE=path):
    the device's float64 rule against disk.polarization, 11 707 synthetic records: largest difference 9.0e-15; numpy's own
        float64 against longdouble on them 1.24e-14 (measured on the CPU; the bound is 4 x that);
    stored (q, u) against the transported truth, 224 rays per spin (1 / 1 / 3 excluded), slots 0 and 1:
        DP45-exact: raw |d(q, u)| median 6.2e-6 / 3.7e-6 / 9.9e-6, max 8.8e-5 / 6.8e-5 / 1.3e-4 (a = 0 / 0.9 / -0.7); beyond the
            position model |d(q, u)/dr| (eps_r + |r'/theta'| eps_theta) e^(pi k) on 2 / 5 / 1 records, by at most 2.1e-5 /
            4.8e-5 / 2.6e-5: EPS_POL = 4.8e-5, asserted at 10 x.  The model sees a displacement along the track only; where
            (q, u) is stationary along the track the hit's cross-track error (its momenta, from the cubic on a step of
            several M) is what is left;
        RK4 float64: raw median 3.8e-7 / 1.8e-6 / 3.1e-7, max 3.1e-3 / 2.4e-2 / 4.8e-3; 1 / 5 / 0 records of 68 / 101 / 55
            outside the model, inside RK4's 10 % tail allowance: eps 0;
    the frame path in float64, 149 of 150 sampled pixels, 149 slot-0 and 13 slot-1 records: DP45-exact none outside (raw
        median 2.5e-6, max 6.8e-5), RK4 4 of 162 (raw median 5.3e-7, max 4.8e-2);
    RK4 float32 against float64, (median, p99): |dq| (2.61e-7, 4.22e-6) / (2.45e-7, 3.65e-6) / (2.81e-7, 2.31e-6), |du|
        (1.69e-7, 2.74e-6) / (1.81e-7, 2.98e-6) / (1.52e-7, 2.41e-6); asserted at 4 x;
    Stokes kernels against longdouble: frames 1.00 ulp of float32 (big), 0.00 (one, strip, pass), bound 2; light curves
        2.8e-16 / 1.4e-14 / 5.1e-13 / 2.9e-14 of their terms' magnitudes, bounds 2.0e-12 / 1.2e-12 / 4.2e-11 / 7.9e-11.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import disk as diskmod
import ltrace
from oracle import oracle
import test_gpu_hit_time as ht
import test_polarization_host as ph
from test_gpu_hit_time import CASES, CONFIGS, CONFIG_IDS, E_PI, FRAME_H, FRAME_W, R_BUDGET, frame_setup, lam_max
from test_hit_time_rule import M, R_OBS, SPINS, THETA_OBS, tracks
from test_hotspot_records_host import LD, Reference, lc_bound, synth, ulps
from test_polarization_host import FIELD, SIN_ZETA_MIN, synth_pol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURE = os.environ.get("LT_POL_MEASURE")   # a path: the figures the tests print are also written there as JSON
# Measured (MEASURED above), asserted at the stated multiple.
EPS_POL = {"dp45_exact": 4.8e-5, "rk4": 0.0}                                  # (q, u) beyond the position model, x 10
Q32 = [((2.61e-7, 4.22e-6), (1.69e-7, 2.74e-6)), ((2.45e-7, 3.65e-6), (1.81e-7, 2.98e-6)),
       ((2.81e-7, 2.31e-6), (1.52e-7, 2.41e-6))]                           # per spin ((median, p99) of |dq|, of |du|), x 4
PROBE_F64_ERR = 1.24e-14                                                        # numpy float64 against longdouble, measured on the CPU
_RECORD = {}


def record(key, value):
    _RECORD[key] = value
    if MEASURE:
        import json
        with open(MEASURE, "w") as f:
            json.dump(dict(build_id=ltrace.build_id(), **_RECORD), f, indent=1, default=float)


def lt_field(f=FIELD, sign=1.0, **kw):
    return ltrace.default_bfield(**dict(dict(b_r=sign * f.b_r, b_phi=sign * f.b_phi, b_z=sign * f.b_z, pol_frac=f.pol_frac), **kw))


# ---- 1. the device's rule ---------------------------------------------------------------------------------------------------
def probe_records(a, r_obs, theta_obs, n, seed):
    """Synthetic null records: r from the ISCO to 40, both signs of p_r and p_theta at the hit, p_r < 0 at the camera."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(float(diskmod.isco(M, a)), 40.0, n)
    L, pth, pth_c = rng.uniform(-5.0, 7.0, n), rng.uniform(-7.0, 7.0, n), rng.uniform(-7.0, 7.0, n)

    def p_r2(rr, s, c, p_theta):
        up = diskmod._raise_index(M, a, rr, s, c, (-np.ones(n), np.zeros(n), p_theta, L))
        sigma, delta = rr * rr + a * a * c * c, rr * rr - 2 * M * rr + a * a
        return -(-up[0] + p_theta * up[2] + L * up[3]) * sigma / delta

    h2 = p_r2(r, np.ones(n), np.zeros(n), pth)
    c2 = p_r2(np.full(n, r_obs), np.full(n, np.sin(theta_obs)), np.full(n, np.cos(theta_obs)), pth_c)
    ok = (h2 > 0) & (c2 > 0)
    hit = np.stack([r, rng.choice([-1.0, 1.0], n) * np.sqrt(np.where(ok, h2, 1.0)), pth], axis=-1)[ok]
    cam = np.stack([-np.sqrt(np.where(ok, c2, 1.0)), pth_c], axis=-1)[ok]
    return L[ok], hit, cam


def probe_set():
    """The ~10 000 records: every spin of the truth set x theta_obs in {1.0, 1.4, pi / 2} x r_obs in {12, 30, 100, 300}."""
    seed = 0
    for a in SPINS:
        for theta_obs in (1.0, 1.4, np.pi / 2):
            for r_obs in (12.0, 30.0, 100.0, 300.0):
                seed += 1
                yield (a, theta_obs, r_obs) + probe_records(a, r_obs, theta_obs, 330, seed)


def probe_float64_error():
    """Largest |float64 - longdouble| of disk.polarization over the probe's records, any of the four components: what
    float64 rounding does to the rule on these inputs.  Measured here, on the CPU: PROBE_F64_ERR."""
    return max(float(np.max(np.abs(diskmod.polarization(M, a, ro, tho, L, hit, cam, FIELD).astype(LD)
                                   - diskmod.polarization(M, a, ro, tho, L, hit, cam, FIELD, dtype=LD))))
               for a, tho, ro, L, hit, cam in probe_set())


def test_probe_against_numpy():
    """The device's float64 rule against disk.polarization, within 4 x what numpy's float64 itself is off from the same
    statement in longdouble on the same records.  (The device contracts multiply-adds and numpy does not, so the two
    differ by rounding.)"""
    total, worst = 0, 0.0
    for a, tho, ro, L, hit, cam in probe_set():
        got = ltrace.polarization_probe(ltrace.Metric(ltrace.METRIC_KERR, 0, M, a), ro, tho, L, hit, cam, lt_field())
        worst = max(worst, float(np.max(np.abs(got - diskmod.polarization(M, a, ro, tho, L, hit, cam, FIELD)))))
        total += L.size
        assert (hit[:, 1] > 0).any() and (hit[:, 1] < 0).any() and (hit[:, 2] > 0).any() and (hit[:, 2] < 0).any()
    err64 = probe_float64_error()
    print(f"probe: {total} records, largest |device - numpy| {worst:.2e}; numpy float64 against longdouble {err64:.2e}")
    record("probe", dict(records=total, worst=worst, float64_error=err64))
    assert 9000 <= total <= 12000
    assert err64 <= 2 * PROBE_F64_ERR          # the written-down figure is this machine's
    assert worst <= 4 * err64


# ---- 2. identity --------------------------------------------------------------------------------------------------------------
_FRAME = {}


def frame_pol(integ="rk4", prec=32):
    """The 96 x 80 frame of tests/test_gpu_hit_time.py, 3 images, per configuration: the polarized trace's outputs, cached."""
    if (integ, prec) not in _FRAME:
        cam, met, o, d = frame_setup(integ, prec)
        _FRAME[integ, prec] = ltrace.trace_disk_pol(cam, met, o, d, lt_field(), max_images=3)
    return _FRAME[integ, prec]


def check_pol_records(pol, hits):
    stored = ~np.isnan(hits[..., 0])
    assert np.array_equal(np.isnan(pol), np.repeat(~stored[..., None], 4, axis=-1))
    p = pol[stored].astype(np.float64)
    lit = p[:, 2] > 0
    assert np.max(np.abs(p[lit, 0] ** 2 + p[lit, 1] ** 2 - 1.0)) <= 4e-7
    assert np.all((p[:, 2] >= 0) & (p[:, 2] <= 1 + 1e-7) & (p[:, 3] >= 0) & (p[:, 3] <= 1 + 1e-7))


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_frame_identity(integ, prec):
    ref, got = ht.frame_hits(integ, prec), frame_pol(integ, prec)
    for k in ("hits", "n_hits", "fa", "winding", "status", "steps"):
        assert np.asarray(got[k]).tobytes() == np.asarray(ref[k]).tobytes(), k
    for k in ("rays", "steps", "rhs_evals", "escaped", "captured", "invalid", "disk", "disk_hits"):
        assert got["stats"][k] == ref["stats"][k], k
    assert ref["stats"]["disk_hits"] > 1000
    check_pol_records(got["pol"], got["hits"])
    # b -> -b: the same records, bit for bit
    cam, met, o, d = frame_setup(integ, prec)
    assert ltrace.trace_disk_pol(cam, met, o, d, lt_field(sign=-1.0), max_images=3, want=("pol",))["pol"].tobytes() == got["pol"].tobytes()


def test_odd_frame_single_image():
    """67 x 45, one image per ray: columns and rows that are no multiple of the 8 x 8 tile."""
    a, tho, ro, rout = CASES[0]
    cam = ltrace.Camera(67, 45, 0.9, 0.62, 0.0, 0.0, ro, tho)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    o, d = ltrace.default_opts(integrator="rk4", precision=32), ltrace.default_disk(r_out=rout)
    ref = ltrace.trace_disk_hits(cam, met, o, d, max_images=1)
    got = ltrace.trace_disk_pol(cam, met, o, d, lt_field(), max_images=1)
    for k in ("hits", "n_hits", "fa", "winding", "status", "steps"):
        assert np.asarray(got[k]).tobytes() == np.asarray(ref[k]).tobytes(), k
    assert got["pol"].shape == (45, 67, 1, 4) and (got["n_hits"] > 1).sum() > 10
    check_pol_records(got["pol"], got["hits"])


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_batch_identity(integ, prec):
    a, tho, ro, rout = CASES[0]
    al, th, ar = ht.fans(ro, rout)
    d = ltrace.default_disk(r_out=rout)
    args = (M, a, ro, al, th, tho, lam_max(ro), d)
    kw = dict(max_images=4, axis_refines=ar, integrator=integ, precision=prec)
    ref, got = ltrace.trace_batch_kerr_disk_hits(*args, **kw), ltrace.trace_batch_kerr_disk_pol(*args, lt_field(), **kw)
    for k in ("hits", "n_hits", "fa", "winding", "status", "rhs_evals"):
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert (ref["n_hits"] > 1).sum() > 40
    check_pol_records(got["pol"], got["hits"])


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_partitions_reassemble(integ, prec):
    whole = frame_pol(integ, prec)
    full = {k: np.empty_like(np.asarray(whole[k])) for k in ("hits", "pol", "n_hits", "fa", "status")}
    for part in range(3):
        cam, met, o, d = frame_setup(integ, prec, n_parts=3, part=part, row_block=16)
        out = ltrace.trace_disk_pol(cam, met, o, d, lt_field(), max_images=3)
        rows = ltrace.global_rows(FRAME_H, 16, 3, part)
        for k in full:
            full[k][rows] = out[k]
    for k in full:
        assert full[k].tobytes() == np.asarray(whole[k]).tobytes(), k


_DUMP = """
import sys
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
import numpy as np, ltrace
from test_gpu_hit_time import frame_setup
from test_gpu_polarization import lt_field
cam, met, o, d = frame_setup(sys.argv[2], int(sys.argv[3]))
out = ltrace.trace_disk_pol(cam, met, o, d, lt_field(), max_images=3)
np.savez(sys.argv[1], **{{k: np.asarray(v) for k, v in out.items() if k != "stats"}})
"""


@pytest.mark.parametrize("integ,prec", CONFIGS, ids=CONFIG_IDS)
def test_ghost_phase_changes_nothing(tmp_path, integ, prec):
    """LT_D_LONG=8 (read once per process, so a child): every long wave spends its steps in the ghost-lane phase; the
    records, momenta and so polarization included, are the default's byte for byte."""
    path = str(tmp_path / "ghost.npz")
    src = _DUMP.format(pkg=os.path.join(ROOT, "light-path-tracer_amd"), root=ROOT, tests=os.path.join(ROOT, "tests"))
    subprocess.run([sys.executable, "-c", src, path, integ, str(prec)], check=True, env=dict(os.environ, LT_D_LONG="8"), timeout=120)
    got, ref = np.load(path), frame_pol(integ, prec)
    for k in ("hits", "pol", "n_hits", "fa", "winding", "status", "steps"):
        assert got[k].tobytes() == np.asarray(ref[k]).tobytes(), k


# ---- 3. the stored records against the truth -------------------------------------------------------------------------------
_PAIRED = {}


def paired_truth(a, rays):
    """Per ray of `rays`: tests/test_gpu_hit_time.py's truth() entry (for the exclusions and |r'/theta'|) and, per annulus
    crossing, the transported truth (q, u), sin zeta and |d(q, u)/dr| along the track, the last from the closed form at the
    two track points around the hit.  -> [(entry, [(k, s_r, qu (2,), sin_zeta, slope (2,)), ...])]."""
    key = (a, tuple(np.concatenate(rays)))
    if key in _PAIRED:
        return _PAIRED[key]
    entries = ht.truth(a, rays)
    hits, t = ph.truth(a, rays)
    trs = {tr["ray"]: tr for tr in tracks(a, rays)}
    by_ray = {}
    for n, h in enumerate(hits):
        y = trs[h["ray"]]["y"]
        i = h["i"]
        ends = diskmod.polarization(M, a, R_OBS, THETA_OBS, h["L"], y[[1, 5, 6], i:i + 2].T, h["cam"], FIELD)[:, :2]
        slope = np.abs(ends[1] - ends[0]) / abs(y[1, i + 1] - y[1, i])
        by_ray.setdefault(h["ray"], []).append((h["slot"], h["hit"][0], t["qu"][n], t["sin_zeta"][n], slope))
    out = []
    for e in entries:
        mine = sorted(by_ray.get(e["ray"], []), key=lambda x: x[0])
        assert len(mine) == len(e["hits"]), (e["ray"], len(mine), len(e["hits"]))
        rows = []
        for (k, rc, _, s_r, _), (slot, r_hit, qu, sz, slope) in zip(e["hits"], mine):
            assert abs(rc - r_hit) <= 1e-5
            rows.append((k, s_r, qu, sz, slope))
        out.append((e, rows))
    _PAIRED[key] = out
    return out


def compare_with_truth(a, pairs, n_hits_of, pol_of, integ, extra=0.0):
    """Slot 0, and slot 1 where it exists: |d(q, u)| <= (10 eps + |d(q, u)/dr| (eps_r + |r'/theta'| eps_theta)) e^(pi k) +
    the probe's bound (1e-13: float64 rounding of the rule, three decades above the measured) + extra.  Rays excluded by
    the truth alone (DP45's margins, tests/test_gpu_hit_time.py) and rays with a hit of sin zeta < 0.05: at most 2 % of the
    case's rays together, that test's cap."""
    eps_r, eps_th, tail = R_BUDGET[integ]
    keep = [(e, rows) for e, rows in pairs if not ht.may_differ(e, float(diskmod.isco(M, a)), 20.0, *R_BUDGET["dp45_exact"][:2])]
    n, outside, resid, raw, slots = 0, 0, [], [], [0, 0]
    for e, rows in keep:
        i = e["ray"]
        if min(n_hits_of(i), 2) != min(len(rows), 2):
            n += 1
            outside += 1
            continue
        for j, (k, s_r, qu, sz, slope) in enumerate(rows[:2]):
            if sz < SIN_ZETA_MIN:
                continue
            err = np.abs(pol_of(i, j)[:2].astype(np.float64) - qu)
            model = slope * (eps_r + s_r * eps_th)
            n += 1
            slots[j] += 1
            resid.append(float(np.max(np.maximum((err - 1e-13 - extra) / E_PI ** k - model, 0.0))))
            raw.append(float(err.max()))
            if np.any(err > (10 * EPS_POL[integ] + model) * E_PI ** k + 1e-13 + extra):
                outside += 1
    dim_rays = sum(any(sz < SIN_ZETA_MIN for _, _, _, sz, _ in rows[:2]) for _, rows in keep)
    kept = len(keep) - dim_rays
    assert kept >= 0.98 * len(pairs), (kept, len(pairs))
    return dict(n=n, outside=outside, slot0=slots[0], slot1=slots[1], max=max(resid), p90=float(np.quantile(resid, 0.9)),
                raw_median=float(np.median(raw)), raw_max=max(raw), excluded=len(pairs) - kept, tail=tail)


@pytest.mark.parametrize("integ", ("dp45_exact", "rk4"))
@pytest.mark.parametrize("a", SPINS)
def test_batch_against_the_truth(a, integ):
    rays = ht.fan()
    pairs = paired_truth(a, rays)
    out = ltrace.trace_batch_kerr_disk_pol(M, a, R_OBS, rays[0], rays[1], THETA_OBS, lam_max(R_OBS), ltrace.default_disk(r_out=20.0),
                                           lt_field(), max_images=2, integrator=integ, precision=64)
    res = compare_with_truth(a, pairs, lambda i: out["n_hits"][i], lambda i, j: out["pol"][i, j], integ)
    print(f"a {a} {integ}: {res['slot0']} slot-0 and {res['slot1']} slot-1 records, {res['excluded']} excluded; (q, u) beyond the position "
          f"model: max {res['max']:.3e}, p90 {res['p90']:.3e}; outside {res['outside']} of {res['n']}; raw |d(q, u)| median "
          f"{res['raw_median']:.3e}, max {res['raw_max']:.3e}")
    record(f"eps_pol/{integ}/a{a:g}", res)
    assert res["slot0"] >= 25
    assert res["outside"] <= res["tail"] * res["n"], res


@pytest.mark.parametrize("integ", ("rk4", "dp45_exact"))
def test_frame_against_the_truth(integ):
    """The same for the frame path in float64 on the 150 sampled pixels of tests/test_gpu_hit_time.py; a frame stores
    (q, u) in float32, so half a spacing of float32 at 1 is added."""
    a = CASES[0][0]
    sample = ht.frame_truth()
    al, th, _ = oracle.pixel_angles(FRAME_H, FRAME_W, *ht.frame_fov())
    rays = (np.array([float(al[iy, ix]) for iy, ix, _ in sample]), np.array([float(th[iy, ix]) for iy, ix, _ in sample]))
    pairs = paired_truth(a, rays)
    where = [(iy, ix) for iy, ix, _ in sample]
    out = frame_pol(integ, 64)
    res = compare_with_truth(a, pairs, lambda i: out["n_hits"][where[i]], lambda i, j: out["pol"][where[i]][j], integ, extra=6e-8)
    print(f"frame, a {a} {integ}: {res['slot0']} slot-0 and {res['slot1']} slot-1 records, {res['excluded']} excluded; outside "
          f"{res['outside']} of {res['n']}; raw |d(q, u)| median {res['raw_median']:.3e}, max {res['raw_max']:.3e}")
    record(f"frame_pol/{integ}", res)
    assert res["slot0"] >= 100
    assert res["outside"] <= res["tail"] * res["n"], res


# ---- 4. float32 against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(SPINS)))
def test_float32_records(si):
    """RK4 float32 against RK4 float64 on the slots both store: (median, p99) of |dq| and of |du|."""
    a = SPINS[si]
    al, th = ht.fan()
    run = lambda prec: ltrace.trace_batch_kerr_disk_pol(M, a, R_OBS, al, th, THETA_OBS, lam_max(R_OBS), ltrace.default_disk(r_out=20.0),
                                                        lt_field(), max_images=2, integrator="rk4", precision=prec)
    o32, o64 = run(32), run(64)
    in32, in64 = ~np.isnan(o32["pol"][..., 0]), ~np.isnan(o64["pol"][..., 0])
    both = in32 & in64 & (o64["pol"][..., 2] >= SIN_ZETA_MIN)
    assert both.sum() >= 0.98 * (in32 | in64).sum() and both.sum() >= 25
    d = np.abs(o32["pol"][both][:, :2] - o64["pol"][both][:, :2])
    got = tuple((float(np.median(d[:, c])), float(np.quantile(d[:, c], 0.99))) for c in range(2))
    print(f"a {a}: float32 - float64 over {both.sum()} records: |dq| median {got[0][0]:.3e} p99 {got[0][1]:.3e}, |du| median "
          f"{got[1][0]:.3e} p99 {got[1][1]:.3e}")
    record(f"q32/a{a:g}", got)
    for c in range(2):
        assert got[c][0] <= 4 * Q32[si][c][0] and got[c][1] <= 4 * Q32[si][c][1]


# ---- 5. the Stokes kernels on synthetic records ----------------------------------------------------------------------------------
# name: (R, W, max_images, M, a, r_out, seed, spot (r_spot, phi0, sigma, exposure, with_disk), light-curve grid)
STOKES_CASES = {"big": (257, 331, 8, 1.0, 0.9, 20.0, 51, (9.0, 0.5, 1.5, 2.0, 1), (5.0, 7.5, 6)),      # a second, partial pass
                "one": (1, 1, 2, 1.0, 0.9, 20.0, 32, (3.0, 1.0, 4.0, 1.0, 1), (5.0, 7.5, 40)),
                "strip": (3, 70, 5, 1.0, 0.0, 20.0, 54, (7.2, 4.0, 4.0, 0.6, 0), (1e5, 11.0, 12)),
                "pass": (256, 256, 2, 1.0, -0.7, 20.0, 55, (10.0, 0.3, 1.5, 2.0, 1), (-3e4, 13.0, 12))}   # exactly one pass
DISK_EXPOSURE = 0.25
_STOKES = {}


def stokes_case(name):
    if name not in _STOKES:
        R, W, m, M_, a, r_out, seed, spot, grid = STOKES_CASES[name]
        hits, n_hits = synth(R, W, m, seed, ltrace.kerr_isco(M_, a), r_out)
        _STOKES[name] = (hits, n_hits, synth_pol((R, W, m), seed + 100), Reference(hits, n_hits))
    return _STOKES[name]


def stokes_reference(ref, pol, M_, a, spot, t_obs, r_in, pol_frac, with_disk):
    """Per stored slot the longdouble terms (e, w q e, w u e), e the mean of the three channels of the spot's light plus,
    with_disk, the disk's; w = Pi sin^2 zeta from the float32 record."""
    es = ref.spot_emission(M_, a, spot, t_obs)
    e = (es[:, 0] + es[:, 1] + es[:, 2]) / 3
    if with_disk:
        ed = ref.disk_emission(r_in, 3.0, DISK_EXPOSURE)
        e = e + (ed[:, 0] + ed[:, 1] + ed[:, 2]) / 3
    p = pol.reshape(-1, ref.m, 4)[ref.pix, ref.slot].astype(LD)
    w = LD(pol_frac) * p[:, 2] * p[:, 2]
    return np.stack([e, w * p[:, 0] * e, w * p[:, 1] * e], axis=-1)


@pytest.mark.parametrize("name", list(STOKES_CASES))
def test_stokes_kernels(name):
    R, W, m, M_, a, r_out, seed, spot, grid = STOKES_CASES[name]
    hits, n_hits, pol, ref = stokes_case(name)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M_, a)
    d = ltrace.default_disk(r_out=r_out, exposure=DISK_EXPOSURE)
    s = ltrace.default_hotspot(r_spot=spot[0], phi0=spot[1], sigma=spot[2], exposure=spot[3], with_disk=spot[4])
    b = lt_field()
    r_in = ltrace.kerr_isco(M_, a)
    assert (n_hits > m).any() or R * W == 1
    # frames: 2 ulp of float32 of the longdouble sums
    worst = 0.0
    for t_obs in (0.0, 333.25, 1e5):
        terms = stokes_reference(ref, pol, M_, a, spot, t_obs, r_in, FIELD.pol_frac, spot[4])
        want = np.zeros((R * W, 3), dtype=LD)
        for j in range(m):
            sel = ref.slot == j
            want[ref.pix[sel]] += terms[sel]
        got = ltrace.shade_stokes(hits, n_hits, pol, met, d, s, b, t_obs)
        assert got.shape == (R, W, 3) and got.dtype == np.float32
        worst = max(worst, float(np.max(ulps(got, want.reshape(R, W, 3)))))
        assert np.all(got[n_hits == 0] == 0)
    assert ltrace.shade_stokes(hits, n_hits, pol, met, d, s, b, 1e5).tobytes() == got.tobytes()                     # run to run
    assert ltrace.shade_stokes(hits, n_hits, pol, met, d, s, lt_field(sign=-1.0), 1e5).tobytes() == got.tobytes()   # b -> -b
    zero = ltrace.shade_stokes(hits, n_hits, pol, met, d, s, lt_field(pol_frac=0.0), 1e5)
    assert np.all(zero[..., 1:] == 0) and zero[..., 0].tobytes() == got[..., 0].tobytes()
    # light curve: I inside the existing test's derived bound, relative; Q and U, sums of terms of both signs, inside the
    # same bound times the sum of their terms' magnitudes; the I column has the bits of lt_hotspot_lightcurve's column 0
    times = grid[0] + grid[1] * np.arange(grid[2])
    lc = ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, b, *grid)
    plain = ltrace.hotspot_lightcurve(hits, n_hits, met, d, s, *grid)
    assert lc.shape == (grid[2], 3) and lc[:, 0].tobytes() == plain[:, 0].tobytes()
    bound = lc_bound(M_, a, spot, times, r_out)
    rel = 0.0
    for i, t in enumerate(times):
        terms = stokes_reference(ref, pol, M_, a, spot, float(t), r_in, FIELD.pol_frac, False)
        want, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
        assert want[0] > 0
        rel = max(rel, float(np.max(np.abs(lc[i].astype(LD) - want) / scale)))
    assert ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, b, *grid).tobytes() == lc.tobytes()
    assert ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, lt_field(sign=-1.0), *grid).tobytes() == lc.tobytes()
    zero = ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, lt_field(pol_frac=0.0), *grid)
    assert np.all(zero[:, 1:] == 0) and zero[:, 0].tobytes() == lc[:, 0].tobytes()
    print(f"{name}: Stokes frames against longdouble, largest difference {worst:.2f} ulp of float32; light curve, largest difference "
          f"relative to the terms' magnitudes {rel:.2e}, bound {bound:.2e}")
    record(f"stokes/{name}", dict(frame_ulp=worst, lc_rel=rel, lc_bound=bound))
    assert worst <= 2
    assert rel <= bound


def test_stokes_dev_entry_points():
    import ctypes as C
    import hipmini
    R, W, m, M_, a, r_out, seed, spot, grid = STOKES_CASES["strip"]
    hits, n_hits, pol, _ = stokes_case("strip")
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M_, a)
    d = ltrace.default_disk(r_out=r_out, exposure=DISK_EXPOSURE)
    s = ltrace.default_hotspot(r_spot=spot[0], phi0=spot[1], sigma=spot[2], exposure=spot[3], with_disk=spot[4])
    dev = []
    for host in (hits, n_hits, pol):
        host = np.ascontiguousarray(host)
        buf = hipmini.DeviceArray(host.shape, host.dtype)
        hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(buf.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1), "hipMemcpy H2D")
        dev.append(buf)
    d_iqu, d_lc = hipmini.DeviceArray((R, W, 3), np.float32), hipmini.DeviceArray((grid[2], 3), np.float64)
    ltrace.shade_stokes_dev(dev[0].ptr, dev[1].ptr, dev[2].ptr, R, W, m, met, d, s, lt_field(), 333.25, d_iqu.ptr)
    ltrace.hotspot_lightcurve_stokes_dev(dev[0].ptr, 0, dev[2].ptr, R, W, m, met, d, s, lt_field(), *grid, d_lc.ptr)
    assert d_iqu.get().tobytes() == ltrace.shade_stokes(hits, n_hits, pol, met, d, s, lt_field(), 333.25).tobytes()
    assert d_lc.get().tobytes() == ltrace.hotspot_lightcurve_stokes(hits, n_hits, pol, met, d, s, lt_field(), *grid).tobytes()


# ---- 6. the Python layers ------------------------------------------------------------------------------------------------------
def test_render_sequence_with_a_field():
    import image_lens
    from metrics import Kerr
    a, tho, ro, rout = CASES[0]
    metric = Kerr(M=M, a=a, integrator="rk4", precision=32)
    dk = diskmod.TransparentDisk(r_out=rout, max_images=3)
    spot = diskmod.HotSpot(r_spot=8.0, phi0=0.5, sigma=1.5, exposure=2.0)
    fov = (np.radians(40.0), np.radians(40.0))
    times = 10.0 * np.arange(3)
    seq = image_lens.render_sequence(None, metric, ro, fov, dk, spot, times, shape=(64, 64), theta_obs=tho, bfield=FIELD)
    plain = image_lens.render_sequence(None, metric, ro, fov, dk, spot, times, shape=(64, 64), theta_obs=tho)
    for k in ("frames", "rgba", "lightcurve", "hits", "n_hits"):
        assert np.asarray(seq[k]).tobytes() == np.asarray(plain[k]).tobytes(), k
    assert "stokes" not in plain
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    cam = image_lens._camera((64, 64), fov, (0.0, 0.0), ro, tho)
    opts = ltrace.default_opts(integrator="rk4", precision=32, schedule="direct", tb_symmetry=0, axis_refine_frac=image_lens.Y_AXIS_REFINE_FRAC)
    direct = ltrace.trace_disk_pol(cam, met, opts, dk.to_lt(), lt_field(), max_images=3)
    assert direct["pol"].tobytes() == seq["pol"].tobytes() and (seq["n_hits"] > 0).sum() > 300
    rec = (direct["hits"], direct["n_hits"], direct["pol"], met, dk.to_lt(), spot.to_lt(), lt_field())
    assert seq["stokes"].shape == (3, 64, 64, 3)
    for i, t in enumerate(times):
        assert ltrace.shade_stokes(*rec, float(t)).tobytes() == seq["stokes"][i].tobytes()
    assert ltrace.hotspot_lightcurve_stokes(*rec, 0.0, 10.0, 3).tobytes() == seq["stokes_lightcurve"].tobytes()
    assert np.array_equal(seq["stokes_lightcurve"][:, 0], seq["lightcurve"][:, 0])
    # the numpy statements on the same records
    ref = diskmod.stokes_frame(M, a, direct["hits"], direct["n_hits"], direct["pol"], dk, spot, 10.0, FIELD)
    assert np.max(ulps(seq["stokes"][1], ref)) <= 2
    lc = diskmod.stokes_lightcurve(M, a, direct["hits"], direct["n_hits"], direct["pol"], spot, times, FIELD)
    assert np.max(np.abs(lc - seq["stokes_lightcurve"])) <= 1e-12 * lc[:, 0].max()
    batch = metric.trace_rays_batch_disk_pol(ro, [0.15, 0.2], [0.4, 2.0], tho, dk, FIELD)
    assert batch["pol"].shape == (2, 3, 4) and batch["n_hits"].max() >= 1


def test_cli_stokes(tmp_path):
    out = str(tmp_path / "pol.png")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "light-path-tracer_amd"))
    base = [sys.executable, os.path.join(ROOT, "light-path-tracer_amd", "image_lens.py"), "--a", "0.9", "--theta-obs", "80", "--r-obs", "50",
            "--disk-images", "3", "--synthetic", "64", "48", "--bfield", "0.3", "0.8", "0.5", "--pol-frac", "0.6", "--output", out]
    subprocess.run(base, check=True, env=env, timeout=120)
    disk_only = np.load(str(tmp_path / "pol_stokes_0000.npy"))
    assert disk_only.shape == (48, 64, 3) and (disk_only[..., 0] > 0).sum() > 200
    assert np.all(np.hypot(disk_only[..., 1], disk_only[..., 2]) <= 0.6 * disk_only[..., 0] * (1 + 1e-6))
    subprocess.run(base + ["--hotspot", "8", "0.5", "1.5", "--times", "0", "10", "2"], check=True, env=env, timeout=120)
    lc = np.load(str(tmp_path / "pol_stokes_lightcurve.npy"))
    frames = [np.load(str(tmp_path / f"pol_stokes_{i:04d}.npy")) for i in range(2)]
    assert lc.shape == (2, 3) and np.all(lc[:, 0] > 0) and not np.array_equal(frames[0], frames[1])


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ph.test_refusals()
    cam, met, o, d = frame_setup()
    inside = ltrace.Camera(64, 48, 0.7, 0.5, 0.0, 0.0, 1.9, np.pi / 2)    # inside the ergosphere: no static observer
    with pytest.raises(ltrace.LtraceError):
        ltrace.trace_disk_pol(inside, met, o, d, lt_field())
    with pytest.raises(ltrace.LtraceError) as ei:
        ltrace.polarization_probe(met, 1.9, np.pi / 2, [2.0], [[8.0, -0.5, 1.0]], [[-0.99, 2.0]], lt_field())
    assert ei.value.code == ltrace.ERR_INVALID_ARG
