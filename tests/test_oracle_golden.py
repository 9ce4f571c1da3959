"""Pin the oracle (oracle/lt_oracle.c) against golden vectors generated from the
imported reference (tests/golden/make_golden.py).  CPU only.

Tolerances: the oracle repeats the reference's float64 operations in the same
order, so agreement is to libm last-bit effects (numpy's sin/cos vs glibc's),
amplified only on chaotic near-critical rays.
"""
import glob
import json
import os

import numpy as np
import pytest

from oracle import oracle


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name), allow_pickle=False)


def test_kerr_rhs_matches_reference(golden_dir):
    """F1: metrics.py:221-303."""
    g = _load(golden_dir, "kerr_rhs.npz")
    for inp, exp in zip(g["inputs"], g["outputs"]):
        out = oracle.kerr_rhs(inp[:5], inp[5], inp[6], inp[7], inp[8], inp[9])
        np.testing.assert_allclose(out, exp, rtol=1e-12, atol=1e-300)


def test_kerr_initial_conditions_match_reference(golden_dir):
    """F2: metrics.py:148-218."""
    g = _load(golden_dir, "kerr_ic.npz")
    for inp, exp in zip(g["inputs"], g["outputs"]):
        ok, st, p_t, p_phi = oracle.kerr_ic(*inp)
        assert float(ok) == exp[0]
        if ok:
            np.testing.assert_allclose(np.concatenate([st, [p_t, p_phi]]), exp[1:], rtol=1e-13, atol=1e-13)


RAY_FILES = sorted(os.path.basename(p) for p in
                   glob.glob(os.path.join(os.path.dirname(__file__), "golden", "rays_*.npz")))


@pytest.mark.parametrize("name", RAY_FILES)
def test_per_ray_traces_match_reference(golden_dir, name):
    """F3: metrics.py:120-145 (schw), :419-567 (dp45), :570-658 (rk4)."""
    g = _load(golden_dir, name)
    meta = json.loads(str(g["meta"]))
    if meta["kind"] == "schw":
        fa, nh, st, ev = oracle.trace_batch_schw(meta["M"], meta["r_obs"], g["alpha"])
    else:
        fa, nh, st, ev = oracle.trace_batch_kerr(meta["M"], meta["a"], meta["r_obs"], g["alpha"],
                                                 g["theta"], theta_obs=meta.get("theta_obs", np.pi / 2),
                                                 axis_refines=g["refine"], integrator=meta["kind"])
    n = fa.size
    same_status = st == g["status"]
    # chaotic near-critical rays may flip on last-bit libm differences: allow <= 1e-4 of pixels
    assert (~same_status).sum() <= max(1, int(1e-4 * n)), f"{(~same_status).sum()} status flips"
    esc = same_status & (st == 1)
    d = np.abs(fa[esc] - g["final_alpha"][esc])
    assert np.nanmax(d) < 1e-6
    assert np.quantile(d, 0.99) <= 1e-9
    ok = same_status
    assert (nh[ok] != g["n_half"][ok]).sum() <= max(1, int(1e-4 * n))
    # RHS evaluation counts are the workload shape: identical except on flipped rays
    assert (ev[ok].astype(np.int64) != g["rhs_evals"][ok]).sum() <= max(2, int(2e-4 * n))
    assert abs(ev.mean() - g["rhs_evals"].mean()) <= 1e-3 * g["rhs_evals"].mean()
    # non-escaped rays carry NaN (metrics.py:667, :678)
    assert np.all(np.isnan(fa[st != 1]) | (st[st != 1] == 1))


def test_psi_frame_and_pixel_angles(golden_dir):
    """F6: image_lens.py:21-69, :72-93."""
    g = _load(golden_dir, "psi_frame.npz")
    for row in g["frames"]:
        d, ex, ey, front = oracle.psi_frame((row[0], row[1]))
        np.testing.assert_allclose(np.concatenate([d, ex, ey]), row[2:11], rtol=0, atol=1e-15)
        assert float(front) == row[11]
    dims = (48, 64)
    fov = (np.radians(52.0), np.radians(40.0))
    for row in g["pix"]:
        al, th, _ = oracle.pixel_angles(dims[0], dims[1], fov[0], fov[1], psi=(row[0], row[1]))
        iy, ix = int(row[2]), int(row[3])
        assert al[iy, ix] == np.float32(row[4])
        if row[4] > 1e-9:     # theta of the BH-centre pixel is atan2(0, 0)-like noise
            assert abs(th[iy, ix] - row[5]) <= 1e-12


LOOKUPS = ["4x6_a0", "4x6_a0p9", "48x64_a0", "48x64_a0p9", "48x64_a0_psi", "48x64_a0p9_psi", "33x40_a0p9"]


@pytest.mark.parametrize("name", LOOKUPS)
def test_lookup_and_render_match_reference(golden_dir, name):
    """F4/F5: image_lens.py:133-152, :155-178, :185-280 (incl. quirks Q1, Q2), :296-397."""
    g = _load(golden_dir, f"lookup_{name}.npz")
    m = json.loads(str(g["meta"]))
    H, W = m["h"], m["w"]
    psi = tuple(m["psi"])
    al, _, _ = oracle.pixel_angles(H, W, m["hfov"], m["vfov"], psi=psi)
    np.testing.assert_array_equal(al, g["alpha_lookup"])        # float32, bit-exact
    kind = "schwarzschild" if m["a"] == 0 else "kerr"
    lk = oracle.lookup(kind, m["M"], m["a"], m["r_obs"], H, W, m["hfov"], m["vfov"], psi=psi,
                       integrator="dp45", tb_symmetry=True)
    assert lk["traced"] == m["traced"]
    fa_ref = g["final_alpha"]
    nan_same = np.isnan(lk["fa"]) == np.isnan(fa_ref)
    assert (~nan_same).sum() <= 1
    both = ~np.isnan(lk["fa"]) & ~np.isnan(fa_ref)
    assert np.max(np.abs(lk["fa"][both] - fa_ref[both])) <= 2e-6
    assert (lk["winding"][nan_same] != g["winding"][nan_same]).sum() <= 1
    # colouring: feed the REFERENCE's lookup so the comparison is exact
    for key, kw in (("lensed", {}), ("lensed_wrap", {"loop_around": True})):
        img = oracle.render(g["background"], fa_ref, g["winding"], m["hfov"], m["vfov"], psi=psi, **kw)
        np.testing.assert_array_equal(img, g[key])
    gray = oracle.render(g["background"][..., 1].copy(), fa_ref, g["winding"], m["hfov"], m["vfov"], psi=psi)
    np.testing.assert_array_equal(gray, g["lensed_gray"])


def test_q1_tb_symmetry_off_by_one(golden_dir):
    """Quirk Q1 (image_lens.py:220, :272-276): mirrored rows are H-1-j, not H-j."""
    g = _load(golden_dir, "lookup_48x64_a0p9.npz")
    fa = g["final_alpha"]
    H = fa.shape[0]
    np.testing.assert_array_equal(np.isnan(fa[H - 1]), np.isnan(fa[0]))
    np.testing.assert_array_equal(fa[H - 1][~np.isnan(fa[0])], fa[0][~np.isnan(fa[0])])


def test_shadow_analytic(golden_dir):
    """F9: black_hole_shadow.py:7-15, :32-37."""
    g = _load(golden_dir, "shadow_analytic.npz")
    img = oracle.shadow_analytic(64, 64, np.radians(40), float(g["alpha_crit"]))
    np.testing.assert_array_equal(img, g["image"])


def test_schwarzschild_traced_shadow_equals_analytic():
    """KAT-2: traced non-escaped set == alpha < alpha_crit set."""
    n = 96
    fov = np.radians(40.0)
    al, _, _ = oracle.pixel_angles(n, n, fov, fov)
    fa, _, st, _ = oracle.trace_batch_schw(1.0, 50.0, al.ravel().astype(np.float64))
    alpha_crit = 0.10200015330371326      # scalars.json schw_alpha_crit["50.0"]
    assert np.array_equal(st != 1, al.ravel().astype(np.float64) < alpha_crit)


def test_scalar_kats(golden_dir):
    """F7: single-ray known answers."""
    with open(os.path.join(golden_dir, "scalars.json")) as f:
        s = json.load(f)
    for key, (fa_e, nh_e, oc) in s["schw_trace_ray"].items():
        fa, nh, st, _ = oracle.trace_batch_schw(1.0, 50.0, np.array([float(key)]))
        assert {1: "escaped", -1: "captured", 0: "invalid"}[int(st[0])] == oc
        if fa_e is not None:
            assert abs(fa[0] - fa_e) < 1e-12
        if oc != "invalid":
            assert nh[0] == nh_e
    for a_key, rec in s["kerr"].items():
        a = float(a_key)
        for rk, ray in rec["rays"].items():
            al, th, rf = rk.split(",")
            for integ in ("dp45", "rk4"):
                fa, nh, st, _ = oracle.trace_batch_kerr(1.0, a, 50.0, [float(al)], [float(th)],
                                                        axis_refines=[int(rf)], integrator=integ)
                exp = ray[integ]
                assert int(st[0]) == exp[0]
                if exp[1] is not None:
                    assert abs(fa[0] - exp[1]) < 1e-10
                if exp[0] != 0:
                    assert nh[0] == exp[2]


# ---------------------------------------------------------------------------------------------
# F10: the dense single-ray path (oracle/lt_oracle_dense.c) against the reference's integrate_geodesic
# ---------------------------------------------------------------------------------------------
def test_rhs8_matches_reference(golden_dir):
    """metrics.py:763-790 (Schwarzschild) and :946-1029 (Kerr) on random off-shell states."""
    g = _load(golden_dir, "dense_tracks.npz")
    for (M, a), st, exp in zip(g["rhs_M_a"], g["rhs_state"], g["rhs_out"]):
        out = oracle.rhs8(0 if a == 0 else 1, M, a, st)
        np.testing.assert_allclose(out, exp, rtol=1e-13, atol=1e-300)


def test_dense_tracks_match_solve_ivp(golden_dir):
    """geodesic_tracer.py:22-71: the restated RK45 takes solve_ivp's steps -- same number of points, same nfev,
    same ending -- and every point agrees to 1e-8 (measured 1.3e-9: last-bit differences of the stage sums
    move the adaptive step sizes by ~1e-11)."""
    g = _load(golden_dir, "dense_tracks.npz")
    off = g["offsets"]
    for i in range(len(off) - 1):
        M, a = g["M_a"][i]
        lam, r_in, r_out = g["stops"][i]
        t, y, status, nfev = oracle.integrate_dense(int(g["metric_id"][i] > 0), M, a, g["state0"][i], lam, r_in, r_out)
        gt, gy = g["t"][off[i]:off[i + 1]], g["y"][:, off[i]:off[i + 1]]
        assert len(t) == len(gt) and nfev == g["nfev"][i], f"track {i}"
        assert (status in (1, 2)) == (g["ivp_status"][i] == 1) and (status == 0) == (g["ivp_status"][i] == 0)
        np.testing.assert_allclose(t, gt, rtol=0, atol=1e-7)
        assert np.max(np.abs(y - gy) / (1 + np.abs(gy))) < 1e-8, f"track {i}"
        lam_end = gt[-1]
        if status == 0:
            assert lam_end == lam
        else:  # the last point sits on the event radius
            assert abs(y[1, -1] - (r_in if status == 1 else r_out)) < 1e-9
        assert (1 if y[1, -1] > 1.1 * r_in else -1) == g["outcome"][i]
