"""CPU tests of the thin accretion disk: the ISCO, the redshift and shading formulas of disk.py, the defaults of
lt_default_disk and the entry points' answer on a machine without a GPU (include/ltrace.h, lt_render_disk)."""
import ctypes as C

import numpy as np
import pytest

import disk
import ltrace
import metrics

KNOWN_ISCO = [(0.0, 6.0), (1.0, 1.0), (-1.0, 9.0), (0.5, 4.2330), (0.9, 2.3209)]


@pytest.mark.parametrize("a,r", KNOWN_ISCO)
def test_isco_known_values(a, r):
    assert ltrace.kerr_isco(1.0, a) == pytest.approx(r, abs=5e-5)
    assert float(disk.isco(1.0, a)) == pytest.approx(r, abs=5e-5)
    assert metrics.Kerr(1.0, a).isco() == pytest.approx(r, abs=5e-5)


@pytest.mark.parametrize("a", [0.0, 0.3, -0.6, 0.998])
def test_isco_scales_linearly_in_mass(a):
    for M in (0.5, 2.0, 7.0):
        assert ltrace.kerr_isco(M, a * M) == pytest.approx(M * ltrace.kerr_isco(1.0, a), rel=1e-13)
        assert float(disk.isco(M, a * M)) == pytest.approx(M * float(disk.isco(1.0, a)), rel=1e-13)
    assert ltrace.kerr_isco(1.0, a) == pytest.approx(float(disk.isco(1.0, a)), rel=1e-14)


def test_isco_rejects_bad_metric():
    assert np.isnan(ltrace.kerr_isco(1.0, 1.5)) and np.isnan(ltrace.kerr_isco(0.0, 0.0))


def test_redshift_schwarzschild_zero_xi():
    r = np.linspace(6.0, 40.0, 50)
    for M in (1.0, 2.5):
        np.testing.assert_allclose(disk.redshift(M, 0.0, r * M, 0.0), np.sqrt(1.0 - 3.0 / r), rtol=1e-14)


def test_redshift_monotone_in_omega_xi():
    for a in (0.0, 0.9, -0.7):
        for r in (disk.isco(1.0, a), 10.0, 30.0):
            om = disk.omega(1.0, a, r)
            xi = np.linspace(-8.0, 0.95 / om, 101)     # photons that can reach the camera: Omega xi < 1
            g = disk.redshift(1.0, a, r, xi)
            assert om > 0
            assert np.all(np.diff(g) > 0)    # g = 1 / (u^t (1 - Omega xi)) grows with Omega xi (while Omega xi < 1)
            assert np.all(np.diff(g[np.argsort(om * xi)]) > 0)


def test_u_t_normalisation():
    # a circular equatorial geodesic is timelike: g_tt + 2 g_tphi Omega + g_phiphi Omega^2 = -1 / (u^t)^2
    for a in (0.0, 0.9, -0.7, 0.998):
        r = np.linspace(float(disk.isco(1.0, a)), 30.0, 20)
        om, ut = disk.omega(1.0, a, r), disk.u_t(1.0, a, r)
        g_tt = -(1 - 2 / r)
        g_tp = -2 * a / r
        g_pp = r * r + a * a + 2 * a * a / r
        np.testing.assert_allclose(g_tt + 2 * g_tp * om + g_pp * om * om, -1.0 / ut ** 2, rtol=1e-12)


def test_shade_formula():
    r, g = np.array([6.0, 9.0, 15.0]), np.array([0.6, 1.0, 1.3])
    rgb = disk.shade(r, g, 6.0)
    x = 6.0 / r
    s = g * x ** 0.75
    ref = np.clip((g ** 4 * x ** 3)[:, None] * np.clip(2 * s[:, None] - 0.5 * np.arange(3), 0, 1), 0, 1)
    np.testing.assert_array_equal(rgb, ref.astype(np.float32))
    np.testing.assert_array_equal(disk.shade(r, g, 6.0, channels=1), ((ref[:, 0] + ref[:, 1] + ref[:, 2]) / 3).astype(np.float32))
    assert rgb.dtype == np.float32


def test_default_disk():
    d = ltrace.default_disk()
    assert (d.r_in, d.r_out, d.q, d.exposure, d.flags) == (0.0, 20.0, 3.0, 1.0, 0)
    assert C.sizeof(ltrace.Disk) == 4 * 8 + 8
    t = disk.ThinDisk()
    assert (t.r_in, t.r_out, t.q, t.exposure) == (None, 20.0, 3.0, 1.0)
    assert t.inner_edge(1.0, 0.9) == pytest.approx(2.3209, abs=5e-5)
    lt = t.to_lt()
    assert (lt.r_in, lt.r_out, lt.q, lt.exposure) == (0.0, 20.0, 3.0, 1.0)


def test_no_device_answers(monkeypatch):
    if ltrace.device_count() > 0:
        pytest.skip("a GPU is visible: the no-device answer is for machines without one")
    lib = ltrace.load()
    cam = ltrace.Camera(16, 16, 0.5, 0.5, 0.0, 0.0, 50.0, 1.4)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    o = ltrace.default_opts()
    d = ltrace.default_disk()
    rc = lib.lt_render_disk(C.byref(cam), C.byref(met), C.byref(o), C.byref(d), None, 3, None, None, None, None, None,
                            None, None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    al = np.zeros(4)
    rc = lib.lt_trace_batch_kerr_disk(1.0, 0.9, 50.0, al.ctypes.data, al.ctypes.data, 1.4, 5000.0, None, 1, 32,
                                      C.byref(d), 4, None, None, None, None, None)
    assert rc == ltrace.ERR_NO_DEVICE
    with pytest.raises(ltrace.LtraceError):
        ltrace.trace_batch_kerr_disk(1.0, 0.9, 50.0, al, al, 1.4, 5000.0, d)
