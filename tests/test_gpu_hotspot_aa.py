"""The supersampled hot-spot and Stokes frames on the GPU (include/ltrace.h, "supersampled hot-spot and Stokes frames";
lt_hotspot_aa.hpp): lt_shade_hotspot_aa and lt_shade_stokes_aa, host and device forms, and the Python layers up to
image_lens.render_sequence(samples=S).

Every assertion is array_equal: there is no tolerance in this file.  The expectation is built from code that is not under
test -- the one-sample entry points lt_shade_hotspot / lt_shade_stokes on the FINE records (tests/test_gpu_hotspot_records.py
and tests/test_gpu_polarization.py hold them to a longdouble reference) and numpy's aa.resolve / aa.to_rgba8 -- and, on
records repeated S times per axis, from the one-sample entry points on the unrepeated records, which a wrong divisor or
a dropped lane cannot share with a mistaken reading of the rule (tests/test_hotspot_aa_host.py says why that is exact).

Shapes: the smallest that reach each edge of the slot arithmetic (P = 256 / S^2 output pixels per workgroup, the lanes
past P S^2 idle, slots numbered over all R W pixels so that a workgroup straddles output rows)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import aa
import disk as diskmod
import ltrace
from test_hotspot_aa_host import replicate
from test_hotspot_records_host import synth
from test_polarization_host import synth_pol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (output R, W, S, max_images, M, a, seed)
SHAPES = {"7x13-S3-K3": (7, 13, 3, 3, 1.0, 0.9, 81),      # P = 28, 4 idle lanes, 3 full workgroups + 7 slots
          "5x9-S5-K8": (5, 9, 5, 8, 1.0, -0.7, 82),       # P = 10, 6 idle lanes
          "3x11-S7-K1": (3, 11, 7, 1, 2.0, 1.2, 83),      # P = 5, 11 idle lanes
          "1x1-S8-K2": (1, 1, 8, 2, 1.0, 0.9, 84),        # P = 4, three dead slots
          "33x20-S2-K5": (33, 20, 2, 5, 1.0, -0.7, 85),   # P = 64, 10 workgroups + 20 slots
          "4x64-S1-K3": (4, 64, 1, 3, 2.0, 1.2, 86),      # S = 1: the one-sample entry points' own outputs
          "6x5-S4-K8": (6, 5, 4, 8, 1.0, 0.9, 87)}        # P = 16, two workgroups, the second with 14 slots
T_OBS = (0.0, 333.25, 1e5)
DISK_EXPOSURE = 0.25
_CASES = {}


class Case:
    def __init__(self, name):
        self.R, self.W, self.S, self.m, self.M, self.a, seed = SHAPES[name]
        R, W, S, m, M_ = self.R, self.W, self.S, self.m, self.M
        self.r_out = 20.0 * M_
        r_in = ltrace.kerr_isco(M_, self.a)
        self.hits, self.n_hits = synth(R * S, W * S, m, seed, r_in, self.r_out)              # the fine records
        self.pol = synth_pol((R * S, W * S, m), seed + 100)
        self.small = synth(R, W, m, seed + 200, r_in, self.r_out) + (synth_pol((R, W, m), seed + 300),)
        rng = np.random.default_rng(seed)
        self.base = {1: rng.uniform(0.0, 0.5, (R * S, W * S)).astype(np.float32),
                     3: rng.uniform(0.0, 0.5, (R * S, W * S, 3)).astype(np.float32)}
        self.small_base = {1: rng.uniform(0.0, 0.5, (R, W)).astype(np.float32), 3: rng.uniform(0.0, 0.5, (R, W, 3)).astype(np.float32)}
        self.met = ltrace.Metric(ltrace.METRIC_KERR, 0, M_, self.a)
        self.disk = ltrace.default_disk(r_out=self.r_out, exposure=DISK_EXPOSURE)
        self.field = ltrace.default_bfield(b_r=0.3, b_phi=0.8, b_z=0.5, pol_frac=0.7)

    def spot(self, with_disk):
        return ltrace.default_hotspot(r_spot=9.0 * self.M, phi0=0.5, sigma=1.5 * self.M, exposure=2.0, with_disk=with_disk)


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def bases(c, which):
    """(base, channels) variants: NULL with 3 and with 1 channel, a 1-channel and a 3-channel fine-size base."""
    return ((None, 3), (None, 1), (which[1], None), (which[3], None))


# ---- 1. against the one-sample entry points on the fine records ----------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_hotspot_frames_are_the_resolve_of_the_fine_frames(name):
    c = case(name)
    assert (c.n_hits > c.m).any() and (c.n_hits == 0).any()
    lit = 0
    for with_disk in (0, 1):
        s = c.spot(with_disk)
        for t_obs in T_OBS:
            for nh in (c.n_hits, None):
                for base, channels in bases(c, c.base):
                    fine = ltrace.shade_hotspot(c.hits, nh, c.met, c.disk, s, t_obs, base=base, channels=channels)
                    got = ltrace.shade_hotspot_aa(c.hits, nh, c.S, c.met, c.disk, s, t_obs, base=base, channels=channels)
                    want = aa.resolve(fine["rgb"], c.S)
                    assert got["rgb"].dtype == np.float32 and got["rgb"].shape == want.shape == ((c.R, c.W) if want.ndim == 2 else (c.R, c.W, 3))
                    assert np.array_equal(got["rgb"], want), (with_disk, t_obs, nh is None, channels)
                    assert np.array_equal(got["rgba"], aa.to_rgba8(want)), (with_disk, t_obs, nh is None, channels)
                    if c.S == 1:
                        assert np.array_equal(got["rgb"], fine["rgb"]) and np.array_equal(got["rgba"], fine["rgba"])
                    if base is None:
                        lit += int((want > 0).sum())
    assert lit > 0
    # either output alone
    s = c.spot(1)
    both = ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25)
    for k in ("rgb", "rgba"):
        assert np.array_equal(ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25, want=(k,))[k], both[k])


@pytest.mark.parametrize("name", list(SHAPES))
def test_stokes_frames_are_the_resolve_of_the_fine_frames(name):
    c = case(name)
    moved = 0
    for with_disk in (0, 1):
        s = c.spot(with_disk)
        for t_obs in T_OBS:
            for nh in (c.n_hits, None):
                fine = ltrace.shade_stokes(c.hits, nh, c.pol, c.met, c.disk, s, c.field, t_obs)
                got = ltrace.shade_stokes_aa(c.hits, nh, c.pol, c.S, c.met, c.disk, s, c.field, t_obs)
                want = aa.resolve(fine, c.S)
                assert got.dtype == np.float32 and got.shape == (c.R, c.W, 3)
                assert np.array_equal(got, want), (with_disk, t_obs, nh is None)
                if c.S == 1:
                    assert np.array_equal(got, fine)
                moved += int((want[..., 1:] != 0).sum())
    assert moved > 0


# ---- 2. on replicated records: the one-sample entry points on the unrepeated records ----------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_replicated_records_give_the_one_sample_frame(name):
    c = case(name)
    hits, n_hits, pol = c.small
    S = c.S
    big = (replicate(hits, S), replicate(n_hits, S), replicate(pol, S))
    for with_disk, t_obs in ((1, 333.25), (0, 1e5)):
        s = c.spot(with_disk)
        for use_counts in (True, False):
            nh, big_nh = (n_hits, big[1]) if use_counts else (None, None)
            for base, channels in bases(c, c.small_base):
                one = ltrace.shade_hotspot(hits, nh, c.met, c.disk, s, t_obs, base=base, channels=channels)
                got = ltrace.shade_hotspot_aa(big[0], big_nh, S, c.met, c.disk, s, t_obs, base=None if base is None else replicate(base, S),
                                              channels=channels)
                assert np.array_equal(got["rgb"], one["rgb"]) and np.array_equal(got["rgba"], one["rgba"]), (with_disk, use_counts, channels)
            one = ltrace.shade_stokes(hits, nh, pol, c.met, c.disk, s, c.field, t_obs)
            assert np.array_equal(ltrace.shade_stokes_aa(big[0], big_nh, big[2], S, c.met, c.disk, s, c.field, t_obs), one)


# ---- 3. device pointers, reproducible bits -----------------------------------------------------------------------------------
def upload(host):
    import hipmini
    host = np.ascontiguousarray(host)
    buf = hipmini.DeviceArray(host.shape, host.dtype)
    hipmini._ok(hipmini.hip().hipMemcpy(C.c_void_p(buf.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1), "hipMemcpy H2D")
    return buf


@pytest.mark.parametrize("name", ["7x13-S3-K3", "1x1-S8-K2", "33x20-S2-K5"])
def test_dev_forms_give_the_host_bytes(name):
    import hipmini
    c = case(name)
    s = c.spot(1)
    d_hits, d_n, d_pol = upload(c.hits), upload(c.n_hits), upload(c.pol)
    for base, channels in bases(c, c.base):
        host = ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25, base=base, channels=channels)
        again = ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25, base=base, channels=channels)
        assert np.array_equal(host["rgb"], again["rgb"]) and np.array_equal(host["rgba"], again["rgba"])
        nch = 1 if host["rgb"].ndim == 2 else 3
        d_base = upload(base) if base is not None else None
        for dn in (d_n.ptr, 0):
            want = host if dn else ltrace.shade_hotspot_aa(c.hits, None, c.S, c.met, c.disk, s, 333.25, base=base, channels=channels)
            d_rgb, d_rgba = hipmini.DeviceArray(host["rgb"].shape, np.float32), hipmini.DeviceArray((c.R, c.W, 4), np.uint8)
            ltrace.shade_hotspot_aa_dev(d_hits.ptr, dn, c.R, c.W, c.S, c.m, c.met, c.disk, s, 333.25, d_base=d_base.ptr if d_base else 0,
                                        channels=nch, d_rgb=d_rgb.ptr, d_rgba=d_rgba.ptr)
            assert np.array_equal(d_rgb.get(), want["rgb"]) and np.array_equal(d_rgba.get(), want["rgba"])
    host = ltrace.shade_stokes_aa(c.hits, c.n_hits, c.pol, c.S, c.met, c.disk, s, c.field, 333.25)
    assert np.array_equal(ltrace.shade_stokes_aa(c.hits, c.n_hits, c.pol, c.S, c.met, c.disk, s, c.field, 333.25), host)
    d_iqu = hipmini.DeviceArray((c.R, c.W, 3), np.float32)
    ltrace.shade_stokes_aa_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, c.R, c.W, c.S, c.m, c.met, c.disk, s, c.field, 333.25, d_iqu.ptr)
    assert np.array_equal(d_iqu.get(), host)


_TORCH = """
import sys
import numpy as np
import torch                      # before the library: torch's HIP runtime must be the first one the process initialises
sys.path[:0] = [{pkg!r}, {root!r}, {tests!r}]
import ltrace
import test_gpu_hotspot_aa as t
c = t.case(sys.argv[1])
s = c.spot(1)
dev = torch.device("cuda:0")
d_hits, d_n, d_pol, d_base = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (c.hits, c.n_hits, c.pol, c.base[3]))
d_rgb = torch.full((c.R, c.W, 3), -1.0, dtype=torch.float32, device=dev)
d_rgba = torch.zeros((c.R, c.W, 4), dtype=torch.uint8, device=dev)
d_iqu = torch.full((c.R, c.W, 3), -1.0, dtype=torch.float32, device=dev)
torch.cuda.synchronize()
ltrace.shade_hotspot_aa_dev(d_hits.data_ptr(), d_n.data_ptr(), c.R, c.W, c.S, c.m, c.met, c.disk, s, 333.25, d_base=d_base.data_ptr(),
                            channels=3, d_rgb=d_rgb.data_ptr(), d_rgba=d_rgba.data_ptr())
ltrace.shade_stokes_aa_dev(d_hits.data_ptr(), d_n.data_ptr(), d_pol.data_ptr(), c.R, c.W, c.S, c.m, c.met, c.disk, s, c.field, 333.25,
                           d_iqu.data_ptr())
torch.cuda.synchronize()
host = ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25, base=c.base[3])
assert np.array_equal(d_rgb.cpu().numpy(), host["rgb"]) and np.array_equal(d_rgba.cpu().numpy(), host["rgba"])
assert np.array_equal(d_iqu.cpu().numpy(), ltrace.shade_stokes_aa(c.hits, c.n_hits, c.pol, c.S, c.met, c.disk, s, c.field, 333.25))
print("torch tensors ok")
"""


def test_dev_forms_on_torch_tensors():
    """The _dev forms on device tensors held through torch (a process of its own: tests/hipmini.py says why)."""
    src = _TORCH.format(pkg=os.path.join(ROOT, "light-path-tracer_amd"), root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", src, "7x13-S3-K3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch tensors ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- 4. one traced case: render_sequence(samples=S) ------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 3])
def test_render_sequence_supersampled(S):
    import image_lens
    from metrics import Kerr
    H, W = 24, 20
    metric = Kerr(M=1.0, a=0.9, integrator="rk4", precision=32)
    dk = diskmod.TransparentDisk(r_out=20.0, max_images=3)
    spot = diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5)
    field = diskmod.BField(0.0, 0.0, 1.0)
    fov = (np.radians(40.0), np.radians(40.0))
    times = 10.0 * np.arange(3)
    src = None if S == 3 else image_lens.synthetic_background(H * S, W * S)        # one with a lensed sky under the frames
    kw = dict(theta_obs=np.radians(80.0), bfield=field)
    seq = image_lens.render_sequence(src, metric, 50.0, fov, dk, spot, times, shape=(H, W), samples=S, **kw)
    fine = image_lens.render_sequence(src, metric, 50.0, fov, dk, spot, times, shape=(H * S, W * S), **kw)
    assert seq["samples"] == S and "samples" not in fine
    assert fine["frames"].shape == (3, H * S, W * S, 3) and seq["frames"].shape == (3, H, W, 3)
    assert seq["rgba"].shape == (3, H, W, 4) and seq["stokes"].shape == (3, H, W, 3)
    for k in ("hits", "n_hits", "pol"):
        assert np.array_equal(np.asarray(seq[k]), np.asarray(fine[k]), equal_nan=True), k
    assert (np.asarray(fine["n_hits"]) > 0).sum() > 0.03 * H * W * S * S
    for i in range(3):
        want = aa.resolve(fine["frames"][i], S)
        assert np.array_equal(seq["frames"][i], want), i
        assert np.array_equal(seq["rgba"][i], aa.to_rgba8(want)), i
        assert np.array_equal(seq["stokes"][i], aa.resolve(fine["stokes"][i], S)), i
    assert not np.array_equal(seq["frames"][0], seq["frames"][2]) and np.any(seq["stokes"][..., 1] != 0)
    assert np.array_equal(seq["lightcurve"], fine["lightcurve"] / np.array([S * S, S ** 3, S ** 3], dtype=np.float64))
    assert np.array_equal(seq["stokes_lightcurve"], fine["stokes_lightcurve"] / np.float64(S * S))
    assert np.all(seq["lightcurve"][:, 0] > 0)


def test_render_sequence_one_sample_changes_no_bit():
    """samples=1 goes through the new entry points and gives what samples=None gives, light curves included."""
    import image_lens
    from metrics import Kerr
    metric = Kerr(M=1.0, a=0.9, integrator="rk4", precision=32)
    dk = diskmod.TransparentDisk(r_out=20.0, max_images=3)
    args = (None, metric, 50.0, (np.radians(40.0), np.radians(40.0)), dk, diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5), [0.0, 10.0])
    kw = dict(shape=(24, 20), theta_obs=np.radians(80.0), bfield=diskmod.BField(0.0, 0.0, 1.0))
    one, plain = image_lens.render_sequence(*args, samples=1, **kw), image_lens.render_sequence(*args, **kw)
    for k in ("frames", "rgba", "stokes", "lightcurve", "stokes_lightcurve", "hits", "n_hits", "pol"):
        assert np.asarray(one[k]).tobytes() == np.asarray(plain[k]).tobytes(), k


def test_cli_supersampled_sequence(tmp_path):
    import matplotlib.image as mpimg
    out = str(tmp_path / "seq.png")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "light-path-tracer_amd"))
    cmd = [sys.executable, os.path.join(ROOT, "light-path-tracer_amd", "image_lens.py"), "--a", "0.9", "--theta-obs", "80", "--r-obs", "50",
           "--disk-images", "3", "--synthetic", "20", "24", "--hotspot", "8", "0", "1.5", "--times", "0", "10", "2", "--bfield", "0", "0", "1",
           "--samples", "2", "--output", out]
    subprocess.run(cmd, check=True, env=env, timeout=120)
    png = mpimg.imread(str(tmp_path / "seq_0001.png"))
    assert png.shape[:2] == (24, 20) and np.load(str(tmp_path / "seq_stokes_0001.npy")).shape == (24, 20, 3)
    assert np.load(str(tmp_path / "seq_lightcurve.npy")).shape == (2, 3)
    r = subprocess.run(cmd + ["--adaptive", "1"], env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode != 0 and "not adaptively sampled" in r.stderr


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    c = case("7x13-S3-K3")
    lib = ltrace.load()
    schw = ltrace.Metric(ltrace.METRIC_SCHWARZSCHILD, 0, 1.0, 0.0)
    ptr = ltrace._np_ptr

    def hotspot(aa_form=True, hits=c.hits, R=c.R, W=c.W, S=c.S, m=c.m, met=c.met, disk=c.disk, spot=None, t_obs=333.25, channels=3):
        spot = spot or c.spot(1)
        rgb, rgba = np.full((c.R * c.S, c.W * c.S, 3), -7.0, np.float32), np.full((c.R * c.S, c.W * c.S, 4), 77, np.uint8)
        head = (ptr(hits), ptr(c.n_hits), R, W) + ((S,) if aa_form else ())
        fn = lib.lt_shade_hotspot_aa if aa_form else lib.lt_shade_hotspot
        rc = fn(*head, m, C.byref(met), C.byref(disk), C.byref(spot), t_obs, None, channels, ptr(rgb), ptr(rgba))
        if rc != ltrace.OK:
            assert np.all(rgb == -7.0) and np.all(rgba == 77)
        return rc

    def stokes(aa_form=True, pol=c.pol, S=c.S, met=c.met, spot=None, field=c.field, t_obs=333.25, no_out=False, m=c.m):
        spot = spot or c.spot(1)
        iqu = np.full((c.R * c.S, c.W * c.S, 3), -7.0, np.float32)
        head = (ptr(c.hits), ptr(c.n_hits), ptr(pol), c.R, c.W) + ((S,) if aa_form else ())
        fn = lib.lt_shade_stokes_aa if aa_form else lib.lt_shade_stokes
        rc = fn(*head, m, C.byref(met), C.byref(c.disk), C.byref(spot), C.byref(field), t_obs, None if no_out else ptr(iqu))
        if rc != ltrace.OK:
            assert np.all(iqu == -7.0)
        return rc

    assert hotspot() == ltrace.OK and stokes() == ltrace.OK
    for S in (0, -1, 9):
        assert hotspot(S=S) == ltrace.ERR_INVALID_ARG and stokes(S=S) == ltrace.ERR_INVALID_ARG
    assert hotspot(S=9, met=schw) == ltrace.ERR_INVALID_ARG            # samples is looked at first
    # what the one-sample entry points refuse, with their codes
    nan_q = ltrace.default_disk(q=float("nan"))
    for kw in (dict(hits=None), dict(met=schw), dict(met=ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 1.5)), dict(R=0), dict(W=-3), dict(m=0),
               dict(m=9), dict(spot=ltrace.default_hotspot(sigma=0.0)), dict(spot=ltrace.default_hotspot(r_spot=-1.0)),
               dict(spot=ltrace.default_hotspot(exposure=float("inf"))), dict(disk=nan_q), dict(channels=2), dict(t_obs=float("nan")),
               dict(t_obs=float("inf")),
               # two faults at once: the first in the one-sample entry point's order decides
               dict(met=schw, channels=2), dict(m=0, spot=ltrace.default_hotspot(sigma=0.0)), dict(channels=2, t_obs=float("nan"))):
        want = hotspot(aa_form=False, **kw)
        assert want in (ltrace.ERR_INVALID_ARG, ltrace.ERR_UNSUPPORTED), kw
        assert hotspot(**kw) == want, kw
    assert hotspot(met=schw) == ltrace.ERR_UNSUPPORTED and hotspot(met=schw, channels=2) == ltrace.ERR_UNSUPPORTED
    for kw in (dict(pol=None), dict(met=schw), dict(field=ltrace.default_bfield(b_z=0.0)), dict(field=ltrace.default_bfield(pol_frac=1.5)),
               dict(spot=ltrace.default_hotspot(sigma=-1.0)), dict(t_obs=float("nan")), dict(no_out=True), dict(m=9),
               dict(met=schw, pol=None), dict(field=ltrace.default_bfield(b_z=0.0), t_obs=float("nan"))):
        want = stokes(aa_form=False, **kw)
        assert want in (ltrace.ERR_INVALID_ARG, ltrace.ERR_UNSUPPORTED), kw
        assert stokes(**kw) == want, kw
    # and the library still works
    s = c.spot(1)
    fine = ltrace.shade_hotspot(c.hits, c.n_hits, c.met, c.disk, s, 333.25)
    assert np.array_equal(ltrace.shade_hotspot_aa(c.hits, c.n_hits, c.S, c.met, c.disk, s, 333.25)["rgb"], aa.resolve(fine["rgb"], c.S))
