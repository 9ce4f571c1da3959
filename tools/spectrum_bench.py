"""What the energy-resolved reduction costs, on the README's sequence frame: 1024^2, Kerr a = 0.9, r_obs = 50,
theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4 float32 -- and on its S = 4 fine
records (4096^2).  Grid: 96 bins on the default range, one plane and one per image order, 24 times over one orbit at
r = 8, for the spot (r 8, phi0 0, sigma 1.5) and for a 256 x 1024 Keplerian table (disk.spiral_map); device buffers.

Two yardsticks, both of which exist without the spectrum kernels:
  (a) the emitter's own light curve on the same records and times (lt_hotspot_lightcurve_dev, lt_diskmap_lightcurve_dev):
      the same evaluation with a three-number reduction, so it is the floor;
  (b) what a user had to do before: shade nothing, copy the records to the host once (timed), and run the numpy statement
      (disk.hotspot_spectrum / disk.diskmap_spectrum) -- timed on --numpy-times times (1 on the fine records) and scaled
      to the 24, because it is a per-time loop.
The convention is tools/diskmap_bench.py's: a sample is --batch calls back to back behind one untimed call and before one
synchronise, the time per call; the candidates run alternately, --reps rounds after one warm-up round; reported: the
median and the range.  No gate.

    python tools/spectrum_bench.py [--size 1024] [--samples 1,4] [--reps 5] [--times 24] [--batch 5] [--numpy-times 3]
                                   [--no-numpy] [--out profiles/spectrum_bench_<build>.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "light-path-tracer_amd"), os.path.join(ROOT, "tests")]

import disk as diskmod  # noqa: E402
import ltrace  # noqa: E402

M_IMAGES = 3
TABLE = (256, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", default="1,4", help="1: the frame's own records; S: the fine records of the S x S supersampled sequence")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--times", type=int, default=24)
    ap.add_argument("--batch", type=int, default=5, help="calls per sample")
    ap.add_argument("--numpy-times", type=int, default=3, help="times the numpy statement is run on (1 on fine records)")
    ap.add_argument("--no-numpy", action="store_true", help="skip yardstick (b): for comparing builds of the kernels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n, T = args.size, args.times
    vfov = np.radians(40.0)
    M, a = 1.0, 0.9
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    disk = ltrace.default_disk(r_out=20.0)
    spot_py = diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5)
    spot = spot_py.to_lt()
    r_in = ltrace.kerr_isco(M, a)
    dmap_py = diskmod.DiskMap(diskmod.spiral_map(*TABLE, r_min=r_in, r_max=20.0), r_min=r_in, r_max=20.0, rotation="kepler")
    dmap, texels = dmap_py.to_lt(), dmap_py.texels
    grids = {"whole": diskmod.Spectrum(), "split": diskmod.Spectrum(split_orders=True)}
    dt = 2 * np.pi * (8.0 ** 1.5 + 0.9) / T
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=a, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=r_in, r_out=20.0,
               max_images=M_IMAGES, table=list(TABLE), spot=[8.0, 0.0, 1.5], n_bins=96, n_times=T, reps=args.reps, batch=args.batch,
               spectrum_blocks=ltrace.SPECTRUM_BLOCKS, integrator="rk4", precision=32, results={})
    sync = lambda: hipmini.hip().hipStreamSynchronize(None)

    def upload(host):
        host = np.ascontiguousarray(host)
        d = hipmini.DeviceArray(host.shape, host.dtype)
        if hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1):
            raise RuntimeError("hipMemcpy to the device failed")
        return d

    def alternately(calls, reps, batch):
        """{name: median ms per call and [min, max]}: the calls one after the other, `reps` rounds after one warm-up round."""
        ms = {k: [] for k in calls}
        for rep in range(reps + 1):
            for name, fn in calls.items():
                fn()
                sync()
                t0 = time.perf_counter()
                for _ in range(batch):
                    fn()
                sync()
                if rep:
                    ms[name].append(1e3 * (time.perf_counter() - t0) / batch)
        return {k: dict(ms=round(float(np.median(v)), 4), range_ms=[round(min(v), 4), round(max(v), 4)]) for k, v in ms.items()}

    o = ltrace.default_opts(integrator="rk4", precision=32, tb_symmetry=0)
    d_tex = upload(texels)
    for S in [int(x) for x in args.samples.split(",")]:
        R = n * S
        cam = ltrace.Camera(R, R, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
        rec = ltrace.trace_disk_hits(cam, met, o, disk, max_images=M_IMAGES, want=("hits", "n_hits"))
        d_hits, d_n = upload(rec["hits"]), upload(rec["n_hits"])
        stored = int(np.minimum(rec["n_hits"], M_IMAGES).sum(dtype=np.int64))
        row = dict(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes), stored_slots=stored)
        d_lc = hipmini.DeviceArray((T, 3), np.float64)
        d_sp = hipmini.DeviceArray((T, M_IMAGES, 98), np.float64)
        head = (d_hits.ptr, d_n.ptr, R, R, M_IMAGES, met, disk)
        calls = {"lightcurve_spot": lambda: ltrace.hotspot_lightcurve_dev(*head, spot, 0.0, dt, T, d_lc.ptr),
                 "lightcurve_map": lambda: ltrace.diskmap_lightcurve_dev(*head, dmap, d_tex.ptr, 0.0, dt, T, d_lc.ptr)}
        for gname, grid in grids.items():
            sp = grid.to_lt()
            calls[f"spectrum_spot_{gname}"] = lambda sp=sp: ltrace.hotspot_spectrum_dev(*head, spot, sp, 0.0, dt, T, d_sp.ptr)
            calls[f"spectrum_map_{gname}"] = lambda sp=sp: ltrace.diskmap_spectrum_dev(*head, dmap, d_tex.ptr, sp, 0.0, dt, T, d_sp.ptr)
        calls["line_disk_whole"] = lambda: ltrace.disk_spectrum_dev(*head, grids["whole"].to_lt(), d_sp.ptr)
        gpu = alternately(calls, args.reps, args.batch)
        row["gpu"] = gpu
        copy_ms, numpy_ms = None, {}
        if not args.no_numpy:
            # (b): the records to the host once, then the numpy statement
            host_hits, host_n = np.empty_like(rec["hits"]), np.empty_like(rec["n_hits"])
            sync()
            t0 = time.perf_counter()
            for host, dev in ((host_hits, d_hits), (host_n, d_n)):
                if hipmini.hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(dev.ptr), host.nbytes, 2):
                    raise RuntimeError("hipMemcpy to the host failed")
            copy_ms = 1e3 * (time.perf_counter() - t0)
            k = 1 if S > 1 else max(1, min(args.numpy_times, T))
            times = dt * np.arange(k)
            numpy_ms = {}
            for name, fn in (("spot", lambda g: diskmod.hotspot_spectrum(M, a, host_hits, host_n, spot_py, g, times)),
                             ("map", lambda g: diskmod.diskmap_spectrum(M, a, host_hits, host_n, dmap_py, g, times))):
                t0 = time.perf_counter()
                got = fn(grids["whole"])
                numpy_ms[name] = 1e3 * (time.perf_counter() - t0) / k
                if name == "spot" and S == 1:     # the statement timed is the one the kernel restates
                    same = ltrace.hotspot_spectrum(host_hits, host_n, met, disk, spot, grids["whole"].to_lt(), 0.0, dt, k)
                    row["numpy_agrees"] = bool(np.allclose(got, same, rtol=1e-9, atol=0.0))
            row["numpy"] = dict(copy_ms=round(copy_ms, 2), times_run=k, ms_per_time=dict((kk, round(v, 2)) for kk, v in numpy_ms.items()),
                                ms_scaled_to_n_times=dict((kk, round(copy_ms + v * T, 1)) for kk, v in numpy_ms.items()))
        ratios = {}
        for em in ("spot", "map"):
            for gname in grids:
                s_ms = gpu[f"spectrum_{em}_{gname}"]["ms"]
                ratios[f"{em}_{gname}"] = dict(spectrum_over_lightcurve=round(s_ms / gpu[f"lightcurve_{em}"]["ms"], 3))
                if numpy_ms:
                    ratios[f"{em}_{gname}"]["numpy_over_spectrum"] = round((copy_ms + numpy_ms[em] * T) / s_ms, 1)
        row["ratios"] = ratios
        res["results"][f"S{S}"] = row
        print(f"S = {S}:", json.dumps(row), flush=True)
        del rec, d_hits, d_n
    out = args.out or os.path.join(ROOT, "profiles", f"spectrum_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
