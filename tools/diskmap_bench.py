"""What the rotating emissivity map's re-shade costs beside the hot spot's, on the README's sequence frame: 1024^2, Kerr
a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4 float32; a
256 x 1024 table (disk.spiral_map) over the disk's annulus, Keplerian and rigid; device buffers throughout.

The yardsticks are the hot spot's own kernels on the same records in the same session -- lt_shade_hotspot_dev (S = 1),
lt_shade_hotspot_aa_dev (S = 4, the fine 4096^2 records) and lt_hotspot_lightcurve_dev at 256 times, spot (r 8, phi0 0,
sigma 1.5) -- never the new kernels themselves.  The convention is tools/hotspot_aa_bench.py's: a sample is --batch
launches back to back behind one untimed launch and before one synchronise, the time per launch; the candidates run
alternately, --reps rounds after one warm-up round; reported: the median and the range.  A light-curve call is 256 times
in one launch pair, so its batch is --lc-batch.  No gate.

At 1024^2 a one-sample launch is about 0.02 ms, the order of the host's cost of enqueueing it, so the kernels themselves
are also compared on a larger frame: --size 4096 --samples 1 (written beside the first file).

    python tools/diskmap_bench.py [--size 1024] [--samples 1,4] [--reps 3] [--times 256] [--batch 50] [--lc-batch 5]
                                  [--out profiles/diskmap_bench_<build>.json]
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
    ap.add_argument("--samples", default="1,4", help="the S to measure: 1 = the one-sample kernels and the light curve, else the aa kernels")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--times", type=int, default=256)
    ap.add_argument("--batch", type=int, default=50, help="launches per sample of a frame call")
    ap.add_argument("--lc-batch", type=int, default=5, help="calls per sample of a light-curve call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n = args.size
    vfov = np.radians(40.0)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    spot = ltrace.default_hotspot(r_spot=8.0, phi0=0.0, sigma=1.5)
    r_in = ltrace.kerr_isco(1.0, 0.9)
    texels = diskmod.spiral_map(*TABLE, r_min=r_in, r_max=20.0)
    maps = {"kepler": diskmod.DiskMap(texels, r_min=r_in, r_max=20.0, rotation="kepler").to_lt(),
            "rigid": diskmod.DiskMap(texels, r_min=r_in, r_max=20.0, rotation="rigid", omega_p=1.0 / (8.0 ** 1.5 + 0.9)).to_lt()}
    period = 2 * np.pi * (8.0 ** 1.5 + 0.9)
    dt = period / args.times
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=r_in, r_out=20.0,
               max_images=M_IMAGES, table=list(TABLE), spot=[8.0, 0.0, 1.5], n_times=args.times, reps=args.reps, batch=args.batch,
               lc_batch=args.lc_batch, integrator="rk4", precision=32, results={})
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
        d_out, d_out8 = hipmini.DeviceArray((n, n, 3), np.float32), hipmini.DeviceArray((n, n, 4), np.uint8)
        row = dict(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes))
        if S == 1:
            calls = {f"diskmap_{k}": (lambda dm=dm: ltrace.shade_diskmap_dev(d_hits.ptr, d_n.ptr, n, n, M_IMAGES, met, disk, dm, d_tex.ptr, 40.0,
                                                                             d_rgb=d_out.ptr, d_rgba=d_out8.ptr)) for k, dm in maps.items()}
            calls["hotspot"] = lambda: ltrace.shade_hotspot_dev(d_hits.ptr, d_n.ptr, n, n, M_IMAGES, met, disk, spot, 40.0, d_rgb=d_out.ptr,
                                                                d_rgba=d_out8.ptr)
        else:
            calls = {f"diskmap_aa_{k}": (lambda dm=dm: ltrace.shade_diskmap_aa_dev(d_hits.ptr, d_n.ptr, n, n, S, M_IMAGES, met, disk, dm, d_tex.ptr,
                                                                                   40.0, d_rgb=d_out.ptr, d_rgba=d_out8.ptr))
                     for k, dm in maps.items()}
            calls["hotspot_aa"] = lambda: ltrace.shade_hotspot_aa_dev(d_hits.ptr, d_n.ptr, n, n, S, M_IMAGES, met, disk, spot, 40.0,
                                                                      d_rgb=d_out.ptr, d_rgba=d_out8.ptr)
        row["frame"] = alternately(calls, args.reps, args.batch)
        if S == 1:
            d_lc = hipmini.DeviceArray((args.times, 3), np.float64)
            lcs = {f"diskmap_{k}": (lambda dm=dm: ltrace.diskmap_lightcurve_dev(d_hits.ptr, d_n.ptr, n, n, M_IMAGES, met, disk, dm, d_tex.ptr, 0.0,
                                                                                dt, args.times, d_lc.ptr)) for k, dm in maps.items()}
            lcs["hotspot"] = lambda: ltrace.hotspot_lightcurve_dev(d_hits.ptr, d_n.ptr, n, n, M_IMAGES, met, disk, spot, 0.0, dt, args.times,
                                                                   d_lc.ptr)
            lc = alternately(lcs, args.reps, args.lc_batch)
            for v in lc.values():
                v["ms_per_time"] = round(v["ms"] / args.times, 5)
            row["lightcurve"] = lc
        res["results"][f"S{S}"] = row
        print(f"S = {S}:", json.dumps(row), flush=True)
        del rec, d_hits, d_n
    out = args.out or os.path.join(ROOT, "profiles", f"diskmap_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
