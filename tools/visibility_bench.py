"""What the visibilities cost, on the spectrum bench's records (tools/spectrum_bench.py): the README's sequence frame --
1024^2, Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4
float32 -- and its S = 4 fine records (4096^2).  24 times over one orbit at r = 8, for the spot (r 8, phi0 0, sigma 1.5)
and for a 256 x 1024 Keplerian table (disk.spiral_map); 64 and 1024 baselines on a radial cut and a grid, one plane and one
per image order; device buffers.  Phase one alone is what a DARK emitter costs (exposure 0: every weight is exactly 0,
every pixel is left out, phase two walks empty lists); one baseline costs phase one plus one wavefront's walk of the
kept pixels, which is what up to 64 baselines cost as well.

Yardsticks, all of which exist without the visibility kernels:
  (a) the emitter's own light curve and dynamic spectrum on the same records and times: the same evaluation of the
      weights with a three-number and a 98-number reduction;
  (b) what a user had to do before: copy the records to the host once (timed) and run the numpy statement
      (disk.hotspot_visibility / disk.diskmap_visibility) -- timed on --numpy-times times with 64 baselines on the frame's own
      records and scaled to the 24 times, because it is a per-time loop (the fine records only with --numpy-fine).
The share of the float64 VALU issue peak uses the operation count of DESIGN.md 10j, read off the kernel's listing: per kept
pixel, owned baseline and batch PHASE_F64 = 28 float64 arithmetic instructions for x, f and sincospi plus two multiply-adds
per accumulator of the batch (NT, the power of two from times x planes up), against 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
(a float64 instruction issues at the full rate); with the 40 selects, moves, compares and integer instructions sincospi
needs as well (PHASE_VALU = 68) the same quotient is the share of all VALU issue slots.  Kept pixels are counted as the
pixels with a stored hit (the spot's Gaussian and the spiral never vanish exactly).
The convention is tools/spectrum_bench.py's: a sample is --batch calls back to back behind one untimed call and before one
synchronise, the time per call; the candidates run alternately, --reps rounds after one warm-up round; reported: the median
and the range.  No gate.

    python tools/visibility_bench.py [--size 1024] [--samples 1,4] [--reps 5] [--times 24] [--batch 3] [--numpy-times 1]
                                     [--no-numpy] [--numpy-fine] [--out profiles/visibility_bench_<build>.json]
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
PHASE_F64, PHASE_VALU = 28, 68     # float64 arithmetic / all VALU instructions of visibility_phase per (kept pixel, baseline): DESIGN.md 10j
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9


def batch_plan(n_times, planes):
    """[(times, NT)] of a call's batches, as launch_visibility forms them."""
    per = min(n_times, max(1, ltrace.VISIBILITY_BATCH_TERMS // planes))
    nt = 1
    while nt < per * planes:
        nt *= 2
    return [(min(per, n_times - first), nt) for first in range(0, n_times, per)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", default="1,4", help="1: the frame's own records; S: the fine records of the S x S supersampled sequence")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--times", type=int, default=24)
    ap.add_argument("--batch", type=int, default=3, help="calls per sample")
    ap.add_argument("--numpy-times", type=int, default=1, help="times the numpy statement is run on")
    ap.add_argument("--no-numpy", action="store_true", help="skip yardstick (b): for comparing builds of the kernels")
    ap.add_argument("--numpy-fine", action="store_true", help="yardstick (b) on the fine records as well (minutes and gigabytes)")
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
    baselines = {1: diskmod.Baselines([(0.05, 0.02)]), 64: diskmod.Baselines.radial(64, 0.5, 30.0), 1024: diskmod.Baselines.grid(32, 32, 0.5)}
    dt = 2 * np.pi * (8.0 ** 1.5 + 0.9) / T
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=a, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=r_in, r_out=20.0,
               max_images=M_IMAGES, table=list(TABLE), spot=[8.0, 0.0, 1.5], n_times=T, reps=args.reps, batch=args.batch,
               visibility_blocks=ltrace.VISIBILITY_BLOCKS, batch_terms=ltrace.VISIBILITY_BATCH_TERMS, phase_f64=PHASE_F64, phase_valu=PHASE_VALU,
               peak_lane_ops_per_s=PEAK_LANE_OPS, integrator="rk4", precision=32, results={})
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
        ns = np.minimum(rec["n_hits"], M_IMAGES)
        stored, lit = int(ns.sum(dtype=np.int64)), int(np.count_nonzero(ns))
        row = dict(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes), stored_slots=stored,
                   lit_pixels=lit)
        d_lc = hipmini.DeviceArray((T, 3), np.float64)
        d_sp = hipmini.DeviceArray((T, M_IMAGES, 98), np.float64)
        d_v = hipmini.DeviceArray((T, M_IMAGES, 1024, 2), np.float64)
        head = (d_hits.ptr, d_n.ptr, R, R, M_IMAGES, met, disk)
        calls = {"lightcurve_spot": lambda: ltrace.hotspot_lightcurve_dev(*head, spot, 0.0, dt, T, d_lc.ptr),
                 "lightcurve_map": lambda: ltrace.diskmap_lightcurve_dev(*head, dmap, d_tex.ptr, 0.0, dt, T, d_lc.ptr)}
        for gname, split in (("whole", False), ("split", True)):
            sp = diskmod.Spectrum(split_orders=split).to_lt()
            calls[f"spectrum_spot_{gname}"] = lambda sp=sp: ltrace.hotspot_spectrum_dev(*head, spot, sp, 0.0, dt, T, d_sp.ptr)
            calls[f"spectrum_map_{gname}"] = lambda sp=sp: ltrace.diskmap_spectrum_dev(*head, dmap, d_tex.ptr, sp, 0.0, dt, T, d_sp.ptr)
            for n_b, bl in baselines.items():
                uv = bl.fine(S)
                calls[f"visibility_spot_{gname}_{n_b}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_dev(*head, spot, uv, split, 0.0, dt, T, d_v.ptr)
                calls[f"visibility_map_{gname}_{n_b}"] = lambda uv=uv, split=split: ltrace.diskmap_visibility_dev(*head, dmap, d_tex.ptr, uv, split, 0.0, dt, T,
                                                                                                               d_v.ptr)
        dark_spot, dark_map = diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5, exposure=0.0).to_lt(), ltrace.default_diskmap()
        for name in ("r_min", "r_max", "n_r", "n_phi", "rotation", "omega_p", "with_disk"):
            setattr(dark_map, name, getattr(dmap, name))
        dark_map.exposure = 0.0
        for gname, split in (("whole", False), ("split", True)):
            uv = baselines[64].fine(S)
            calls[f"phase_one_spot_{gname}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_dev(*head, dark_spot, uv, split, 0.0, dt, T, d_v.ptr)
            calls[f"phase_one_map_{gname}"] = lambda uv=uv, split=split: ltrace.diskmap_visibility_dev(*head, dark_map, d_tex.ptr, uv, split, 0.0, dt, T,
                                                                                                     d_v.ptr)
        calls["visibility_disk_whole_64"] = lambda: ltrace.disk_visibility_dev(*head, baselines[64].fine(S), False, d_v.ptr)
        gpu = alternately(calls, args.reps, args.batch)
        row["gpu"] = gpu
        copy_ms, numpy_ms = None, {}
        if not args.no_numpy and (S == 1 or args.numpy_fine):
            # (b): the records to the host once, then the numpy statement on 64 baselines
            host_hits, host_n = np.empty_like(rec["hits"]), np.empty_like(rec["n_hits"])
            sync()
            t0 = time.perf_counter()
            for host, dev in ((host_hits, d_hits), (host_n, d_n)):
                if hipmini.hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(dev.ptr), host.nbytes, 2):
                    raise RuntimeError("hipMemcpy to the host failed")
            copy_ms = 1e3 * (time.perf_counter() - t0)
            k = max(1, min(args.numpy_times, T))
            times = dt * np.arange(k)
            uv = baselines[64].fine(S)
            for name, fn in (("spot", lambda: diskmod.hotspot_visibility(M, a, host_hits, host_n, spot_py, uv, False, times)),
                             ("map", lambda: diskmod.diskmap_visibility(M, a, host_hits, host_n, dmap_py, uv, False, times))):
                t0 = time.perf_counter()
                got = fn()
                numpy_ms[name] = 1e3 * (time.perf_counter() - t0) / k
                if name == "spot" and S == 1:     # the statement timed is the one the kernel restates
                    same = ltrace.hotspot_visibility(host_hits, host_n, met, disk, spot, uv, False, 0.0, dt, k)
                    row["numpy_agrees"] = bool(np.all(np.abs(got - same) <= 1e-9 * np.abs(same[..., :1])))
            row["numpy"] = dict(copy_ms=round(copy_ms, 2), times_run=k, n_baselines=64, ms_per_time=dict((kk, round(v, 2)) for kk, v in numpy_ms.items()),
                                ms_scaled_to_n_times=dict((kk, round(copy_ms + v * T, 1)) for kk, v in numpy_ms.items()))
        ratios = {}
        for em in ("spot", "map"):
            for gname, planes in (("whole", 1), ("split", M_IMAGES)):
                plan = batch_plan(T, planes)
                for n_b in baselines:
                    v_ms = gpu[f"visibility_{em}_{gname}_{n_b}"]["ms"]
                    ops = sum(lit * n_b * (PHASE_F64 + 2 * nt) for _, nt in plan)
                    valu = sum(lit * n_b * (PHASE_VALU + 2 * nt) for _, nt in plan)
                    r = dict(batches=len(plan), nt=plan[0][1], visibility_over_lightcurve=round(v_ms / gpu[f"lightcurve_{em}"]["ms"], 3),
                             visibility_over_spectrum=round(v_ms / gpu[f"spectrum_{em}_{gname}"]["ms"], 3),
                             phase_one_share=round(gpu[f"phase_one_{em}_{gname}"]["ms"] / v_ms * -(-n_b // 256), 3), f64_valu_ops=ops,
                             share_of_f64_valu_peak=round(ops / (v_ms * 1e-3) / PEAK_LANE_OPS, 4),
                             share_of_valu_issue=round(valu / (v_ms * 1e-3) / PEAK_LANE_OPS, 4))
                    if numpy_ms and n_b == 64 and gname == "whole":
                        r["numpy_over_visibility"] = round((copy_ms + numpy_ms[em] * T) / v_ms, 1)
                    ratios[f"{em}_{gname}_{n_b}"] = r
        row["ratios"] = ratios
        res["results"][f"S{S}"] = row
        print(f"S = {S}:", json.dumps(row), flush=True)
        del rec, d_hits, d_n
    out = args.out or os.path.join(ROOT, "profiles", f"visibility_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
