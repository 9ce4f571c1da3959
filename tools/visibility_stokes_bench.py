"""What the polarized visibilities cost, on the frame of tools/visibility_bench.py: 1024^2, Kerr a = 0.9,
r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4 float32, traced with a
vertical field (lt_trace_disk_pol) -- and its S = 4 fine records (4096^2).  24 times over one orbit at r = 8 for the spot
(r 8, phi0 0, sigma 1.5); 64 baselines on a radial cut and 1024 on a grid, one plane and one per image order; device buffers.

The yardstick is lt_hotspot_visibility_dev on the same records: the I-only call, whose numbers the I plane repeats.  It is
measured twice: alternately with the polarized call in this process, and -- so that the comparison is with a library that
has no polarized kernels at all -- by a run of this tool with --unpolarized-only --package <a built package of the commit
before>, whose JSON --yardstick merges.  Both runs belong in one session on one device.

The operation count is 10j's: per kept pixel, owned baseline and batch PHASE_F64 = 28 float64 arithmetic instructions for
the phase plus two multiply-adds per accumulator of the batch.  The I-only call keeps NT = 16 accumulators and needs
ceil(times / (16 // planes)) batches; the polarized call keeps 3 x 5 = 15 and needs ceil(times x planes / 5).  `predicted`
is the quotient of the two counts: what the polarized call would cost if both ran at the same share of the issue peak.
The convention is tools/visibility_bench.py's: a sample is --batch calls back to back behind one untimed call and before one
synchronise; the candidates run alternately, --reps rounds after one warm-up round; reported: the median and the range.
No gate.

    python tools/visibility_stokes_bench.py [--size 1024] [--samples 1,4] [--reps 5] [--times 24] [--batch 3]
                                            [--unpolarized-only] [--package DIR] [--yardstick JSON] [--out JSON]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

M_IMAGES = 3
PHASE_F64 = 28                     # float64 arithmetic instructions of visibility_phase per (kept pixel, baseline): DESIGN.md 10j
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9
BATCH_TERMS, STOKES_PAIRS = 16, 5


def plain_batches(n_times, planes):
    """Accumulators of every batch of lt_hotspot_visibility, as launch_visibility forms them."""
    per = min(n_times, max(1, BATCH_TERMS // planes))
    nt = 1
    while nt < per * planes:
        nt *= 2
    return [nt] * -(-n_times // per)


def stokes_batches(n_times, planes):
    """Accumulators of every batch of lt_hotspot_visibility_stokes, as launch_visibility forms them from pairs."""
    pairs = n_times * planes
    per = min(pairs, STOKES_PAIRS)
    np_ = next(k for k in (1, 2, 3, 5) if k >= per)
    return [3 * np_] * -(-pairs // per)


def count(batches, lit, n_b):
    return sum(lit * n_b * (PHASE_F64 + 2 * nt) for nt in batches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--samples", default="1,4", help="1: the frame's own records; S: the fine records of the S x S supersampled sequence")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--times", type=int, default=24)
    ap.add_argument("--batch", type=int, default=3, help="calls per sample")
    ap.add_argument("--unpolarized-only", action="store_true", help="time lt_hotspot_visibility_dev alone: what a yardstick run does")
    ap.add_argument("--package", default=os.path.join(ROOT, "light-path-tracer_amd"), help="the built package to import ltrace and disk from")
    ap.add_argument("--yardstick", default=None, help="the JSON of an --unpolarized-only run of the same session to compare with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path[:0] = [os.path.abspath(args.package), os.path.join(ROOT, "tests")]
    import disk as diskmod
    import ltrace
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n, T = args.size, args.times
    vfov = np.radians(40.0)
    M, a = 1.0, 0.9
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    disk = ltrace.default_disk(r_out=20.0)
    spot = diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5).to_lt()
    field = diskmod.BField(0.0, 0.0, 1.0, pol_frac=0.7).to_lt()
    baselines = {64: diskmod.Baselines.radial(64, 0.5, 30.0), 1024: diskmod.Baselines.grid(32, 32, 0.5)}
    dt = 2 * np.pi * (8.0 ** 1.5 + 0.9) / T
    res = dict(build=ltrace.build_id(), mode="unpolarized-only" if args.unpolarized_only else "polarized", frame=f"{n}x{n}", a=a, r_obs=50.0,
               theta_obs_deg=80.0, vfov_deg=40.0, r_out=20.0, max_images=M_IMAGES, spot=[8.0, 0.0, 1.5], field=[0.0, 0.0, 1.0, 0.7], n_times=T,
               reps=args.reps, batch=args.batch, phase_f64=PHASE_F64, peak_lane_ops_per_s=PEAK_LANE_OPS, integrator="rk4", precision=32, results={})
    yard = None
    if args.yardstick:
        with open(args.yardstick) as f:
            yard = json.load(f)
        res["yardstick_build"] = yard["build"]
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
    for S in [int(x) for x in args.samples.split(",")]:
        R = n * S
        cam = ltrace.Camera(R, R, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
        rec = ltrace.trace_disk_pol(cam, met, o, disk, field, max_images=M_IMAGES, want=("hits", "n_hits", "pol"))
        d_hits, d_n = upload(rec["hits"]), upload(rec["n_hits"])
        ns = np.minimum(rec["n_hits"], M_IMAGES)
        lit = int(np.count_nonzero(ns))
        row = dict(integrate_ms=rec["stats"]["integrate_ms"], stored_slots=int(ns.sum(dtype=np.int64)), lit_pixels=lit)
        head = (d_hits.ptr, d_n.ptr, R, R, M_IMAGES, met, disk)
        d_v = hipmini.DeviceArray((T, M_IMAGES, 1024, 2), np.float64)
        calls = {}
        if not args.unpolarized_only:
            d_pol = upload(rec["pol"])
            d_vs = hipmini.DeviceArray((T, M_IMAGES, 3, 1024, 2), np.float64)
            shead = (d_hits.ptr, d_n.ptr, d_pol.ptr, R, R, M_IMAGES, met, disk)
        for gname, split in (("whole", False), ("split", True)):
            for n_b, bl in baselines.items():
                uv = bl.fine(S)
                calls[f"visibility_{gname}_{n_b}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_dev(*head, spot, uv, split, 0.0, dt, T, d_v.ptr)
                if not args.unpolarized_only:
                    calls[f"stokes_{gname}_{n_b}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_stokes_dev(*shead, spot, field, uv, split, 0.0, dt,
                                                                                                                    T, d_vs.ptr)
        if not args.unpolarized_only:
            dark = diskmod.HotSpot(r_spot=8.0, phi0=0.0, sigma=1.5, exposure=0.0).to_lt()      # every weight exactly 0: phase one alone
            for gname, split in (("whole", False), ("split", True)):
                uv = baselines[64].fine(S)
                calls[f"phase_one_visibility_{gname}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_dev(*head, dark, uv, split, 0.0, dt, T, d_v.ptr)
                calls[f"phase_one_stokes_{gname}"] = lambda uv=uv, split=split: ltrace.hotspot_visibility_stokes_dev(*shead, dark, field, uv, split, 0.0,
                                                                                                                    dt, T, d_vs.ptr)
            calls["stokes_disk_whole_64"] = lambda: ltrace.disk_visibility_stokes_dev(*shead, field, baselines[64].fine(S), False, d_vs.ptr)
        gpu = alternately(calls, args.reps, args.batch)
        row["gpu"] = gpu
        if not args.unpolarized_only:
            ratios = {}
            for gname, planes in (("whole", 1), ("split", M_IMAGES)):
                pb, sb = plain_batches(T, planes), stokes_batches(T, planes)
                for n_b in baselines:
                    key = f"{gname}_{n_b}"
                    s_ms, v = gpu[f"stokes_{key}"]["ms"], gpu[f"visibility_{key}"]
                    ops = count(sb, lit, n_b)
                    r = dict(batches=len(sb), nt=sb[0], unpolarized_batches=len(pb), unpolarized_nt=pb[0], f64_valu_ops=ops,
                             predicted=round(ops / count(pb, lit, n_b), 3), stokes_over_visibility=round(s_ms / v["ms"], 3),
                             visibility_range_relative=round((v["range_ms"][1] - v["range_ms"][0]) / v["ms"], 4),
                             phase_one_share=round(gpu[f"phase_one_stokes_{gname}"]["ms"] / s_ms * -(-n_b // 256), 3),
                             unpolarized_phase_one_share=round(gpu[f"phase_one_visibility_{gname}"]["ms"] / v["ms"] * -(-n_b // 256), 3),
                             share_of_f64_valu_peak=round(ops / (s_ms * 1e-3) / PEAK_LANE_OPS, 4))
                    if yard is not None:
                        y = yard["results"][f"S{S}"]["gpu"][f"visibility_{key}"]
                        r.update(yardstick_ms=y["ms"], yardstick_range_ms=y["range_ms"], stokes_over_yardstick=round(s_ms / y["ms"], 3),
                                 visibility_over_yardstick=round(v["ms"] / y["ms"], 3))
                    ratios[key] = r
            row["ratios"] = ratios
        res["results"][f"S{S}"] = row
        print(f"S = {S}:", json.dumps(row), flush=True)
        del rec, d_hits, d_n
    name = "visibility_yardstick" if args.unpolarized_only else "visibility_stokes_bench"
    out = args.out or os.path.join(ROOT, "profiles", f"{name}_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
