"""What a disk movie's five products cost beside the rotating map's, on the README's sequence frame: 1024^2, Kerr a = 0.9,
r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4 float32, and its S = 4
fine records; movies of 1, 8 and 64 frames of 256 x 1024 texels (1, 8 and 64 MB: inside one XCD's 4 MiB L2, beyond it,
and in the Infinity Cache), Keplerian rotation, device buffers throughout.  Every movie's clock is set from the records'
own delays so that the emission times of the call span the whole movie: frame 0 at the 0.5th percentile of the emission
times, the last frame at the 99.5th (one frame: held).  The few rays that circle the hole many times arrive thousands of M
late; they see a held end frame.

The yardstick of every product is the map's matching entry point -- lt_shade_diskmap_dev, lt_shade_diskmap_aa_dev (S = 4),
lt_diskmap_lightcurve_dev, lt_diskmap_spectrum_dev (96 bins), lt_diskmap_visibility_dev (64 baselines), 24 times -- on the
same records with one 256 x 1024 table in the same session, never the new kernels themselves.  --yardstick-lib PATH takes
the map's entry points from another build of the library (the parent commit's, where this build changed the map's
kernels' code objects); without it they are this build's.  By the code a slot's
gathers go from 4 to 8 and the rest is unchanged, so a ratio between 1 and 2 is expected for the frames, nearer 1 for the
spectrum and the visibilities, whose fixed-order reductions dominate.  The convention is tools/diskmap_bench.py's: a sample
is --batch calls back to back behind one untimed call and before one synchronise, the time per call; the candidates run
alternately, --reps rounds after one warm-up round; reported: the median and the range, and per movie the ratio of the
medians to the map's.  The map's own range is the yardstick's run-to-run spread.  No gate.

    python tools/diskmovie_bench.py [--size 1024] [--frames 1,8,64] [--reps 5] [--times 24] [--batch 50] [--seq-batch 5]
                                    [--yardstick-lib PATH] [--out profiles/diskmovie_bench_<build>.json]
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
T_OBS, DT_OBS = 400.0, 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--frames", default="1,8,64", help="the movies' n_frames")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--times", type=int, default=24)
    ap.add_argument("--batch", type=int, default=50, help="calls per sample of a frame call")
    ap.add_argument("--seq-batch", type=int, default=5, help="calls per sample of a light curve, a spectrum or a visibility")
    ap.add_argument("--yardstick-lib", default=None, help="a libltrace_hip.so whose lt_*diskmap*_dev are the yardstick (default: this build's)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n = args.size
    vfov = np.radians(40.0)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    r_in = ltrace.kerr_isco(1.0, 0.9)
    table = diskmod.spiral_map(*TABLE, r_min=r_in, r_max=20.0)
    dmap = diskmod.DiskMap(table, r_min=r_in, r_max=20.0, rotation="kepler").to_lt()
    n_frames = [int(x) for x in args.frames.split(",")]
    rng = np.random.default_rng(1)
    # every frame its own table: the spiral times a smooth random brightening, so that no two frames share a cache line
    tables = {f: (table[None] * rng.uniform(0.5, 1.5, (f, 1, 1))).astype(np.float32) for f in n_frames}
    ylib = ltrace.load()
    if args.yardstick_lib:
        ylib = C.CDLL(args.yardstick_lib)
        for name in ("lt_shade_diskmap_dev", "lt_shade_diskmap_aa_dev", "lt_diskmap_lightcurve_dev", "lt_diskmap_spectrum_dev",
                     "lt_diskmap_visibility_dev"):
            getattr(ylib, name).restype, getattr(ylib, name).argtypes = ltrace.SIGNATURES[name]
        ylib.lt_build_id.restype = C.c_char_p
    spec = ltrace.default_spectrum(g_min=0.0625, g_max=1.5625, n_bins=96)
    uv = np.ascontiguousarray(diskmod.Baselines.radial(64, 0.25, 30.0).uv)
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=r_in, r_out=20.0,
               max_images=M_IMAGES, table=list(TABLE), n_frames=n_frames, movie_bytes={str(f): int(tables[f].nbytes) for f in n_frames},
               rotation="kepler", boundary="hold", n_times=args.times, n_bins=96, n_baselines=64, reps=args.reps, batch=args.batch,
               seq_batch=args.seq_batch, integrator="rk4", precision=32,
               yardstick="the map's entry point, same session, from " + (f"the library of build {ylib.lt_build_id().decode()}" if args.yardstick_lib
                                                                        else "this build"),
               results={})
    sync = lambda: hipmini.hip().hipStreamSynchronize(None)
    ref = lambda x: C.byref(x)

    def ok(rc):
        if rc:
            raise RuntimeError(f"the yardstick's call failed ({rc})")

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
        out = {k: dict(ms=round(float(np.median(v)), 4), range_ms=[round(min(v), 4), round(max(v), 4)]) for k, v in ms.items()}
        for k, v in out.items():
            v["ratio_to_map"] = round(v["ms"] / out["map"]["ms"], 3)
        out["map"]["range_rel"] = round((out["map"]["range_ms"][1] - out["map"]["range_ms"][0]) / out["map"]["ms"], 3)
        return out

    def clock(f, t_lo, t_hi):
        """The lt_diskmovie of f frames whose epochs span the emission times t_lo ... t_hi."""
        return ltrace.default_diskmovie(t0=float(t_lo), dt_frame=float((t_hi - t_lo) / max(f - 1, 1)), n_frames=f, boundary="hold")

    o = ltrace.default_opts(integrator="rk4", precision=32, tb_symmetry=0)
    d_map = upload(table)
    d_tex = {f: upload(tables[f]) for f in n_frames}
    t_last = T_OBS + DT_OBS * (args.times - 1)
    for S in (1, 4):
        R = n * S
        cam = ltrace.Camera(R, R, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
        rec = ltrace.trace_disk_hits(cam, met, o, disk, max_images=M_IMAGES, want=("hits", "n_hits"))
        stored = np.arange(M_IMAGES) < np.minimum(rec["n_hits"], M_IMAGES)[..., None]
        delays = rec["hits"][..., 3][stored]
        d_lo, d_hi = (float(x) for x in np.percentile(delays, [0.5, 99.5]))
        d_hits, d_n = upload(rec["hits"]), upload(rec["n_hits"])
        d_out, d_out8 = hipmini.DeviceArray((n, n, 3), np.float32), hipmini.DeviceArray((n, n, 4), np.uint8)
        row = dict(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes), delays=[float(delays.min()), float(delays.max())],
                   delays_spanned=[d_lo, d_hi])
        head = (d_hits.ptr, d_n.ptr, n, n)
        emitter = (ref(met), ref(disk), ref(dmap), d_map.ptr)                      # the map's arguments as the C entry points take them
        one = {f: clock(f, T_OBS - d_hi, T_OBS - d_lo) for f in n_frames}         # one observer time
        seq = {f: clock(f, T_OBS - d_hi, t_last - d_lo) for f in n_frames}        # the sequence's times
        if S == 1:
            calls = {"map": lambda: ok(ylib.lt_shade_diskmap_dev(*head, M_IMAGES, *emitter, T_OBS, None, 3, d_out.ptr, d_out8.ptr))}
            for f in n_frames:
                calls[f"movie_{f}"] = lambda f=f: ltrace.shade_diskmovie_dev(*head, M_IMAGES, met, disk, dmap, one[f], d_tex[f].ptr, T_OBS,
                                                                             d_rgb=d_out.ptr, d_rgba=d_out8.ptr)
            row["frame"] = alternately(calls, args.reps, args.batch)
            times = (T_OBS, DT_OBS, args.times)
            d_lc = hipmini.DeviceArray((args.times, 3), np.float64)
            calls = {"map": lambda: ok(ylib.lt_diskmap_lightcurve_dev(*head, M_IMAGES, *emitter, *times, d_lc.ptr))}
            for f in n_frames:
                calls[f"movie_{f}"] = lambda f=f: ltrace.diskmovie_lightcurve_dev(*head, M_IMAGES, met, disk, dmap, seq[f], d_tex[f].ptr, *times,
                                                                                  d_lc.ptr)
            row["lightcurve"] = alternately(calls, args.reps, args.seq_batch)
            d_sp = hipmini.DeviceArray((args.times, 1, 98), np.float64)
            calls = {"map": lambda: ok(ylib.lt_diskmap_spectrum_dev(*head, M_IMAGES, *emitter, ref(spec), *times, d_sp.ptr))}
            for f in n_frames:
                calls[f"movie_{f}"] = lambda f=f: ltrace.diskmovie_spectrum_dev(*head, M_IMAGES, met, disk, dmap, seq[f], d_tex[f].ptr, spec, *times,
                                                                                d_sp.ptr)
            row["spectrum"] = alternately(calls, args.reps, args.seq_batch)
            d_vis = hipmini.DeviceArray((args.times, 1, 64, 2), np.float64)
            calls = {"map": lambda: ok(ylib.lt_diskmap_visibility_dev(*head, M_IMAGES, *emitter, uv.ctypes.data, 64, 0, *times, d_vis.ptr))}
            for f in n_frames:
                calls[f"movie_{f}"] = lambda f=f: ltrace.diskmovie_visibility_dev(*head, M_IMAGES, met, disk, dmap, seq[f], d_tex[f].ptr, uv, False,
                                                                                  *times, d_vis.ptr)
            row["visibility"] = alternately(calls, args.reps, args.seq_batch)
        else:
            calls = {"map": lambda: ok(ylib.lt_shade_diskmap_aa_dev(*head, S, M_IMAGES, *emitter, T_OBS, None, 3, d_out.ptr, d_out8.ptr))}
            for f in n_frames:
                calls[f"movie_{f}"] = lambda f=f: ltrace.shade_diskmovie_aa_dev(*head, S, M_IMAGES, met, disk, dmap, one[f], d_tex[f].ptr, T_OBS,
                                                                                d_rgb=d_out.ptr, d_rgba=d_out8.ptr)
            row["frame_aa"] = alternately(calls, args.reps, max(args.batch // 2, 1))
        res["results"][f"S{S}"] = row
        print(f"S = {S}:", json.dumps(row), flush=True)
        del rec, d_hits, d_n
    out = args.out or os.path.join(ROOT, "profiles", f"diskmovie_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
