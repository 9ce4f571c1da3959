"""Cost of the hit times and the hot spot on the frame of DESIGN.md 10b: 4096^2, Kerr a = 0.9, r_obs = 50, theta_obs =
80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray.  Reports, for RK4 float32 and DP45 (exact
controller) float64, the integrate kernel's HIP-event time of the timed trace (lt_trace_disk_hits) against the thin
disk's (lt_render_disk_images), the two run alternately in one session (median of --reps after one warm-up each); the
wave iterations of both (the timed trace has no far-field streak); then the time per lt_shade_hotspot_dev call and per
256-time lt_hotspot_lightcurve_dev call on the float32 trace's hits, on device buffers.  The timed kernel's registers
are in profiles/hit_time_resources.txt.  No gate.

    python tools/hotspot_bench.py [--size 4096] [--reps 5] [--out profiles/hotspot_bench_<build>.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "light-path-tracer_amd"), os.path.join(ROOT, "tests")]

import ltrace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import ctypes as C
    import hipmini   # raw device buffers on the library's own HIP runtime
    n = args.size
    vfov = np.radians(40.0)
    cam = ltrace.Camera(n, n, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    spot = ltrace.default_hotspot(r_spot=8.0, sigma=1.5)
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0,
               r_in=ltrace.kerr_isco(1.0, 0.9), r_out=20.0, max_images=3, reps=args.reps, configs={})
    hits = None
    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        calls = dict(images=lambda: ltrace.render_disk_images(cam, met, o, disk, max_images=3, want=("n_hits",)),
                     timed=lambda: ltrace.trace_disk_hits(cam, met, o, disk, max_images=3, want=("hits", "n_hits")))
        ms = dict(images=[], timed=[])
        last = {}
        for rep in range(args.reps + 1):      # alternately; the first round warms up
            for name, call in calls.items():
                last[name] = call()
                if rep:
                    ms[name].append(last[name]["stats"]["integrate_ms"])
        row = {k: dict(integrate_ms=round(float(np.median(v)), 4), wave_iters=last[k]["stats"]["wave_iters"],
                       epilogue_ms=round(float(last[k]["stats"]["epilogue_ms"]), 4)) for k, v in ms.items()}
        row["timed_over_images"] = round(row["timed"]["integrate_ms"] / row["images"]["integrate_ms"], 4)
        res["configs"][f"{integ}_f{prec}"] = row
        print(integ, prec, json.dumps(row), flush=True)
        if hits is None:
            hits = last["timed"]
    def upload(host):
        host = np.ascontiguousarray(host)
        d = hipmini.DeviceArray(host.shape, host.dtype)
        if hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1):
            raise RuntimeError("hipMemcpy to the device failed")
        return d

    d_hits, d_n = upload(hits["hits"]), upload(hits["n_hits"])
    d_rgb, d_rgba = hipmini.DeviceArray((n, n, 3), np.float32), hipmini.DeviceArray((n, n, 4), np.uint8)
    d_lc = hipmini.DeviceArray((256, 3), np.float64)
    sync = lambda: hipmini.hip().hipStreamSynchronize(None)

    def timed(fn, reps):
        fn()
        sync()
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            sync()
            t.append(1e3 * (time.perf_counter() - t0))
        return round(float(np.median(t)), 4)

    res["shade_ms"] = timed(lambda: ltrace.shade_hotspot_dev(d_hits.ptr, d_n.ptr, n, n, 3, met, disk, spot, 40.0, d_rgb=d_rgb.ptr,
                                                           d_rgba=d_rgba.ptr), args.reps)
    res["lightcurve_256_ms"] = timed(lambda: ltrace.hotspot_lightcurve_dev(d_hits.ptr, d_n.ptr, n, n, 3, met, disk, spot, 0.0, 2.0, 256,
                                                                          d_lc.ptr), args.reps)
    print(json.dumps({k: res[k] for k in ("shade_ms", "lightcurve_256_ms")}), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"hotspot_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
