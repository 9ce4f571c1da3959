"""Cost of the accretion disk on the integrate kernel: a 4096^2 frame (Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg,
vfov 40 deg) rendered with the disk (r_out = 20, r_in = ISCO; lt_render_disk), with the optically thin disk keeping
3 images per ray (lt_render_disk_images) and without a disk (lt_render, same camera, every row traced), for RK4
float32 and DP45 (exact controller) float64.  Reports Mrays/s of the frame, the integrate kernel's HIP-event time
(median of --reps after one warm-up), the fraction of pixels on the disk and, for the thin disk, the fraction with a
higher-order image and the hits per ray; no gate.

    python tools/disk_bench.py [--size 4096] [--reps 5] [--out profiles/disk_bench_<build>.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "light-path-tracer_amd")]

import ltrace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    n = args.size
    vfov = np.radians(40.0)
    cam = ltrace.Camera(n, n, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    want = ("status",)
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0,
               r_in=ltrace.kerr_isco(1.0, 0.9), r_out=20.0, reps=args.reps, configs={})
    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        row = {}
        for name, call in (("plain", lambda: ltrace.render(cam, met, o, want=want)),
                           ("disk", lambda: ltrace.render_disk(cam, met, o, disk, want=want)),
                           ("images", lambda: ltrace.render_disk_images(cam, met, o, disk, max_images=3,
                                                                        want=want + ("n_hits",)))):
            call()
            ms, wall, out = [], [], None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                out = call()
                wall.append(time.perf_counter() - t0)
                ms.append(out["stats"]["integrate_ms"])
            k = float(np.median(ms))
            row[name] = dict(integrate_ms=round(k, 4), mrays_s=round(n * n / (k * 1e-3) / 1e6, 1),
                             call_ms=round(1e3 * float(np.median(wall)), 3),
                             steps_per_ray=round(out["stats"]["steps"] / out["stats"]["rays"], 2))
            if name == "disk":
                row["disk_fraction"] = round(float((out["status"] == ltrace.STATUS_DISK).mean()), 4)
            if name == "images":
                row["images"]["epilogue_ms"] = round(float(out["stats"]["epilogue_ms"]), 4)
                row["images"]["hit_fraction"] = round(float((out["n_hits"] > 0).mean()), 4)
                row["images"]["higher_order_fraction"] = round(float((out["n_hits"] > 1).mean()), 4)
                row["images"]["hits_per_ray"] = round(out["stats"]["disk_hits"] / out["stats"]["rays"], 4)
        row["integrate_ratio"] = round(row["disk"]["integrate_ms"] / row["plain"]["integrate_ms"], 4)
        row["images_integrate_ratio"] = round(row["images"]["integrate_ms"] / row["plain"]["integrate_ms"], 4)
        res["configs"][f"{integ}_f{prec}"] = row
        print(integ, prec, json.dumps(row), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"disk_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
