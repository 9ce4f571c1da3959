"""Cost of the linear polarization on the frame of DESIGN.md 10b: 4096^2, Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg,
vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray.  Reports, for RK4 float32 and DP45 (exact controller)
float64, the HIP-event times of the integrate kernel and of the epilogue of the polarized trace (lt_trace_disk_pol)
against the timed trace's (lt_trace_disk_hits), the two run alternately in one session (median of --reps after one
warm-up each); then the time per lt_shade_stokes_dev call and per 256-time lt_hotspot_lightcurve_stokes_dev call on the
float32 trace's records, on device buffers, against lt_shade_hotspot_dev and lt_hotspot_lightcurve_dev.  The kernels'
registers are in profiles/polarization_resources.txt.  No gate.

    python tools/pol_bench.py [--size 4096] [--reps 3] [--out profiles/pol_bench_<build>.json]
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
    ap.add_argument("--reps", type=int, default=3)
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
    field = ltrace.default_bfield(b_r=0.3, b_phi=0.8, b_z=0.5)
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0,
               r_in=ltrace.kerr_isco(1.0, 0.9), r_out=20.0, max_images=3, reps=args.reps, configs={})
    rec = None
    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        calls = dict(timed=lambda: ltrace.trace_disk_hits(cam, met, o, disk, max_images=3, want=("hits", "n_hits")),
                     pol=lambda: ltrace.trace_disk_pol(cam, met, o, disk, field, max_images=3, want=("hits", "n_hits", "pol")))
        ms = {k: dict(integrate_ms=[], epilogue_ms=[]) for k in calls}
        last = {}
        for rep in range(args.reps + 1):      # alternately; the first round warms up
            for name, call in calls.items():
                last[name] = call()
                if rep:
                    for k in ms[name]:
                        ms[name][k].append(last[name]["stats"][k])
        row = {name: {k: round(float(np.median(v)), 4) for k, v in m.items()} for name, m in ms.items()}
        row["timed"]["integrate_range_ms"] = [round(float(min(ms["timed"]["integrate_ms"])), 4), round(float(max(ms["timed"]["integrate_ms"])), 4)]
        row["pol_over_timed"] = round(row["pol"]["integrate_ms"] / row["timed"]["integrate_ms"], 4)
        res["configs"][f"{integ}_f{prec}"] = row
        print(integ, prec, json.dumps(row), flush=True)
        if rec is None:
            rec = last["pol"]
        last.clear()

    def upload(host):
        host = np.ascontiguousarray(host)
        d = hipmini.DeviceArray(host.shape, host.dtype)
        if hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1):
            raise RuntimeError("hipMemcpy to the device failed")
        return d

    d_hits, d_n, d_pol = upload(rec["hits"]), upload(rec["n_hits"]), upload(rec["pol"])
    d_rgb, d_iqu = hipmini.DeviceArray((n, n, 3), np.float32), hipmini.DeviceArray((n, n, 3), np.float32)
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

    pairs = dict(shade_ms=lambda: ltrace.shade_hotspot_dev(d_hits.ptr, d_n.ptr, n, n, 3, met, disk, spot, 40.0, d_rgb=d_rgb.ptr),
                 shade_stokes_ms=lambda: ltrace.shade_stokes_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, n, n, 3, met, disk, spot, field, 40.0, d_iqu.ptr),
                 lightcurve_256_ms=lambda: ltrace.hotspot_lightcurve_dev(d_hits.ptr, d_n.ptr, n, n, 3, met, disk, spot, 0.0, 2.0, 256, d_lc.ptr),
                 lightcurve_stokes_256_ms=lambda: ltrace.hotspot_lightcurve_stokes_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, n, n, 3, met, disk, spot,
                                                                                        field, 0.0, 2.0, 256, d_lc.ptr))
    for name, fn in pairs.items():
        res[name] = timed(fn, args.reps)
    print(json.dumps({k: res[k] for k in pairs}), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"pol_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
