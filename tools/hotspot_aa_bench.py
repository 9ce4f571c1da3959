"""What aliasing costs a hot spot's light curve, and what the fused re-shade + resolve costs, on the README's sequence
frame: 1024^2, Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray,
spot (r 8, phi0 0, sigma 1.5), field (0, 0, 1); RK4 float32 and DP45 (exact controller) float64.

1. Aliasing.  The fine camera (1024 S)^2 is traced at S = 1, 2, 4 and the spot's light curve taken over one orbital period
   at 256 times, total and per image order (order j: lt_hotspot_lightcurve on hits[:, :, j:j+1, :] with n_hits NULL), in
   output-pixel units (column 0 / S^2).  Reported: the largest and the RMS difference of S = 1 and S = 2 from S = 4,
   relative to the S = 4 curve's peak.
2. Fusion.  On the S = 2 and S = 4 records on the device, run alternately in one session, median of --reps with the range
   (a device-only sample is --batch launches back to back, the time per launch):
   (a) lt_shade_hotspot_aa_dev;  (b) lt_shade_hotspot_dev on the same fine records, the fine frame left on the device;
   (c) (b), the device-to-host copy of the fine rgb into pinned memory, aa.resolve on the host;  the same three for Stokes.
No gate.

    python tools/hotspot_aa_bench.py [--size 1024] [--reps 3] [--times 256] [--batch 50] [--out profiles/hotspot_aa_bench_<build>.json]
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

import aa  # noqa: E402
import ltrace  # noqa: E402

SAMPLES = (1, 2, 4)
M_IMAGES = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--times", type=int, default=256)
    ap.add_argument("--batch", type=int, default=50, help="launches per sample of a device-only call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n = args.size
    vfov = np.radians(40.0)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    spot = ltrace.default_hotspot(r_spot=8.0, phi0=0.0, sigma=1.5)
    field = ltrace.default_bfield(b_r=0.0, b_phi=0.0, b_z=1.0)
    period = 2 * np.pi * (8.0 ** 1.5 + 0.9)
    dt = period / args.times
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0,
               r_in=ltrace.kerr_isco(1.0, 0.9), r_out=20.0, max_images=M_IMAGES, spot=[8.0, 0.0, 1.5], period=period,
               n_times=args.times, reps=args.reps, batch=args.batch, configs={})
    sync = lambda: hipmini.hip().hipStreamSynchronize(None)

    def upload(host):
        host = np.ascontiguousarray(host)
        d = hipmini.DeviceArray(host.shape, host.dtype)
        if hipmini.hip().hipMemcpy(C.c_void_p(d.ptr), C.c_void_p(host.ctypes.data), host.nbytes, 1):
            raise RuntimeError("hipMemcpy to the device failed")
        return d

    def fetch(d, host):
        if hipmini.hip().hipMemcpy(C.c_void_p(host.ctypes.data), C.c_void_p(d.ptr), host.nbytes, 2):
            raise RuntimeError("hipMemcpy to the host failed")

    def alternately(calls, reps, batch):
        """{name: median ms per call and [min, max]}: the calls one after the other, `reps` rounds after one warm-up round.
        A device-only call (name without "host") is a fraction of a millisecond, so a sample is `batch` launches back to back
        behind one untimed launch and before one synchronise: a single launch after the host's resolve times the
        chip's wake-up as well (measured: 0.046 ms on every call that followed host work, whatever the kernel)."""
        ms = {k: [] for k in calls}
        for rep in range(reps + 1):
            for name, fn in calls.items():
                n = 1 if "host" in name else batch
                fn()
                sync()
                t0 = time.perf_counter()
                for _ in range(n):
                    fn()
                sync()
                if rep:
                    ms[name].append(1e3 * (time.perf_counter() - t0) / n)
        return {k: dict(ms=round(float(np.median(v)), 4), range_ms=[round(min(v), 4), round(max(v), 4)]) for k, v in ms.items()}

    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        row = dict(curves={}, aliasing={}, fusion={})
        curves = {}
        for S in SAMPLES:
            cam = ltrace.Camera(n * S, n * S, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
            rec = ltrace.trace_disk_pol(cam, met, o, disk, field, max_images=M_IMAGES, want=("hits", "n_hits", "pol"))
            hits, n_hits, pol = rec["hits"], rec["n_hits"], rec["pol"]
            # ---- 1. the light curves, output-pixel units
            lc = {"total": ltrace.hotspot_lightcurve(hits, n_hits, met, disk, spot, 0.0, dt, args.times)[:, 0] / (S * S)}
            for j in range(M_IMAGES):
                lc[f"order{j}"] = ltrace.hotspot_lightcurve(np.ascontiguousarray(hits[:, :, j:j + 1, :]), None, met, disk, spot, 0.0, dt,
                                                            args.times)[:, 0] / (S * S)
            curves[S] = lc
            row["curves"][f"S{S}"] = {k: dict(peak=float(v.max()), mean=float(v.mean())) for k, v in lc.items()}
            print(integ, prec, f"S = {S}: integrate {rec['stats']['integrate_ms']:.2f} ms, peaks",
                  {k: f"{v.max():.4g}" for k, v in lc.items()}, flush=True)
            # ---- 2. the fused kernels against the one-sample kernels on the same fine records
            if S > 1:
                R = n * S
                d_hits, d_n, d_pol = upload(hits), upload(n_hits), upload(pol)
                d_fine, d_fine8 = hipmini.DeviceArray((R, R, 3), np.float32), hipmini.DeviceArray((R, R, 4), np.uint8)
                d_out, d_out8 = hipmini.DeviceArray((n, n, 3), np.float32), hipmini.DeviceArray((n, n, 4), np.uint8)
                h_fine = ltrace.pinned_empty((R, R, 3), np.float32)
                shade = lambda: ltrace.shade_hotspot_dev(d_hits.ptr, d_n.ptr, R, R, M_IMAGES, met, disk, spot, 40.0, d_rgb=d_fine.ptr,
                                                         d_rgba=d_fine8.ptr)
                stokes = lambda: ltrace.shade_stokes_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, R, R, M_IMAGES, met, disk, spot, field, 40.0,
                                                         d_fine.ptr)
                kept = {}

                def today(fn, key):
                    fn()
                    fetch(d_fine, h_fine)
                    kept[key] = aa.resolve(h_fine, S)

                calls = dict(
                    hotspot_aa=lambda: ltrace.shade_hotspot_aa_dev(d_hits.ptr, d_n.ptr, n, n, S, M_IMAGES, met, disk, spot, 40.0,
                                                                   d_rgb=d_out.ptr, d_rgba=d_out8.ptr),
                    hotspot_fine=shade, hotspot_fine_copy_host_resolve=lambda: today(shade, "rgb"),
                    stokes_aa=lambda: ltrace.shade_stokes_aa_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, n, n, S, M_IMAGES, met, disk, spot, field,
                                                                 40.0, d_out.ptr),
                    stokes_fine=stokes, stokes_fine_copy_host_resolve=lambda: today(stokes, "iqu"))
                fus = alternately(calls, args.reps, args.batch)
                # the fused outputs are the host resolve's, bit for bit (the tests' assertion, here at full size)
                ltrace.shade_stokes_aa_dev(d_hits.ptr, d_n.ptr, d_pol.ptr, n, n, S, M_IMAGES, met, disk, spot, field, 40.0, d_out.ptr)
                same_iqu = bool(np.array_equal(d_out.get(), kept["iqu"]))
                calls["hotspot_aa"]()
                fus["equal_host_resolve"] = dict(rgb=bool(np.array_equal(d_out.get(), kept["rgb"])), iqu=same_iqu)
                fus["fine_record_bytes"] = int(hits.nbytes + pol.nbytes + n_hits.nbytes)
                row["fusion"][f"S{S}"] = fus
                print(integ, prec, f"S = {S}:", json.dumps(fus), flush=True)
                del d_hits, d_n, d_pol, d_fine, d_fine8, h_fine
            del rec, hits, n_hits, pol
        ref = curves[SAMPLES[-1]]
        for S in SAMPLES[:-1]:
            row["aliasing"][f"S{S}_vs_S{SAMPLES[-1]}"] = {
                k: dict(max_rel_peak=float(np.max(np.abs(curves[S][k] - ref[k])) / ref[k].max()),
                        rms_rel_peak=float(np.sqrt(np.mean((curves[S][k] - ref[k]) ** 2)) / ref[k].max())) for k in ref}
        print(integ, prec, "aliasing:", json.dumps(row["aliasing"]), flush=True)
        res["configs"][f"{integ}_f{prec}"] = row
    out = args.out or os.path.join(ROOT, "profiles", f"hotspot_aa_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
