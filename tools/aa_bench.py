"""Cost of a supersampled frame (lt_render_aa) against the only way to get one without it: the existing entry point on the
fine frame, the S^2 times larger copy, and a box filter on the host (aa.resolve).

The demo view (Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20) at --size^2 output pixels,
S = 2 and 4, plain and optically thin disk (3 images per ray), RK4 float32 and DP45 (exact controller) float64, no
background.  For every configuration, alternating after one warm-up of each:
  A  the mode's own call on the fine frame, rgb into pinned memory, then aa.resolve;
  B  lt_render_aa, automatic band (one band at these sizes), rgb into pinned memory;
  C  lt_render_aa in bands of --band-rows output rows.
Reports the medians of the prologue / integrate / epilogue HIP-event sums and of the wall time of the call (A: with and
without the host resolve), and the ray-record bytes of a band (lt_aa_band_bytes); no gate.

    python tools/aa_bench.py [--size 1024] [--reps 5] [--band-rows 256] [--out profiles/aa_bench_<build>.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "light-path-tracer_amd")]

import aa  # noqa: E402
import ltrace  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band-rows", type=int, default=256)
    ap.add_argument("--samples", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    n = args.size
    vfov = np.radians(40.0)
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9)
    disk = ltrace.default_disk(r_out=20.0)
    cam = ltrace.Camera(n, n, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
    res = dict(build=ltrace.build_id(), output_frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_out=20.0,
               max_images=3, reps=args.reps, band_rows=args.band_rows, configs={})
    med = lambda v: round(float(np.median(v)), 4)
    for integ, prec in (("rk4", 32), ("dp45_exact", 64)):
        o = ltrace.default_opts(integrator=integ, precision=prec, tb_symmetry=0)
        for mode in ("plain", "disk_images"):
            d = None if mode == "plain" else disk
            for S in args.samples:
                fine = ltrace.Camera(n * S, n * S, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
                if mode == "plain":
                    fine_call = lambda: ltrace.render(fine, met, o, want=("rgb",))
                else:
                    fine_call = lambda: ltrace.render_disk_images(fine, met, o, disk, max_images=3, want=("rgb",))
                calls = {"fine_frame": fine_call}
                for name, band in (("aa_auto", 0), ("aa_banded", args.band_rows)):
                    a = ltrace.default_aa(samples=S, mode=mode, max_images=3, band_rows=band)
                    calls[name] = (lambda a=a: ltrace.render_aa(cam, met, o, a, disk=d, want=("rgb",)))
                t = {k: dict(prologue_ms=[], integrate_ms=[], epilogue_ms=[], call_ms=[]) for k in calls}
                resolve_ms, same = [], True
                for call in calls.values():
                    call()
                for _ in range(args.reps):
                    outs = {}
                    for k, call in calls.items():
                        t0 = time.perf_counter()
                        out = call()
                        t[k]["call_ms"].append(1e3 * (time.perf_counter() - t0))
                        for w in ("prologue_ms", "integrate_ms", "epilogue_ms"):
                            t[k][w].append(out["stats"][w])
                        outs[k] = out
                    t0 = time.perf_counter()
                    host = aa.resolve(np.asarray(outs["fine_frame"]["rgb"]), S)
                    resolve_ms.append(1e3 * (time.perf_counter() - t0))
                    same = same and all(outs[k]["rgb"].tobytes() == host.tobytes() for k in ("aa_auto", "aa_banded"))
                row = {k: {w: med(v) for w, v in tv.items()} for k, tv in t.items()}
                row["fine_frame"]["host_resolve_ms"] = med(resolve_ms)
                row["fine_frame"]["call_plus_resolve_ms"] = round(row["fine_frame"]["call_ms"] + row["fine_frame"]["host_resolve_ms"], 4)
                row["fine_frame"]["integrate_ms_min_max"] = [round(min(t["fine_frame"]["integrate_ms"]), 4), round(max(t["fine_frame"]["integrate_ms"]), 4)]
                row["fine_frame"]["rgb_bytes"] = int(outs["fine_frame"]["rgb"].nbytes)
                for name, band in (("aa_auto", 0), ("aa_banded", args.band_rows)):
                    a = ltrace.default_aa(samples=S, mode=mode, max_images=3, band_rows=band)
                    nbytes, rows, bands = ltrace.aa_band_bytes(cam, met, o, a, disk=d)
                    row[name].update(band_rows=rows, bands=bands, band_record_bytes=nbytes, rgb_bytes=int(outs[name]["rgb"].nbytes))
                row["byte_identical_to_host_resolve"] = bool(same)
                row["rays"] = int(outs["aa_auto"]["stats"]["rays"])
                key = f"{integ}_f{prec}|{mode}|S{S}"
                res["configs"][key] = row
                print(key, json.dumps(row), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"aa_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
