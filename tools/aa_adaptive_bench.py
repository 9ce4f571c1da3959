"""Cost and error of adaptive supersampling (lt_render_aa_adaptive) beside the frame it approximates (lt_render_aa at S_hi).

The demo view (Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20) at --size^2 output pixels, no
background, plain and optically thin disk (3 images per ray), RK4 float32 and DP45 (exact controller) float64.  For every
configuration, alternating after one warm-up of each call, medians of --reps:
  aa_S1, aa_S2, aa_S4, aa_S8       lt_render_aa, rgb into pinned memory;
  adaptive_<lo>_<hi>_<off|default>  lt_render_aa_adaptive at (1, 4), (2, 4), (1, 8), rgb and level into pinned memory, with
                                    the colour test off (contrast = -1) and at the library's default.
Per adaptive row: N / (W H); the prologue / integrate / epilogue HIP-event sums and the wall time of the call; the figure
to hold it against, t(LO) + N / (W H) t(HI), from the lt_render_aa rows of the same loop; and the error the shortcut
introduces: max and mean |adaptive - HI| of rgb over the pixels that were NOT refined (the refined ones are HI's, bit for
bit).

The flag kernel has no event of its own (its time is part of prologue_ms).  It is measured on a view where nothing is
flagged (the same camera turned away from the hole, psi_x = 1 rad): there both calls reuse their ray records, the
adaptive call launches nothing after the flag kernel, and adaptive.prologue_ms - aa_S1.prologue_ms is the flag kernel
alone (the count's memset is enqueued before the first event); reported once per contrast setting (it reads rgb only
when the colour test is on).

--parent-root DIR: a checkout of the parent commit with its library built.  A fresh child process imports ltrace from
there and times lt_render_aa at the same settings (the yardstick: lt_render_aa must cost what it cost before this tool's
build), recorded under "parent_build".

    python tools/aa_adaptive_bench.py [--size 1024] [--reps 5] [--parent-root DIR] [--out profiles/aa_adaptive_bench_<build>.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = (1, 2, 4, 8)
PAIRS = ((1, 4), (2, 4), (1, 8))
CONFIGS = (("rk4", 32), ("dp45_exact", 64))
MODES = ("plain", "disk_images")
med = lambda v: round(float(np.median(v)), 4)


def _scene(ltrace, n, psi_x=0.0):
    vfov = np.radians(40.0)
    return (ltrace.Camera(n, n, vfov, vfov, 0.0, psi_x, 50.0, np.radians(80.0)), ltrace.Metric(ltrace.METRIC_KERR, 0, 1.0, 0.9),
            ltrace.default_disk(r_out=20.0))


def _timed(calls, reps):
    """Every call once to warm up, then `reps` rounds of all of them in turn: {name: lists of the stage sums and the
    wall time}, and each call's last result."""
    t = {k: dict(prologue_ms=[], integrate_ms=[], epilogue_ms=[], call_ms=[]) for k in calls}
    outs = {}
    for call in calls.values():
        call()
    for _ in range(reps):
        for k, call in calls.items():
            t0 = time.perf_counter()
            out = call()
            t[k]["call_ms"].append(1e3 * (time.perf_counter() - t0))
            for w in ("prologue_ms", "integrate_ms", "epilogue_ms"):
                t[k][w].append(out["stats"][w])
            outs[k] = out
    return {k: {w: med(v) for w, v in tv.items()} for k, tv in t.items()}, outs


def yardstick(ltrace, n, reps):
    """lt_render_aa alone, with whatever build `ltrace` loads."""
    ltrace.require_gpu()
    cam, met, disk = _scene(ltrace, n)
    res = dict(build=ltrace.build_id(), configs={})
    for integ, prec in CONFIGS:
        o = ltrace.default_opts(integrator=integ, precision=prec)
        for mode in MODES:
            d = None if mode == "plain" else disk
            calls = {f"aa_S{S}": (lambda S=S: ltrace.render_aa(cam, met, o, ltrace.default_aa(samples=S, mode=mode, max_images=3), disk=d, want=("rgb",)))
                     for S in SAMPLES}
            res["configs"][f"{integ}_f{prec}|{mode}"] = _timed(calls, reps)[0]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--root", default=ROOT, help="the checkout whose package and library are measured")
    ap.add_argument("--yardstick", action="store_true", help="time lt_render_aa alone and print the result as one JSON line")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path[:0] = [args.root, os.path.join(args.root, "light-path-tracer_amd")]
    import ltrace
    n = args.size
    if args.yardstick:
        print("YARDSTICK " + json.dumps(yardstick(ltrace, n, args.reps)), flush=True)
        return
    parent = None
    if args.parent_root:   # before this process opens the GPU's queues for its own timings; a fresh process, its own library
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--yardstick", "--root", os.path.abspath(args.parent_root), "--size", str(n),
                            "--reps", str(args.reps)], check=True, capture_output=True, text=True)
        parent = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("YARDSTICK ")][-1][len("YARDSTICK "):])
    ltrace.require_gpu()
    cam, met, disk = _scene(ltrace, n)
    res = dict(build=ltrace.build_id(), output_frame=f"{n}x{n}", a=0.9, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_out=20.0, max_images=3,
               reps=args.reps, default_contrast=float(ltrace.default_aa_adaptive().contrast), parent_build=parent, flag_kernel_ms={}, configs={})
    contrasts = (("off", -1.0), ("default", res["default_contrast"]))

    # the flag kernel alone: a view where nothing is flagged
    away, _, _ = _scene(ltrace, n, psi_x=1.0)
    o = ltrace.default_opts()
    calls = {"aa_S1": lambda: ltrace.render_aa(away, met, o, ltrace.default_aa(samples=1), want=("rgb",))}
    for cname, cval in contrasts:
        a = ltrace.default_aa_adaptive(samples_lo=1, samples_hi=4, contrast=cval)
        calls[cname] = (lambda a=a: ltrace.render_aa_adaptive(away, met, o, a, want=("rgb", "level")))
    row, outs = _timed(calls, args.reps)
    for cname, _ in contrasts:
        assert outs[cname]["stats"]["refined"] == 0
        res["flag_kernel_ms"][cname] = round(row[cname]["prologue_ms"] - row["aa_S1"]["prologue_ms"], 4)
    res["flag_kernel_ms"]["how"] = "adaptive.prologue_ms - aa_S1.prologue_ms on a view where nothing is flagged (psi_x = 1 rad)"
    print("flag kernel", json.dumps(res["flag_kernel_ms"]), flush=True)

    for integ, prec in CONFIGS:
        o = ltrace.default_opts(integrator=integ, precision=prec)
        for mode in MODES:
            d = None if mode == "plain" else disk
            calls = {f"aa_S{S}": (lambda S=S: ltrace.render_aa(cam, met, o, ltrace.default_aa(samples=S, mode=mode, max_images=3), disk=d, want=("rgb",)))
                     for S in SAMPLES}
            for lo, hi in PAIRS:
                for cname, cval in contrasts:
                    a = ltrace.default_aa_adaptive(samples_lo=lo, samples_hi=hi, mode=mode, max_images=3, contrast=cval)
                    calls[f"adaptive_{lo}_{hi}_{cname}"] = (lambda a=a: ltrace.render_aa_adaptive(cam, met, o, a, disk=d, want=("rgb", "level")))
            row, outs = _timed(calls, args.reps)
            for lo, hi in PAIRS:
                hi_rgb = np.asarray(outs[f"aa_S{hi}"]["rgb"])
                for cname, _ in contrasts:
                    k = f"adaptive_{lo}_{hi}_{cname}"
                    got = outs[k]
                    keep = np.asarray(got["level"]) == lo
                    err = np.abs(np.asarray(got["rgb"]).astype(np.float64) - hi_rgb)[keep]
                    frac = got["stats"]["refined"] / float(n * n)
                    assert np.asarray(got["rgb"])[~keep].tobytes() == hi_rgb[~keep].tobytes()     # refined pixels are HI's
                    row[k].update(refined=got["stats"]["refined"], refined_fraction=round(frac, 6), rays=got["stats"]["rays"],
                                  flag_kernel_ms=res["flag_kernel_ms"][cname],
                                  model_call_ms=round(row[f"aa_S{lo}"]["call_ms"] + frac * row[f"aa_S{hi}"]["call_ms"], 4),
                                  model_integrate_ms=round(row[f"aa_S{lo}"]["integrate_ms"] + frac * row[f"aa_S{hi}"]["integrate_ms"], 4),
                                  speedup_over_hi_call=round(row[f"aa_S{hi}"]["call_ms"] / row[k]["call_ms"], 3),
                                  err_max_unrefined=float(err.max()) if err.size else 0.0, err_mean_unrefined=float(err.mean()) if err.size else 0.0,
                                  unrefined_pixels_that_differ=int(np.any(err.reshape(-1, 3) > 0, axis=1).sum()))
            for S in SAMPLES:
                row[f"aa_S{S}"]["rays"] = outs[f"aa_S{S}"]["stats"]["rays"]
            key = f"{integ}_f{prec}|{mode}"
            res["configs"][key] = row
            print(key, json.dumps(row), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"aa_adaptive_bench_{res['build']}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
