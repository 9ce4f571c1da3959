"""What the reverberation response costs, on the spectrum bench's records (tools/spectrum_bench.py): the README's sequence frame --
1024^2, Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4
float32.  lt_disk_transfer_dev with the tables of a lamp post at h = 6 on three grids, device buffers:
    64 x 96     n_tau x n_bins, one plane: 6 468 keys, two key tiles;
    126 x 254   the cap, 32 768 keys in one plane: eight key tiles;
    100 x 100   one plane per image order: 3 x 102 x 102 = 31 212 keys, eight key tiles.

Yardstick: lt_disk_spectrum_dev on the same records with the grid's g axis (and its planes), from the library built from the
PARENT commit (--parent-lib; loaded into the same process beside this checkout's, so both see the same device buffers) and
from this checkout's own.  The candidates run alternately; the yardstick's own run-to-run range stands beside every ratio.
By the code a grid of one tile does the spectrum's work plus two interpolations; a grid of T tiles evaluates every slot T
times and merges each key once, so the merge and the owner's adds stay what they were and the evaluation is multiplied.
The convention is tools/spectrum_bench.py's: a sample is --batch calls back to back behind one untimed call and before one
synchronise, the time per call; --reps rounds after one warm-up round; reported: the median and the range.  No gate.

    python tools/transfer_bench.py [--size 1024] [--reps 7] [--batch 5] [--parent-lib ab_builds/libltrace_parent.so]
                                   [--out profiles/transfer_bench_<build>.json]
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
GRIDS = {"64x96": (64, 96, False), "126x254": (126, 254, False), "3x100x100": (100, 100, True)}
TILE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=5, help="calls per sample")
    ap.add_argument("--parent-lib", default=None, help="libltrace_hip.so built from the parent commit: the yardstick's build")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n = args.size
    vfov = np.radians(40.0)
    M, a, h = 1.0, 0.9, 6.0
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    disk = ltrace.default_disk(r_out=20.0)
    r_in = float(diskmod.isco(M, a))
    lamp = diskmod.Lamppost(M, a, h)
    delay, emis = lamp.tables(r_in, 20.0, 1024)
    t_ref = lamp.t_ref(50.0, np.radians(80.0))
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=a, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=r_in, r_out=20.0,
               max_images=M_IMAGES, lamppost_h=h, table_nodes=int(delay.size), t_ref=t_ref, reps=args.reps, batch=args.batch,
               spectrum_blocks=ltrace.SPECTRUM_BLOCKS, tile_keys=TILE, integrator="rk4", precision=32)
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

    parent = None
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        res_t, arg_t = ltrace.SIGNATURES["lt_disk_spectrum_dev"]
        parent.lt_disk_spectrum_dev.restype, parent.lt_disk_spectrum_dev.argtypes = res_t, arg_t
        parent.lt_build_id.restype = C.c_char_p
        res["parent_build"] = parent.lt_build_id().decode()

    o = ltrace.default_opts(integrator="rk4", precision=32, tb_symmetry=0)
    cam = ltrace.Camera(n, n, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
    rec = ltrace.trace_disk_hits(cam, met, o, disk, max_images=M_IMAGES, want=("hits", "n_hits"))
    d_hits, d_n, d_delay, d_emis = upload(rec["hits"]), upload(rec["n_hits"]), upload(delay), upload(emis)
    d_tf = hipmini.DeviceArray((ltrace.TRANSFER_MAX_KEYS,), np.float64)
    d_line = hipmini.DeviceArray((M_IMAGES * 514,), np.float64)
    head = (d_hits.ptr, d_n.ptr, n, n, M_IMAGES, met, disk)
    calls, keys, contributing = {}, {}, None
    for name, (n_tau, n_bins, split) in GRIDS.items():
        spec = diskmod.Spectrum(0.1, 1.7, n_bins, split_orders=split)
        grid = diskmod.TransferGrid(0.0, 128.0, n_tau)
        sp, lt = spec.to_lt(), grid.to_lt(r_in, 20.0, delay.size, t_ref)
        keys[name] = ltrace.transfer_keys(sp, lt, M_IMAGES)
        calls[f"transfer_{name}"] = lambda sp=sp, lt=lt: ltrace.disk_transfer_dev(*head, sp, lt, d_delay.ptr, d_emis.ptr, d_tf.ptr)
        calls[f"spectrum_{name}"] = lambda sp=sp: ltrace.disk_spectrum_dev(*head, sp, d_line.ptr)
        if parent is not None:
            def parent_call(sp=sp):
                if parent.lt_disk_spectrum_dev(d_hits.ptr, d_n.ptr, n, n, M_IMAGES, C.byref(met), C.byref(disk), C.byref(sp), d_line.ptr):
                    raise RuntimeError("the parent build's lt_disk_spectrum_dev failed")
            calls[f"parent_spectrum_{name}"] = parent_call
        if contributing is None:
            on = diskmod.transfer_slots(rec["hits"], rec["n_hits"], 1.0, spec, grid, r_in, 20.0, delay, emis, t_ref)[0]
            contributing = int(on.sum())
            # the device's answer against the numpy statement, once, on the first grid
            want = diskmod.disk_transfer(rec["hits"], rec["n_hits"], 1.0, spec, grid, r_in, 20.0, delay, emis, t_ref)
            calls[f"transfer_{name}"]()
            sync()
            got = d_tf.get()[:want.size].reshape(want.shape)
            res["agrees_with_numpy"] = bool(np.array_equal(got != 0, want != 0) and np.all(np.abs(got - want) <= 1e-11 * np.abs(want)))
    res.update(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes),
               contributing_slots=contributing, stored_slots=int(np.minimum(rec["n_hits"], M_IMAGES).sum()))
    gpu = alternately(calls, args.reps, args.batch)
    res["gpu"] = gpu
    ratios = {}
    for name in GRIDS:
        t = gpu[f"transfer_{name}"]
        yard = gpu[f"parent_spectrum_{name}" if parent is not None else f"spectrum_{name}"]
        ratios[name] = dict(keys=keys[name], tiles=(keys[name] + TILE - 1) // TILE, transfer_ms=t["ms"], yardstick_ms=yard["ms"],
                            yardstick="parent build" if parent is not None else "this build",
                            transfer_over_spectrum=round(t["ms"] / yard["ms"], 3),
                            yardstick_range_over_median=[round(yard["range_ms"][0] / yard["ms"], 3), round(yard["range_ms"][1] / yard["ms"], 3)],
                            transfer_range_over_median=[round(t["range_ms"][0] / t["ms"], 3), round(t["range_ms"][1] / t["ms"], 3)],
                            ns_per_stored_slot_and_tile=round(t["ms"] * 1e6 / (res["stored_slots"] * ((keys[name] + TILE - 1) // TILE)), 4))
        if parent is not None:
            ratios[name]["this_build_spectrum_over_parent"] = round(gpu[f"spectrum_{name}"]["ms"] / yard["ms"], 3)
    res["ratios"] = ratios
    print(json.dumps(res), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"transfer_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
