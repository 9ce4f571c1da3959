"""What the polarized thermal continuum costs beside the unpolarized one, on the thermal bench's frame (tools/thermal_bench.py):
1024^2, Kerr a = 0.9, r_obs = 50, theta_obs = 80 deg, vfov 40 deg, disk r_out = 20 (r_in = ISCO), 3 images per ray, RK4
float32, traced once by lt_trace_disk_pol with the field (0, 0, 1).  lt_disk_thermal_spectrum_stokes_dev of a 4096-node
Novikov-Thorne table and the 257-node Chandrasekhar fit at 64, 256 and 1024 log-spaced frequencies, one plane and one per
image order, and lt_shade_thermal_stokes_dev at 3 and 16 bands; device buffers.

Yardstick: lt_disk_thermal_spectrum_dev (lt_shade_thermal_dev for the bands) of the same build on the same records at the
same frequencies -- the kernel this one adds three fmas per entry and frequency to, beside its expm1 and its division.
The two run alternately; the yardstick's own run-to-run range stands beside every ratio.  --images 8 traces eight images
per ray instead, the case whose lists are walked in two halves (lt_thermal_stokes.hpp); the file name then says so.
RESOURCES are the compiler's figures for the kernels (-Rpass-analysis=kernel-resource-usage, gfx950) and the launch's LDS:
they are constants of the build, recorded here so that a profile carries them.
The convention is tools/spectrum_bench.py's: a sample is --batch calls back to back behind one untimed call and before one
synchronise, the time per call; the candidates run alternately, --reps rounds after one warm-up round; reported: the median
and the range.  No gate.

    python tools/thermal_stokes_bench.py [--size 1024] [--images 3] [--reps 5] [--batch 3]
                                         [--out profiles/thermal_stokes_bench_<build>.json]
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

COUNTS = (64, 256, 1024)
# VGPRs of k_thermal_spectrum_stokes_partial<1> / <8> beside k_thermal_spectrum_partial<1> / <8> and the scratch bytes a lane
# (the launch bound holds <8> to 128 registers, five spill); LDS bytes of a workgroup and the workgroups a CU's 160 KiB and
# its 512 VGPRs per SIMD hold, at 3 and 8 images (confirmed unchanged by profiles/thermal_fold_check.txt, part B)
RESOURCES = dict(vgprs=dict(stokes_whole=95, stokes_split=128, thermal_whole=93, thermal_split=107),
                 scratch_bytes=dict(stokes_whole=0, stokes_split=24, thermal_whole=0, thermal_split=0),
                 lds_bytes={"3": dict(stokes=25360, thermal=6928), "8": dict(stokes=33808, thermal=18448)},
                 workgroups_per_cu={"3": dict(stokes=4, thermal=4), "8": dict(stokes=4, thermal=4)},
                 lists_in_lds={"3": 4, "8": 2})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--images", type=int, default=3, help="images per ray (max_images)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=3, help="calls per sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ltrace.require_gpu()
    import hipmini   # raw device buffers on the library's own HIP runtime
    n, m = args.size, args.images
    vfov = np.radians(40.0)
    M, a = 1.0, 0.9
    met = ltrace.Metric(ltrace.METRIC_KERR, 0, M, a)
    disk = ltrace.default_disk(r_out=20.0)
    td = {False: diskmod.ThermalDisk.novikov_thorne(M, a, 20.0, t_max=1.0, f_col=1.7),
          True: diskmod.ThermalDisk.novikov_thorne(M, a, 20.0, t_max=1.0, f_col=1.7, split_orders=True)}
    atm = diskmod.Atmosphere.chandrasekhar()
    freqs = {k: np.exp(np.linspace(np.log(1e-3), np.log(60.0), k)) for k in COUNTS}
    res = dict(build=ltrace.build_id(), frame=f"{n}x{n}", a=a, r_obs=50.0, theta_obs_deg=80.0, vfov_deg=40.0, r_in=ltrace.kerr_isco(M, a),
               r_out=20.0, max_images=m, table_nodes=td[False].n_r, atmosphere_nodes=atm.n_mu, t_max=1.0, f_col=1.7, reps=args.reps,
               batch=args.batch, spectrum_blocks=ltrace.SPECTRUM_BLOCKS, integrator="rk4", precision=32, resources=RESOURCES)
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
    cam = ltrace.Camera(n, n, vfov, vfov, 0.0, 0.0, 50.0, np.radians(80.0))
    rec = ltrace.trace_disk_pol(cam, met, o, disk, ltrace.default_bfield(b_r=0.0, b_phi=0.0, b_z=1.0), max_images=m, want=("hits", "n_hits", "pol"))
    d_hits, d_n, d_pol = upload(rec["hits"]), upload(rec["n_hits"]), upload(rec["pol"])
    d_flux, d_limb, d_deg = upload(td[False].flux), upload(atm.limb), upload(atm.poldeg)
    emits = diskmod.thermal_coeffs(rec["hits"], rec["n_hits"], td[False])[2] & diskmod.atmosphere_weights(rec["pol"], atm)[1]
    emitting = int(emits.sum())
    res.update(integrate_ms=rec["stats"]["integrate_ms"], record_bytes=int(rec["hits"].nbytes + rec["n_hits"].nbytes + rec["pol"].nbytes),
               emitting_slots=emitting, lit_pixels=int(emits.any(axis=-1).sum()))
    d_nu = {k: upload(v) for k, v in freqs.items()}
    d_sp = hipmini.DeviceArray((m, 3, 1024), np.float64)
    d_img = hipmini.DeviceArray((16, 3, n, n), np.float32)
    head, tail = (d_hits.ptr, d_n.ptr), (n, n, m, met, disk)
    air = (atm.n_mu, d_limb.ptr, d_deg.ptr)
    calls = {}
    for gname, split in (("whole", False), ("split", True)):
        lt = td[split].to_lt()
        for k in COUNTS:
            calls[f"stokes_{gname}_{k}"] = lambda lt=lt, k=k: ltrace.thermal_spectrum_stokes_dev(*head, d_pol.ptr, *tail, lt, d_flux.ptr, *air,
                                                                                               d_nu[k].ptr, k, d_sp.ptr)
            calls[f"thermal_{gname}_{k}"] = lambda lt=lt, k=k: ltrace.thermal_spectrum_dev(*head, *tail, lt, d_flux.ptr, d_nu[k].ptr, k, d_sp.ptr)
    lt = td[False].to_lt()
    for k in (3, 16):
        calls[f"stokes_bands_{k}"] = lambda k=k: ltrace.shade_thermal_stokes_dev(*head, d_pol.ptr, *tail, lt, d_flux.ptr, *air, d_nu[64].ptr, k,
                                                                                 d_img.ptr)
        calls[f"thermal_bands_{k}"] = lambda k=k: ltrace.shade_thermal_dev(*head, *tail, lt, d_flux.ptr, d_nu[64].ptr, k, d_img.ptr)
    gpu = alternately(calls, args.reps, args.batch)
    res["gpu"] = gpu
    ratios = {}
    for key in [f"{g}_{k}" for g in ("whole", "split") for k in COUNTS] + ["bands_3", "bands_16"]:
        s, t = gpu["stokes_" + key], gpu["thermal_" + key]
        r = dict(stokes_over_thermal=round(s["ms"] / t["ms"], 3),
                 thermal_range_over_median=[round(t["range_ms"][0] / t["ms"], 3), round(t["range_ms"][1] / t["ms"], 3)])
        if not key.startswith("bands"):
            r["ns_per_slot_and_freq"] = round(s["ms"] * 1e6 / (emitting * int(key.split("_")[1])), 4)
        ratios[key] = r
    res["ratios"] = ratios
    # the bits the header promises, on this frame: the isotropic atmosphere's I plane is the unpolarized spectrum
    iso = diskmod.Atmosphere.isotropic()
    nu = freqs[64]
    same = ltrace.thermal_spectrum_stokes(rec["hits"], rec["n_hits"], rec["pol"], met, disk, td[True].to_lt(), td[True].flux, iso.limb, iso.poldeg, nu)
    plain = ltrace.thermal_spectrum(rec["hits"], rec["n_hits"], met, disk, td[True].to_lt(), td[True].flux, nu)
    res["isotropic_i_plane_has_the_unpolarized_bits"] = bool(np.ascontiguousarray(same[:, 0]).tobytes() == plain.tobytes())
    sp = ltrace.thermal_spectrum_stokes(rec["hits"], rec["n_hits"], rec["pol"], met, disk, td[False].to_lt(), td[False].flux, atm.limb, atm.poldeg, nu)
    deg, ang = diskmod.polarization_degree_angle(sp)
    res["polarization"] = dict(nu=[float(nu[i]) for i in (20, 40, 50)], degree=[round(float(deg[0, i]), 5) for i in (20, 40, 50)],
                               angle_deg=[round(float(np.degrees(ang[0, i])), 2) for i in (20, 40, 50)])
    print(json.dumps(res), flush=True)
    out = args.out or os.path.join(ROOT, "profiles", f"thermal_stokes_bench_{res['build']}{'' if n == 1024 else '_' + str(n)}"
                                                     f"{'' if m == 3 else '_m' + str(m)}.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
