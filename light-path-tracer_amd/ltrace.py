"""ctypes binding of libltrace_hip.so (C-ABI: include/ltrace.h).

Thin by design: structs, argument marshalling and error translation only.  The
library is the product; it is HIP-only.  If the shared object is missing, or no
GPU is visible, calls raise -- there is no CPU fallback here or anywhere in this
package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LTRACE_LIB", os.path.join(_HERE, "lib", "libltrace_hip.so"))

OK, ERR_INVALID_ARG, ERR_HIP, ERR_NO_DEVICE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4
METRIC_SCHWARZSCHILD, METRIC_KERR = 0, 1
INTEGRATOR_DP45, INTEGRATOR_RK4, INTEGRATOR_DP45_EXACT = 0, 1, 2
SCHED_DIRECT, SCHED_QUEUE = 0, 1
STAT_RAYS, STAT_STEPS, STAT_RHS_EVALS, STAT_ESCAPED, STAT_CAPTURED, STAT_INVALID = range(6)
STAT_WAVE_ITERS, STAT_WAVES, STAT_CLK_CYCLES, STAT_CLK_TICKS = 6, 7, 8, 9
STAT_BG_TILES_LDS, STAT_BG_TILES_GLOBAL = 10, 11
STAT_DISK = 12
STAT_DISK_HITS = 13
STAT_AA_REFINED = 14
STAT_EQ_ITERS = 15
DISK_MAX_IMAGES = 8
STATUS_DISK = 2
STAT_WORDS = 16

INTEGRATORS = {"dp45": INTEGRATOR_DP45, "rk4": INTEGRATOR_RK4, "dp45_exact": INTEGRATOR_DP45_EXACT}
SCHEDULES = {"direct": SCHED_DIRECT, "queue": SCHED_QUEUE}


class LtraceError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libltrace_hip error {code}: {msg}")
        self.code = code


class Camera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("hfov", C.c_double), ("vfov", C.c_double),
                ("psi_y", C.c_double), ("psi_x", C.c_double),
                ("r_obs", C.c_double), ("theta_obs", C.c_double)]


class Metric(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("M", C.c_double), ("a", C.c_double)]


class Opts(C.Structure):
    _fields_ = [("integrator", C.c_int32), ("precision", C.c_int32), ("schedule", C.c_int32),
                ("tb_symmetry", C.c_int32), ("loop_around", C.c_int32), ("row_block", C.c_int32),
                ("n_parts", C.c_int32), ("part", C.c_int32),
                ("axis_refine_frac", C.c_double), ("phi_max", C.c_double), ("h_max", C.c_double),
                ("stream", C.c_void_p), ("timing", C.c_int32), ("bg_sampling", C.c_int32),
                ("block_owner", C.c_void_p), ("n_blocks", C.c_int32), ("reserved", C.c_int32)]


BG_LDS_TILES, BG_GLOBAL = 0, 1


class DenseOpts(C.Structure):
    _fields_ = [("lambda_max", C.c_double), ("r_stop_inner", C.c_double), ("r_stop_outer", C.c_double),
                ("rtol", C.c_double), ("atol", C.c_double), ("max_step", C.c_double),
                ("max_points", C.c_int64), ("max_attempts", C.c_int32), ("length_binning", C.c_int32),
                ("stream", C.c_void_p)]


class Disk(C.Structure):
    """lt_disk: thin Keplerian accretion disk (r_in <= 0: the ISCO)."""
    _fields_ = [("r_in", C.c_double), ("r_out", C.c_double), ("q", C.c_double), ("exposure", C.c_double),
                ("flags", C.c_int32), ("reserved", C.c_int32)]


class HotSpot(C.Structure):
    """lt_hotspot: a Gaussian spot on the circular equatorial orbit at r_spot (azimuth phi0 at coordinate time 0)."""
    _fields_ = [("r_spot", C.c_double), ("phi0", C.c_double), ("sigma", C.c_double), ("exposure", C.c_double),
                ("with_disk", C.c_int32), ("reserved", C.c_int32)]


class DiskMap(C.Structure):
    """lt_diskmap: the annulus, rotation and brightness of an (n_r, n_phi) emissivity table on the disk."""
    _fields_ = [("r_min", C.c_double), ("r_max", C.c_double), ("omega_p", C.c_double), ("exposure", C.c_double),
                ("n_r", C.c_int32), ("n_phi", C.c_int32), ("rotation", C.c_int32), ("with_disk", C.c_int32)]


MAP_KEPLERIAN, MAP_RIGID = 0, 1


class DiskMovie(C.Structure):
    """lt_diskmovie: the clock of (n_frames, n_r, n_phi) emissivity tables -- frame q at t0 + q dt_frame -- and what
    happens beyond them (MOVIE_HOLD / MOVIE_LOOP)."""
    _fields_ = [("t0", C.c_double), ("dt_frame", C.c_double), ("n_frames", C.c_int32), ("boundary", C.c_int32)]


MOVIE_HOLD, MOVIE_LOOP = 0, 1


class Spectrum(C.Structure):
    """lt_spectrum: a linear grid in g = E_obs / E_rest (n_bins bins, an underflow and an overflow column)."""
    _fields_ = [("g_min", C.c_double), ("g_max", C.c_double), ("n_bins", C.c_int32), ("split_orders", C.c_int32)]


SPECTRUM_MAX_BINS, SPECTRUM_BLOCKS, SPECTRUM_WORKSPACE_BYTES = 512, 256, 64 << 20
VISIBILITY_MAX_BASELINES, VISIBILITY_BLOCKS, VISIBILITY_BATCH_TERMS, VISIBILITY_WORKSPACE_BYTES = 1024, 256, 16, 64 << 20
VISIBILITY_STOKES_BATCH_PAIRS = 5


class Thermal(C.Structure):
    """lt_thermal: the range and size of a radial flux table, the temperature scale t_max (a frequency), the
    colour-correction factor and the brightness of the disk's thermal continuum."""
    _fields_ = [("r_min", C.c_double), ("r_max", C.c_double), ("t_max", C.c_double), ("f_col", C.c_double), ("exposure", C.c_double),
                ("n_r", C.c_int32), ("split_orders", C.c_int32)]


THERMAL_MAX_NODES, THERMAL_MAX_FREQS, THERMAL_MAX_BANDS = 65536, 1024, 16


class Atmosphere(C.Structure):
    """lt_atmosphere: the size of a scattering atmosphere's two tables on mu (limb, poldeg), node i at mu = i / (n_mu - 1)."""
    _fields_ = [("n_mu", C.c_int32), ("reserved", C.c_int32)]


ATMOSPHERE_MAX_NODES = 4096


class Transfer(C.Structure):
    """lt_transfer: the delay grid of a transfer function, the range and size of its two radial tables (delay, emis) and
    the direct flash's arrival time t_ref that every delay is counted from."""
    _fields_ = [("tau_min", C.c_double), ("tau_max", C.c_double), ("n_tau", C.c_int32), ("n_r", C.c_int32),
                ("r_min", C.c_double), ("r_max", C.c_double), ("t_ref", C.c_double)]


TRANSFER_MAX_TAU, TRANSFER_MAX_KEYS = 1024, 32768


class BField(C.Structure):
    """lt_bfield: the field's components in the emitter's frame and the polarization fraction."""
    _fields_ = [("b_r", C.c_double), ("b_phi", C.c_double), ("b_z", C.c_double), ("pol_frac", C.c_double)]


class AA(C.Structure):
    """lt_aa: supersampling (samples x samples rays per pixel; band_rows 0 = automatic)."""
    _fields_ = [("samples", C.c_int32), ("mode", C.c_int32), ("max_images", C.c_int32), ("band_rows", C.c_int32)]


class AAAdaptive(C.Structure):
    """lt_aa_adaptive: samples_lo^2 rays for every pixel, samples_hi^2 for the pixels on an edge (contrast < 0: the
    colour test is off; band_rows / chunk_pixels 0 = automatic)."""
    _fields_ = [("samples_lo", C.c_int32), ("samples_hi", C.c_int32), ("mode", C.c_int32), ("max_images", C.c_int32),
                ("band_rows", C.c_int32), ("chunk_pixels", C.c_int32), ("contrast", C.c_float), ("reserved", C.c_int32)]


AA_PLAIN, AA_DISK, AA_DISK_IMAGES = 0, 1, 2
AA_MAX_SAMPLES = 8
AA_BAND_BYTES = 2 << 30

TRACK_RANGE_END, TRACK_CAPTURE_EVENT, TRACK_ESCAPE_EVENT, TRACK_FAILED, TRACK_ATTEMPT_LIMIT = 0, 1, 2, -1, -2


class Stats(C.Structure):
    _fields_ = [("counters", C.c_uint64 * STAT_WORDS),
                ("prologue_ms", C.c_double), ("integrate_ms", C.c_double), ("epilogue_ms", C.c_double)]


_dp = C.POINTER(C.c_double)
_lib = None

# name -> (restype, argtypes); every symbol include/ltrace.h declares
SIGNATURES = {
    "lt_version": (C.c_int, []),
    "lt_build_id": (C.c_char_p, []),
    "lt_host_alloc": (C.c_void_p, [C.c_size_t]),
    "lt_host_free": (C.c_int, [C.c_void_p]),
    "lt_render_multi": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.POINTER(Stats)]),
    "lt_last_error": (C.c_char_p, []),
    "lt_device_count": (C.c_int, []),
    "lt_set_device": (C.c_int, [C.c_int]),
    "lt_shutdown": (C.c_int, []),
    "lt_release_stream": (C.c_int, [C.c_void_p]),
    "lt_default_opts": (None, [C.POINTER(Opts)]),
    "lt_trace_batch_schw": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_int64, C.c_double, C.c_double,
                                      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_trace_batch_kerr": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
                                      C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_trace_batch_kerr_general_probe": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
                                                    C.c_double, C.c_void_p, C.c_int, C.c_int64,
                                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_kerr_rhs_probe": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "lt_kerr_rhs_form_probe": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "lt_kerr_step_probe": (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                     C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_dp45_attempt_probe": (C.c_int, [C.c_double] * 4 + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 6),
    "lt_dp45_advance_probe": (C.c_int, [C.c_double] * 4 + [C.c_void_p] * 8 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 4),
    "lt_dp45_controller_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "lt_ic_probe": (C.c_int, [C.c_int] + [C.c_double] * 4 + [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_void_p]),
    "lt_rk4_advance_probe": (C.c_int, [C.c_double] * 5 + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 3),
    "lt_schw_trace_probe": (C.c_int, [C.c_double] * 4 + [C.c_void_p] * 2 + [C.c_int64, C.c_int] + [C.c_void_p] * 4),
    "lt_extract_probe": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]
                         + [C.c_void_p] * 4),
    "lt_math32_probe": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]),
    "lt_math64_probe": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_disk_crossing_probe": (C.c_int, [C.POINTER(Metric), C.c_double, C.c_double] + [C.c_void_p] * 5 + [C.c_int64, C.c_int]
                               + [C.c_void_p] * 3),
    "lt_disk_advance_probe": (C.c_int, [C.POINTER(Metric)] + [C.c_double] * 5 + [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int64]
                              + [C.c_void_p] * 5),
    "lt_disk_shade_probe": (C.c_int, [C.POINTER(Metric), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int64] + [C.c_void_p] * 3),
    "lt_disk_timed_advance_probe": (C.c_int, [C.POINTER(Metric)] + [C.c_double] * 5 + [C.c_int] * 3 + [C.c_void_p] * 10
                                    + [C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 11),
    "lt_set_eq_streak": (C.c_int, [C.c_int]),
    "lt_set_unit_streak": (C.c_int, [C.c_int]),
    "lt_set_tail_split": (C.c_int, [C.c_int]),
    "lt_tail_split_counts": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lt_tail_split_plan": (C.c_int, [C.c_int32] * 7 + [C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    "lt_sincos_q1_probe": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "lt_local_rows": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "lt_global_row": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "lt_render_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_render": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.POINTER(Stats)]),
    "lt_scatter_rows_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p]),
    "lt_scatter_rows_indexed_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "lt_timing_collect": (C.c_int, [_dp, _dp, _dp, C.POINTER(C.c_int32)]),
    "lt_ic_reuse_counts": (None, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "lt_pixel_angles": (C.c_int, [C.POINTER(Camera), C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_shade": (C.c_int, [C.POINTER(Camera), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p]),
    "lt_default_dense_opts": (None, [C.POINTER(DenseOpts)]),
    "lt_integrate_dense": (C.c_int, [C.POINTER(Metric), C.POINTER(DenseOpts), C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_integrate_dense_dev": (C.c_int, [C.POINTER(Metric), C.POINTER(DenseOpts), C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_rhs8_probe": (C.c_int, [C.POINTER(Metric), C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_dense_predict_lengths": (C.c_int, [C.POINTER(Metric), C.POINTER(DenseOpts), C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_default_disk": (None, [C.POINTER(Disk)]),
    "lt_kerr_isco": (C.c_double, [C.c_double, C.c_double]),
    "lt_render_disk_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.c_void_p,
                                     C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "lt_render_disk": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.POINTER(Stats)]),
    "lt_trace_batch_kerr_disk": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
                                           C.c_double, C.c_void_p, C.c_int, C.c_int, C.POINTER(Disk), C.c_int64,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_render_disk_images_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk),
                                            C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_render_disk_images": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk),
                                        C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "lt_trace_batch_kerr_disk_images": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                  C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.POINTER(Disk),
                                                  C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]),
    "lt_trace_disk_hits_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_trace_disk_hits": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "lt_trace_batch_kerr_disk_hits": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                                C.c_double, C.c_double, C.c_void_p, C.c_int, C.c_int, C.POINTER(Disk),
                                                C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "lt_step_time_probe": (C.c_int, [C.POINTER(Metric), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_int, C.c_void_p]),
    "lt_time_rates_probe": (C.c_int, [C.POINTER(Metric), C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    "lt_default_hotspot": (None, [C.POINTER(HotSpot)]),
    "lt_shade_hotspot_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                       C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                       C.c_void_p]),
    "lt_shade_hotspot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                   C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "lt_hotspot_lightcurve_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                            C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_double, C.c_int32,
                                            C.c_void_p]),
    "lt_hotspot_lightcurve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                        C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_double, C.c_int32,
                                        C.c_void_p]),
    "lt_default_bfield": (None, [C.POINTER(BField)]),
    "lt_trace_disk_pol_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.POINTER(BField),
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "lt_trace_disk_pol": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(Disk), C.POINTER(BField),
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.POINTER(Stats)]),
    "lt_trace_batch_kerr_disk_pol": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
                                               C.c_double, C.c_void_p, C.c_int, C.c_int, C.POINTER(Disk), C.POINTER(BField),
                                               C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_polarization_probe": (C.c_int, [C.POINTER(Metric), C.c_double, C.c_double, C.POINTER(BField), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p]),
    "lt_shade_stokes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                      C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_double, C.c_void_p]),
    "lt_shade_stokes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                  C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_double, C.c_void_p]),
    "lt_hotspot_lightcurve_stokes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                   C.POINTER(Metric), C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField),
                                                   C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_hotspot_lightcurve_stokes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                               C.POINTER(Metric), C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField),
                                               C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_shade_hotspot_aa_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                          C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                          C.c_void_p]),
    "lt_shade_hotspot_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                      C.POINTER(Disk), C.POINTER(HotSpot), C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                      C.c_void_p]),
    "lt_shade_stokes_aa_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.POINTER(Metric), C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_double,
                                         C.c_void_p]),
    "lt_shade_stokes_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.POINTER(Metric), C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_double,
                                     C.c_void_p]),
    "lt_default_diskmap": (None, [C.POINTER(DiskMap)]),
    "lt_default_spectrum": (None, [C.POINTER(Spectrum)]),
    "lt_disk_spectrum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                    C.POINTER(Spectrum), C.c_void_p]),
    "lt_hotspot_spectrum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                       C.POINTER(HotSpot), C.POINTER(Spectrum), C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_diskmap_spectrum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                       C.POINTER(DiskMap), C.c_void_p, C.POINTER(Spectrum), C.c_double, C.c_double, C.c_int32,
                                       C.c_void_p]),
    "lt_disk_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                    C.POINTER(Spectrum), C.c_void_p]),
    "lt_hotspot_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                       C.POINTER(HotSpot), C.POINTER(Spectrum), C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_diskmap_spectrum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                       C.POINTER(DiskMap), C.c_void_p, C.POINTER(Spectrum), C.c_double, C.c_double, C.c_int32,
                                       C.c_void_p]),
    "lt_visibility_batch_times": (C.c_int32, [C.c_int32, C.c_int32]),
    "lt_disk_visibility_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                   C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_hotspot_visibility_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                      C.POINTER(HotSpot), C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_diskmap_visibility_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                      C.POINTER(DiskMap), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                      C.c_void_p]),
    "lt_disk_visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                   C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_hotspot_visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                      C.POINTER(HotSpot), C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_diskmap_visibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                      C.POINTER(DiskMap), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                      C.c_void_p]),
    "lt_visibility_stokes_batch_pairs": (C.c_int32, []),
    "lt_disk_visibility_stokes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                          C.POINTER(Disk), C.POINTER(BField), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_hotspot_visibility_stokes_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                             C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_disk_visibility_stokes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                          C.POINTER(Disk), C.POINTER(BField), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "lt_hotspot_visibility_stokes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                             C.POINTER(Disk), C.POINTER(HotSpot), C.POINTER(BField), C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_double, C.c_double, C.c_int32, C.c_void_p]),
    "lt_shade_diskmap_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                       C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p]),
    "lt_shade_diskmap": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                   C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p]),
    "lt_shade_diskmap_aa_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                          C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p]),
    "lt_shade_diskmap_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                      C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_void_p, C.c_int32,
                                      C.c_void_p, C.c_void_p]),
    "lt_diskmap_lightcurve_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                            C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                            C.c_void_p]),
    "lt_diskmap_lightcurve": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                        C.POINTER(Disk), C.POINTER(DiskMap), C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                        C.c_void_p]),
    "lt_default_diskmovie": (None, [C.POINTER(DiskMovie)]),
    "lt_default_aa": (None, [C.POINTER(AA)]),
    "lt_render_aa_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AA), C.POINTER(Disk),
                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_render_aa": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AA), C.POINTER(Disk),
                               C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "lt_aa_band_bytes": (C.c_int64, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AA), C.POINTER(Disk),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "lt_default_aa_adaptive": (None, [C.POINTER(AAAdaptive)]),
    "lt_render_aa_adaptive_dev": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AAAdaptive),
                                            C.POINTER(Disk), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "lt_render_aa_adaptive": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AAAdaptive),
                                        C.POINTER(Disk), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "lt_aa_adaptive_plan": (C.c_int, [C.POINTER(Camera), C.POINTER(Metric), C.POINTER(Opts), C.POINTER(AAAdaptive),
                                      C.POINTER(Disk), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
}


# the thermal continuum: (hits, n_hits, R, W, max_images, metric, disk, thermal, flux, nu, n_freq, out)
SIGNATURES["lt_default_thermal"] = (None, [C.POINTER(Thermal)])
for _name in ("lt_disk_thermal_spectrum", "lt_shade_thermal"):
    for _suffix in ("", "_dev"):
        SIGNATURES[_name + _suffix] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric), C.POINTER(Disk),
                                                 C.POINTER(Thermal), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])

# the polarized thermal continuum: (hits, n_hits, pol, R, W, max_images, metric, disk, thermal, flux, atmosphere, limb, poldeg, nu, n_freq, out)
for _name in ("lt_disk_thermal_spectrum_stokes", "lt_shade_thermal_stokes"):
    for _suffix in ("", "_dev"):
        SIGNATURES[_name + _suffix] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                                 C.POINTER(Disk), C.POINTER(Thermal), C.c_void_p, C.POINTER(Atmosphere), C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_int32, C.c_void_p])


# the reverberation response: (hits, n_hits, R, W, max_images, metric, disk, spec, transfer, delay, emis, out)
SIGNATURES["lt_default_transfer"] = (None, [C.POINTER(Transfer)])
for _suffix in ("", "_dev"):
    SIGNATURES["lt_disk_transfer" + _suffix] = (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(Metric),
                                                          C.POINTER(Disk), C.POINTER(Spectrum), C.POINTER(Transfer), C.c_void_p, C.c_void_p,
                                                          C.c_void_p])


def _movie_signature(name):
    """The map's signature with `const lt_diskmovie *movie` after `map`."""
    res, args = SIGNATURES[name]
    at = args.index(C.POINTER(DiskMap)) + 1
    return res, args[:at] + [C.POINTER(DiskMovie)] + args[at:]


# the movie's ten entry points: lt_shade_diskmovie[_aa][_dev], lt_diskmovie_{lightcurve,spectrum,visibility}[_dev]
for _name in ("lt_shade_diskmap", "lt_shade_diskmap_aa", "lt_diskmap_lightcurve", "lt_diskmap_spectrum", "lt_diskmap_visibility"):
    for _suffix in ("", "_dev"):
        SIGNATURES[_name.replace("diskmap", "diskmovie") + _suffix] = _movie_signature(_name + _suffix)


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _check(rc):
    if rc != OK:
        raise LtraceError(rc, load().lt_last_error().decode("utf-8", "replace"))


def device_count():
    return int(load().lt_device_count())


def require_gpu():
    if device_count() <= 0:
        raise LtraceError(ERR_NO_DEVICE, "no HIP device visible; this package has no CPU path")


def _default(struct, fn, kw, names=None):
    """A `struct` filled by the library's `fn` (an lt_default_*), then the keywords set in their order; names: {keyword:
    {name: value}} for the keywords that may be given by name."""
    s = struct()
    getattr(load(), fn)(C.byref(s))
    for k, v in kw.items():
        if names and k in names and isinstance(v, str):
            v = names[k][v]
        setattr(s, k, v)
    return s


def default_opts(**kw):
    o = _default(Opts, "lt_default_opts", {})
    for k, v in kw.items():                      # (block_owner sets n_blocks as well: the keywords keep their order)
        if k == "integrator" and isinstance(v, str):
            v = INTEGRATORS[v]
        if k == "schedule" and isinstance(v, str):
            v = SCHEDULES[v]
        if k == "block_owner":
            set_block_owner(o, v)
            continue
        setattr(o, k, v)
    return o


def set_block_owner(opts, owner):
    """Attach a row-block -> partition table (uint16, one entry per row block) to opts; None = block-cyclic."""
    if owner is None:
        opts.block_owner, opts.n_blocks, opts._owner_keep = None, 0, None
        return
    tab = np.ascontiguousarray(owner, dtype=np.uint16)
    opts._owner_keep = tab                       # the struct only holds the address
    opts.block_owner, opts.n_blocks = tab.ctypes.data, tab.size


def owned_rows(height, row_block, owner, part):
    """Global row index of every local row of partition `part` under a block-owner table (ascending)."""
    owner = np.asarray(owner)
    rows = [np.arange(b * row_block, min((b + 1) * row_block, height)) for b in np.nonzero(owner == part)[0]]
    return np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, dtype=np.int64)


def _np_ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _p(x):
    """A device address given as an integer (tensor.data_ptr()); 0 = NULL."""
    return C.c_void_p(x) if x else None


def _out(a, dtype, n, name):
    if a is None:
        return None
    if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.size == n
            and a.flags.writeable):
        raise ValueError(f"{name} must be a writable C-contiguous {np.dtype(dtype).name} array of {n} elements")
    return a


def trace_batch_schw(M, r_obs, alphas, out_fa, out_w, phi_max=50.0, h_max=0.05, precision=32,
                     out_status=None, out_rhs_evals=None):
    """In-place twin of _trace_rays_batch_schwarzschild (reference metrics.py:661-668)."""
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    n = al.size
    _out(out_fa, np.float64, n, "out_fa")
    _out(out_w, np.int64, n, "out_w")
    _out(out_status, np.int8, n, "out_status")
    _out(out_rhs_evals, np.uint32, n, "out_rhs_evals")
    _check(load().lt_trace_batch_schw(M, r_obs, _np_ptr(al), n, phi_max, h_max, precision,
                                      _np_ptr(out_fa), _np_ptr(out_w), _np_ptr(out_status),
                                      _np_ptr(out_rhs_evals)))


def _ray_inputs(alphas, thetas, axis_refines):
    """The rays of a batch call as the library reads them -> (alphas f64, thetas f64, axis_refines u8 or None, n)."""
    al = np.ascontiguousarray(alphas, dtype=np.float64)
    th = np.ascontiguousarray(thetas, dtype=np.float64)
    n = al.size
    if th.size != n:
        raise ValueError("alphas and thetas differ in length")
    ar = None
    if axis_refines is not None:
        ar = np.ascontiguousarray(axis_refines).astype(np.uint8)
        if ar.size != n:
            raise ValueError("axis_refines has the wrong length")
    return al, th, ar, n


def _named(table, v):
    """An integrator / schedule given by name or by the library's value."""
    return table[v] if isinstance(v, str) else v


def trace_batch_kerr(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, axis_refines, out_fa, out_w,
                     integrator=INTEGRATOR_RK4, precision=32, schedule=SCHED_DIRECT,
                     out_status=None, out_rhs_evals=None):
    """In-place twin of _trace_rays_batch_kerr (reference metrics.py:671-679)."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    _out(out_fa, np.float64, n, "out_fa")
    _out(out_w, np.int64, n, "out_w")
    _out(out_status, np.int8, n, "out_status")
    _out(out_rhs_evals, np.uint32, n, "out_rhs_evals")
    integrator, schedule = _named(INTEGRATORS, integrator), _named(SCHEDULES, schedule)
    _check(load().lt_trace_batch_kerr(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max, _np_ptr(ar),
                                      integrator, precision, schedule, n, _np_ptr(out_fa), _np_ptr(out_w),
                                      _np_ptr(out_status), _np_ptr(out_rhs_evals)))


def trace_batch_kerr_general_probe(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, axis_refines, out_fa, out_w,
                                   precision=32, out_status=None, out_rhs_evals=None):
    """trace_batch_kerr (RK4) by the general iteration alone, without the far-field streak: the streak's yardstick
    (lt_trace_batch_kerr_general_probe)."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    _out(out_fa, np.float64, n, "out_fa")
    _out(out_w, np.int64, n, "out_w")
    _out(out_status, np.int8, n, "out_status")
    _out(out_rhs_evals, np.uint32, n, "out_rhs_evals")
    _check(load().lt_trace_batch_kerr_general_probe(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max, _np_ptr(ar),
                                                    precision, n, _np_ptr(out_fa), _np_ptr(out_w), _np_ptr(out_status),
                                                    _np_ptr(out_rhs_evals)))


def kerr_rhs_probe(M, a, states, p_phi, precision=32):
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    pp = np.ascontiguousarray(p_phi, dtype=np.float64).ravel()
    out = np.empty_like(st)
    _check(load().lt_kerr_rhs_probe(M, a, _np_ptr(st), _np_ptr(pp), st.shape[0], precision, _np_ptr(out)))
    return out


RHS_FORMS = {"checked": 0, "unchecked": 1, "packed": 2, "packed_last": 3}
STEP_FORMS = {"checked": 0, "fast": 1, "fast_q1": 2, "packed": 3}


def kerr_rhs_form_probe(M, a, states, p_phi, precision=32, form="checked"):
    """The right-hand side in one of the forms the steps use (RHS_FORMS; lt_kerr_rhs_form_probe) -> (n,5) float64."""
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    pp = np.ascontiguousarray(p_phi, dtype=np.float64).ravel()
    out = np.empty_like(st)
    _check(load().lt_kerr_rhs_form_probe(M, a, _np_ptr(st), _np_ptr(pp), st.shape[0], precision, RHS_FORMS[form], _np_ptr(out)))
    return out


def kerr_step_probe(M, a, states, p_phi, h, refine=None, precision=32, form="checked"):
    """One RK4 step from each of n states in one of the step's forms (STEP_FORMS; lt_kerr_step_probe).
    -> dict(states (n,5), min_r (n,), max_d (n,), cs (n,2)): float64 holding the values of the precision computed in."""
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    n = st.shape[0]
    pp = np.ascontiguousarray(p_phi, dtype=np.float64).ravel()
    hh = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)))
    rf = np.zeros(n, dtype=np.uint8) if refine is None else np.ascontiguousarray(np.broadcast_to(np.asarray(refine), (n,))).astype(np.uint8)
    out, mr, md, cs = np.empty_like(st), np.empty(n), np.empty(n), np.empty((n, 2))
    _check(load().lt_kerr_step_probe(M, a, _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(hh), n, precision, STEP_FORMS[form],
                                     _np_ptr(out), _np_ptr(mr), _np_ptr(md), _np_ptr(cs)))
    return dict(states=out, min_r=mr, max_d=md, cs=cs)


def _dp45_rows(states, p_phi, h, refine, k1, sc0):
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    n = st.shape[0]
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p_phi, dtype=np.float64), (n,)))
    hh = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), (n,)))
    rf = np.zeros(n, dtype=np.uint8) if refine is None else np.ascontiguousarray(np.broadcast_to(np.asarray(refine), (n,))).astype(np.uint8)
    kk = None if k1 is None else np.ascontiguousarray(k1, dtype=np.float64).reshape(n, 5)
    sc = None if sc0 is None else np.ascontiguousarray(sc0, dtype=np.float64).reshape(n, 2)
    return st, n, pp, hh, rf, kk, sc


def dp45_attempt_probe(M, a, states, p_phi, h, refine=None, k1=None, sc0=None, exact=True, checked=False, r_obs=50.0,
                       lambda_max=5000.0):
    """One DP45 step attempt per state in the checked or the branch-free form (lt_dp45_attempt_probe), float64.
    -> dict(next (n,5), k7 (n,5), sc (n,2) [sin, cos] of the candidate's polar angle, err_sq, min_r, max_d (n,))."""
    st, n, pp, hh, rf, kk, sc = _dp45_rows(states, p_phi, h, refine, k1, sc0)
    nxt, k7, osc = np.empty_like(st), np.empty_like(st), np.empty((n, 2))
    err, mr, md = np.empty(n), np.empty(n), np.empty(n)
    _check(load().lt_dp45_attempt_probe(M, a, r_obs, lambda_max, _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(kk), _np_ptr(sc),
                                        _np_ptr(hh), n, int(bool(exact)), int(bool(checked)), _np_ptr(nxt), _np_ptr(k7), _np_ptr(osc),
                                        _np_ptr(err), _np_ptr(mr), _np_ptr(md)))
    return dict(next=nxt, k7=k7, sc=osc, err_sq=err, min_r=mr, max_d=md)


def dp45_advance_probe(M, a, states, p_phi, h, refine=None, k1=None, sc0=None, lam=None, steps=None, exact=True, n_attempts=1,
                       r_obs=50.0, lambda_max=5000.0):
    """Up to n_attempts iterations of the DP45 loop body per state (lt_dp45_advance_probe); rows 64 b ... 64 b + 63 share a
    wavefront.  -> dict(event, steps, attempts (n,) int32, state (n,5), k1 (n,5), sc (n,2), lam, h (n,))."""
    st, n, pp, hh, rf, kk, sc = _dp45_rows(states, p_phi, h, refine, k1, sc0)
    ll = None if lam is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,)))
    ss = None if steps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(steps), (n,))).astype(np.uint32)
    out, ok1, misc, oi = np.empty_like(st), np.empty_like(st), np.empty((n, 4)), np.empty((n, 3), dtype=np.int32)
    _check(load().lt_dp45_advance_probe(M, a, r_obs, lambda_max, _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(kk), _np_ptr(sc),
                                        _np_ptr(hh), _np_ptr(ll), _np_ptr(ss), n, int(bool(exact)), int(n_attempts), _np_ptr(out),
                                        _np_ptr(ok1), _np_ptr(misc), _np_ptr(oi)))
    return dict(event=oi[:, 0].copy(), steps=oi[:, 1].copy(), attempts=oi[:, 2].copy(), state=out, k1=ok1, sc=misc[:, :2].copy(),
                lam=misc[:, 2].copy(), h=misc[:, 3].copy())


def dp45_controller_probe(err_sq, h, exact=True):
    """The DP45 step-size controller on any (err_sq, h) (lt_dp45_controller_probe) -> (reject (n,) bool, h_next (n,))."""
    e = np.ascontiguousarray(err_sq, dtype=np.float64).ravel()
    hh = np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), e.shape))
    rj, out = np.empty(e.size, dtype=np.uint8), np.empty(e.size)
    _check(load().lt_dp45_controller_probe(int(bool(exact)), _np_ptr(e), _np_ptr(hh), e.size, _np_ptr(rj), _np_ptr(out)))
    return rj.astype(bool), out


FLAG_OK, FLAG_REFINE, FLAG_PAD = 1, 2, 4                                # flags of a ray record (lt_ic_probe)
EV_CAPTURED, EV_INVALID, EV_ESCAPED, EV_MAXRANGE, EV_PAD, EV_RUNNING = -1, 0, 1, 2, 3, 4   # events of a final record


def ic_probe(kind, M, a, r_obs, theta_obs, alphas, thetas=None, refines=None, precision=64):
    """The ray records the array prologue stores (lt_ic_probe) -> (n_q,4) float64, n_q = n rounded up to a multiple of 64:
    p_r, p_theta, p_phi, flags (Kerr) or w0, 0, 0, flags (Schwarzschild); the rows from n on are padding (FLAG_PAD)."""
    al = np.ascontiguousarray(alphas, dtype=np.float64).ravel()
    n = al.size
    th = None if thetas is None else np.ascontiguousarray(np.broadcast_to(np.asarray(thetas, dtype=np.float64), (n,)))
    rf = None if refines is None else np.ascontiguousarray(np.broadcast_to(np.asarray(refines), (n,))).astype(np.uint8)
    out = np.empty(((n + 63) // 64 * 64, 4))
    _check(load().lt_ic_probe(int(kind), M, a, r_obs, theta_obs, _np_ptr(al), _np_ptr(th), _np_ptr(rf), n, precision, _np_ptr(out)))
    return out


def rk4_advance_probe(M, a, states, p_phi, refine=None, lam=None, h_retry=None, steps=None, precision=64, n_iters=1, r_obs=50.0,
                      lambda_max=5000.0, h_max=1.0):
    """Up to n_iters iterations (step attempts) of the fixed-step RK4 loop body per state (lt_rk4_advance_probe); rows
    64 b ... 64 b + 63 share a wavefront.  -> dict(event, steps, iters (n,) int32, state (n,5), lam, h_retry (n,))."""
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    n = st.shape[0]
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p_phi, dtype=np.float64), (n,)))
    rf = np.zeros(n, dtype=np.uint8) if refine is None else np.ascontiguousarray(np.broadcast_to(np.asarray(refine), (n,))).astype(np.uint8)
    ll = None if lam is None else np.ascontiguousarray(np.broadcast_to(np.asarray(lam, dtype=np.float64), (n,)))
    hr = None if h_retry is None else np.ascontiguousarray(np.broadcast_to(np.asarray(h_retry, dtype=np.float64), (n,)))
    ss = None if steps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(steps), (n,))).astype(np.uint32)
    out, misc, oi = np.empty_like(st), np.empty((n, 2)), np.empty((n, 3), dtype=np.int32)
    _check(load().lt_rk4_advance_probe(M, a, r_obs, lambda_max, h_max, _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(ll), _np_ptr(hr),
                                       _np_ptr(ss), n, precision, int(n_iters), _np_ptr(out), _np_ptr(misc), _np_ptr(oi)))
    return dict(event=oi[:, 0].copy(), steps=oi[:, 1].copy(), iters=oi[:, 2].copy(), state=out, lam=misc[:, 0].copy(),
                h_retry=misc[:, 1].copy())


def schw_trace_probe(M, r_obs, u0, w0, phi_max=50.0, h_max=0.05, precision=64):
    """The Schwarzschild integrator from supplied starts (lt_schw_trace_probe).
    -> dict(u, w, phi_last (n,), event, steps, full_steps (n,) int32, n_full, h_last: the host's step plan for the call)."""
    uu = np.ascontiguousarray(u0, dtype=np.float64).ravel()
    n = uu.size
    ww = np.ascontiguousarray(np.broadcast_to(np.asarray(w0, dtype=np.float64), (n,)))
    out, oi = np.empty((n, 3)), np.empty((n, 3), dtype=np.int32)
    nf, hl = C.c_uint32(0), C.c_double(0.0)
    _check(load().lt_schw_trace_probe(M, r_obs, phi_max, h_max, _np_ptr(uu), _np_ptr(ww), n, precision, _np_ptr(out), _np_ptr(oi),
                                      C.cast(C.byref(nf), C.c_void_p), C.cast(C.byref(hl), C.c_void_p)))
    return dict(u=out[:, 0].copy(), w=out[:, 1].copy(), phi_last=out[:, 2].copy(), event=oi[:, 0].copy(), steps=oi[:, 1].copy(),
                full_steps=oi[:, 2].copy(), n_full=int(nf.value), h_last=float(hl.value))


def extract_probe(kind, M, a, fin0, fin1, precision=64, integrator=INTEGRATOR_RK4, h_schw=0.05):
    """The array epilogue on final records in the integrate kernels' layout (lt_extract_probe): fin0, fin1 (n,4).
    -> dict(fa (n,) NaN unless escaped, winding (n,) i64, status (n,) i8, evals (n,) u32)."""
    f0 = np.ascontiguousarray(fin0, dtype=np.float64).reshape(-1, 4)
    f1 = np.ascontiguousarray(fin1, dtype=np.float64).reshape(-1, 4)
    n = f0.shape[0]
    if f1.shape[0] != n:
        raise ValueError("fin0 and fin1 differ in length")
    fa, w, st, ev = np.empty(n), np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int8), np.empty(n, dtype=np.uint32)
    _check(load().lt_extract_probe(int(kind), M, a, h_schw, _named(INTEGRATORS, integrator), _np_ptr(f0), _np_ptr(f1), n, precision,
                                   _np_ptr(fa), _np_ptr(w), _np_ptr(st), _np_ptr(ev)))
    return dict(fa=fa, winding=w, status=st, evals=ev)


MATH32_WHICH = {"sincos": 0, "sincos_small": 1, "rcp_pos": 2, "sincos_shift": 3, "pow_minus_tenth": 4}
MATH64_WHICH = {"sincos": 0, "sincos_small": 1, "rcp_pos": 2, "pow_m02": 3, "sincos_f32": 4, "pow_minus_tenth_f32": 5, "sincos_exact": 6}


def math32_probe(which, bits_lo, bits_hi, bases=None):
    """Accuracy sweep of one float32 primitive over every float32 with bit pattern in [bits_lo, bits_hi], compared with
    float64 on the device (lt_math32_probe).  -> dict(compared, and per measure (value, argument bits or None):
    abs_sin, abs_cos, ulp_sin, ulp_cos, abs_angle; differing, first_differing)."""
    out = np.zeros(13, dtype=np.uint64)
    b = None if bases is None else np.ascontiguousarray(bases, dtype=np.float32).ravel()
    _check(load().lt_math32_probe(MATH32_WHICH[which], int(bits_lo), int(bits_hi), _np_ptr(b), 0 if b is None else b.size,
                                  _np_ptr(out)))
    val = out.view(np.float64)
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    res = dict(compared=int(out[0]), differing=int(out[9]), first_differing=None if out[10] == none else int(out[10]))
    for m, name in ((0, "abs_sin"), (1, "abs_cos"), (2, "ulp_sin"), (3, "ulp_cos"), (5, "abs_angle")):
        res[name] = (float(val[1 + 2 * m]), None if out[2 + 2 * m] == none else int(out[2 + 2 * m]))
    return res


def math64_probe(which, x):
    """A float64 primitive on the device, values in, values out (lt_math64_probe) -> (n,2)."""
    xx = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.empty((xx.size, 2))
    _check(load().lt_math64_probe(MATH64_WHICH[which], _np_ptr(xx), xx.size, _np_ptr(out)))
    return out


def set_eq_streak(on):
    """Enable / disable the float32 streak's fixed-quadrant loop for the launches that follow; returns the previous setting."""
    return bool(load().lt_set_eq_streak(int(bool(on))))


def set_unit_streak(on):
    """Enable / disable the unit-step form of the fixed-quadrant loop for the launches that follow; returns the previous setting."""
    return bool(load().lt_set_unit_streak(int(bool(on))))


def set_tail_split(tile_rows):
    """The tail split of the frame path for the frames that follow: -1 automatic, 0 off, n > 0 that many tile rows; returns
    the previous setting."""
    return int(load().lt_set_tail_split(int(tile_rows)))


def tail_split_counts():
    """(split, whole): frames whose integrate launch was split in two / that ran as one launch."""
    a, b = C.c_uint64(), C.c_uint64()
    load().lt_tail_split_counts(C.byref(a), C.byref(b))
    return int(a.value), int(b.value)


def tail_split_plan(tiles_x, tiles_y, strip_x0, strip_x1, hot_y1, slots, request):
    """(split, ty_split, pos_split) of lt_tail_split_plan; needs no device."""
    ty, pos = C.c_int32(), C.c_int64()
    r = load().lt_tail_split_plan(tiles_x, tiles_y, strip_x0, strip_x1, hot_y1, slots, request, C.byref(ty), C.byref(pos))
    if r < 0:
        raise LtraceError(ERR_INVALID_ARG, "lt_tail_split_plan: the arguments describe no frame")
    return bool(r), int(ty.value), int(pos.value)


def sincos_q1_probe(bits_lo, bits_hi):
    """Both float32 sincos forms on every float32 with bit pattern in [bits_lo, bits_hi], compared on the device:
    dict(compared, differing, outside_k1, first_differing_bits, band=(lo, hi))."""
    out = np.zeros(4, dtype=np.uint64)
    band = np.zeros(2, dtype=np.float32)
    _check(load().lt_sincos_q1_probe(int(bits_lo), int(bits_hi), _np_ptr(out), _np_ptr(band)))
    return dict(compared=int(out[0]), differing=int(out[1]), outside_k1=int(out[2]), first_differing_bits=int(out[3]),
                band=(float(band[0]), float(band[1])))


def local_rows(height, row_block, n_parts, part):
    return int(load().lt_local_rows(height, row_block, n_parts, part))


def global_rows(height, row_block, n_parts, part):
    """Global row index of every local row of a partition (host helper for tests / gathers)."""
    n = local_rows(height, row_block, n_parts, part)
    lib = load()
    return np.array([lib.lt_global_row(i, row_block, n_parts, part) for i in range(n)], dtype=np.int64)


# ---- pinned output arrays -----------------------------------------------------------------------------
# lt_render writes a destination that lies in pinned host memory by DMA straight from the device; a pageable
# numpy array costs an extra pass through the library's staging area.  render() therefore hands out arrays
# backed by lt_host_alloc blocks.  Blocks are recycled by size once the last numpy view of them is gone
# (allocating pinned memory costs milliseconds, a 4096^2 frame every call).
import threading
import weakref

_pinned_free = {}     # nbytes -> [address, ...]
_PINNED_POOL_LIMIT = int(os.environ.get("LTRACE_PINNED_POOL_MB", "2048")) << 20
_PINNED_OUTPUTS = os.environ.get("LTRACE_PINNED_OUTPUTS", "1") != "0"    # 0: render() returns ordinary numpy arrays
_pinned_pooled = 0
_pinned_lock = threading.Lock()      # finalizers run on whatever thread drops the last reference


def _pinned_release(addr, nbytes):
    global _pinned_pooled
    if _lib is None:
        return
    with _pinned_lock:
        if _pinned_pooled + nbytes <= _PINNED_POOL_LIMIT:
            _pinned_free.setdefault(nbytes, []).append(addr)
            _pinned_pooled += nbytes
            return
    _lib.lt_host_free(C.c_void_p(addr))


def pinned_empty(shape, dtype, strict=False):
    """numpy array of `shape` / `dtype` in pinned host memory (lt_host_alloc); freed or recycled when the array
    and all its views are gone.  Ordinary memory for empty arrays, with LTRACE_PINNED_OUTPUTS=0, and -- unless
    `strict` -- when the pinned allocation fails (a caller that keeps many frames alive holds that much
    non-swappable memory; lt_render accepts a pageable destination, it is only slower the first time it sees it)."""
    global _pinned_pooled
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    if nbytes == 0 or (not _PINNED_OUTPUTS and not strict):
        return np.empty(shape, dtype=dtype)
    nbytes = (nbytes + 4095) & ~4095
    addr = None
    with _pinned_lock:
        lst = _pinned_free.get(nbytes)
        if lst:
            addr = lst.pop()
            _pinned_pooled -= nbytes
    if addr is None:
        addr = load().lt_host_alloc(nbytes)
        if not addr:
            if strict:
                raise LtraceError(ERR_HIP, load().lt_last_error().decode("utf-8", "replace"))
            return np.empty(shape, dtype=dtype)
    buf = (C.c_ubyte * nbytes).from_address(addr)
    weakref.finalize(buf, _pinned_release, addr, nbytes).atexit = False   # at exit the process frees it
    n = int(np.prod(shape, dtype=np.int64))
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


def _frame_outputs(rows, W, nch, gray, want):
    out = {}
    if "fa" in want:
        out["fa"] = pinned_empty((rows, W), np.float32)
    if "winding" in want:
        out["winding"] = pinned_empty((rows, W), np.uint16)
    if "status" in want:
        out["status"] = pinned_empty((rows, W), np.int8)
    if "steps" in want:
        out["steps"] = pinned_empty((rows, W), np.uint32)
    if "rgb" in want:
        out["rgb"] = pinned_empty((rows, W) if gray else (rows, W, nch), np.float32)
    if "rgba" in want:
        out["rgba"] = pinned_empty((rows, W, 4), np.uint8)
    return out


def _frame_rows(cam, opts):
    if opts.block_owner:
        rows = len(owned_rows(cam.height, opts.row_block or 16, opts._owner_keep, opts.part))
    else:
        rows = local_rows(cam.height, opts.row_block or 16, opts.n_parts or 1, opts.part)
    if rows < 0 or cam.width <= 0:
        raise LtraceError(ERR_INVALID_ARG, f"bad frame {cam.width}x{cam.height} or partition {opts.part}/{opts.n_parts}")
    return rows


def _background(cam, background):
    if background is None:
        return None, 3, False
    bg = np.ascontiguousarray(background, dtype=np.float32)
    if bg.shape[:2] != (cam.height, cam.width):
        raise ValueError("background must have the frame's height and width")
    nch = 1 if bg.ndim == 2 else bg.shape[2]
    if nch not in (1, 3):
        raise ValueError("background must be grayscale or RGB")
    return bg, nch, bg.ndim == 2


def render(cam, metric, opts, background=None, want=("fa", "winding", "status", "steps", "rgb", "rgba")):
    """Host-pointer frame render (lt_render).  Returns dict of numpy arrays (pinned memory) + 'stats'."""
    rows = _frame_rows(cam, opts)
    bg, nch, gray = _background(cam, background)
    out = _frame_outputs(rows, cam.width, nch, gray, want)
    st = Stats()
    _check(load().lt_render(C.byref(cam), C.byref(metric), C.byref(opts), _np_ptr(bg), nch,
                            _np_ptr(out.get("fa")), _np_ptr(out.get("winding")), _np_ptr(out.get("status")),
                            _np_ptr(out.get("steps")), _np_ptr(out.get("rgb")), _np_ptr(out.get("rgba")),
                            C.byref(st)))
    out["stats"] = stats_dict(st.counters, st.prologue_ms, st.integrate_ms, st.epilogue_ms)
    return out


def render_multi(cam, metric, opts, n_gpus, devices=None, background=None,
                 want=("fa", "winding", "status", "steps", "rgb", "rgba")):
    """One frame on `n_gpus` devices of this node from this one process (lt_render_multi): full-frame arrays."""
    bg, nch, gray = _background(cam, background)
    out = _frame_outputs(cam.height, cam.width, nch, gray, want)
    dv = None
    if devices is not None:
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        if dv.size != n_gpus:
            raise ValueError("devices must list one device per partition")
    st = Stats()
    _check(load().lt_render_multi(C.byref(cam), C.byref(metric), C.byref(opts), int(n_gpus), _np_ptr(dv), _np_ptr(bg), nch,
                                  _np_ptr(out.get("fa")), _np_ptr(out.get("winding")), _np_ptr(out.get("status")),
                                  _np_ptr(out.get("steps")), _np_ptr(out.get("rgb")), _np_ptr(out.get("rgba")),
                                  C.byref(st)))
    out["stats"] = stats_dict(st.counters, st.prologue_ms, st.integrate_ms, st.epilogue_ms)
    return out


def build_id():
    return load().lt_build_id().decode()


def pixel_angles(cam, axis_refine_frac=0.07, want_theta=True):
    """(alpha (H,W) f32, theta (H,W) f64 or None, axis_refine_cols (W,) bool) -- lt_pixel_angles."""
    H, W = cam.height, cam.width
    alpha = np.empty((H, W), dtype=np.float32)
    theta = np.empty((H, W), dtype=np.float64) if want_theta else None
    cols = np.zeros(W, dtype=np.uint8)
    _check(load().lt_pixel_angles(C.byref(cam), axis_refine_frac, _np_ptr(alpha), _np_ptr(theta), _np_ptr(cols)))
    return alpha, theta, cols.astype(bool)


def shade(cam, background, fa, winding=None, loop_around=False, want_rgba=False):
    """render_lensed_image twin (lt_shade): returns rgb like the background (and rgba8 if asked)."""
    bg = np.ascontiguousarray(background, dtype=np.float32)
    H, W = bg.shape[:2]
    if (H, W) != (cam.height, cam.width):
        raise ValueError("background and camera sizes differ")
    nch = 1 if bg.ndim == 2 else bg.shape[2]
    fa32 = np.ascontiguousarray(fa, dtype=np.float32)
    wd = None if winding is None else np.ascontiguousarray(winding, dtype=np.uint16)
    if fa32.shape != (H, W) or (wd is not None and wd.shape != (H, W)):
        raise ValueError("lookup shapes must be (H, W)")
    rgb = np.empty_like(bg)
    rgba = np.empty((H, W, 4), dtype=np.uint8) if want_rgba else None
    _check(load().lt_shade(C.byref(cam), int(bool(loop_around)), _np_ptr(bg), nch, _np_ptr(fa32), _np_ptr(wd),
                           _np_ptr(rgb), _np_ptr(rgba)))
    return (rgb, rgba) if want_rgba else rgb


def default_dense_opts(**kw):
    return _default(DenseOpts, "lt_default_dense_opts", {k: v for k, v in kw.items() if v is not None})


def integrate_dense(metric, state0, opts=None):
    """Batched integrate_geodesic (lt_integrate_dense): state0 (n, 8) ->
    (t (n, max_points), y (n, max_points, 8), count (n,), status (n,), nfev (n,)).
    Track i is t[i, :m], y[i, :m].T (= solution.t, solution.y of the reference) with m = min(count[i], max_points)."""
    o = opts or default_dense_opts()
    s0 = np.ascontiguousarray(state0, dtype=np.float64).reshape(-1, 8)
    n, mp = s0.shape[0], int(o.max_points)
    if mp < 2:
        raise LtraceError(ERR_INVALID_ARG, "max_points must be at least 2")
    t = np.empty((n, mp), dtype=np.float64)
    y = np.empty((n, mp, 8), dtype=np.float64)
    count = np.zeros(n, dtype=np.int32)
    status = np.zeros(n, dtype=np.int8)
    nfev = np.zeros(n, dtype=np.int32)
    _check(load().lt_integrate_dense(C.byref(metric), C.byref(o), _np_ptr(s0), n, _np_ptr(t), _np_ptr(y),
                                     _np_ptr(count), _np_ptr(status), _np_ptr(nfev)))
    return t, y, count, status, nfev


def integrate_dense_dev(metric, opts, d_state0, n, d_t, d_y, d_count, d_status, d_nfev):
    """Device-pointer form (integers, e.g. tensor.data_ptr()); asynchronous on opts.stream."""
    _check(load().lt_integrate_dense_dev(C.byref(metric), C.byref(opts), C.c_void_p(d_state0), n, C.c_void_p(d_t),
                                         C.c_void_p(d_y), C.c_void_p(d_count), C.c_void_p(d_status),
                                         C.c_void_p(d_nfev)))


def dense_predict_lengths(metric, state0, opts=None):
    """Predicted step attempts per track (uint16, clamped to 2047): what the length-binned dense launch sorts by."""
    o = opts or default_dense_opts()
    s0 = np.ascontiguousarray(state0, dtype=np.float64).reshape(-1, 8)
    key = np.zeros(s0.shape[0], dtype=np.uint16)
    _check(load().lt_dense_predict_lengths(C.byref(metric), C.byref(o), _np_ptr(s0), s0.shape[0], _np_ptr(key)))
    return key


def rhs8_probe(metric, states):
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 8)
    out = np.empty_like(st)
    _check(load().lt_rhs8_probe(C.byref(metric), _np_ptr(st), st.shape[0], _np_ptr(out)))
    return out


def stats_dict(counters, prologue_ms=0.0, integrate_ms=0.0, epilogue_ms=0.0):
    c = [int(x) for x in counters]
    clk = c[STAT_CLK_CYCLES] / c[STAT_CLK_TICKS] * 100.0 if c[STAT_CLK_TICKS] else 0.0   # ticks are 100 MHz
    return dict(rays=c[STAT_RAYS], steps=c[STAT_STEPS], rhs_evals=c[STAT_RHS_EVALS], escaped=c[STAT_ESCAPED],
                captured=c[STAT_CAPTURED], invalid=c[STAT_INVALID], wave_iters=c[STAT_WAVE_ITERS],
                waves=c[STAT_WAVES], clock_mhz=clk, bg_tiles_lds=c[STAT_BG_TILES_LDS],
                bg_tiles_global=c[STAT_BG_TILES_GLOBAL], eq_iters=c[STAT_EQ_ITERS],
                prologue_ms=prologue_ms, integrate_ms=integrate_ms, epilogue_ms=epilogue_ms)


def _disk_stats(st):
    """stats_dict of a call's Stats with the disk's counters: 'disk' (rays with a hit) and 'disk_hits' (all hits)."""
    d = stats_dict(st.counters, st.prologue_ms, st.integrate_ms, st.epilogue_ms)
    d["disk"] = int(st.counters[STAT_DISK])
    d["disk_hits"] = int(st.counters[STAT_DISK_HITS])
    return d


def render_dev(cam, metric, opts, d_bg=0, bg_channels=3, d_fa=0, d_w=0, d_status=0, d_steps=0, d_rgb=0, d_rgba=0,
               d_stats=0):
    """Device-pointer frame render (lt_render_dev); pointers are integers (tensor.data_ptr()), 0 = NULL.
    Asynchronous on opts.stream."""
    _check(load().lt_render_dev(C.byref(cam), C.byref(metric), C.byref(opts), _p(d_bg), bg_channels, _p(d_fa), _p(d_w),
                                _p(d_status), _p(d_steps), _p(d_rgb), _p(d_rgba), _p(d_stats)))


def scatter_rows_dev(d_part, d_full, height, width, elem_bytes, row_block, n_parts, part, stream=0):
    _check(load().lt_scatter_rows_dev(C.c_void_p(d_part), C.c_void_p(d_full), height, width, elem_bytes, row_block,
                                      n_parts, part, _p(stream)))


def scatter_rows_indexed_dev(d_rows, d_full, d_row_index, n_rows, height, row_bytes, stream=0):
    """Source row i (device, row_bytes each) -> row d_row_index[i] (device int64) of the full frame; one launch."""
    _check(load().lt_scatter_rows_indexed_dev(C.c_void_p(d_rows), C.c_void_p(d_full), C.c_void_p(d_row_index), n_rows, height,
                                              row_bytes, _p(stream)))


def timing_collect():
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    n = C.c_int32()
    _check(load().lt_timing_collect(C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
    return dict(prologue_ms=a.value, integrate_ms=b.value, epilogue_ms=c.value, calls=n.value)


def ic_reuse_counts():
    """(hits, misses): frames that reused the ray records of their stream / that ran the camera prologue."""
    h, m = C.c_uint64(), C.c_uint64()
    load().lt_ic_reuse_counts(C.byref(h), C.byref(m))
    return int(h.value), int(m.value)


def release_stream(stream_ptr):
    """Free the library's buffers of (current device, stream) -- before the stream is destroyed."""
    _check(load().lt_release_stream(_p(stream_ptr)))


def shutdown():
    if _lib is not None:
        _lib.lt_shutdown()
        with _pinned_lock:
            blocks = [addr for lst in _pinned_free.values() for addr in lst]
            _pinned_free.clear()
            globals()['_pinned_pooled'] = 0
        for addr in blocks:
            _lib.lt_host_free(C.c_void_p(addr))


# ---- thin accretion disk (lt_render_disk) ---------------------------------------------------------------------------
def default_disk(**kw):
    """lt_disk with the library's defaults (r_in = ISCO, r_out = 20, q = 3, exposure = 1); keywords override.
    r_in=None means the ISCO."""
    return _default(Disk, "lt_default_disk", {k: 0.0 if k == "r_in" and v is None else v for k, v in kw.items()})


def kerr_isco(M, a):
    """ISCO radius of the circular equatorial orbit in +phi (lt_kerr_isco; host only)."""
    return float(load().lt_kerr_isco(float(M), float(a)))


def render_disk(cam, metric, opts, disk, background=None,
                want=("fa", "winding", "status", "steps", "rgb", "rgba", "disk")):
    """Host-pointer frame render with the accretion disk (lt_render_disk).  As render(), plus 'disk':
    (rows, W, 3) float32 (r_hit, phi_hit, g), NaN off the disk; stats gain 'disk' (rays that ended on it)."""
    rows = _frame_rows(cam, opts)
    bg, nch, gray = _background(cam, background)
    out = _frame_outputs(rows, cam.width, nch, gray, want)
    if "disk" in want:
        out["disk"] = pinned_empty((rows, cam.width, 3), np.float32)
    st = Stats()
    _check(load().lt_render_disk(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), _np_ptr(bg), nch,
                                 _np_ptr(out.get("fa")), _np_ptr(out.get("winding")), _np_ptr(out.get("status")),
                                 _np_ptr(out.get("steps")), _np_ptr(out.get("disk")), _np_ptr(out.get("rgb")),
                                 _np_ptr(out.get("rgba")), C.byref(st)))
    out["stats"] = stats_dict(st.counters, st.prologue_ms, st.integrate_ms, st.epilogue_ms)
    out["stats"]["disk"] = int(st.counters[STAT_DISK])
    return out


def render_disk_dev(cam, metric, opts, disk, d_bg=0, bg_channels=3, d_fa=0, d_w=0, d_status=0, d_steps=0, d_disk=0,
                    d_rgb=0, d_rgba=0, d_stats=0):
    """Device-pointer form of render_disk (lt_render_disk_dev); pointers are integers, 0 = NULL.  Asynchronous."""
    _check(load().lt_render_disk_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), _p(d_bg), bg_channels,
                                     _p(d_fa), _p(d_w), _p(d_status), _p(d_steps), _p(d_disk), _p(d_rgb), _p(d_rgba), _p(d_stats)))


def trace_batch_kerr_disk(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, disk, axis_refines=None,
                          integrator=INTEGRATOR_RK4, precision=32):
    """Batch twin with the accretion disk (lt_trace_batch_kerr_disk) ->
    dict(fa (n,) f64, winding (n,) i64, status (n,) i8, disk (n, 3) f64 (r_hit, phi_hit, g), rhs_evals (n,) u32)."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    integrator = _named(INTEGRATORS, integrator)
    out = dict(fa=np.empty(n), winding=np.empty(n, dtype=np.int64), status=np.empty(n, dtype=np.int8),
               disk=np.empty((n, 3)), rhs_evals=np.empty(n, dtype=np.uint32))
    _check(load().lt_trace_batch_kerr_disk(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max, _np_ptr(ar),
                                           integrator, precision, C.byref(disk), n, _np_ptr(out["fa"]),
                                           _np_ptr(out["winding"]), _np_ptr(out["status"]), _np_ptr(out["disk"]),
                                           _np_ptr(out["rhs_evals"])))
    return out


# ---- optically thin disk: every image (lt_render_disk_images) ------------------------------------------------------
def render_disk_images(cam, metric, opts, disk, max_images=3, background=None,
                       want=("fa", "winding", "status", "steps", "rgb", "rgba", "images", "n_hits")):
    """Host-pointer frame render with the optically thin disk (lt_render_disk_images).  As render(), plus 'images':
    (rows, W, max_images, 3) float32 (r_hit, phi_hit, g) of the first max_images hits along the ray, NaN in unused
    slots, and 'n_hits': (rows, W) uint8, every hit of the ray (saturating at 255); stats gain 'disk' (rays with a hit)
    and 'disk_hits' (all hits).  fa / winding / status / steps are render()'s."""
    rows = _frame_rows(cam, opts)
    bg, nch, gray = _background(cam, background)
    out = _frame_outputs(rows, cam.width, nch, gray, want)
    if "images" in want:
        out["images"] = pinned_empty((rows, cam.width, int(max_images), 3), np.float32)
    if "n_hits" in want:
        out["n_hits"] = pinned_empty((rows, cam.width), np.uint8)
    st = Stats()
    _check(load().lt_render_disk_images(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), int(max_images),
                                        _np_ptr(bg), nch, _np_ptr(out.get("fa")), _np_ptr(out.get("winding")),
                                        _np_ptr(out.get("status")), _np_ptr(out.get("steps")), _np_ptr(out.get("images")),
                                        _np_ptr(out.get("n_hits")), _np_ptr(out.get("rgb")), _np_ptr(out.get("rgba")),
                                        C.byref(st)))
    out["stats"] = _disk_stats(st)
    return out


def render_disk_images_dev(cam, metric, opts, disk, max_images=3, d_bg=0, bg_channels=3, d_fa=0, d_w=0, d_status=0,
                           d_steps=0, d_images=0, d_n_hits=0, d_rgb=0, d_rgba=0, d_stats=0):
    """Device-pointer form of render_disk_images (lt_render_disk_images_dev); pointers are integers, 0 = NULL.
    Asynchronous."""
    _check(load().lt_render_disk_images_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), int(max_images),
                                            _p(d_bg), bg_channels, _p(d_fa), _p(d_w), _p(d_status), _p(d_steps), _p(d_images),
                                            _p(d_n_hits), _p(d_rgb), _p(d_rgba), _p(d_stats)))


def trace_batch_kerr_disk_images(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, disk, max_images=3,
                                 axis_refines=None, integrator=INTEGRATOR_RK4, precision=32):
    """Batch twin with the optically thin disk (lt_trace_batch_kerr_disk_images) -> dict(fa (n,) f64, winding (n,) i64,
    status (n,) i8 (trace_batch_kerr's), images (n, max_images, 3) f64 (r_hit, phi_hit, g), NaN in unused slots,
    n_hits (n,) i32, rhs_evals (n,) u32)."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    integrator = _named(INTEGRATORS, integrator)
    m = int(max_images)
    out = dict(fa=np.empty(n), winding=np.empty(n, dtype=np.int64), status=np.empty(n, dtype=np.int8),
               images=np.empty((n, max(m, 0), 3)), n_hits=np.empty(n, dtype=np.int32),
               rhs_evals=np.empty(n, dtype=np.uint32))
    _check(load().lt_trace_batch_kerr_disk_images(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max,
                                                  _np_ptr(ar), integrator, precision, C.byref(disk), m, n,
                                                  _np_ptr(out["fa"]), _np_ptr(out["winding"]), _np_ptr(out["status"]),
                                                  _np_ptr(out["images"]), _np_ptr(out["n_hits"]),
                                                  _np_ptr(out["rhs_evals"])))
    return out


# ---- hit times and the orbiting hot spot (lt_trace_disk_hits, lt_shade_hotspot, lt_hotspot_lightcurve) ------------
def trace_disk_hits(cam, metric, opts, disk, max_images=3, want=("fa", "winding", "status", "steps", "hits", "n_hits")):
    """Host-pointer timed trace of the optically thin disk (lt_trace_disk_hits): render_disk_images() without the colour,
    with 'hits' (rows, W, max_images, 4) float32 (r_hit, phi_hit, g, light-travel time to the camera), NaN in unused
    slots, in place of 'images'."""
    rows = _frame_rows(cam, opts)
    out = _frame_outputs(rows, cam.width, 3, False, [k for k in want if k in ("fa", "winding", "status", "steps")])
    if "hits" in want:
        out["hits"] = pinned_empty((rows, cam.width, int(max_images), 4), np.float32)
    if "n_hits" in want:
        out["n_hits"] = pinned_empty((rows, cam.width), np.uint8)
    st = Stats()
    _check(load().lt_trace_disk_hits(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), int(max_images),
                                     _np_ptr(out.get("fa")), _np_ptr(out.get("winding")), _np_ptr(out.get("status")),
                                     _np_ptr(out.get("steps")), _np_ptr(out.get("hits")), _np_ptr(out.get("n_hits")),
                                     C.byref(st)))
    out["stats"] = _disk_stats(st)
    return out


def trace_disk_hits_dev(cam, metric, opts, disk, max_images=3, d_fa=0, d_w=0, d_status=0, d_steps=0, d_hits=0, d_n_hits=0,
                        d_stats=0):
    """Device-pointer form of trace_disk_hits (lt_trace_disk_hits_dev); pointers are integers, 0 = NULL.  Asynchronous."""
    _check(load().lt_trace_disk_hits_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), int(max_images),
                                         _p(d_fa), _p(d_w), _p(d_status), _p(d_steps), _p(d_hits), _p(d_n_hits), _p(d_stats)))


def trace_batch_kerr_disk_hits(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, disk, max_images=3,
                               axis_refines=None, integrator=INTEGRATOR_RK4, precision=32):
    """Batch twin of the timed trace (lt_trace_batch_kerr_disk_hits): trace_batch_kerr_disk_images() with 'hits'
    (n, max_images, 4) f64 (r_hit, phi_hit, g, light-travel time) in place of 'images'."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    integrator = _named(INTEGRATORS, integrator)
    m = int(max_images)
    out = dict(fa=np.empty(n), winding=np.empty(n, dtype=np.int64), status=np.empty(n, dtype=np.int8),
               hits=np.empty((n, max(m, 0), 4)), n_hits=np.empty(n, dtype=np.int32),
               rhs_evals=np.empty(n, dtype=np.uint32))
    _check(load().lt_trace_batch_kerr_disk_hits(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max,
                                                _np_ptr(ar), integrator, precision, C.byref(disk), m, n,
                                                _np_ptr(out["fa"]), _np_ptr(out["winding"]), _np_ptr(out["status"]),
                                                _np_ptr(out["hits"]), _np_ptr(out["n_hits"]), _np_ptr(out["rhs_evals"])))
    return out


def step_time_probe(metric, p_phi, y0, y1, h, tau=1.0, precision=64):
    """The device's own step rule (lt_step_time_probe) on n steps: y0, y1 (n, 4) (r, theta, p_r, p_theta); p_phi, h, tau
    scalars or (n,).  -> (n,) float64."""
    y0 = np.ascontiguousarray(y0, dtype=np.float64).reshape(-1, 4)
    y1 = np.ascontiguousarray(y1, dtype=np.float64).reshape(-1, 4)
    n = y0.shape[0]
    pp, hh, tt = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))) for x in (p_phi, h, tau))
    out = np.empty(n)
    _check(load().lt_step_time_probe(C.byref(metric), _np_ptr(pp), _np_ptr(y0), _np_ptr(y1), _np_ptr(hh), _np_ptr(tt), n,
                                     int(precision), _np_ptr(out)))
    return out


def time_rates_probe(metric, p_phi, y, precision=64):
    """The rates a lane carries (lt_time_rates_probe) at n states y (n, 4) (r, theta, p_r, p_theta) -> (n, 3) float64
    (t', r', theta') holding the values of the precision computed in."""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1, 4)
    n = y.shape[0]
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p_phi, dtype=np.float64), (n,)))
    out = np.empty((n, 3))
    _check(load().lt_time_rates_probe(C.byref(metric), _np_ptr(pp), _np_ptr(y), n, int(precision), _np_ptr(out)))
    return out


EV_DISK = 5                                                              # the event of a row that hit the disk


def disk_crossing_probe(metric, y0, y1, p_phi, h, t_end=1.0, r_in=0.0, r_out=20.0, precision=64):
    """The device's crossing search (lt_disk_crossing_probe) on n steps: y0, y1 (n,5); p_phi, h, t_end scalars or (n,).
    -> dict(found (n,) bool, hit (n,5), tau (n,)): float64 holding the values of the precision computed in."""
    y0 = np.ascontiguousarray(y0, dtype=np.float64).reshape(-1, 5)
    y1 = np.ascontiguousarray(y1, dtype=np.float64).reshape(-1, 5)
    n = y0.shape[0]
    pp, hh, tt = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))) for x in (p_phi, h, t_end))
    found, hit, tau = np.empty(n, dtype=np.uint8), np.empty((n, 5)), np.empty(n)
    _check(load().lt_disk_crossing_probe(C.byref(metric), r_in, r_out, _np_ptr(y0), _np_ptr(y1), _np_ptr(pp), _np_ptr(hh), _np_ptr(tt),
                                         n, int(precision), _np_ptr(found), _np_ptr(hit), _np_ptr(tau)))
    return dict(found=found.astype(bool), hit=hit, tau=tau)


def disk_advance_probe(metric, states, p_phi, integrator=INTEGRATOR_RK4, precision=64, lam=0.0, h=0.0, refine=None, steps=None,
                       act=True, r_in=0.0, r_out=20.0, r_obs=50.0, lambda_max=5000.0, h_max=1.0):
    """One iteration of an integrator with the disk test behind it per state (lt_disk_advance_probe); rows 64 b ... 64 b + 63
    share a wavefront.  h: RK4's h_retry, DP45's step size.  -> dict(event, steps (n,) int32, is_hit (n,) bool, state (n,5),
    lam, h (n,), hit (n,5), on_y1 (n,5), on_h, on_tau (n,))."""
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    n = st.shape[0]
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p_phi, dtype=np.float64), (n,)))
    rf = np.zeros(n, dtype=np.uint8) if refine is None else np.ascontiguousarray(np.broadcast_to(np.asarray(refine), (n,))).astype(np.uint8)
    ss = np.zeros(n, dtype=np.uint32) if steps is None else np.ascontiguousarray(np.broadcast_to(np.asarray(steps), (n,))).astype(np.uint32)
    ac = np.ascontiguousarray(np.broadcast_to(np.asarray(act), (n,))).astype(np.uint8)
    aux = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in (lam, h)], axis=1))
    out, oa, oi, oh, oo = np.empty_like(st), np.empty((n, 2)), np.empty((n, 3), dtype=np.int32), np.empty((n, 5)), np.empty((n, 7))
    _check(load().lt_disk_advance_probe(C.byref(metric), r_obs, lambda_max, h_max, r_in, r_out, int(integrator), int(precision),
                                        _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(aux), _np_ptr(ss), _np_ptr(ac), n, _np_ptr(out),
                                        _np_ptr(oa), _np_ptr(oi), _np_ptr(oh), _np_ptr(oo)))
    return dict(event=oi[:, 0].copy(), steps=oi[:, 1].copy(), is_hit=oi[:, 2] != 0, state=out, lam=oa[:, 0].copy(), h=oa[:, 1].copy(),
                hit=oh, on_y1=oo[:, :5].copy(), on_h=oo[:, 5].copy(), on_tau=oo[:, 6].copy())


TIMED_CARRY = ("state", "lam", "h", "steps", "k1", "sc", "t_hi", "t_lo", "rate", "have", "n")  # what a lane hands to its next iteration


def disk_timed_advance_probe(metric, states, p_phi, integrator=INTEGRATOR_RK4, precision=64, pol=False, lam=0.0, h=0.0, refine=None,
                             steps=None, act=True, k1=None, sc=None, t_hi=0.0, t_lo=0.0, rate=None, have=False, n=0, max_images=2,
                             iters=1, trace=False, r_in=0.0, r_out=20.0, r_obs=50.0, lambda_max=5000.0, h_max=1.0):
    """Up to `iters` iterations of the timed (pol: the polarized) trace's lane per state (lt_disk_timed_advance_probe); rows
    64 b ... 64 b + 63 share a wavefront.  h: RK4's h_retry, DP45's step size; k1, sc: DP45's carried derivative and [sin, cos]
    (None: from the state); t_hi, t_lo, rate (rows,3), have, n: the lane's carried time, rates and hit count.  A result's
    TIMED_CARRY entries, passed back as keywords, resume the lane exactly.
    -> dict(event, steps, iters (rows,) int32, state (rows,5), lam, h (rows,), k1 (rows,5), sc (rows,2), t_hi, t_lo (rows,), rate
    (rows,3), have (rows,) bool, n (rows,) int32, img (max_images, rows, 2), tim (max_images, rows), mom (max_images, rows, 2),
    trace (iters, rows, 7) or None: r, theta, p_r, p_theta, h counted, dt added, hits counted after each iteration)."""
    st = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 5)
    m = st.shape[0]
    col = lambda x, dt=np.float64: np.ascontiguousarray(np.broadcast_to(np.asarray(x), (m,))).astype(dt)
    pp = col(p_phi)
    rf = np.zeros(m, dtype=np.uint8) if refine is None else col(refine, np.uint8)
    ss = np.zeros(m, dtype=np.uint32) if steps is None else col(steps, np.uint32)
    ac = col(act, np.uint8)
    aux = np.ascontiguousarray(np.stack([col(lam), col(h)], axis=1))
    kk = None if k1 is None else np.ascontiguousarray(k1, dtype=np.float64).reshape(m, 5)
    sc0 = None if sc is None else np.ascontiguousarray(sc, dtype=np.float64).reshape(m, 2)
    rt = np.zeros((m, 3)) if rate is None else np.asarray(rate, dtype=np.float64).reshape(m, 3)
    lane = np.ascontiguousarray(np.concatenate([np.stack([col(t_hi), col(t_lo)], axis=1), rt], axis=1))
    lane_int = np.ascontiguousarray(np.stack([col(have, np.int32), col(n, np.int32)], axis=1))
    mi, it = int(max_images), int(iters)
    out, oa, ok, osc = np.empty_like(st), np.empty((m, 2)), np.empty((m, 5)), np.empty((m, 2))
    oi, ol, oli = np.empty((m, 3), dtype=np.int32), np.empty((m, 5)), np.empty((m, 2), dtype=np.int32)
    img, tim, mom = np.empty((max(mi, 0), m, 2)), np.empty((max(mi, 0), m)), np.empty((max(mi, 0), m, 2))
    tr = np.empty((max(it, 0), m, 7)) if trace else None
    _check(load().lt_disk_timed_advance_probe(C.byref(metric), r_obs, lambda_max, h_max, r_in, r_out, int(integrator), int(precision),
                                              int(bool(pol)), _np_ptr(st), _np_ptr(pp), _np_ptr(rf), _np_ptr(aux), _np_ptr(ss), _np_ptr(ac),
                                              _np_ptr(kk), _np_ptr(sc0), _np_ptr(lane), _np_ptr(lane_int), m, mi, it, _np_ptr(out),
                                              _np_ptr(oa), _np_ptr(ok), _np_ptr(osc), _np_ptr(oi), _np_ptr(ol), _np_ptr(oli), _np_ptr(img),
                                              _np_ptr(tim), _np_ptr(mom), _np_ptr(tr)))
    return dict(event=oi[:, 0].copy(), steps=oi[:, 1].copy(), iters=oi[:, 2].copy(), state=out, lam=oa[:, 0].copy(), h=oa[:, 1].copy(),
                k1=ok, sc=osc, t_hi=ol[:, 0].copy(), t_lo=ol[:, 1].copy(), rate=ol[:, 2:].copy(), have=oli[:, 0] != 0, n=oli[:, 1].copy(),
                img=img, tim=tim, mom=mom, trace=tr)


def disk_shade_probe(metric, r, phi=0.0, xi=0.0, g=np.nan, r_in=0.0, q=3.0, exposure=1.0):
    """The closed forms of a disk hit on the device (lt_disk_shade_probe): r (n,), phi, xi, g scalars or (n,) (g NaN: the
    emission and the colour take the device's own g).  -> dict(g, phi (n,), emission (n,3) float64, half_orbits (n,) int64,
    shade1 (n,), shade3 (n,3) float32)."""
    r = np.asarray(r, dtype=np.float64).ravel()
    n = r.size
    inp = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in (r, phi, xi, g)], axis=1))
    o64, oh, o32 = np.empty((n, 5)), np.empty(n, dtype=np.int64), np.empty((n, 4), dtype=np.float32)
    _check(load().lt_disk_shade_probe(C.byref(metric), r_in, q, exposure, _np_ptr(inp), n, _np_ptr(o64), _np_ptr(oh), _np_ptr(o32)))
    return dict(g=o64[:, 0].copy(), phi=o64[:, 1].copy(), emission=o64[:, 2:].copy(), half_orbits=oh, shade1=o32[:, 0].copy(),
                shade3=o32[:, 1:].copy())


def default_hotspot(**kw):
    """lt_hotspot with the library's defaults (r_spot 8, phi0 0, sigma 1, exposure 1, with_disk 1); keywords override."""
    return _default(HotSpot, "lt_default_hotspot", kw)


def _hit_arrays(hits, n_hits):
    hits = np.ascontiguousarray(hits, dtype=np.float32)
    if hits.ndim != 4 or hits.shape[3] != 4:
        raise ValueError("hits must be (rows, W, max_images, 4)")
    nh = None
    if n_hits is not None:
        nh = np.ascontiguousarray(n_hits, dtype=np.uint8)
        if nh.shape != hits.shape[:2]:
            raise ValueError("n_hits must be (rows, W)")
    return hits, nh


def _shade_frame(fn, hits, nh, R, W, mid, base, channels, want):
    """The host-pointer call fn(hits, n_hits, R, W, *mid, base, channels, rgb, rgba) of a re-shade whose base has the
    records' rows and width -> dict(rgb, rgba) of (R, W) pixels."""
    b = None
    nch = 3 if channels is None else int(channels)
    if base is not None:
        b = np.ascontiguousarray(base, dtype=np.float32)
        if b.shape[:2] != hits.shape[:2]:
            raise ValueError("base must have the records' rows and width")
        nch = 1 if b.ndim == 2 else b.shape[2]
    gray = nch == 1 and (b is None or b.ndim == 2)
    out = {}
    if "rgb" in want:
        out["rgb"] = np.empty((R, W) if gray else (R, W, nch), dtype=np.float32)
    if "rgba" in want:
        out["rgba"] = np.empty((R, W, 4), dtype=np.uint8)
    _check(fn(_np_ptr(hits), _np_ptr(nh), R, W, *mid, _np_ptr(b), nch, _np_ptr(out.get("rgb")), _np_ptr(out.get("rgba"))))
    return out


def shade_hotspot(hits, n_hits, metric, disk, spot, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The frame at observer time t_obs from stored hits (lt_shade_hotspot).  base: (rows, W) or (rows, W, 3) float32
    or None (black; `channels` 1 or 3 then picks the output's shape, default 3).  -> dict(rgb, rgba)."""
    hits, nh = _hit_arrays(hits, n_hits)
    R, W, m = hits.shape[:3]
    return _shade_frame(load().lt_shade_hotspot, hits, nh, R, W, (m, C.byref(metric), C.byref(disk), C.byref(spot), float(t_obs)),
                        base, channels, want)


def shade_hotspot_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spot, t_obs, d_base=0, channels=3, d_rgb=0,
                      d_rgba=0):
    """Device-pointer form of shade_hotspot (lt_shade_hotspot_dev); enqueues on the default stream."""
    _check(load().lt_shade_hotspot_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                       C.byref(spot), float(t_obs), _p(d_base), channels, _p(d_rgb), _p(d_rgba)))


def hotspot_lightcurve(hits, n_hits, metric, disk, spot, t_start, dt, n_times):
    """The spot's light curve (lt_hotspot_lightcurve) -> (n_times, 3) float64: per time the sums of e, e ix, e iy."""
    hits, nh = _hit_arrays(hits, n_hits)
    R, W, m = hits.shape[:3]
    out = np.empty((int(n_times), 3))
    _check(load().lt_hotspot_lightcurve(_np_ptr(hits), _np_ptr(nh), R, W, m, C.byref(metric), C.byref(disk), C.byref(spot),
                                        float(t_start), float(dt), int(n_times), _np_ptr(out)))
    return out


def hotspot_lightcurve_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spot, t_start, dt, n_times, d_out):
    """Device-pointer form of hotspot_lightcurve (lt_hotspot_lightcurve_dev); enqueues on the default stream."""
    _check(load().lt_hotspot_lightcurve_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric),
                                            C.byref(disk), C.byref(spot), float(t_start), float(dt), int(n_times), _p(d_out)))


# ---- linear polarization (lt_trace_disk_pol, lt_shade_stokes, lt_hotspot_lightcurve_stokes) ------------------------
def default_bfield(**kw):
    """lt_bfield with the library's defaults ((b_r, b_phi, b_z) = (0, 0, 1), pol_frac 0.7); keywords override."""
    return _default(BField, "lt_default_bfield", kw)


def trace_disk_pol(cam, metric, opts, disk, field, max_images=3,
                   want=("fa", "winding", "status", "steps", "hits", "n_hits", "pol")):
    """Host-pointer polarized trace (lt_trace_disk_pol): trace_disk_hits() plus 'pol' (rows, W, max_images, 4) float32
    (q, u, sin zeta, mu), NaN in unused slots."""
    rows = _frame_rows(cam, opts)
    out = _frame_outputs(rows, cam.width, 3, False, [k for k in want if k in ("fa", "winding", "status", "steps")])
    for name in ("hits", "pol"):
        if name in want:
            out[name] = pinned_empty((rows, cam.width, int(max_images), 4), np.float32)
    if "n_hits" in want:
        out["n_hits"] = pinned_empty((rows, cam.width), np.uint8)
    st = Stats()
    _check(load().lt_trace_disk_pol(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), C.byref(field), int(max_images),
                                    _np_ptr(out.get("fa")), _np_ptr(out.get("winding")), _np_ptr(out.get("status")),
                                    _np_ptr(out.get("steps")), _np_ptr(out.get("hits")), _np_ptr(out.get("n_hits")),
                                    _np_ptr(out.get("pol")), C.byref(st)))
    out["stats"] = _disk_stats(st)
    return out


def trace_disk_pol_dev(cam, metric, opts, disk, field, max_images=3, d_fa=0, d_w=0, d_status=0, d_steps=0, d_hits=0, d_n_hits=0,
                       d_pol=0, d_stats=0):
    """Device-pointer form of trace_disk_pol (lt_trace_disk_pol_dev); pointers are integers, 0 = NULL.  Asynchronous."""
    _check(load().lt_trace_disk_pol_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(disk), C.byref(field), int(max_images),
                                        _p(d_fa), _p(d_w), _p(d_status), _p(d_steps), _p(d_hits), _p(d_n_hits), _p(d_pol),
                                        _p(d_stats)))


def trace_batch_kerr_disk_pol(M, a, r_obs, alphas, thetas, theta_obs, lambda_max, disk, field, max_images=3,
                              axis_refines=None, integrator=INTEGRATOR_RK4, precision=32):
    """Batch twin of the polarized trace (lt_trace_batch_kerr_disk_pol): trace_batch_kerr_disk_hits() plus 'pol'
    (n, max_images, 4) f64 (q, u, sin zeta, mu)."""
    al, th, ar, n = _ray_inputs(alphas, thetas, axis_refines)
    integrator = _named(INTEGRATORS, integrator)
    m = int(max_images)
    out = dict(fa=np.empty(n), winding=np.empty(n, dtype=np.int64), status=np.empty(n, dtype=np.int8),
               hits=np.empty((n, max(m, 0), 4)), n_hits=np.empty(n, dtype=np.int32), pol=np.empty((n, max(m, 0), 4)),
               rhs_evals=np.empty(n, dtype=np.uint32))
    _check(load().lt_trace_batch_kerr_disk_pol(M, a, r_obs, _np_ptr(al), _np_ptr(th), theta_obs, lambda_max, _np_ptr(ar),
                                               integrator, precision, C.byref(disk), C.byref(field), m, n, _np_ptr(out["fa"]),
                                               _np_ptr(out["winding"]), _np_ptr(out["status"]), _np_ptr(out["hits"]),
                                               _np_ptr(out["n_hits"]), _np_ptr(out["pol"]), _np_ptr(out["rhs_evals"])))
    return out


def polarization_probe(metric, r_obs, theta_obs, p_phi, hit, cam, field):
    """The device's own polarization rule (lt_polarization_probe) on n records: hit (n, 3) (r, p_r, p_theta at the hit),
    cam (n, 2) (p_r, p_theta at the camera), p_phi scalar or (n,).  -> (n, 4) float64 (q, u, sin zeta, mu)."""
    hit = np.ascontiguousarray(hit, dtype=np.float64).reshape(-1, 3)
    cam = np.ascontiguousarray(cam, dtype=np.float64).reshape(-1, 2)
    n = hit.shape[0]
    if cam.shape[0] != n:
        raise ValueError("hit and cam differ in length")
    pp = np.ascontiguousarray(np.broadcast_to(np.asarray(p_phi, dtype=np.float64), (n,)))
    out = np.empty((n, 4))
    _check(load().lt_polarization_probe(C.byref(metric), float(r_obs), float(theta_obs), C.byref(field), _np_ptr(pp), _np_ptr(hit),
                                        _np_ptr(cam), n, _np_ptr(out)))
    return out


def _pol_array(pol, hits):
    pol = np.ascontiguousarray(pol, dtype=np.float32)
    if pol.shape != hits.shape:
        raise ValueError("pol must have the hits' shape (rows, W, max_images, 4)")
    return pol


def shade_stokes(hits, n_hits, pol, metric, disk, spot, field, t_obs):
    """The Stokes frame at observer time t_obs from stored records (lt_shade_stokes) -> (rows, W, 3) float32 (I, Q, U)."""
    hits, nh = _hit_arrays(hits, n_hits)
    pol = _pol_array(pol, hits)
    R, W, m = hits.shape[:3]
    out = np.empty((R, W, 3), dtype=np.float32)
    _check(load().lt_shade_stokes(_np_ptr(hits), _np_ptr(nh), _np_ptr(pol), R, W, m, C.byref(metric), C.byref(disk), C.byref(spot),
                                  C.byref(field), float(t_obs), _np_ptr(out)))
    return out


def shade_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, spot, field, t_obs, d_iqu):
    """Device-pointer form of shade_stokes (lt_shade_stokes_dev); enqueues on the default stream."""
    _check(load().lt_shade_stokes_dev(_p(d_hits), _p(d_n_hits), _p(d_pol), rows, width, max_images, C.byref(metric), C.byref(disk),
                                      C.byref(spot), C.byref(field), float(t_obs), _p(d_iqu)))


def hotspot_lightcurve_stokes(hits, n_hits, pol, metric, disk, spot, field, t_start, dt, n_times):
    """The spot's Stokes light curve (lt_hotspot_lightcurve_stokes) -> (n_times, 3) float64: per time the sums of I, Q, U."""
    hits, nh = _hit_arrays(hits, n_hits)
    pol = _pol_array(pol, hits)
    R, W, m = hits.shape[:3]
    out = np.empty((int(n_times), 3))
    _check(load().lt_hotspot_lightcurve_stokes(_np_ptr(hits), _np_ptr(nh), _np_ptr(pol), R, W, m, C.byref(metric), C.byref(disk),
                                               C.byref(spot), C.byref(field), float(t_start), float(dt), int(n_times), _np_ptr(out)))
    return out


def hotspot_lightcurve_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, spot, field, t_start, dt, n_times,
                                  d_out):
    """Device-pointer form of hotspot_lightcurve_stokes (lt_hotspot_lightcurve_stokes_dev); enqueues on the default stream."""
    _check(load().lt_hotspot_lightcurve_stokes_dev(_p(d_hits), _p(d_n_hits), _p(d_pol), rows, width, max_images, C.byref(metric),
                                                   C.byref(disk), C.byref(spot), C.byref(field), float(t_start), float(dt),
                                                   int(n_times), _p(d_out)))


# ---- supersampled hot-spot and Stokes frames (lt_shade_hotspot_aa, lt_shade_stokes_aa) -------------------------------
def _fine_shape(hits, samples):
    """(R, W, S) of the output frame of fine records (R S, W S, max_images, 4)."""
    S = int(samples)
    if S < 1 or hits.shape[0] % S or hits.shape[1] % S:
        raise ValueError(f"fine records of {hits.shape[:2]} pixels are not {S} x {S} samples per pixel")
    return hits.shape[0] // S, hits.shape[1] // S, S


def shade_hotspot_aa(hits, n_hits, samples, metric, disk, spot, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The supersampled frame at observer time t_obs (lt_shade_hotspot_aa): shade_hotspot() of the FINE records hits
    (rows S, W S, max_images, 4), n_hits (rows S, W S) or None and base (rows S, W S[, 3]) or None, resolved S x S -> 1 on
    the GPU.  -> dict(rgb (rows, W[, 3]), rgba (rows, W, 4)); ValueError where the fine shape is no multiple of samples."""
    hits, nh = _hit_arrays(hits, n_hits)
    R, W, S = _fine_shape(hits, samples)
    return _shade_frame(load().lt_shade_hotspot_aa, hits, nh, R, W,
                        (S, hits.shape[2], C.byref(metric), C.byref(disk), C.byref(spot), float(t_obs)), base, channels, want)


def shade_hotspot_aa_dev(d_hits, d_n_hits, rows, width, samples, max_images, metric, disk, spot, t_obs, d_base=0, channels=3,
                         d_rgb=0, d_rgba=0):
    """Device-pointer form of shade_hotspot_aa (lt_shade_hotspot_aa_dev): rows, width of the OUTPUT; enqueues on the
    default stream."""
    _check(load().lt_shade_hotspot_aa_dev(_p(d_hits), _p(d_n_hits), rows, width, samples, max_images, C.byref(metric),
                                          C.byref(disk), C.byref(spot), float(t_obs), _p(d_base), channels, _p(d_rgb), _p(d_rgba)))


def shade_stokes_aa(hits, n_hits, pol, samples, metric, disk, spot, field, t_obs):
    """The supersampled Stokes frame at t_obs (lt_shade_stokes_aa): shade_stokes() of the FINE records, resolved S x S -> 1
    on the GPU -> (rows, W, 3) float32 (I, Q, U)."""
    hits, nh = _hit_arrays(hits, n_hits)
    pol = _pol_array(pol, hits)
    R, W, S = _fine_shape(hits, samples)
    out = np.empty((R, W, 3), dtype=np.float32)
    _check(load().lt_shade_stokes_aa(_np_ptr(hits), _np_ptr(nh), _np_ptr(pol), R, W, S, hits.shape[2], C.byref(metric),
                                     C.byref(disk), C.byref(spot), C.byref(field), float(t_obs), _np_ptr(out)))
    return out


def shade_stokes_aa_dev(d_hits, d_n_hits, d_pol, rows, width, samples, max_images, metric, disk, spot, field, t_obs, d_iqu):
    """Device-pointer form of shade_stokes_aa (lt_shade_stokes_aa_dev): rows, width of the OUTPUT; enqueues on the default
    stream."""
    _check(load().lt_shade_stokes_aa_dev(_p(d_hits), _p(d_n_hits), _p(d_pol), rows, width, samples, max_images, C.byref(metric),
                                         C.byref(disk), C.byref(spot), C.byref(field), float(t_obs), _p(d_iqu)))


# ---- a rotating emissivity map on the disk (lt_shade_diskmap, lt_shade_diskmap_aa, lt_diskmap_lightcurve) ----------------
MAP_ROTATIONS = {"kepler": MAP_KEPLERIAN, "rigid": MAP_RIGID}


def default_diskmap(**kw):
    """lt_diskmap with the library's defaults (r_min 6, r_max 20, omega_p 0, exposure 1, 1 x 1 texels, Keplerian,
    with_disk 1); keywords override (rotation: "kepler" / "rigid" or the LT_MAP_* value)."""
    return _default(DiskMap, "lt_default_diskmap", kw, {"rotation": MAP_ROTATIONS})


def _texel_array(dmap, texels):
    """The table as the library reads it: C-contiguous float32 of exactly (dmap.n_r, dmap.n_phi) -- the kernels index it
    with the struct's sizes, so any other shape is refused here."""
    t = np.ascontiguousarray(texels, dtype=np.float32)
    if t.shape != (int(dmap.n_r), int(dmap.n_phi)):
        raise ValueError(f"texels must be (n_r, n_phi) = {(int(dmap.n_r), int(dmap.n_phi))}; got {t.shape}")
    return t


def shade_diskmap(hits, n_hits, metric, disk, dmap, texels, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The frame of a rotating emissivity map at observer time t_obs from stored hits (lt_shade_diskmap).  dmap: an
    ltrace.DiskMap, texels (n_r, n_phi) float32; everything else as shade_hotspot.  -> dict(rgb, rgba)."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _texel_array(dmap, texels)
    R, W, m = hits.shape[:3]
    return _shade_frame(load().lt_shade_diskmap, hits, nh, R, W,
                        (m, C.byref(metric), C.byref(disk), C.byref(dmap), _np_ptr(tex), float(t_obs)), base, channels, want)


def shade_diskmap_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, d_texels, t_obs, d_base=0, channels=3,
                      d_rgb=0, d_rgba=0):
    """Device-pointer form of shade_diskmap (lt_shade_diskmap_dev): d_texels holds dmap.n_r x dmap.n_phi float32; enqueues
    on the default stream."""
    _check(load().lt_shade_diskmap_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                       C.byref(dmap), _p(d_texels), float(t_obs), _p(d_base), channels, _p(d_rgb), _p(d_rgba)))


def shade_diskmap_aa(hits, n_hits, samples, metric, disk, dmap, texels, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The supersampled frame of a rotating emissivity map (lt_shade_diskmap_aa): shade_diskmap() of the FINE records
    (rows S, W S, max_images, 4) and base (rows S, W S[, 3]), resolved S x S -> 1 on the GPU.  -> dict(rgb (rows, W[, 3]),
    rgba (rows, W, 4)); ValueError where the fine shape is no multiple of samples."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _texel_array(dmap, texels)
    R, W, S = _fine_shape(hits, samples)
    return _shade_frame(load().lt_shade_diskmap_aa, hits, nh, R, W,
                        (S, hits.shape[2], C.byref(metric), C.byref(disk), C.byref(dmap), _np_ptr(tex), float(t_obs)), base, channels, want)


def shade_diskmap_aa_dev(d_hits, d_n_hits, rows, width, samples, max_images, metric, disk, dmap, d_texels, t_obs, d_base=0,
                         channels=3, d_rgb=0, d_rgba=0):
    """Device-pointer form of shade_diskmap_aa (lt_shade_diskmap_aa_dev): rows, width of the OUTPUT; enqueues on the
    default stream."""
    _check(load().lt_shade_diskmap_aa_dev(_p(d_hits), _p(d_n_hits), rows, width, samples, max_images, C.byref(metric),
                                          C.byref(disk), C.byref(dmap), _p(d_texels), float(t_obs), _p(d_base), channels,
                                          _p(d_rgb), _p(d_rgba)))


def diskmap_lightcurve(hits, n_hits, metric, disk, dmap, texels, t_start, dt, n_times):
    """The map's light curve (lt_diskmap_lightcurve) -> (n_times, 3) float64: per time the sums of e, e ix, e iy."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _texel_array(dmap, texels)
    R, W, m = hits.shape[:3]
    out = np.empty((int(n_times), 3))
    _check(load().lt_diskmap_lightcurve(_np_ptr(hits), _np_ptr(nh), R, W, m, C.byref(metric), C.byref(disk), C.byref(dmap),
                                        _np_ptr(tex), float(t_start), float(dt), int(n_times), _np_ptr(out)))
    return out


def diskmap_lightcurve_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, d_texels, t_start, dt, n_times, d_out):
    """Device-pointer form of diskmap_lightcurve (lt_diskmap_lightcurve_dev); enqueues on the default stream."""
    _check(load().lt_diskmap_lightcurve_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                            C.byref(dmap), _p(d_texels), float(t_start), float(dt), int(n_times), _p(d_out)))


# ---- energy-resolved light (lt_disk_spectrum, lt_hotspot_spectrum, lt_diskmap_spectrum) ---------------------------------
def default_spectrum(**kw):
    """lt_spectrum with the library's defaults (g 0.0625 ... 1.5625, 96 bins, not split); keywords override."""
    return _default(Spectrum, "lt_default_spectrum", kw)


def spectrum_planes(spec, max_images):
    """Planes of a spectrum's output: 1, or max_images with split_orders."""
    return int(max_images) if spec.split_orders else 1


def spectrum_batch_times(spec, max_images):
    """Times one launch of a spectrum's first stage holds: its partials, SPECTRUM_BLOCKS histograms of float64 per time,
    stay within SPECTRUM_WORKSPACE_BYTES (at least one time); longer sequences run in batches of this many."""
    return max(1, SPECTRUM_WORKSPACE_BYTES // (SPECTRUM_BLOCKS * spectrum_planes(spec, max_images) * (int(spec.n_bins) + 2) * 8))


def _spectrum_out(spec, max_images, n_times):
    """The output of a spectrum call; sized by the header's limits so that a grid the library will refuse allocates little."""
    bins = min(max(int(spec.n_bins), 0), SPECTRUM_MAX_BINS)
    return np.empty((max(int(n_times), 0), spectrum_planes(spec, min(max(int(max_images), 0), 8)), bins + 2))


def _times(t_start, dt, n_times):
    """The argument tail of a call over observer times t_start + i dt."""
    return float(t_start), float(dt), int(n_times)


def _spectrum(fn, records, emitter, spec, times):
    """The host-pointer call fn(hits, n_hits, R, W, max_images, *emitter, spec, *times, out) of a spectrum -> its
    (n_times, planes, n_bins + 2) output.  records: _hit_arrays' pair; emitter: metric, disk and the emitter's own
    arguments as ctypes passes them; times: _times' tail, or () for the disk's one row."""
    R, W, m = records[0].shape[:3]
    out = _spectrum_out(spec, m, times[2] if times else 1)
    _check(fn(*map(_np_ptr, records), R, W, m, *emitter, C.byref(spec), *times, _np_ptr(out)))
    return out


def disk_spectrum(hits, n_hits, metric, disk, spec):
    """The stationary disk's line profile from stored hits (lt_disk_spectrum) -> (planes, n_bins + 2) float64: column 0
    the underflow, the last the overflow; plane j the image order j with spec.split_orders."""
    return _spectrum(load().lt_disk_spectrum, _hit_arrays(hits, n_hits), (C.byref(metric), C.byref(disk)), spec, ())[0]


def disk_spectrum_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spec, d_out):
    """Device-pointer form of disk_spectrum (lt_disk_spectrum_dev); enqueues on the default stream."""
    _check(load().lt_disk_spectrum_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                       C.byref(spec), _p(d_out)))


def hotspot_spectrum(hits, n_hits, metric, disk, spot, spec, t_start, dt, n_times):
    """The spot's dynamic spectrum (lt_hotspot_spectrum) -> (n_times, planes, n_bins + 2) float64 at t_start + i dt."""
    return _spectrum(load().lt_hotspot_spectrum, _hit_arrays(hits, n_hits), (C.byref(metric), C.byref(disk), C.byref(spot)), spec,
                     _times(t_start, dt, n_times))


def hotspot_spectrum_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spot, spec, t_start, dt, n_times, d_out):
    """Device-pointer form of hotspot_spectrum (lt_hotspot_spectrum_dev); enqueues on the default stream."""
    _check(load().lt_hotspot_spectrum_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                          C.byref(spot), C.byref(spec), *_times(t_start, dt, n_times), _p(d_out)))


def diskmap_spectrum(hits, n_hits, metric, disk, dmap, texels, spec, t_start, dt, n_times):
    """The map's dynamic spectrum (lt_diskmap_spectrum) -> (n_times, planes, n_bins + 2) float64 at t_start + i dt."""
    records = _hit_arrays(hits, n_hits)
    tex = _texel_array(dmap, texels)
    return _spectrum(load().lt_diskmap_spectrum, records, (C.byref(metric), C.byref(disk), C.byref(dmap), _np_ptr(tex)), spec,
                     _times(t_start, dt, n_times))


def diskmap_spectrum_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, d_texels, spec, t_start, dt, n_times, d_out):
    """Device-pointer form of diskmap_spectrum (lt_diskmap_spectrum_dev); enqueues on the default stream."""
    _check(load().lt_diskmap_spectrum_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                          C.byref(dmap), _p(d_texels), C.byref(spec), *_times(t_start, dt, n_times), _p(d_out)))


# ---- thermal continuum (lt_disk_thermal_spectrum, lt_shade_thermal) -----------------------------------------------------------
def default_thermal(**kw):
    """lt_thermal with the library's defaults (r 6 ... 20, t_max 1, f_col 1, exposure 1, 2 nodes, not split); keywords override."""
    return _default(Thermal, "lt_default_thermal", kw)


def _radial_table(name, table, n_r):
    """A radial table as the library reads it: float64, contiguous, (n_r,); one that is not the struct's n_r never reaches it."""
    table = np.ascontiguousarray(table, dtype=np.float64)
    if table.shape != (int(n_r),):
        raise ValueError(f"{name} must be (n_r,) = ({int(n_r)},), got {table.shape}")
    return table


def _thermal_arrays(thermal, flux, nu, limit):
    """(flux, nu) as the library reads them; more frequencies than an output is sized for never reach it."""
    flux = _radial_table("flux", flux, thermal.n_r)
    nu = np.ascontiguousarray(nu, dtype=np.float64).ravel()
    if nu.size > limit:
        raise ValueError(f"at most {limit} frequencies, got {nu.size}")
    return flux, nu


def _atmosphere_tables(limb, poldeg):
    """(lt_atmosphere, limb, poldeg) as the library reads them: two float64 tables of one size, 2 ... ATMOSPHERE_MAX_NODES nodes."""
    limb, poldeg = np.ascontiguousarray(limb, dtype=np.float64), np.ascontiguousarray(poldeg, dtype=np.float64)
    if limb.ndim != 1 or limb.shape != poldeg.shape or not 2 <= limb.size <= ATMOSPHERE_MAX_NODES:
        raise ValueError(f"limb and poldeg must both be (n_mu,), n_mu 2 ... {ATMOSPHERE_MAX_NODES}; got {limb.shape} and {poldeg.shape}")
    return Atmosphere(limb.size, 0), limb, poldeg


def _thermal(fn, records, metric, disk, thermal, flux, nu, bands, atmosphere=None):
    """One host-form thermal product fn of the checked records (the polarization records behind them with an atmosphere =
    (limb, poldeg)): the tables and frequencies as the library reads them, and the output -- (planes, n_freq) float64 of a
    spectrum, (n_bands, rows, W) float32 of band images, with an atmosphere a Stokes axis of 3 before the last axis or two."""
    R, W, m = records[0].shape[:3]
    flux, nu = _thermal_arrays(thermal, flux, nu, THERMAL_MAX_BANDS if bands else THERMAL_MAX_FREQS)
    atm, stokes = (), ()
    if atmosphere is not None:
        a, limb, poldeg = _atmosphere_tables(*atmosphere)
        atm, stokes = (C.byref(a), _np_ptr(limb), _np_ptr(poldeg)), (3,)
    if bands:
        out = np.empty((nu.size,) + stokes + (R, W), dtype=np.float32)
    else:
        out = np.empty((min(m, DISK_MAX_IMAGES) if thermal.split_orders else 1,) + stokes + (nu.size,))
    _check(fn(*map(_np_ptr, records), R, W, m, C.byref(metric), C.byref(disk), C.byref(thermal), _np_ptr(flux), *atm, _np_ptr(nu), nu.size,
              _np_ptr(out)))
    return out


def thermal_spectrum(hits, n_hits, metric, disk, thermal, flux, nu):
    """The disk's thermal spectrum from stored hits (lt_disk_thermal_spectrum) -> (planes, n_freq) float64, the flux density
    at the frequencies nu summed over all pixels and stored slots; plane j the image order j with thermal.split_orders."""
    return _thermal(load().lt_disk_thermal_spectrum, _hit_arrays(hits, n_hits), metric, disk, thermal, flux, nu, False)


def thermal_spectrum_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, thermal, d_flux, d_nu, n_freq, d_out):
    """Device-pointer form of thermal_spectrum (lt_disk_thermal_spectrum_dev); enqueues on the default stream."""
    _check(load().lt_disk_thermal_spectrum_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                               C.byref(thermal), _p(d_flux), _p(d_nu), n_freq, _p(d_out)))


def shade_thermal(hits, n_hits, metric, disk, thermal, flux, nu):
    """The disk's thermal band images from stored hits (lt_shade_thermal) -> (n_bands, rows, W) float32, unclamped."""
    return _thermal(load().lt_shade_thermal, _hit_arrays(hits, n_hits), metric, disk, thermal, flux, nu, True)


def shade_thermal_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, thermal, d_flux, d_nu, n_freq, d_out):
    """Device-pointer form of shade_thermal (lt_shade_thermal_dev); enqueues on the default stream."""
    _check(load().lt_shade_thermal_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk), C.byref(thermal),
                                       _p(d_flux), _p(d_nu), n_freq, _p(d_out)))


# ---- reverberation (lt_disk_transfer) -----------------------------------------------------------------------------------------
def default_transfer(**kw):
    """lt_transfer with the library's defaults (tau 0 ... 256, 64 bins, 2 nodes on r 6 ... 20, t_ref 0); keywords override."""
    return _default(Transfer, "lt_default_transfer", kw)


def transfer_keys(spec, transfer, max_images):
    """Keys of a transfer function's output, planes (n_tau + 2) (n_bins + 2); at most TRANSFER_MAX_KEYS."""
    return spectrum_planes(spec, max_images) * (int(transfer.n_tau) + 2) * (int(spec.n_bins) + 2)


def _transfer_tables(transfer, delay, emis):
    """(delay, emis) as the library reads them."""
    return _radial_table("delay", delay, transfer.n_r), _radial_table("emis", emis, transfer.n_r)


def disk_transfer(hits, n_hits, metric, disk, spec, transfer, delay, emis):
    """The disk's delay-energy transfer function from stored hits (lt_disk_transfer) -> (planes, n_tau + 2, n_bins + 2)
    float64: per image order (with spec.split_orders; else one plane) and delay bin the line's histogram over g; row and
    column 0 the underflows, the last the overflows."""
    hits, nh = _hit_arrays(hits, n_hits)
    R, W, m = hits.shape[:3]
    delay, emis = _transfer_tables(transfer, delay, emis)
    if transfer_keys(spec, transfer, min(max(m, 0), DISK_MAX_IMAGES)) > TRANSFER_MAX_KEYS or not 1 <= int(transfer.n_tau) <= TRANSFER_MAX_TAU:
        out = np.empty((1, 1, 1))                              # (the library refuses this grid: an output it will not touch)
    else:
        out = np.empty((spectrum_planes(spec, m), int(transfer.n_tau) + 2, min(max(int(spec.n_bins), 0), SPECTRUM_MAX_BINS) + 2))
    _check(load().lt_disk_transfer(_np_ptr(hits), _np_ptr(nh), R, W, m, C.byref(metric), C.byref(disk), C.byref(spec), C.byref(transfer),
                                   _np_ptr(delay), _np_ptr(emis), _np_ptr(out)))
    return out


def disk_transfer_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spec, transfer, d_delay, d_emis, d_out):
    """Device-pointer form of disk_transfer (lt_disk_transfer_dev); enqueues on the default stream."""
    _check(load().lt_disk_transfer_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk), C.byref(spec),
                                       C.byref(transfer), _p(d_delay), _p(d_emis), _p(d_out)))


# ---- visibilities (lt_disk_visibility, lt_hotspot_visibility, lt_diskmap_visibility) ---------------------------------------
def visibility_planes(split_orders, max_images):
    """Planes of a visibility's output: 1, or max_images with split_orders."""
    return int(max_images) if split_orders else 1


def visibility_batch_times(split_orders, max_images):
    """Times a workgroup of the visibilities' first stage accumulates at once (lt_visibility_batch_times):
    max(1, VISIBILITY_BATCH_TERMS // planes); longer sequences run in batches of this many.  Needs no GPU."""
    return int(load().lt_visibility_batch_times(int(max_images), int(bool(split_orders))))


def _uv_array(uv):
    """The baselines as the library reads them: C-contiguous float64 (n, 2), cycles per pixel of the record buffer."""
    uv = np.ascontiguousarray(uv, dtype=np.float64)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError(f"uv must be (n_baselines, 2); got {uv.shape}")
    return uv


def _visibility_out(uv, split_orders, max_images, n_times):
    """The float64 (n_times, planes, n_baselines, 2) output of a visibility call; sized by the header's limits so that a
    call the library will refuse allocates little."""
    n_b = min(uv.shape[0], VISIBILITY_MAX_BASELINES)
    return np.empty((max(int(n_times), 0), visibility_planes(split_orders, min(max(int(max_images), 0), 8)), n_b, 2))


def _complex(out):
    """(..., 2) float64 (re, im) as complex128 (...)."""
    return np.ascontiguousarray(out).view(np.complex128)[..., 0]


def _visibility(fn, records, emitter, uv, split_orders, times, out_of=_visibility_out):
    """The host-pointer call fn(*records, R, W, max_images, *emitter, uv, n_baselines, split_orders, *times, out) of a
    visibility -> complex128 of out_of's shape.  records: _hit_arrays' pair, with the polarization records behind it
    where the call takes them; emitter: metric, disk and the emitter's own arguments as ctypes passes them; times:
    _times' tail, or () for the disk's one row."""
    uv = _uv_array(uv)
    R, W, m = records[0].shape[:3]
    out = out_of(uv, split_orders, m, times[2] if times else 1)
    _check(fn(*map(_np_ptr, records), R, W, m, *emitter, _np_ptr(uv), uv.shape[0], int(bool(split_orders)), *times, _np_ptr(out)))
    return _complex(out)


def _visibility_dev(fn, d_records, shape, emitter, uv, split_orders, times, d_out):
    """The device-pointer call of a visibility: d_records, shape = (rows, width, max_images), then as _visibility; uv stays
    a host array."""
    uv = _uv_array(uv)
    _check(fn(*map(_p, d_records), *shape, *emitter, _np_ptr(uv), uv.shape[0], int(bool(split_orders)), *times, _p(d_out)))


def disk_visibility(hits, n_hits, metric, disk, uv, split_orders=False):
    """The stationary disk's visibilities from stored hits (lt_disk_visibility) -> (planes, n_baselines) complex128.  uv
    (n_baselines, 2) float64 in cycles per pixel of the records, |u|, |v| <= 0.5; plane j the image order j with
    split_orders.  The phase's origin is pixel (0, 0)."""
    return _visibility(load().lt_disk_visibility, _hit_arrays(hits, n_hits), (C.byref(metric), C.byref(disk)), uv, split_orders, ())[0]


def disk_visibility_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, uv, split_orders, d_out):
    """Device-pointer form of disk_visibility (lt_disk_visibility_dev): uv stays a host array, d_out holds
    (1, planes, n_baselines, 2) float64; enqueues on the default stream."""
    _visibility_dev(load().lt_disk_visibility_dev, (d_hits, d_n_hits), (rows, width, max_images), (C.byref(metric), C.byref(disk)), uv,
                    split_orders, (), d_out)


def hotspot_visibility(hits, n_hits, metric, disk, spot, uv, split_orders, t_start, dt, n_times):
    """The spot's visibilities (lt_hotspot_visibility) -> (n_times, planes, n_baselines) complex128 at t_start + i dt."""
    return _visibility(load().lt_hotspot_visibility, _hit_arrays(hits, n_hits), (C.byref(metric), C.byref(disk), C.byref(spot)), uv,
                       split_orders, _times(t_start, dt, n_times))


def hotspot_visibility_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, spot, uv, split_orders, t_start, dt, n_times, d_out):
    """Device-pointer form of hotspot_visibility (lt_hotspot_visibility_dev); uv stays a host array."""
    _visibility_dev(load().lt_hotspot_visibility_dev, (d_hits, d_n_hits), (rows, width, max_images),
                    (C.byref(metric), C.byref(disk), C.byref(spot)), uv, split_orders, _times(t_start, dt, n_times), d_out)


def diskmap_visibility(hits, n_hits, metric, disk, dmap, texels, uv, split_orders, t_start, dt, n_times):
    """The map's visibilities (lt_diskmap_visibility) -> (n_times, planes, n_baselines) complex128 at t_start + i dt."""
    records = _hit_arrays(hits, n_hits)
    tex = _texel_array(dmap, texels)
    return _visibility(load().lt_diskmap_visibility, records, (C.byref(metric), C.byref(disk), C.byref(dmap), _np_ptr(tex)), uv,
                       split_orders, _times(t_start, dt, n_times))


def diskmap_visibility_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, d_texels, uv, split_orders, t_start, dt, n_times,
                           d_out):
    """Device-pointer form of diskmap_visibility (lt_diskmap_visibility_dev); uv stays a host array."""
    _visibility_dev(load().lt_diskmap_visibility_dev, (d_hits, d_n_hits), (rows, width, max_images),
                    (C.byref(metric), C.byref(disk), C.byref(dmap), _p(d_texels)), uv, split_orders, _times(t_start, dt, n_times), d_out)


# ---- a disk movie: tables that change with time (lt_shade_diskmovie, lt_shade_diskmovie_aa, lt_diskmovie_*) ---------------
MOVIE_BOUNDARIES = {"hold": MOVIE_HOLD, "loop": MOVIE_LOOP}


def default_diskmovie(**kw):
    """lt_diskmovie with the library's defaults (t0 0, dt_frame 1, 1 frame, hold); keywords override (boundary: "hold" /
    "loop" or the LT_MOVIE_* value)."""
    return _default(DiskMovie, "lt_default_diskmovie", kw, {"boundary": MOVIE_BOUNDARIES})


def _movie_array(dmap, movie, texels):
    """The movie's tables as the library reads them: C-contiguous float32 of exactly (movie.n_frames, dmap.n_r, dmap.n_phi)
    -- the kernels index them with the structs' sizes, so any other shape is refused here."""
    t = np.ascontiguousarray(texels, dtype=np.float32)
    want = (int(movie.n_frames), int(dmap.n_r), int(dmap.n_phi))
    if t.shape != want:
        raise ValueError(f"texels must be (n_frames, n_r, n_phi) = {want}; got {t.shape}")
    return t


def shade_diskmovie(hits, n_hits, metric, disk, dmap, movie, texels, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The frame of a disk movie at observer time t_obs from stored hits (lt_shade_diskmovie).  dmap: an ltrace.DiskMap,
    movie: an ltrace.DiskMovie, texels (n_frames, n_r, n_phi) float32; everything else as shade_diskmap.  -> dict(rgb, rgba)."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _movie_array(dmap, movie, texels)
    R, W, m = hits.shape[:3]
    return _shade_frame(load().lt_shade_diskmovie, hits, nh, R, W,
                        (m, C.byref(metric), C.byref(disk), C.byref(dmap), C.byref(movie), _np_ptr(tex), float(t_obs)), base, channels, want)


def shade_diskmovie_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, movie, d_texels, t_obs, d_base=0, channels=3,
                        d_rgb=0, d_rgba=0):
    """Device-pointer form of shade_diskmovie (lt_shade_diskmovie_dev): d_texels holds movie.n_frames x dmap.n_r x dmap.n_phi
    float32; enqueues on the default stream."""
    _check(load().lt_shade_diskmovie_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                         C.byref(dmap), C.byref(movie), _p(d_texels), float(t_obs), _p(d_base), channels, _p(d_rgb),
                                         _p(d_rgba)))


def shade_diskmovie_aa(hits, n_hits, samples, metric, disk, dmap, movie, texels, t_obs, base=None, channels=None, want=("rgb", "rgba")):
    """The supersampled frame of a disk movie (lt_shade_diskmovie_aa): shade_diskmovie() of the FINE records
    (rows S, W S, max_images, 4) and base (rows S, W S[, 3]), resolved S x S -> 1 on the GPU.  -> dict(rgb (rows, W[, 3]),
    rgba (rows, W, 4)); ValueError where the fine shape is no multiple of samples."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _movie_array(dmap, movie, texels)
    R, W, S = _fine_shape(hits, samples)
    return _shade_frame(load().lt_shade_diskmovie_aa, hits, nh, R, W,
                        (S, hits.shape[2], C.byref(metric), C.byref(disk), C.byref(dmap), C.byref(movie), _np_ptr(tex), float(t_obs)), base,
                        channels, want)


def shade_diskmovie_aa_dev(d_hits, d_n_hits, rows, width, samples, max_images, metric, disk, dmap, movie, d_texels, t_obs, d_base=0,
                           channels=3, d_rgb=0, d_rgba=0):
    """Device-pointer form of shade_diskmovie_aa (lt_shade_diskmovie_aa_dev): rows, width of the OUTPUT; enqueues on the
    default stream."""
    _check(load().lt_shade_diskmovie_aa_dev(_p(d_hits), _p(d_n_hits), rows, width, samples, max_images, C.byref(metric),
                                            C.byref(disk), C.byref(dmap), C.byref(movie), _p(d_texels), float(t_obs), _p(d_base),
                                            channels, _p(d_rgb), _p(d_rgba)))


def diskmovie_lightcurve(hits, n_hits, metric, disk, dmap, movie, texels, t_start, dt, n_times):
    """The movie's light curve (lt_diskmovie_lightcurve) -> (n_times, 3) float64: per time the sums of e, e ix, e iy."""
    hits, nh = _hit_arrays(hits, n_hits)
    tex = _movie_array(dmap, movie, texels)
    R, W, m = hits.shape[:3]
    out = np.empty((int(n_times), 3))
    _check(load().lt_diskmovie_lightcurve(_np_ptr(hits), _np_ptr(nh), R, W, m, C.byref(metric), C.byref(disk), C.byref(dmap),
                                          C.byref(movie), _np_ptr(tex), float(t_start), float(dt), int(n_times), _np_ptr(out)))
    return out


def diskmovie_lightcurve_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, movie, d_texels, t_start, dt, n_times, d_out):
    """Device-pointer form of diskmovie_lightcurve (lt_diskmovie_lightcurve_dev); enqueues on the default stream."""
    _check(load().lt_diskmovie_lightcurve_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                              C.byref(dmap), C.byref(movie), _p(d_texels), float(t_start), float(dt), int(n_times),
                                              _p(d_out)))


def diskmovie_spectrum(hits, n_hits, metric, disk, dmap, movie, texels, spec, t_start, dt, n_times):
    """The movie's dynamic spectrum (lt_diskmovie_spectrum) -> (n_times, planes, n_bins + 2) float64 at t_start + i dt."""
    records = _hit_arrays(hits, n_hits)
    tex = _movie_array(dmap, movie, texels)
    return _spectrum(load().lt_diskmovie_spectrum, records, (C.byref(metric), C.byref(disk), C.byref(dmap), C.byref(movie), _np_ptr(tex)),
                     spec, _times(t_start, dt, n_times))


def diskmovie_spectrum_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, movie, d_texels, spec, t_start, dt, n_times,
                           d_out):
    """Device-pointer form of diskmovie_spectrum (lt_diskmovie_spectrum_dev); enqueues on the default stream."""
    _check(load().lt_diskmovie_spectrum_dev(_p(d_hits), _p(d_n_hits), rows, width, max_images, C.byref(metric), C.byref(disk),
                                            C.byref(dmap), C.byref(movie), _p(d_texels), C.byref(spec), *_times(t_start, dt, n_times),
                                            _p(d_out)))


def diskmovie_visibility(hits, n_hits, metric, disk, dmap, movie, texels, uv, split_orders, t_start, dt, n_times):
    """The movie's visibilities (lt_diskmovie_visibility) -> (n_times, planes, n_baselines) complex128 at t_start + i dt."""
    records = _hit_arrays(hits, n_hits)
    tex = _movie_array(dmap, movie, texels)
    return _visibility(load().lt_diskmovie_visibility, records,
                       (C.byref(metric), C.byref(disk), C.byref(dmap), C.byref(movie), _np_ptr(tex)), uv, split_orders,
                       _times(t_start, dt, n_times))


def diskmovie_visibility_dev(d_hits, d_n_hits, rows, width, max_images, metric, disk, dmap, movie, d_texels, uv, split_orders, t_start, dt,
                             n_times, d_out):
    """Device-pointer form of diskmovie_visibility (lt_diskmovie_visibility_dev); uv stays a host array."""
    _visibility_dev(load().lt_diskmovie_visibility_dev, (d_hits, d_n_hits), (rows, width, max_images),
                    (C.byref(metric), C.byref(disk), C.byref(dmap), C.byref(movie), _p(d_texels)), uv, split_orders,
                    _times(t_start, dt, n_times), d_out)


# ---- polarized visibilities (lt_disk_visibility_stokes, lt_hotspot_visibility_stokes) -------------------------------------
def visibility_stokes_batch_pairs():
    """(time, plane) pairs a workgroup of the polarized visibilities' first stage accumulates at once
    (lt_visibility_stokes_batch_pairs): VISIBILITY_STOKES_BATCH_PAIRS, three terms each.  Needs no GPU."""
    return int(load().lt_visibility_stokes_batch_pairs())


def _visibility_stokes_out(uv, split_orders, max_images, n_times):
    """The float64 (n_times, planes, 3, n_baselines, 2) output of a polarized visibility call, sized as _visibility_out."""
    shape = _visibility_out(uv, split_orders, max_images, 0).shape
    return np.empty((max(int(n_times), 0), shape[1], 3, shape[2], 2))


def _pol_records(hits, n_hits, pol):
    """_hit_arrays' pair with the checked polarization records behind it."""
    records = _hit_arrays(hits, n_hits)
    return records + (_pol_array(pol, records[0]),)


def disk_visibility_stokes(hits, n_hits, pol, metric, disk, field, uv, split_orders=False):
    """The stationary disk's polarized visibilities (lt_disk_visibility_stokes) -> (planes, 3, n_baselines) complex128, the
    Stokes axis (I, Q, U); pol the (rows, W, max_images, 4) records of trace_disk_pol, the rest as disk_visibility.  The I
    plane has disk_visibility's bits."""
    return _visibility(load().lt_disk_visibility_stokes, _pol_records(hits, n_hits, pol), (C.byref(metric), C.byref(disk), C.byref(field)),
                       uv, split_orders, (), _visibility_stokes_out)[0]


def disk_visibility_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, field, uv, split_orders, d_out):
    """Device-pointer form of disk_visibility_stokes (lt_disk_visibility_stokes_dev): uv stays a host array, d_out holds
    (1, planes, 3, n_baselines, 2) float64; enqueues on the default stream."""
    _visibility_dev(load().lt_disk_visibility_stokes_dev, (d_hits, d_n_hits, d_pol), (rows, width, max_images),
                    (C.byref(metric), C.byref(disk), C.byref(field)), uv, split_orders, (), d_out)


def hotspot_visibility_stokes(hits, n_hits, pol, metric, disk, spot, field, uv, split_orders, t_start, dt, n_times):
    """The spot's polarized visibilities (lt_hotspot_visibility_stokes) -> (n_times, planes, 3, n_baselines) complex128 at
    t_start + i dt, the Stokes axis (I, Q, U).  The I plane has hotspot_visibility's bits."""
    return _visibility(load().lt_hotspot_visibility_stokes, _pol_records(hits, n_hits, pol),
                       (C.byref(metric), C.byref(disk), C.byref(spot), C.byref(field)), uv, split_orders, _times(t_start, dt, n_times),
                       _visibility_stokes_out)


def hotspot_visibility_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, spot, field, uv, split_orders, t_start, dt,
                                  n_times, d_out):
    """Device-pointer form of hotspot_visibility_stokes (lt_hotspot_visibility_stokes_dev); uv stays a host array."""
    _visibility_dev(load().lt_hotspot_visibility_stokes_dev, (d_hits, d_n_hits, d_pol), (rows, width, max_images),
                    (C.byref(metric), C.byref(disk), C.byref(spot), C.byref(field)), uv, split_orders, _times(t_start, dt, n_times), d_out)


# ---- polarized thermal continuum (lt_disk_thermal_spectrum_stokes, lt_shade_thermal_stokes) --------------------------------
def thermal_spectrum_stokes(hits, n_hits, pol, metric, disk, thermal, flux, limb, poldeg, nu):
    """The thermal spectrum of a scattering atmosphere from stored hits (lt_disk_thermal_spectrum_stokes) -> (planes, 3, n_freq)
    float64, the Stokes axis (I, Q, U); pol the (rows, W, max_images, 4) records of trace_disk_pol for the field (0, 0, 1), limb
    and poldeg the atmosphere's tables on mu, the rest as thermal_spectrum.  With limb = 1 the I plane has thermal_spectrum's bits."""
    return _thermal(load().lt_disk_thermal_spectrum_stokes, _pol_records(hits, n_hits, pol), metric, disk, thermal, flux, nu, False,
                    (limb, poldeg))


def thermal_spectrum_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, thermal, d_flux, n_mu, d_limb, d_poldeg, d_nu,
                                n_freq, d_out):
    """Device-pointer form of thermal_spectrum_stokes (lt_disk_thermal_spectrum_stokes_dev); enqueues on the default stream."""
    _check(load().lt_disk_thermal_spectrum_stokes_dev(_p(d_hits), _p(d_n_hits), _p(d_pol), rows, width, max_images, C.byref(metric),
                                                      C.byref(disk), C.byref(thermal), _p(d_flux), C.byref(Atmosphere(int(n_mu), 0)),
                                                      _p(d_limb), _p(d_poldeg), _p(d_nu), n_freq, _p(d_out)))


def shade_thermal_stokes(hits, n_hits, pol, metric, disk, thermal, flux, limb, poldeg, nu):
    """The band images of a scattering atmosphere from stored hits (lt_shade_thermal_stokes) -> (n_bands, 3, rows, W) float32,
    unclamped, the Stokes axis (I, Q, U).  With limb = 1 the I planes have shade_thermal's bits."""
    return _thermal(load().lt_shade_thermal_stokes, _pol_records(hits, n_hits, pol), metric, disk, thermal, flux, nu, True, (limb, poldeg))


def shade_thermal_stokes_dev(d_hits, d_n_hits, d_pol, rows, width, max_images, metric, disk, thermal, d_flux, n_mu, d_limb, d_poldeg, d_nu,
                             n_freq, d_out):
    """Device-pointer form of shade_thermal_stokes (lt_shade_thermal_stokes_dev); enqueues on the default stream."""
    _check(load().lt_shade_thermal_stokes_dev(_p(d_hits), _p(d_n_hits), _p(d_pol), rows, width, max_images, C.byref(metric), C.byref(disk),
                                              C.byref(thermal), _p(d_flux), C.byref(Atmosphere(int(n_mu), 0)), _p(d_limb), _p(d_poldeg),
                                              _p(d_nu), n_freq, _p(d_out)))


# ---- supersampled frames (lt_render_aa) ---------------------------------------------------------------------------
AA_MODES = {"plain": AA_PLAIN, "disk": AA_DISK, "disk_images": AA_DISK_IMAGES}


def _aa_keywords(a, kw):
    for k, v in kw.items():
        if k == "mode" and isinstance(v, str):
            v = AA_MODES[v]
        setattr(a, k, v)
    return a


def default_aa(**kw):
    """lt_aa with the library's defaults (samples = 2, plain mode, 3 images, automatic bands); keywords override."""
    return _aa_keywords(_default(AA, "lt_default_aa", {}), kw)


def _fine_background(cam, samples, background):
    if background is None:
        return None, 3, False
    bg = np.ascontiguousarray(background, dtype=np.float32)
    # (a sample count the library refuses is left for it to refuse)
    if 1 <= samples <= AA_MAX_SAMPLES and bg.shape[:2] != (cam.height * samples, cam.width * samples):
        raise ValueError("background must have the fine frame's size: (height * samples, width * samples)")
    nch = 1 if bg.ndim == 2 else bg.shape[2]
    if nch not in (1, 3):
        raise ValueError("background must be grayscale or RGB")
    return bg, nch, bg.ndim == 2


def _aa_render(fn, cam, metric, opts, aa, disk, rows, bgs, nch, gray, want, planes):
    """The host-pointer call fn of render_aa / render_aa_adaptive: 'rgb', 'rgba' and the uint8 `planes` (name -> trailing
    shape, in the call's order) that `want` names, in pinned memory, and 'stats' with the disk's counters; and the
    call's Stats."""
    out = _frame_outputs(rows, cam.width, nch, gray, [w for w in want if w in ("rgb", "rgba")])
    for name, tail in planes.items():
        if name in want:
            out[name] = pinned_empty((rows, cam.width) + tail, np.uint8)
    st = Stats()
    _check(fn(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(aa), None if disk is None else C.byref(disk),
              *[_np_ptr(bg) for bg in bgs], nch, _np_ptr(out.get("rgb")), _np_ptr(out.get("rgba")),
              *[_np_ptr(out.get(name)) for name in planes], C.byref(st)))
    out["stats"] = _disk_stats(st)
    return out, st


def render_aa(cam, metric, opts, aa, disk=None, background=None, want=("rgb", "rgba", "cover")):
    """Host-pointer supersampled frame (lt_render_aa): aa.samples^2 rays per pixel, resolved on the GPU.  background:
    the FINE-size image (H * samples, W * samples[, 3]) or None.  disk: an ltrace.Disk for the disk modes.  Returns
    'rgb' (rows, W[, 3]) float32, 'rgba' (rows, W, 4) uint8, 'cover' (rows, W, 4) uint8 (sub-rays escaped / captured /
    invalid / on the disk) in pinned memory, and 'stats' (the fine frame's counters; kernel times summed over bands)."""
    rows = _frame_rows(cam, opts)
    bg, nch, gray = _fine_background(cam, int(aa.samples), background)
    return _aa_render(load().lt_render_aa, cam, metric, opts, aa, disk, rows, [bg], nch, gray, want,
                      {"cover": (4,)})[0]


def render_aa_dev(cam, metric, opts, aa, disk=None, d_bg=0, bg_channels=3, d_rgb=0, d_rgba=0, d_cover=0, d_stats=0):
    """Device-pointer form of render_aa (lt_render_aa_dev); pointers are integers, 0 = NULL.  Asynchronous."""
    _check(load().lt_render_aa_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(aa),
                                   None if disk is None else C.byref(disk), _p(d_bg), bg_channels, _p(d_rgb), _p(d_rgba),
                                   _p(d_cover), _p(d_stats)))


def aa_band_bytes(cam, metric, opts, aa, disk=None):
    """(bytes of ray records the largest band needs, output rows per band, bands) of a render_aa call (lt_aa_band_bytes;
    host arithmetic, no GPU needed)."""
    rows, bands = C.c_int32(), C.c_int32()
    n = int(load().lt_aa_band_bytes(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(aa),
                                    None if disk is None else C.byref(disk), C.byref(rows), C.byref(bands)))
    if n < 0:
        _check(n)
    return n, int(rows.value), int(bands.value)


# ---- adaptive supersampling (lt_render_aa_adaptive) ---------------------------------------------------------------
def default_aa_adaptive(**kw):
    """lt_aa_adaptive with the library's defaults (samples_lo = 1, samples_hi = 4, plain mode, 3 images, automatic
    bands and chunks, contrast = 0.0625); keywords override."""
    return _aa_keywords(_default(AAAdaptive, "lt_default_aa_adaptive", {}), kw)


def render_aa_adaptive(cam, metric, opts, adaptive, disk=None, background_lo=None, background_hi=None,
                       want=("rgb", "rgba", "cover", "level")):
    """Host-pointer adaptively supersampled frame (lt_render_aa_adaptive): adaptive.samples_lo^2 rays for every pixel,
    adaptive.samples_hi^2 for the pixels on an edge.  background_lo / background_hi: the images at the two fine sizes,
    (H * samples_lo, W * samples_lo[, 3]) and (H * samples_hi, W * samples_hi[, 3]), or both None.  Returns 'rgb',
    'rgba', 'cover' as render_aa, 'level' (H, W) uint8 (the samples per axis each pixel got) and 'stats' with
    'refined', the number of refined pixels."""
    rows = _frame_rows(cam, opts)
    if (background_lo is None) != (background_hi is None):
        raise ValueError("background_lo and background_hi are both None or both given")
    bg_lo, nch, gray = _fine_background(cam, int(adaptive.samples_lo), background_lo)
    bg_hi, nch_hi, gray_hi = _fine_background(cam, int(adaptive.samples_hi), background_hi)
    if (nch, gray) != (nch_hi, gray_hi):
        raise ValueError("background_lo and background_hi differ in their channels")
    out, st = _aa_render(load().lt_render_aa_adaptive, cam, metric, opts, adaptive, disk, rows, [bg_lo, bg_hi], nch, gray,
                         want, {"cover": (4,), "level": ()})
    out["stats"]["refined"] = int(st.counters[STAT_AA_REFINED])
    return out


def render_aa_adaptive_dev(cam, metric, opts, adaptive, disk=None, d_bg_lo=0, d_bg_hi=0, bg_channels=3, d_rgb=0, d_rgba=0,
                           d_cover=0, d_level=0, d_stats=0):
    """Device-pointer form of render_aa_adaptive (lt_render_aa_adaptive_dev); pointers are integers, 0 = NULL.  Waits
    for opts.stream once, between the two passes."""
    _check(load().lt_render_aa_adaptive_dev(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(adaptive),
                                            None if disk is None else C.byref(disk), _p(d_bg_lo), _p(d_bg_hi), bg_channels,
                                            _p(d_rgb), _p(d_rgba), _p(d_cover), _p(d_level), _p(d_stats)))


def aa_adaptive_plan(cam, metric, opts, adaptive, disk=None):
    """(bytes of ray records the base pass's largest band needs, refined pixels per chunk) of a render_aa_adaptive call
    (lt_aa_adaptive_plan; host arithmetic, no GPU needed); raises with the call's refusals."""
    nbytes, chunk = C.c_int64(), C.c_int64()
    _check(load().lt_aa_adaptive_plan(C.byref(cam), C.byref(metric), C.byref(opts), C.byref(adaptive),
                                      None if disk is None else C.byref(disk), C.byref(nbytes), C.byref(chunk)))
    return int(nbytes.value), int(chunk.value)
