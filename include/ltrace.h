/*
 * include/ltrace.h -- C-ABI of libltrace_hip.so, the MI355X (gfx950) null-geodesic
 * ray-tracing library.
 *
 * This is the drop-in boundary for the per-pixel backward light-ray integrator of
 * dhg14n9/Light-path-tracer.  Plain pointers and sizes only; no torch / numpy types.
 * Every entry point names the reference interface it replaces (file:line in the
 * reference tree).  The library is HIP-only: with no usable GPU every compute entry
 * point returns LT_ERR_NO_DEVICE -- there is no CPU fallback.
 *
 * Return convention: 0 on success, a negative LT_ERR_* code otherwise;
 * lt_last_error() returns a thread-local message for the most recent failure.
 */
#ifndef LTRACE_H
#define LTRACE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LT_VERSION 200 /* 0.2.0: lt_stats grew to 16 counters; per-stream workspaces; lt_render_multi */

#define LT_OK 0
#define LT_ERR_INVALID_ARG (-1)
#define LT_ERR_HIP (-2)
#define LT_ERR_NO_DEVICE (-3)
#define LT_ERR_UNSUPPORTED (-4)

/* metric kinds: metrics.py:735 (Schwarzschild), :840 (Kerr) */
#define LT_METRIC_SCHWARZSCHILD 0
#define LT_METRIC_KERR 1

/* integrators: metrics.py:419-567 (DP45, the reference's production Kerr path, float64 only)
 *              metrics.py:570-658 (radius-banded fixed-step RK4; float32 or float64)
 * Schwarzschild always uses its orbit-equation RK4, metrics.py:49-117. */
#define LT_INTEGRATOR_DP45 0
#define LT_INTEGRATOR_RK4 1
#define LT_INTEGRATOR_DP45_EXACT 2 /* DP45 with the step-size controller evaluated in float64, operation by operation as
                                      metrics.py:506-522, :560-564 write it (LT_INTEGRATOR_DP45 evaluates it in float32, free
                                      of divisions and pow).  Divisions and the power are ~1-ulp reciprocal / Newton forms, not
                                      IEEE library calls: an accept / reject decision can differ from the reference's only
                                      when err_norm is within a few ulp of 1 (measured: no golden ray) */

/* ray -> lane scheduling of the integrate kernel */
#define LT_SCHED_DIRECT 0 /* one work-item per ray, one 8x8 pixel tile per wavefront        */
#define LT_SCHED_QUEUE 1  /* persistent wavefronts, ray queue, ballot/prefix-sum lane refill */

/* per-ray status, as the reference's integrators return it (metrics.py:69, :125) */
#define LT_STATUS_ESCAPED 1
#define LT_STATUS_CAPTURED (-1)
#define LT_STATUS_INVALID 0
#define LT_STATUS_DISK 2 /* lt_render_disk / lt_trace_batch_kerr_disk only: the ray ended on the accretion disk */

/* Pinhole camera of image_lens.py:133-152 / :193-208 (pixel corners, no +0.5).
 * psi = (pitch_up, yaw_right) BH offset in radians, image_lens.py:21-61. */
typedef struct lt_camera {
    int32_t width, height;
    double hfov, vfov;
    double psi_y, psi_x;
    double r_obs;     /* observer radius (in the same units as M) */
    double theta_obs; /* observer inclination; the reference only ever uses pi/2 */
} lt_camera;

typedef struct lt_metric {
    int32_t kind; /* LT_METRIC_* */
    int32_t reserved;
    double M;
    double a; /* spin, |a| <= M; ignored for Schwarzschild */
} lt_metric;

typedef struct lt_opts {
    int32_t integrator;      /* LT_INTEGRATOR_*; Kerr only */
    int32_t precision;       /* 32 or 64: arithmetic of the integrate kernel */
    int32_t schedule;        /* LT_SCHED_* */
    int32_t tb_symmetry;     /* 0 = trace every row; 1 = reference behaviour incl. its
                                off-by-one mirror (image_lens.py:218-220, :272-276) */
    int32_t loop_around;     /* render_loop_around of image_lens.py:296-298 */
    int32_t row_block;       /* rows per block of the block-cyclic row partition (>0) */
    int32_t n_parts;         /* number of partitions (GPUs); 1 = whole frame */
    int32_t part;            /* this call renders blocks b with b % n_parts == part */
    double axis_refine_frac; /* Y_AXIS_REFINE_FRAC = 0.07, image_lens.py:14 */
    double phi_max;          /* Schwarzschild: 50.0 (metrics.py:833) */
    double h_max;            /* Schwarzschild: 0.05 (metrics.py:833); Kerr RK4: 1.0 (metrics.py:677) */
    void *stream;            /* hipStream_t to launch on; NULL = the default stream */
    int32_t timing;          /* !=0: bracket each kernel with HIP events (lt_timing_collect) */
    int32_t bg_sampling;     /* LT_BG_*: how the epilogue reads the background image */
    const uint16_t *block_owner; /* NULL: row block b belongs to partition b % n_parts (block-cyclic).  Else a HOST
                                array of n_blocks = ceil(height / row_block) entries, block_owner[b] in [0, n_parts):
                                any assignment of row blocks to partitions (e.g. cost-weighted from the previous
                                frame's step counts, sharding.balance_blocks).  A partition's local rows are its
                                blocks in ascending order.  Read during the call only. */
    int32_t n_blocks;        /* entries of block_owner (checked against the frame) */
    int32_t reserved;
} lt_opts;

/* background sampling of the epilogue kernel (same texels, bit-identical images) */
#define LT_BG_LDS_TILES 0 /* source bounding box of each 256-pixel group staged in LDS by coalesced row reads;
                             groups whose box does not fit (strong lensing) use the global gather */
#define LT_BG_GLOBAL 1    /* one global nearest-neighbour read per pixel */

/* Counters produced by the epilogue kernel (one 64-bit word each, device or host). */
#define LT_STAT_RAYS 0      /* rays integrated */
#define LT_STAT_STEPS 1     /* sum over rays of integrator steps (RK4 steps / DP45 attempts) */
#define LT_STAT_RHS_EVALS 2 /* sum over rays of right-hand-side evaluations */
#define LT_STAT_ESCAPED 3
#define LT_STAT_CAPTURED 4
#define LT_STAT_INVALID 5
/* Produced by the integrate kernel itself (Kerr; zero for Schwarzschild): the work it issued and the
 * clock the chip held while it ran.  bench.py prices its executed-instruction roofline in these. */
#define LT_STAT_WAVE_ITERS 6 /* sum over wavefronts of integrator loop iterations the wavefront issued */
#define LT_STAT_WAVES 7      /* wavefronts of the integrate kernel                                     */
#define LT_STAT_CLK_CYCLES 8 /* shader-clock cycles (s_memtime) over the lifetime of every 64th wave   */
#define LT_STAT_CLK_TICKS 9  /* 100 MHz real-time ticks (s_memrealtime) over the same lifetimes        */
#define LT_STAT_BG_TILES_LDS 10    /* epilogue, lensed background: 256-pixel groups whose source texels were staged in LDS */
#define LT_STAT_BG_TILES_GLOBAL 11 /* ... and groups that fell back to the per-pixel global gather                  */
#define LT_STAT_DISK 12            /* lt_render_disk_dev: rays that ended on the accretion disk                        */
                                   /* (lt_render_disk_images_dev: rays with at least one hit)                          */
#define LT_STAT_DISK_HITS 13       /* lt_render_disk_images_dev: hits of the optically thin disk, all rays              */
#define LT_STAT_AA_REFINED 14      /* lt_render_aa_adaptive_dev: pixels that were refined (traced at samples_hi)         */
#define LT_STAT_EQ_ITERS 15        /* integrate kernel, float32 RK4: those of LT_STAT_WAVE_ITERS that the far-field streak took in its
                                      fixed-quadrant loop (lt_set_eq_streak); the only counter the switch changes               */
#define LT_STAT_WORDS 16

typedef struct lt_stats {
    uint64_t counters[LT_STAT_WORDS];
    double prologue_ms, integrate_ms, epilogue_ms; /* HIP-event times of the three kernels */
} lt_stats;

/* ---- library / device ------------------------------------------------------------- */
int lt_version(void);
/* Hash of the kernel sources and compiler flags this binary was built from (set by the build script);
 * profiles under profiles/ carry it so that a figure measured on another build is never reused. */
const char *lt_build_id(void);
const char *lt_last_error(void);
int lt_device_count(void);
int lt_set_device(int device);
/* Frees workspaces, staging buffers and events created lazily by the calls below.
 *
 * Concurrency contract.  Everything the library allocates on a caller's behalf -- the ray records of
 * lt_render_dev, the device-side outputs and the pinned staging of lt_render and of the batch twins --
 * is owned per (device, stream): calls on DIFFERENT streams of a device never share memory and may be
 * in flight at the same time; calls on the SAME stream are ordered by the stream.  The host-pointer
 * entry points (lt_render, lt_trace_batch_*, lt_integrate_dense ...) are synchronous and must not be
 * entered from two host threads with the same stream at once.  The batch twins always use the default
 * (NULL) stream, like the reference's synchronous calls.  Buffers grow to the largest frame seen and are
 * then reused: nothing is allocated per call. */
int lt_shutdown(void);
/* Frees what the library holds for (current device, stream) after draining the stream: call it before destroying
 * a stream that was used with the library (otherwise its buffers stay until lt_shutdown). */
int lt_release_stream(void *stream);
void lt_default_opts(lt_opts *o);

/* ---- array-in / array-out twins of the reference batch drivers ---------------------- *
 * HOST pointers; the library stages H2D / D2H itself.  Same meaning as the reference:   *
 * out_fa[i] = final_alpha if the ray escaped else NaN; out_w[i] = number of half orbits. */

/* Replaces Schwarzschild.trace_rays_batch (metrics.py:831-833) ->
 * _trace_rays_batch_schwarzschild (metrics.py:661-668).  precision 32 or 64.
 * out_status / out_rhs_evals (4 per RK4 step) may be NULL. */
int lt_trace_batch_schw(double M, double r_obs, const double *alphas, int64_t n, double phi_max,
                        double h_max, int precision, double *out_fa, int64_t *out_w,
                        int8_t *out_status, uint32_t *out_rhs_evals);

/* Replaces Kerr.trace_rays_batch (metrics.py:1128-1132) -> _trace_rays_batch_kerr
 * (metrics.py:671-679).  integrator LT_INTEGRATOR_*, precision 32 or 64 (DP45: 64 only).
 * axis_refines: one byte per ray (numpy bool), may be NULL (= all false).
 * out_status / out_rhs_evals may be NULL. */
int lt_trace_batch_kerr(double M, double a, double r_obs, const double *alphas, const double *thetas,
                        double theta_obs, double lambda_max, const uint8_t *axis_refines,
                        int integrator, int precision, int schedule, int64_t n, double *out_fa,
                        int64_t *out_w, int8_t *out_status, uint32_t *out_rhs_evals);

/* Device probe for the tests: lt_trace_batch_kerr with the fixed-step RK4 integrator, every ray traced by the general
 * iteration alone (the far-field streak is never entered, no ghost lanes).  The streak takes the same steps by the same
 * arithmetic, so lt_trace_batch_kerr must agree with this bit for bit, in the evaluation counts too. */
int lt_trace_batch_kerr_general_probe(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                      double theta_obs, double lambda_max, const uint8_t *axis_refines, int precision,
                                      int64_t n, double *out_fa, int64_t *out_w, int8_t *out_status,
                                      uint32_t *out_rhs_evals);

/* The float32 far-field streak's fixed-quadrant loop: on != 0 enables it, 0 disables it, for every Kerr
 * launch enqueued afterwards (the default: on, or LT_EQ_STREAK=0/1 in the environment when the library is loaded).  It
 * changes no output and no counter but LT_STAT_EQ_ITERS.  Returns the previous setting. */
int lt_set_eq_streak(int on);

/* The unit-step form of that loop, taken by a wavefront whose rays all step by exactly 1 and are far from
 * the end of the affine range: on != 0 enables it, 0 disables it, for every Kerr launch enqueued afterwards (the default:
 * on, or LT_UNIT_STREAK=0/1 in the environment when the library is loaded).  It changes no output and no counter.
 * Returns the previous setting. */
int lt_set_unit_streak(int on);

/* The tail split of the frame path: a Kerr frame of the direct schedule integrates the last tile rows of
 * its tile queue with a launch of its own on a side stream of the library's, which takes the wave slots the main launch
 * leaves free while it runs dry; the rows above are shaded while that second launch ends.  tile_rows: -1 an automatic
 * size (about one fill of the device's wave slots; frames too short for it are not split), 0 off, n > 0 that many tile
 * rows (8 pixel rows each), at most what lies below the frame's hot rectangle.  For every frame enqueued afterwards; the
 * default is -1, or LT_TAIL_SPLIT in the environment when the library is loaded.  Frames with a disk, supersampling,
 * tb_symmetry, the queue schedule, the Schwarzschild metric or LT_BG_LDS_TILES with a background, and frames on a stream
 * that is being captured, are never split.  It changes no output and no counter; with opts->timing the integrate time of
 * a split frame includes the shading that overlaps it.  Everything is joined back into opts->stream before the call
 * returns.  Returns the previous setting. */
int lt_set_tail_split(int tile_rows);

/* *split = frames that were split that way, *whole = frames of lt_render_dev and its relatives that were not, both since
 * the library was loaded, over all devices and streams; either may be NULL.  Needs no device. */
void lt_tail_split_counts(uint64_t *split, uint64_t *whole);

/* Where the tail split cuts a frame of tiles_x x tiles_y tiles (8 x 8 pixels) whose tile queue begins with the strip of
 * tile columns [strip_x0, strip_x1) and a hot rectangle that ends above tile row hot_y1 (0: none), on a device of `slots`
 * wave slots, for the setting `request` (lt_set_tail_split): *ty_split = the first tile row and *pos_split = the first
 * queue position of the second part (tiles_y and tiles_x * tiles_y where the frame is not split).  Returns 1 if the frame
 * is split, 0 if not, -1 on arguments that describe no frame.  Host arithmetic only (test probe). */
int lt_tail_split_plan(int32_t tiles_x, int32_t tiles_y, int32_t strip_x0, int32_t strip_x1, int32_t hot_y1, int32_t slots,
                       int32_t request, int32_t *ty_split, int64_t *pos_split);

/* Device probe of the float32 sincos for the tests: every float32 x with bit pattern in [bits_lo, bits_hi] goes through
 * the general form and through the fixed-quadrant form.  out[0] = values compared, out[1] = values for which either
 * result differs in any bit, out[2] = values that do not reduce to the quadrant k = 1, out[3] = bit pattern of the
 * first (lowest) x that differs.  band[0..1] = the band (lo, hi) the streak uses. */
int lt_sincos_q1_probe(uint32_t bits_lo, uint32_t bits_hi, uint64_t out[4], float band[2]);

/* Device probe of the inlined Kerr right-hand side (metrics.py:221-303) for parity tests:
 * states (n,5) [r, theta, phi, p_r, p_theta], p_phi (n), out (n,5); host pointers, float64 I/O,
 * evaluated in float32 or float64 on the GPU. */
int lt_kerr_rhs_probe(double M, double a, const double *states, const double *p_phi, int64_t n,
                      int precision, double *out);

/* The same right-hand side in each form the RK4 steps evaluate it in.  form 0: checked (lt_kerr_rhs_probe), 1: without
 * the r <= r_cut handling, 2: the packed lone-wave form, 3: the packed form in the shape of a step's last stage, its
 * three velocities rebuilt from the factors it hands out (2, 3: float32 only).  All four agree bit for bit for r > r_cut. */
int lt_kerr_rhs_form_probe(double M, double a, const double *states, const double *p_phi, int64_t n, int precision,
                           int form, double *out);

/* Device probe of one RK4 step (metrics.py:306-323) per state: states (n,5), p_phi (n), refine (n) (axis-refine flag of
 * the ray), h (n) the step sizes; out_states (n,5).  form 0: the checked step, 1: the branch-free step, 2: its
 * fixed-quadrant form (valid for a polar angle inside the streak's band, lt_sincos_q1_probe), 3: the packed lone-wave step
 * (2, 3: float32 only).  out_min_r / out_max_d (n): the smallest stage radius and largest stage angle offset that forms
 * 1..3 report (the step is valid iff min_r > 1.001 r_plus and max_d <= 0.25; NaN for form 0).  out_cs (n,2), may be NULL:
 * the [cos, sin] of the new polar angle that form 3 hands to the next step (NaN otherwise). */
int lt_kerr_step_probe(double M, double a, const double *states, const double *p_phi, const uint8_t *refine,
                       const double *h, int64_t n, int precision, int form, double *out_states, double *out_min_r,
                       double *out_max_d, double *out_cs);

/* ---- the float64 DP45 integrator block by block (parity probes; they call the functions the integrate kernels call) ---- *
 * Common inputs: the metric (M, a), the observer radius (r_escape = 2 r_obs) and lambda_max; per row: states (n,5), p_phi (n),
 * refine (n) the ray's axis-refine flag (tolerances 1e-10 / 1e-8 in place of 1e-8 / 1e-6), k1 (n,5) the carried derivative
 * and sc0 (n,2) the carried [sin, cos] of the polar angle -- either may be NULL: computed from the state as at a ray's start --
 * and h (n) the step size.  exact != 0: the controller of LT_INTEGRATOR_DP45_EXACT. */

/* One step attempt per row, checked != 0 in the form with the in-line r <= r_cut and |dtheta| > 0.25 handling, else in the
 * branch-free form.  out_next, out_k7 (n,5): the candidate state and its derivative; out_sc (n,2): [sin, cos] of its polar
 * angle; out_err_sq (n): the squared error norm (err_norm = sqrt(err_sq / 5)); out_min_r, out_max_d (n): the smallest stage
 * radius and the largest stage angle offset the branch-free form reports (stages only, the candidate's own turn not counted; it is valid iff min_r > 1.001 r_plus and
 * max_d <= 0.25; NaN for the checked form). */
int lt_dp45_attempt_probe(double M, double a, double r_obs, double lambda_max, const double *states, const double *p_phi,
                          const uint8_t *refine, const double *k1, const double *sc0, const double *h, int64_t n, int exact,
                          int checked, double *out_next, double *out_k7, double *out_sc, double *out_err_sq,
                          double *out_min_r, double *out_max_d);

/* Up to n_attempts iterations of the loop body metrics.py:454-564 per row, ending at the first that ends the ray.  lam (n)
 * and steps (n) (attempts made so far), NULL: zeros.  Rows 64 b ... 64 b + 63 share a wavefront.  out_states, out_k1 (n,5);
 * out_misc (n,4): sin, cos of the polar angle as carried, lam, h; out_int (n,3): the event (4 still running, 2 out of range
 * or attempts, 0 invalid, -1 captured, 1 escaped), steps, attempts made by this call. */
int lt_dp45_advance_probe(double M, double a, double r_obs, double lambda_max, const double *states, const double *p_phi,
                          const uint8_t *refine, const double *k1, const double *sc0, const double *h, const double *lam,
                          const uint32_t *steps, int64_t n, int exact, int n_attempts, double *out_states, double *out_k1,
                          double *out_misc, int32_t *out_int);

/* The step-size controller alone (the function advance() calls) on any (err_sq, h): out_reject (n) 1 where the attempt is
 * rejected, out_h (n) the step size the loop goes on with (metrics.py:514-522, :560-564). */
int lt_dp45_controller_probe(int exact, const double *err_sq, const double *h, int64_t n, uint8_t *out_reject, double *out_h);

/* ---- a ray's two ends and the RK4 loop body (parity probes; they run the kernels and functions the product runs) ---- */

/* The ray records of k_prologue_arrays as stored, for kind LT_METRIC_KERR (alphas, thetas (n)) or LT_METRIC_SCHWARZSCHILD
 * (alphas; thetas may be NULL), refines (n) or NULL.  out_records (n_q,4) float64, n_q = n rounded up to a multiple of 64:
 * the record of precision 32 / 64 widened -- p_r, p_theta, p_phi, flags (Kerr) or w0, 0, 0, flags (Schwarzschild); flags
 * 1 the ray is valid, 2 axis-refine, 4 a padding row (every row from n on). */
int lt_ic_probe(int kind, double M, double a, double r_obs, double theta_obs, const double *alphas, const double *thetas,
                const uint8_t *refines, int64_t n, int precision, double *out_records);

/* Up to n_iters iterations of the fixed-step RK4 loop body (metrics.py:596-655, kerr_rk4_advance) per row, ending at the
 * first that ends the ray.  states (n,5), p_phi (n), refine (n); lam (n), h_retry (n) (> 0: the halved step size a failed
 * attempt left for the next iteration) and steps (n), NULL: zeros; h_max the base step.  One iteration is one step ATTEMPT:
 * a reference iteration whose step is halved k times takes k + 1 of them, and the row stands at a reference iteration
 * boundary where out h_retry == 0.  Rows 64 b ... 64 b + 63 share a wavefront.  out_states (n,5); out_misc (n,2): lam,
 * h_retry; out_int (n,3): the event (4 still running, 2 out of range, 0 invalid, -1 captured, 1 escaped), steps (attempts
 * so far), iterations made by this call. */
int lt_rk4_advance_probe(double M, double a, double r_obs, double lambda_max, double h_max, const double *states,
                         const double *p_phi, const uint8_t *refine, const double *lam, const double *h_retry,
                         const uint32_t *steps, int64_t n, int precision, int n_iters, double *out_states, double *out_misc,
                         int32_t *out_int);

/* The Schwarzschild integrator (metrics.py:66-117, schw_trace) from a supplied start (u0, w0) (n) instead of the observer's;
 * M, r_obs, phi_max and h_max become the kernel's constants exactly as for lt_trace_batch_schw (one step: phi_max = h_max).
 * out (n,3): u, w, phi_last (the part of the last, shorter or interrupted, step used); out_int (n,3): the event (-1, 1, or
 * 2 at the range end), steps taken (the ending one included: rhs_evals = 4 steps), full steps (phi_f = full steps * h_max +
 * phi_last).  out_n_full, out_h_last (may be NULL): the host's step plan for the call -- n_full steps of h_max, then one of
 * h_last if h_last > 0; they are set for n = 0 too, for which no device is needed. */
int lt_schw_trace_probe(double M, double r_obs, double phi_max, double h_max, const double *u0, const double *w0, int64_t n,
                        int precision, double *out, int32_t *out_int, uint32_t *out_n_full, double *out_h_last);

/* k_epilogue_arrays on final records in the integrate kernels' own layout, fin0, fin1 (n,4) float64, rounded to float32 on
 * the host first for precision 32:  Kerr fin0 = (r, theta, phi, p_r), fin1 = (p_theta, p_phi, event, steps);  Schwarzschild
 * fin0 = (u, w, phi_last, full steps), fin1 = (0, 0, event, steps), h_schw the step size the full steps are multiplied by.
 * event: -1 captured, 1 escaped, 2 range end, 0 invalid, 3 padding.  integrator sets the evaluation count per step
 * (LT_INTEGRATOR_*).  out_fa (n) NaN unless escaped, out_w (n), out_status (n), out_evals (n). */
int lt_extract_probe(int kind, double M, double a, double h_schw, int integrator, const double *fin0, const double *fin1,
                     int64_t n, int precision, double *out_fa, int64_t *out_w, int8_t *out_status, uint32_t *out_evals);

/* Accuracy sweep of a float32 math primitive of the integrators: every float32 with bit pattern in [bits_lo, bits_hi]
 * (at most 2^30 of them) goes through the primitive and through a float64 yardstick, compared on the device.
 *   which 0: sincos(x)        1: the small-angle sincos(d), |d| <= 0.25       (yardstick: the float64 sincos)
 *         2: the reciprocal of a positive normal x                             (yardstick: 1.0 / x)
 *         3: sin and cos of th0 + d rotated from the float32 (sin, cos)(th0), in the scalar and in the packed form, d
 *            swept, for each of the n_bases (1..16) angles th0 in `bases`; the yardstick is the float64 rotation of those
 *            float32 (sin, cos)(th0), so that the base's own rounding is not counted again.
 * out[13]: out[0] = values compared (which 3: per base), then five pairs (largest value as the bits of a double, the
 * argument that reached it, the lowest if several; which 3: base index << 32 | bits of d):
 *   out[1], out[2]: absolute error of the sine;  out[3], out[4]: of the cosine (which 2: unused);
 *   out[5], out[6]: error of the sine (which 2: of the reciprocal) in ulps of the true value;  out[7], out[8]: cosine;
 *   out[9], out[10] (which 3): the NUMBER of (base, d) for which scalar and packed form differ in a bit, and the first;
 *   out[11], out[12] (which 3): absolute error of either value against the float64 sincos of (double)th0 + d.
 *   which 4: z^(-1/10) of the float32 DP45 step controller (yardstick: the float64 pow(z, -0.1)).  out[1], out[2]: the
 *            largest relative error among the results that are positive and finite, and its argument; out[9], out[10]: the
 *            NUMBER of arguments whose result is not a positive finite number, and the first. */
int lt_math32_probe(int which, uint32_t bits_lo, uint32_t bits_hi, const float *bases, int n_bases, uint64_t *out);

/* The float64 primitives the yardsticks above and the float64 integrators are made of, values in and values out:
 * x (n), out (n,2).  which 0: sincos -> [sin, cos]; 1: small-angle sincos (|x| <= 0.25) -> [sin, cos]; 2: reciprocal of a
 * positive normal x -> [1/x, 0]; 3: x^(-1/5) of the step controllers, clamped outside [1e-6, 1e4] -> [value, 0];
 * 4: the FLOAT32 sincos of (float)x -> [sin, cos], for tests that need its values and not its error;
 * 5: the float32 controller's (float)x^(-1/10) -> [value, 0], whatever x is;
 * 6: the correctly rounded sincos of the prologue (angles of a few radians) -> [sin, cos]. */
int lt_math64_probe(int which, const double *x, int64_t n, double *out);

/* ---- the disk test block by block (parity probes; they call the functions the disk kernels call; the disk itself is     *
 * described under "thin Keplerian accretion disk" below).  r_in, r_out: the annulus, resolved and refused as a disk call   *
 * does it (r_in <= 0: the ISCO), then rounded to the precision computed in, as the integrate kernels get them. ---- */

/* The crossing of the plane on one step per row (disk_crossing): y0, y1 (n,5) the step's ends [r, theta, phi, p_r, p_theta],
 * p_phi (n), h (n) its length, t_end (n) the fraction of the step that is searched (1, or less where the step was cut at a
 * capture / escape radius).  out_found (n): 1 where the Hermite cubic of theta crosses pi/2 on [0, t_end] and the crossing
 * point lies in the annulus; out_hit (n,5): the crossing state (theta exactly pi/2 in the precision computed in) and out_tau
 * (n) the root, wherever the cubic crosses -- in the annulus or not -- and NaN elsewhere.  Float64 I/O. */
int lt_disk_crossing_probe(const lt_metric *metric, double r_in, double r_out, const double *y0, const double *y1,
                           const double *p_phi, const double *h, const double *t_end, int64_t n, int precision,
                           uint8_t *out_found, double *out_hit, double *out_tau);

/* One iteration of an integrator with the disk test behind it (disk_advance) per row: LT_INTEGRATOR_RK4 (precision 32, 64)
 * or LT_INTEGRATOR_DP45_EXACT (64).  states (n,5), p_phi (n), refine (n), steps (n) as for lt_rk4_advance_probe /
 * lt_dp45_advance_probe; aux (n,2): lam and h_retry (RK4), lam and h (DP45; its carried derivative and sincos are computed
 * from the state); act (n): 0 where the lane's hit is to be ignored.  Rows 64 b ... 64 b + 63 share a wavefront.
 * out_state (n,5), out_aux (n,2): the integrator's state after the iteration (a hit does not replace it here);
 * out_int (n,3): the event (5 where the row hit the disk, else the integrator's), steps, 1 if the row hit;
 * out_hit (n,5): the hit state; out_on (n,7): the step the hit lies on -- its end state (5), its length, the root.  NaN where
 * nothing was written (the root is written wherever the crossing was searched and the cubic crossed). */
int lt_disk_advance_probe(const lt_metric *metric, double r_obs, double lambda_max, double h_max, double r_in, double r_out,
                          int integrator, int precision, const double *states, const double *p_phi, const uint8_t *refine,
                          const double *aux, const uint32_t *steps, const uint8_t *act, int64_t n, double *out_state,
                          double *out_aux, int32_t *out_int, double *out_hit, double *out_on);

/* Up to `iters` iterations of the timed trace's lane (pol = 0: DiskTimedStep::advance of lt_trace_disk_hits; pol = 1:
 * DiskPolStep::advance of lt_trace_disk_pol) per row, by the calls the tile loop makes (begin_tile, bind, advance):
 * LT_INTEGRATOR_RK4 (32, 64), LT_INTEGRATOR_DP45 and LT_INTEGRATOR_DP45_EXACT (64).  A row leaves the loop at its first
 * event other than 4 (running).  Inputs as lt_disk_advance_probe, plus what a lane carries between iterations, so that N
 * calls of one iteration resume exactly: k1 (n,5) and sc0 (n,2), DP45's carried derivative and [sin, cos] (NULL: computed
 * from the state, as at a start; ignored by RK4); lane (n,5): t_hi, t_lo and the rates t', r', theta' at the state; lane_int
 * (n,2): 1 if the rates are set, the hits counted so far.
 * out_state (n,5), out_aux (n,2), out_k1 (n,5), out_sc (n,2) (NaN for RK4), out_lane (n,5), out_lane_int (n,2): the same after
 * the last iteration; out_int (n,3): the last event, steps, iterations run.  The records, slot-major as the kernels keep them
 * and NaN where nothing was stored: out_img (max_images, n, 2) (r, phi), out_tim (max_images, n), out_mom (max_images, n, 2)
 * (p_r, p_theta; NaN with pol = 0).  out_trace (iters, n, 7), may be NULL: after each iteration r, theta, p_r, p_theta, the
 * h counted (0 where the attempt added no time) and the dt added -- evaluated by the probe itself from the step's ends and the
 * lane's rates by the lane's own statements, and tied to the lane through out_lane's (t_hi, t_lo) -- and the hits counted so far; NaN for iterations a row did not run.  Every value
 * is the T computed, widened to float64. */
int lt_disk_timed_advance_probe(const lt_metric *metric, double r_obs, double lambda_max, double h_max, double r_in, double r_out,
                                int integrator, int precision, int pol, const double *states, const double *p_phi,
                                const uint8_t *refine, const double *aux, const uint32_t *steps, const uint8_t *act,
                                const double *k1, const double *sc0, const double *lane, const int32_t *lane_int, int64_t n,
                                int32_t max_images, int32_t iters, double *out_state, double *out_aux, double *out_k1,
                                double *out_sc, int32_t *out_int, double *out_lane, int32_t *out_lane_int, double *out_img,
                                double *out_tim, double *out_mom, double *out_trace);

/* The closed forms a hit goes through on its way to a pixel, as the disk epilogues state them.  in (n,4): r, phi (unwrapped),
 * xi, g_given.  out_f64 (n,5): g(r, xi), phi wrapped to [0, 2 pi), then the unclamped emission E (3) from the float32-rounded
 * (r, g) -- of g_given instead of g where g_given is not NaN; out_half (n): the half orbits of phi; out_f32 (n,4): the disk
 * colour of that float32 (r, g) with one channel, then with three.  r_in <= 0: the ISCO; q, exposure as lt_disk. */
int lt_disk_shade_probe(const lt_metric *metric, double r_in, double q, double exposure, const double *in, int64_t n,
                        double *out_f64, int64_t *out_half, float *out_f32);

/* ---- fused frame path ---------------------------------------------------------------- *
 * Replaces, in one call, build_alpha_lookup (image_lens.py:133-152),                     *
 * precompute_final_alpha_lookup / _2d (image_lens.py:155-178 / :185-280) and             *
 * render_lensed_image (image_lens.py:296-397) + the float->RGBA8 step of                 *
 * mpimg.imsave (image_lens.py:510).  Nothing per-ray crosses PCIe on the way in.         */

/* Number of image rows partition `part` of `n_parts` owns (block-cyclic, blocks of row_block). */
int64_t lt_local_rows(int32_t height, int32_t row_block, int32_t n_parts, int32_t part);
/* Global row index of local row `local_row` of that partition. */
int64_t lt_global_row(int64_t local_row, int32_t row_block, int32_t n_parts, int32_t part);

/* DEVICE pointers (any may be NULL = not wanted), sized for R = lt_local_rows(...) rows:
 *   d_bg     (H, W, bg_channels) float32 background, the FULL frame on every partition
 *            (NULL: shadow render, escaped pixels white);  bg_channels 1 or 3
 *   d_fa     (R, W) float32 final_alpha lookup (NaN unless escaped)
 *   d_w      (R, W) uint16 winding lookup
 *   d_status (R, W) int8
 *   d_steps  (R, W) uint32 integrator steps of the ray
 *   d_rgb    (R, W, bg_channels or 3) float32 lensed image, as render_lensed_image returns it
 *   d_rgba   (R, W, 4) uint8, as imsave writes it
 *   d_stats  LT_STAT_WORDS uint64 counters, ACCUMULATED into (caller zeroes)
 * Asynchronous on opts->stream. */
int lt_render_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts,
                  const float *d_bg, int32_t bg_channels, float *d_fa, uint16_t *d_w,
                  int8_t *d_status, uint32_t *d_steps, float *d_rgb, uint8_t *d_rgba,
                  uint64_t *d_stats);

/* Same with HOST pointers (stages the background H2D, results D2H, synchronises); stats may be NULL.
 * Device-side buffers persist per (device, stream).  Every output is copied straight into the caller's memory:
 * into a block from lt_host_alloc (or other pinned / registered host memory) by DMA at PCIe rate; into pageable
 * memory through the HIP runtime, which pins the pages on the fly (about 10x slower the first time a buffer is
 * used, PCIe rate when the same buffer is passed again). */
int lt_render(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts,
              const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w,
              int8_t *out_status, uint32_t *out_steps, float *out_rgb, uint8_t *out_rgba,
              lt_stats *stats);

/* Pinned host memory for the outputs of the host-pointer entry points (NULL on failure, see
 * lt_last_error); ltrace.py hands such blocks out as numpy arrays. */
void *lt_host_alloc(size_t bytes);
int lt_host_free(void *p);

/* One frame on several GPUs of this node from ONE process (SURVEY 8b `lt_render_multi`): partition p of
 * n_gpus (block-cyclic rows, opts->row_block; opts->n_parts / part / stream are ignored) is rendered on
 * device devices[p] (NULL: device p), all partitions concurrently, and every device copies its rows
 * straight into the caller's full-frame HOST arrays -- no device-to-device gather.  `devices` may name
 * one device several times (partitions then queue on it).  Outputs as lt_render, sized for the FULL
 * (H, W) frame; stats sums the counters and takes the slowest device's kernel times.
 * The RCCL gather of the north-star contract is the multi-process path (sharding.FrameGather / bench.py). */
int lt_render_multi(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, int32_t n_gpus,
                    const int32_t *devices, const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w,
                    int8_t *out_status, uint32_t *out_steps, float *out_rgb, uint8_t *out_rgba, lt_stats *stats);

/* ---- the first and the last stage on their own (HOST pointers) ------------------------------ *
 * The reference's pipeline is three calls; lt_render fuses them, these keep each call a GPU twin. */

/* Replaces build_alpha_lookup (image_lens.py:133-152) and the theta / axis-refine-column part of
 * precompute_final_alpha_lookup_2d (image_lens.py:193-216).  Any output may be NULL:
 * out_alpha (H, W) float32, out_theta (H, W) float64, out_axis_cols (W) bytes. */
int lt_pixel_angles(const lt_camera *cam, double axis_refine_frac, float *out_alpha, double *out_theta,
                    uint8_t *out_axis_cols);

/* Replaces render_lensed_image (image_lens.py:296-397) for caller-supplied lookups (+ imsave's RGBA8):
 * bg (H, W, bg_channels) float32, fa (H, W) float32, winding (H, W) uint16 or NULL;
 * out_rgb (H, W, bg_channels) float32 and / or out_rgba (H, W, 4) uint8. */
int lt_shade(const lt_camera *cam, int32_t loop_around, const float *bg, int32_t bg_channels, const float *fa,
             const uint16_t *winding, float *out_rgb, uint8_t *out_rgba);

/* Scatter a partition's (R, W, elem_bytes) rows into the full (H, W, elem_bytes) frame
 * (device pointers, async on `stream`): the un-permute step after the multi-GPU gather. */
int lt_scatter_rows_dev(const void *d_part, void *d_full, int32_t height, int32_t width,
                        int32_t elem_bytes, int32_t row_block, int32_t n_parts, int32_t part,
                        void *stream);

/* The same for ANY assignment of rows (e.g. the frame as rank 0 received it, partition after partition, under a
 * row-block -> rank table): d_rows holds n_rows rows of row_bytes bytes, source row i goes to row d_row_index[i] of
 * d_full (height rows).  d_row_index is a DEVICE array of n_rows int64; entries outside [0, height) are skipped.
 * One launch per 65535 rows, asynchronous on `stream`. */
int lt_scatter_rows_indexed_dev(const void *d_rows, void *d_full, const int64_t *d_row_index, int64_t n_rows,
                                int64_t height, int64_t row_bytes, void *stream);

/* ---- batched dense trajectories ------------------------------------------------------------- *
 * Replaces geodesic_tracer.integrate_geodesic (geodesic_tracer.py:22-71) -- solve_ivp(RK45) on     *
 * metric.geodesic_equations (metrics.py:763-790 / :946-1029) with a capture and an escape radius   *
 * event -- for n 8-D initial states (t, r, theta, phi, p_t, p_r, p_theta, p_phi) at once, as      *
 * metric.initial_conditions returns them (metrics.py:792-808 / :1032-1107).  float64.              */
typedef struct lt_dense_opts {
    double lambda_max;   /* affine range, geodesic_tracer.py:22 (1000)                                  */
    double r_stop_inner; /* < 0: the metric's capture radius 1.01 r_plus (geodesic_tracer.py:43-44)     */
    double r_stop_outer; /* < 0: twice each track's start radius (geodesic_tracer.py:45-46)             */
    double rtol, atol;   /* geodesic_tracer.py:64-65 (1e-8, 1e-10)                                      */
    double max_step;     /* geodesic_tracer.py:63 (1.0)                                                 */
    int64_t max_points;  /* record capacity per track (>= 2)                                            */
    int32_t max_attempts; /* guard against a track that never ends (status -2); solve_ivp has none      */
    int32_t length_binning; /* order of the launch, never of the output: 1 = predict every track's length with a cheap
                               loose-tolerance pass and launch the tracks of every window of 2048 longest first, so that
                               the 64 tracks of a wavefront end together (records are byte-identical either way); -1 = caller order;
                               0 = automatic (binned when the batch is at least twice what the chip holds at once) */
    void *stream;        /* hipStream_t; NULL = the default stream                                      */
} lt_dense_opts;
void lt_default_dense_opts(lt_dense_opts *o);

/* Track status: which of solve_ivp's endings the track took. */
#define LT_TRACK_RANGE_END 0   /* lambda_max reached (solve_ivp status 0)        */
#define LT_TRACK_CAPTURE_EVENT 1 /* r fell through r_stop_inner (status 1, event 0) */
#define LT_TRACK_ESCAPE_EVENT 2  /* r rose through r_stop_outer (status 1, event 1) */
#define LT_TRACK_FAILED (-1)     /* step size underflow (solve_ivp status -1)       */
#define LT_TRACK_ATTEMPT_LIMIT (-2)

/* HOST pointers.  state0 (n, 8).  Records are track-major, the reference's solution.t / solution.y per track:
 *   out_t (n, max_points), out_y (n, max_points, 8): track i's k-th point is out_t[i*max_points + k],
 *   out_y[(i*max_points + k)*8 + c] -- solution.t[k], solution.y[c, k].  (Version 100 wrote them point-major.)
 *   A track that ended on a radius event and whose record has room holds ONE more value, out_t[i*max_points + count]:
 *   the affine parameter at which the step containing the event would have ended (solve_ivp's `solution.sol` interpolates
 *   the last stretch with the dense output of that whole step; geodesic_tracer.Track.sol rebuilds it from this).
 *   out_count (n): points of the complete record.  If it exceeds max_points only the first
 *   max_points - 1 points are kept and the last slot holds the final point.
 *   out_status (n): LT_TRACK_*.   out_nfev (n): right-hand-side evaluations (solution.nfev). */
int lt_integrate_dense(const lt_metric *metric, const lt_dense_opts *opts, const double *state0, int64_t n,
                       double *out_t, double *out_y, int32_t *out_count, int8_t *out_status, int32_t *out_nfev);
/* Same with DEVICE pointers, asynchronous on opts->stream. */
int lt_integrate_dense_dev(const lt_metric *metric, const lt_dense_opts *opts, const double *d_state0, int64_t n,
                           double *d_out_t, double *d_out_y, int32_t *d_out_count, int8_t *d_out_status,
                           int32_t *d_out_nfev);
/* Diagnostic: the keys the length-binned launch orders the tracks by -- predicted step attempts of each track,
 * clamped to 2047 -- from the loose-tolerance predictor pass alone.  HOST pointers, out_key (n) uint16. */
int lt_dense_predict_lengths(const lt_metric *metric, const lt_dense_opts *opts, const double *state0, int64_t n,
                             uint16_t *out_key);
/* Device probe of the 8-D right-hand side for parity tests: states (n, 8) -> out (n, 8), host pointers. */
int lt_rhs8_probe(const lt_metric *metric, const double *states, int64_t n, double *out);

/* ---- thin Keplerian accretion disk ------------------------------------------------------------------- *
 * The frame of lt_render with a geometrically thin, optically thick disk in the equatorial plane theta = pi/2,   *
 * r_in <= r <= r_out.  Kerr only (a Schwarzschild hole is Kerr with a = 0).                                      *
 *                                                                                                               *
 * Material moves on circular equatorial geodesics orbiting in +phi (prograde for a > 0, retrograde for a < 0):   *
 *   Omega = sqrt(M) / (r^(3/2) + a sqrt(M)),                                                                     *
 *   u^t   = (r^(3/2) + a sqrt(M)) / (r^(3/4) sqrt(r^(3/2) - 3 M r^(1/2) + 2 a sqrt(M)))   (signed a).            *
 * r_in <= 0 means the ISCO of that orbit direction (Bardeen-Press-Teukolsky, lt_kerr_isco); otherwise the call  *
 * requires r_isco <= r_in < r_out < r_obs (LT_ERR_INVALID_ARG).                                                  *
 *                                                                                                               *
 * Hit: backward from the camera, the first strict sign change of theta - pi/2 between two consecutive accepted  *
 * states of the integrator whose crossing point has r_in <= r <= r_out.  Landing exactly on pi/2 from off the    *
 * plane counts as a crossing; a ray that lies in the plane (p_theta = 0) never hits; crossings outside the       *
 * annulus do not stop the ray.  The crossing point is the root of theta = pi/2 on the cubic Hermite interpolant  *
 * of the step in lambda (derivatives from the Kerr right-hand side at both ends); r, phi and the momenta are    *
 * interpolated on the same cubic.  A step that both crosses the disk and ends the ray by capture or escape is     *
 * tested between the previous state and the step's terminal (interpolated) state: the sign change is looked for  *
 * between those two, the crossing point is the root on the cubic of the FULL step (under DP45 the full step is   *
 * retaken as one RK4 step of the same length: DP45's own end state is gone by then), and the disk wins if the    *
 * root lies at or before the fraction of the step at which the ray ended: the capture / escape radius on the     *
 * chord in r of that full step (under DP45 the retaken step's chord, within the step's error of DP45's own).     *
 * The ray then ends with status LT_STATUS_DISK.                                                                  *
 *                                                                                                               *
 * Redshift: the camera's ray has E = -p_t = 1 and xi = p_phi; it stands for the photon the camera receives (the   *
 * convention of the background lookup), so g = nu_obs / nu_em = 1 / (u^t (1 - Omega xi)), in float64.           *
 * Shading, from the float32 (r_hit, g) of the disk output:                                                      *
 *   I = exposure g^4 (r_in / r)^q,  s = g (r_in / r)^(3/4),                                                      *
 *   ramp(s) = (clamp(2s, 0, 1), clamp(2s - 0.5, 0, 1), clamp(2s - 1, 0, 1)),  rgb = clamp(I ramp(s), 0, 1);      *
 * with a 1-channel background the disk value is the mean of the three.  Disk pixels occlude the background; every *
 * other pixel is exactly lt_render's pixel of the same camera with tb_symmetry = 0.                             */
typedef struct lt_disk {
    double r_in;     /* <= 0: the ISCO                  */
    double r_out;    /* 20                              */
    double q;        /* emissivity index, 3             */
    double exposure; /* 1                               */
    int32_t flags, reserved; /* 0 */
} lt_disk;
void lt_default_disk(lt_disk *d);
/* ISCO radius of the circular equatorial orbit in +phi (prograde for a > 0); host only, works without a GPU.
 * NaN unless M > 0 and |a| <= M. */
double lt_kerr_isco(double M, double a);

/* lt_render_dev with the disk.  Outputs as there, plus
 *   d_disk (R, W, 3) float32 (r_hit, phi_hit in [0, 2 pi), g), NaN where the ray missed the disk.
 * Disk pixels: fa = NaN, winding = half orbits up to the hit, status = LT_STATUS_DISK.  Stats also count
 * LT_STAT_DISK.  Partitions (n_parts, part, block_owner) as in lt_render_dev; tb_symmetry is ignored (every row is
 * traced).  LT_ERR_UNSUPPORTED for LT_METRIC_SCHWARZSCHILD and for LT_SCHED_QUEUE. */
int lt_render_disk_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                       const float *d_bg, int32_t bg_channels, float *d_fa, uint16_t *d_w, int8_t *d_status,
                       uint32_t *d_steps, float *d_disk, float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats);
/* The same with HOST pointers, staged like lt_render. */
int lt_render_disk(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                   const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w, int8_t *out_status,
                   uint32_t *out_steps, float *out_disk, float *out_rgb, uint8_t *out_rgba, lt_stats *stats);
/* lt_trace_batch_kerr with the disk (direct schedule): out_disk (n, 3) float64 (r_hit, phi_hit, g), NaN off the
 * disk; out_status LT_STATUS_DISK on it.  HOST pointers; out_status / out_disk / out_rhs_evals may be NULL. */
int lt_trace_batch_kerr_disk(double M, double a, double r_obs, const double *alphas, const double *thetas,
                             double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                             int precision, const lt_disk *disk, int64_t n, double *out_fa, int64_t *out_w,
                             int8_t *out_status, double *out_disk, uint32_t *out_rhs_evals);

/* ---- optically thin disk: every image of the disk --------------------------------------------------- *
 * The disk of lt_render_disk (same annulus, orbit, r_in resolution, refusals and redshift g), but it emits and does *
 * not absorb: a ray records its crossings and keeps going, so the picture shows the higher-order images (light     *
 * that went round the hole once or more before it left the disk: the photon ring) as well as the direct one.       *
 *                                                                                                               *
 * Hit: every strict sign change of theta - pi/2 between two consecutive accepted states whose crossing point      *
 * lies in [r_in, r_out], found exactly as lt_render_disk finds its first one (same Hermite refinement, same       *
 * handling of a step that also ends the ray by capture or escape).  The ray's state and event are left as the     *
 * integrator produced them: fa, winding, status and steps are lt_render's (tb_symmetry = 0) on every pixel, and   *
 * stats words 0-5 are lt_render's.  Slot j holds the (j+1)-th hit along the backward ray; the call keeps the first *
 * max_images hits (1 <= max_images <= LT_DISK_MAX_IMAGES) and counts all of them.  Slot 0 is lt_render_disk's hit, *
 * bit for bit, and a ray has a hit exactly where lt_render_disk gives LT_STATUS_DISK.                             *
 *                                                                                                               *
 * Colour, float64: base = lt_render's shaded pixel of the same camera with tb_symmetry = 0, or 0 without a         *
 * background (the shadow render's white sky would saturate every escaped pixel).  Each stored hit adds, from the   *
 * float32 (r, g) of its slot and with s and ramp as in lt_render_disk,                                            *
 *   E_j = exposure g^4 (r_in / r)^q ramp(s)   (unclamped; a 1-channel background takes the mean of the three),     *
 *   rgb = clamp(base + sum_j E_j, 0, 1): base first, then the slots in order, then rounded to float32.            *
 * A pixel without a stored hit is base itself, so with a background it is lt_render's pixel.  With one hit over a  *
 * black base, below saturation, the colour equals lt_render_disk's disk colour exactly.  RGBA8 as everywhere.     */
#define LT_DISK_MAX_IMAGES 8

/* lt_render_disk_dev with the optically thin disk.  Outputs as lt_render_dev, plus
 *   d_images (R, W, max_images, 3) float32 (r_hit, phi_hit in [0, 2 pi), g), NaN in unused slots (may be NULL);
 *   d_n_hits (R, W) uint8: the ray's hits, saturating at 255 (may be NULL).
 * Stats: words 0-5 as lt_render_dev, LT_STAT_DISK rays with at least one hit, LT_STAT_DISK_HITS all hits.
 * RK4 float32 / float64, DP45 and DP45-exact float64.  Partitions as lt_render_disk_dev; tb_symmetry is ignored.
 * LT_ERR_UNSUPPORTED for LT_METRIC_SCHWARZSCHILD and LT_SCHED_QUEUE; LT_ERR_INVALID_ARG for max_images outside
 * [1, LT_DISK_MAX_IMAGES] and as lt_render_disk_dev for the disk. */
int lt_render_disk_images_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                              int32_t max_images, const float *d_bg, int32_t bg_channels, float *d_fa, uint16_t *d_w,
                              int8_t *d_status, uint32_t *d_steps, float *d_images, uint8_t *d_n_hits, float *d_rgb,
                              uint8_t *d_rgba, uint64_t *d_stats);
/* The same with HOST pointers, staged like lt_render_disk. */
int lt_render_disk_images(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                          int32_t max_images, const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w,
                          int8_t *out_status, uint32_t *out_steps, float *out_images, uint8_t *out_n_hits,
                          float *out_rgb, uint8_t *out_rgba, lt_stats *stats);
/* lt_trace_batch_kerr with the optically thin disk (direct schedule): out_images (n, max_images, 3) float64
 * (r_hit, phi_hit in [0, 2 pi), g), NaN in unused slots; out_n_hits (n) int32, every hit of the ray.  out_status is
 * lt_trace_batch_kerr's.  HOST pointers; out_status / out_images / out_n_hits / out_rhs_evals may be NULL. */
int lt_trace_batch_kerr_disk_images(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                    double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                    int precision, const lt_disk *disk, int32_t max_images, int64_t n, double *out_fa,
                                    int64_t *out_w, int8_t *out_status, double *out_images, int32_t *out_n_hits,
                                    uint32_t *out_rhs_evals);

/* ---- hit times and an orbiting hot spot re-shaded from one trace -------------------------------------- *
 * lt_trace_disk_hits is lt_render_disk_images' trace with one more number per hit: the coordinate time the light   *
 * needs from the hit to the camera.  With that stored, a picture of something that MOVES on the disk -- here a     *
 * bright spot on a circular orbit -- at any observer time is a re-shade of the stored hits (lt_shade_hotspot), and  *
 * a light curve is a reduction over them (lt_hotspot_lightcurve): one trace, then passes of epilogue size.         *
 *                                                                                                               *
 * Time.  With the tracers' convention (E = 1, L = p_phi)                                                          *
 *   dt/dlambda (r, theta) = [ (r^2 + a^2) P / Delta + a (L - a sin^2 theta) ] / Sigma,   P = r^2 + a^2 - a L,      *
 * positive outside the horizon; the elapsed time is counted from the camera along the backward ray.  It does not  *
 * feed back into the ray: it is a quadrature over the accepted steps, and no step changes.  Per accepted step      *
 * y0 -> y1 of length h (a rejected or retried attempt adds nothing)                                                *
 *   dt_step = h/6 ( t'(y0) + 4 t'(y_m) + t'(y1) ),                                                                 *
 * y_m the step's cubic Hermite at 1/2: r_m = (r0 + r1)/2 + h/8 (r'0 - r'1), the same for theta, with               *
 * r' = Delta p_r / Sigma and theta' = p_theta / Sigma: local error O(h^5), RK4's own order.  A hit at the fraction  *
 * tau of its step (lt_render_disk's Hermite refinement) applies the same rule to [0, tau], with the cubic's states  *
 * at tau/2 and tau; on a step that also ends the ray, to the retaken full step.  The sum over the steps is a        *
 * compensated (two-term) sum.  disk.step_time (Python) states the rule in numpy; lt_step_time_probe runs the        *
 * device's.                                                                                                       *
 *                                                                                                               *
 * The timed trace takes every step in the general iteration: the far-field streak, which takes up to 64 steps       *
 * without showing their ends, is off.  Its steps are the general iteration's arithmetic, so every output the two    *
 * calls share -- r, phi, g of every slot, n_hits, fa, winding, status, steps, stats words 0-5, LT_STAT_DISK,        *
 * LT_STAT_DISK_HITS -- equals lt_render_disk_images' bit for bit; only LT_STAT_WAVE_ITERS and LT_STAT_EQ_ITERS       *
 * may differ.                                                                                                     *
 *                                                                                                               *
 * Supersampled hot-spot frames are lt_shade_hotspot_aa's ("supersampled hot-spot and Stokes frames" below).         *
 * Out of scope: lt_render_multi and the multi-process path.                                                       */

/* lt_render_disk_images_dev without the colour outputs and with
 *   d_hits (R, W, max_images, 4) float32 (r_hit, phi_hit in [0, 2 pi), g, elapsed time), NaN in unused slots
 * in place of d_images.  RK4 float32 / float64, DP45 and DP45-exact float64, direct schedule; partitions, stats and
 * refusals as lt_render_disk_images_dev. */
int lt_trace_disk_hits_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                           int32_t max_images, float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps,
                           float *d_hits, uint8_t *d_n_hits, uint64_t *d_stats);
/* The same with HOST pointers, staged like lt_render_disk_images. */
int lt_trace_disk_hits(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                       int32_t max_images, float *out_fa, uint16_t *out_w, int8_t *out_status, uint32_t *out_steps,
                       float *out_hits, uint8_t *out_n_hits, lt_stats *stats);
/* lt_trace_batch_kerr_disk_images with out_hits (n, max_images, 4) float64 in place of out_images. */
int lt_trace_batch_kerr_disk_hits(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                  double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                  int precision, const lt_disk *disk, int32_t max_images, int64_t n, double *out_fa,
                                  int64_t *out_w, int8_t *out_status, double *out_hits, int32_t *out_n_hits,
                                  uint32_t *out_rhs_evals);
/* The device's own dt_step on [0, tau] of n steps, for parity tests: p_phi (n), y0 and y1 (n, 4: r, theta, p_r,
 * p_theta), h (n), tau (n), out (n), all float64 HOST arrays; the arithmetic runs in `precision` (32 or 64). */
int lt_step_time_probe(const lt_metric *metric, const double *p_phi, const double *y0, const double *y1, const double *h,
                       const double *tau, int64_t n, int precision, double *out);
/* The rates a lane carries from one step to the next: out (n, 3) = t', r', theta' at y (n, 4: r, theta, p_r, p_theta). */
int lt_time_rates_probe(const lt_metric *metric, const double *p_phi, const double *y, int64_t n, int precision, double *out);

/* A spot of Gaussian profile on the circular equatorial orbit of the disk's direction at r_spot, at azimuth phi0 at
 * coordinate time 0: phi_s(t) = phi0 + Omega(r_spot) t, Omega = sqrt(M) / (r^1.5 + a sqrt(M)). */
typedef struct lt_hotspot {
    double r_spot, phi0;
    double sigma;      /* width of the profile, > 0 (LT_ERR_INVALID_ARG otherwise) */
    double exposure;   /* brightness scale of the spot, >= 0 */
    int32_t with_disk; /* nonzero: the stationary disk's light is added as lt_render_disk_images adds it */
    int32_t reserved;
} lt_hotspot;
void lt_default_hotspot(lt_hotspot *spot); /* r_spot 8, phi0 0, sigma 1, exposure 1, with_disk 1 */

/* The frame at observer time t_obs from stored hits: hits (R, W, max_images, 4) float32 and n_hits (R, W) uint8 as
 * lt_trace_disk_hits wrote them (n_hits NULL: a slot is stored where its r is not NaN).  Per stored slot, in float64
 * from the float32 record,
 *   t_em = t_obs - dt,  phi_s = phi0 + Omega(r_spot) t_em,  d^2 = r^2 + r_s^2 - 2 r r_s cos(phi - phi_s),
 *   w = exp(-d^2 / 2 sigma^2),  E_spot = exposure g^4 w ramp(g),
 *   rgb = clamp(base + sum_j (with_disk E_j^disk + E_j^spot), 0, 1),
 * E^disk and ramp as in lt_render_disk_images (the disk's exposure is lt_disk's), base first, then the slots in order,
 * each slot's disk term before its spot term; a pixel without a stored hit keeps base.  base (R, W, channels) float32
 * or NULL (black); channels 1 (the mean of the three) or 3; out_rgb (R, W, channels) float32 and out_rgba (R, W, 4)
 * uint8, written as everywhere, either may be NULL.  With with_disk = 1 and exposure = 0 over a black base the frame
 * is lt_render_disk_images' rgb bit for bit.  The _dev form takes DEVICE pointers and enqueues on the default stream. */
int lt_shade_hotspot_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                         const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs,
                         const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba);
int lt_shade_hotspot(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                     const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs, const float *base,
                     int32_t channels, float *out_rgb, uint8_t *out_rgba);
/* The spot's light curve at t_start + i dt, i < n_times (<= 65535): out (n_times, 3) float64 = per time the sums of e,
 * e ix and e iy over all pixels (column ix, row iy of the buffer) and stored slots, e the mean of E_spot's channels.
 * No clamping, no base.  Two-stage reduction in a fixed order without floating-point atomics: the result is bitwise
 * the same run to run. */
int lt_hotspot_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                              const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                              int32_t n_times, double *d_out);
int lt_hotspot_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                          const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                          int32_t n_times, double *out);

/* ---- linear polarization of the disk's images and hot-spot Q-U loops --------------------------------------- *
 * lt_trace_disk_pol is lt_trace_disk_hits' trace with one more record per hit: (q, u, sin zeta, mu), the direction  *
 * of linear polarization at the camera and two angles at the emitter.  No equation is added to the ray: in Kerr the *
 * complex Walker-Penrose constant kappa of (k, f) is conserved along a null geodesic, so the polarization at the    *
 * camera is a closed-form function of the state at the hit and the state at the camera.  The integrate kernel keeps *
 * (p_r, p_theta) of every stored hit; a float64 epilogue does the rest.                                             *
 *                                                                                                               *
 * The photon.  The tracers integrate the backward ray with E = 1, L = p_phi; the photon the camera receives has, at  *
 * a point of the ray, the covariant momentum k = (-1, -p_r, -p_theta, L) -- the reading under which g uses xi = L.  *
 *                                                                                                               *
 * Emitter.  The disk's material: the circular equatorial geodesic in +phi, Omega and u^t as in lt_render_disk.  Its  *
 * orthonormal frame at the hit (theta = pi/2, Sigma = r^2): e_(r) = (0, sqrt(Delta)/r, 0, 0), e_(z) = -d_theta / r,  *
 * e_(phi) the unit vector of the t-phi plane orthogonal to u, ~ (-u_phi, 0, 0, u_t), signed so that its phi part is  *
 * positive.  The field has constant components (b_r, b_phi, b_z) in that frame; only its direction matters.  With    *
 * k^ the unit spatial part of k in the frame (components on e_(r), e_(phi), e_(z), a right-handed triad):            *
 *   sin zeta = |k^ x b^|,  f = (k^ x b^) / sin zeta, lifted by the triad (no time part in the frame, so f.k = 0),      *
 *   mu = |k^ . e_(z)|;  where sin^2 zeta < 1e-24 the record is q = u = sin zeta = 0.                                  *
 *                                                                                                               *
 * Transport.  With contravariant components, at (r, theta),                                                       *
 *   kappa = (A - i B)(r - i a cos theta),                                                                          *
 *   A = (k^t f^r - k^r f^t) + a sin^2 theta (k^r f^phi - k^phi f^r),                                                *
 *   B = [ (r^2 + a^2)(k^phi f^theta - k^theta f^phi) - a (k^t f^theta - k^theta f^t) ] sin theta.                    *
 * One function evaluates it at both ends, so a sign or conjugation convention cancels.                              *
 *                                                                                                               *
 * Camera.  The static observer at (r_obs, theta_obs) (LT_ERR_INVALID_ARG where g_tt >= 0 there, or on the axis):     *
 * e_t ~ d_t, e_r ~ d_r, e_theta ~ d_theta, e_phi ~ d_phi - (g_tphi / g_tt) d_t.  The camera-end momentum is the      *
 * ray's own initial record and its L.  With n^ the unit spatial direction of k in that tetrad, the screen basis is   *
 * north e_2 ~ -e_theta + n^theta n^ and e_1 = e_2 x n^ in the right-handed triad (r, theta, phi).  For a camera that  *
 * looks at the hole with psi = 0, e_1 ~ +e_phi points towards decreasing column index (the rays with L > 0 are at    *
 * the larger columns) and e_2 towards increasing row index (the rays that leave the camera southward, p_theta > 0,   *
 * are at the smaller rows).  Real (x, y) solve x kappa(e_1) + y kappa(e_2) = kappa_hit; then                          *
 *   q = (x^2 - y^2) / (x^2 + y^2) = cos 2 chi,  u = 2 x y / (x^2 + y^2) = sin 2 chi,                                   *
 * chi the electric vector's angle from e_1 towards e_2.  No angle is stored, so there is no branch cut.               *
 *                                                                                                               *
 * Stokes parameters.  Per stored slot, e = the mean of the three channels of the light the slot contributes (the     *
 * disk's E^disk if with_disk, plus the spot's E_spot, both unclamped):                                              *
 *   I += e,  Q += Pi sin^2 zeta e q,  U += Pi sin^2 zeta e u,                                                        *
 * Pi = pol_frac in [0, 1].  Nothing is clamped and there is no base.  disk.polarization / disk.stokes_frame /        *
 * disk.stokes_lightcurve (Python) state all of it in numpy; lt_polarization_probe runs the device's rule.           *
 *                                                                                                               *
 * Supersampled polarized frames are lt_shade_stokes_aa's ("supersampled hot-spot and Stokes frames" below).          *
 * Out of scope: lt_render_multi and the multi-process path, circular polarization and Faraday effects.              */
typedef struct lt_bfield {
    double b_r, b_phi, b_z; /* components in the emitter's frame; not all zero (LT_ERR_INVALID_ARG otherwise) */
    double pol_frac;        /* Pi, in [0, 1] */
} lt_bfield;
void lt_default_bfield(lt_bfield *field); /* (0, 0, 1), pol_frac 0.7 */

/* lt_trace_disk_hits_dev plus d_pol (R, W, max_images, 4) float32 (q, u, sin zeta, mu), NaN in unused slots.  Every
 * output and stats word it shares with lt_trace_disk_hits_dev equals that call's bit for bit.  Configurations,
 * partitions and refusals as there. */
int lt_trace_disk_pol_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                          const lt_bfield *field, int32_t max_images, float *d_fa, uint16_t *d_w, int8_t *d_status,
                          uint32_t *d_steps, float *d_hits, uint8_t *d_n_hits, float *d_pol, uint64_t *d_stats);
/* The same with HOST pointers. */
int lt_trace_disk_pol(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                      const lt_bfield *field, int32_t max_images, float *out_fa, uint16_t *out_w, int8_t *out_status,
                      uint32_t *out_steps, float *out_hits, uint8_t *out_n_hits, float *out_pol, lt_stats *stats);
/* lt_trace_batch_kerr_disk_hits plus out_pol (n, max_images, 4) float64. */
int lt_trace_batch_kerr_disk_pol(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                 double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                 int precision, const lt_disk *disk, const lt_bfield *field, int32_t max_images, int64_t n,
                                 double *out_fa, int64_t *out_w, int8_t *out_status, double *out_hits, int32_t *out_n_hits,
                                 double *out_pol, uint32_t *out_rhs_evals);
/* The device's own rule on n synthetic records, for parity tests: p_phi (n), hit (n, 3: r, p_r, p_theta of the backward
 * ray at the hit), cam (n, 2: its p_r, p_theta at the camera), out (n, 4: q, u, sin zeta, mu), float64 HOST arrays. */
int lt_polarization_probe(const lt_metric *metric, double r_obs, double theta_obs, const lt_bfield *field,
                          const double *p_phi, const double *hit, const double *cam, int64_t n, double *out);
/* The Stokes frame at observer time t_obs from stored records: hits and n_hits as lt_shade_hotspot takes them, pol
 * (R, W, max_images, 4) float32 as lt_trace_disk_pol wrote it; out_iqu (R, W, 3) float32 = (I, Q, U), summed in float64
 * over the stored slots in order.  The _dev form takes DEVICE pointers and enqueues on the default stream. */
int lt_shade_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                        int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                        const lt_bfield *field, double t_obs, float *d_iqu);
int lt_shade_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t max_images,
                    const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_bfield *field, double t_obs,
                    float *out_iqu);
/* The spot's Stokes light curve at t_start + i dt, i < n_times (<= 65535): out (n_times, 3) float64 = per time the sums
 * of I, Q, U of the spot alone over all pixels and stored slots.  lt_hotspot_lightcurve's two-stage reduction in its
 * fixed order, without floating-point atomics: bitwise the same run to run, and column 0 has the bits of
 * lt_hotspot_lightcurve's column 0. */
int lt_hotspot_lightcurve_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                     int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                     const lt_bfield *field, double t_start, double dt, int32_t n_times, double *d_out);
int lt_hotspot_lightcurve_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                 int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                 const lt_bfield *field, double t_start, double dt, int32_t n_times, double *out);

/* ---- supersampled hot-spot and Stokes frames, resolved on the GPU ------------------------------------------ *
 * A hot spot's higher-order images are arcs a fraction of a pixel wide, so a one-ray-per-pixel sequence flickers.      *
 * These entry points re-shade the records of the FINE camera (the same camera with width W S and height H S,          *
 * "supersampled frames" below; S = samples, 1 <= S <= LT_AA_MAX_SAMPLES = 8) and resolve them in one kernel: only     *
 * the (R, W) output is written and comes back.                                                                    *
 *                                                                                                               *
 * Fine records.  What lt_trace_disk_hits[_dev] / lt_trace_disk_pol[_dev] write for the fine camera:                    *
 *   hits (R S, W S, max_images, 4) float32;  n_hits (R S, W S) uint8, or NULL with lt_shade_hotspot's meaning;          *
 *   pol (R S, W S, max_images, 4) float32.                                                                         *
 * R, W are OUTPUT rows and columns; fine pixel (y S + j, x S + i) is sub-sample (j, i) of output pixel (y, x).  For a    *
 * partition the fine rows are the fine frame's partition with row blocks of row_block S, as in lt_render_aa, so local *
 * fine row y S + j belongs to local output row y.                                                                  *
 *                                                                                                               *
 * Rule.  The value of a fine pixel is the float32 value lt_shade_hotspot (lt_shade_stokes) writes for that pixel of    *
 * the fine buffers -- same arithmetic, same order, the clamp included for rgb; base, when given, is the fine-size      *
 * (R S, W S, channels) buffer.  The output pixel is the resolve of lt_render_aa: the S^2 float32 values added in       *
 * float64 in row-major order (j outer, i inner) from 0.0, divided by (double)(S S), rounded to float32; RGBA8 from     *
 * that float32 as everywhere.  So rgb is, bit for bit, aa.resolve (Python) of the frame lt_shade_hotspot returns for   *
 * the fine records, iqu the same of lt_shade_stokes', and with samples = 1 both are those entry points' outputs.        *
 * No floating-point atomics; no result depends on the launch geometry.                                              *
 *                                                                                                               *
 * Refusals.  LT_ERR_NO_DEVICE without a GPU; then samples outside [1, LT_AA_MAX_SAMPLES]: LT_ERR_INVALID_ARG; then       *
 * everything lt_shade_hotspot / lt_shade_stokes refuse, with their codes, in their order.                            *
 *                                                                                                               *
 * The light curve needs no entry point: lt_hotspot_lightcurve / lt_hotspot_lightcurve_stokes called with (R S, W S)   *
 * and the fine records are the supersampled curves in FINE-pixel units -- the sums over S^2 sub-samples per pixel,      *
 * the first moments in fine columns and rows.  In output-pixel units: column 0 / S^2 and the moments / S^3 for the      *
 * first, all three columns / S^2 for the Stokes curve (image_lens.render_sequence does so).                           *
 *                                                                                                               *
 * Out of scope: lt_render_multi, the multi-process path, adaptive sampling of sequences.                             */
int lt_shade_hotspot_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                            int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                            double t_obs, const float *d_base /* (R S, W S, channels) or NULL */, int32_t channels,
                            float *d_rgb /* (R, W, channels) */, uint8_t *d_rgba /* (R, W, 4) */);
/* The same with HOST pointers, staged like lt_shade_hotspot; only the resolved outputs come back. */
int lt_shade_hotspot_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples, int32_t max_images,
                        const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs, const float *base,
                        int32_t channels, float *out_rgb, uint8_t *out_rgba);
int lt_shade_stokes_aa_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                           int32_t samples, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_hotspot *spot, const lt_bfield *field, double t_obs, float *d_iqu /* (R, W, 3) */);
int lt_shade_stokes_aa(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t samples,
                       int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                       const lt_bfield *field, double t_obs, float *out_iqu);

/* ---- a rotating emissivity map on the disk, shaded from stored hits ------------------------------------------ *
 * lt_shade_hotspot looks at one Gaussian spot on one orbit.  These entry points look an emissivity up in a table on   *
 * the disk instead -- spiral arms, clumps, several spots, a snapshot of a simulation -- and turn the table since       *
 * t = 0, each ring at the disk's own Keplerian rate (the pattern shears) or all of it at one pattern speed.  The       *
 * records are lt_trace_disk_hits' (r, phi, g, dt), so the light-travel delay is taken per image order, as the hot      *
 * spot takes it, and nothing is traced again: a frame, a supersampled frame and a light curve, at epilogue cost.       *
 *                                                                                                               *
 * The map.  texels (n_r, n_phi) float32, row-major with phi contiguous, plus lt_diskmap.  Texel (i, k) is the          *
 * emissivity at t = 0 at radius r_min + (i + 1/2)(r_max - r_min)/n_r and azimuth (k + 1/2) 2 pi/n_phi.  Texels must be  *
 * finite and are not checked.                                                                                    *
 *                                                                                                               *
 * Rule.  Per stored slot (hits and n_hits as lt_shade_hotspot takes them), in float64 from the float32 record, in      *
 * this order:                                                                                                    *
 *   1. t_em = t_obs - dt;  Omega = sqrt(M) / (r^1.5 + a sqrt(M)) of the hit's own r for LT_MAP_KEPLERIAN (the disk's    *
 *      rate, the expression of the hot spot's orbit), Omega = omega_p for LT_MAP_RIGID;                               *
 *   2. psi = wrap_2pi(phi - Omega t_em), the azimuth unwound to t = 0, in [0, 2 pi);                                   *
 *   3. v = (r - r_min)/(r_max - r_min) n_r - 1/2, clamped to [0, n_r - 1];  i0 = min(floor(v), n_r - 1),               *
 *      i1 = min(i0 + 1, n_r - 1),  f_r = v - i0: constant extrapolation over the outer half texels;                   *
 *   4. u = psi (n_phi/2 pi) - 1/2;  k0 = floor(u) mod n_phi (-1 is n_phi - 1),  k1 = (k0 + 1) mod n_phi,                *
 *      f_phi = u - floor(u): the seam is periodic;                                                                 *
 *   5. m = (1 - f_r)[(1 - f_phi) T[i0,k0] + f_phi T[i0,k1]] + f_r[(1 - f_phi) T[i1,k0] + f_phi T[i1,k1]];              *
 *      m = 0 where r < r_min, r > r_max or r is NaN, the float32 r compared exactly against the doubles;              *
 *   6. E_map = exposure g^4 m ramp(g) -- the hot spot's law with w replaced by m -- and                               *
 *      rgb = clamp(base + sum_j (with_disk E_j^disk + E_j^map), 0, 1),                                                *
 *      base first, then the slots in order, each slot's disk term before its map term; a pixel without a stored hit   *
 *      keeps base.  One channel: the mean of the three, as lt_shade_hotspot.                                          *
 * base, channels, out_rgb, out_rgba, M and everything else as lt_shade_hotspot takes them.  An all-zero table with      *
 * with_disk = 1 gives lt_shade_hotspot's frame of a spot with exposure 0.  disk.sample_map / disk.map_emission /        *
 * disk.shade_diskmap / disk.diskmap_lightcurve (Python) state the rule in numpy.                                      *
 *                                                                                                               *
 * Supersampled frames.  lt_shade_diskmap_aa takes the FINE records and base of "supersampled hot-spot and Stokes        *
 * frames" above; R, W are OUTPUT rows and columns and `samples` follows them.  The result is by definition, and bit    *
 * for bit, aa.resolve (Python) of the frame lt_shade_diskmap returns for the fine records; samples = 1 is              *
 * lt_shade_diskmap.  The light curve of fine records is lt_diskmap_lightcurve called with (R S, W S): column 0 / S^2   *
 * and the moments / S^3 in output-pixel units (image_lens.render_sequence does so).                                  *
 *                                                                                                               *
 * Light curve.  out (n_times, 3) float64 at t_start + i dt, i < n_times (<= 65535): the sums of e, e ix and e iy over   *
 * all pixels and stored slots, e the mean of E_map's channels.  No clamp, no base; lt_hotspot_lightcurve's two-stage    *
 * reduction in its fixed order, without floating-point atomics: bitwise the same run to run.                          *
 *                                                                                                               *
 * Refusals, in this order.  No GPU: LT_ERR_NO_DEVICE (the _aa forms then refuse samples outside                        *
 * [1, LT_AA_MAX_SAMPLES]: LT_ERR_INVALID_ARG); null hits / metric / disk / map / texels: LT_ERR_INVALID_ARG; a metric    *
 * that is not LT_METRIC_KERR: LT_ERR_UNSUPPORTED; then LT_ERR_INVALID_ARG for a bad metric, an empty frame, max_images,  *
 * the map's fields in the struct's order, the disk's q / exposure, channels, and t_obs or t_start / dt / n_times.       *
 *                                                                                                               *
 * Out of scope: polarized maps, a map plus a spot in one call, lt_render_multi and the multi-process path, adaptive   *
 * sampling of sequences.  Tables that change with time are "a disk movie" below.                                   */
#define LT_MAP_KEPLERIAN 0
#define LT_MAP_RIGID 1

typedef struct lt_diskmap {
    double r_min, r_max; /* the annulus the table covers, 0 < r_min < r_max, finite */
    double omega_p;      /* pattern speed for LT_MAP_RIGID (finite; ignored for LT_MAP_KEPLERIAN) */
    double exposure;     /* brightness scale, finite, >= 0 */
    int32_t n_r, n_phi;  /* >= 1 each, n_r n_phi <= 2^26 */
    int32_t rotation;    /* LT_MAP_KEPLERIAN: every radius turns at the disk's own Omega(r); LT_MAP_RIGID: all at omega_p */
    int32_t with_disk;   /* nonzero: the stationary disk's light is added as lt_shade_hotspot adds it */
} lt_diskmap;
void lt_default_diskmap(lt_diskmap *map); /* r_min 6, r_max 20, omega_p 0, exposure 1, 1 x 1 texels, Keplerian, with_disk 1 */

/* The _dev forms take DEVICE pointers (d_texels too) and enqueue on the default stream. */
int lt_shade_diskmap_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                         const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                         double t_obs, const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba);
/* The same with HOST pointers, staged like lt_shade_hotspot; the texels are one more input. */
int lt_shade_diskmap(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                     const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels, double t_obs,
                     const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba);
int lt_shade_diskmap_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                            int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                            const float *d_texels, double t_obs, const float *d_base /* (R S, W S, channels) or NULL */,
                            int32_t channels, float *d_rgb /* (R, W, channels) */, uint8_t *d_rgba /* (R, W, 4) */);
/* The same with HOST pointers; only the resolved outputs come back. */
int lt_shade_diskmap_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples, int32_t max_images,
                        const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels, double t_obs,
                        const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba);
int lt_diskmap_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                              const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                              double t_start, double dt, int32_t n_times, double *d_out);
int lt_diskmap_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                          const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                          double t_start, double dt, int32_t n_times, double *out);

/* ---- energy-resolved light: line profiles and dynamic spectra binned from the stored hits -------------------- *
 * Every product above is bolometric: g^4 times an emissivity through the colour ramp.  These entry points bin the      *
 * same unclamped intensities by the redshift factor g = E_obs / E_rest each record stores: for the stationary disk the  *
 * relativistically broadened line (lt_disk_spectrum), for the moving emitters the dynamic spectrum, flux per energy bin *
 * per observer time (lt_hotspot_spectrum, lt_diskmap_spectrum).  Every image order is binned at its own emission time   *
 * t_obs - dt, so the photon ring draws the spot's trail in g again, delayed.  A fourth reduction over the records of     *
 * lt_trace_disk_hits, next to the frame, the supersampled frame and the light curve; nothing is traced again.            *
 *                                                                                                               *
 * Grid.  lt_spectrum is a linear grid in g: 0 < g_min < g_max, both finite, n_bins in 1 ... LT_SPECTRUM_MAX_BINS.        *
 *                                                                                                               *
 * Bin of a hit, in float64 from the stored float32 g, in exactly this form (a subtraction followed by a                *
 * multiplication: nothing an fma can contract, so every statement of the rule picks the same bin):                      *
 *     inv_dg = n_bins / (g_max - g_min)          (computed once on the host)                                           *
 *     x = (double)g                                                                                                  *
 *     k = x < g_min ? 0 : x >= g_max ? n_bins + 1 : 1 + min((int)floor((x - g_min) * inv_dg), n_bins - 1)              *
 * Column 0 is the underflow, column n_bins + 1 the overflow; bin k = 1 ... n_bins is half-open,                        *
 * [g_min + (k - 1) dg, g_min + k dg).  A stored slot whose g is NaN is skipped; nothing else is filtered.              *
 *                                                                                                               *
 * Weight of a hit, float64: the unclamped intensity the emitter's frames and light curve multiply the ramp with,       *
 *     the disk:  disk.exposure g^4 (r_in / r)^q                                                                        *
 *     the spot:  spot.exposure g^4 exp(-d^2 / 2 sigma^2)      at t_obs - dt  ("hit times and an orbiting hot spot")     *
 *     the map:   map.exposure g^4 m                           the table turned to t_obs - dt ("a rotating emissivity map") *
 * (with_disk is not looked at: a spectrum is one emitter's).  The stored slots are the re-shades': the first            *
 * min(n_hits, max_images), or the leading slots whose r is not NaN when n_hits is NULL.                              *
 *                                                                                                               *
 * Times.  Row i is at t_i = t_start + i dt, the product rounded and then the sum (no fma), i < n_times <= 65535.        *
 *                                                                                                               *
 * Output.  float64 (n_times, planes, n_bins + 2), lt_disk_spectrum one row (1, planes, n_bins + 2).  planes is 1, or    *
 * max_images with split_orders: plane j then holds the hits stored in slot j, image order j.  An empty bin is exactly   *
 * 0.0.  A row summed over all columns and planes is the emitter's bolometric light at that time.                     *
 *                                                                                                               *
 * Order of every sum (it depends on R, W, max_images and the grid alone, never on scheduling; no floating-point        *
 * atomics anywhere, so a result is the same bits run after run and whatever batch of times a row is computed in).      *
 * Key = plane (n_bins + 2) + k.  Workgroup b of LT_SPECTRUM_BLOCKS walks the chunks of 256 pixels                      *
 * p = 256 (b + c LT_SPECTRUM_BLOCKS) + i, c ascending (the light curve's stride order).  Within a chunk, wavefront      *
 * w = i div 64 adds, for every slot j, the weights of a key over its 64 lanes l = i mod 64 with the butterfly           *
 * l ^ 32, l ^ 16, ... l ^ 1 (lanes without that key add +0.0, which changes no bit; so do entries of weight exactly 0).  *
 * The owner of a key adds these sums to the workgroup's accumulator ordered by w, then j; the final stage adds a         *
 * time's LT_SPECTRUM_BLOCKS partials per key, b ascending.                                                          *
 * The partials live in a grow-only workspace of at most LT_SPECTRUM_WORKSPACE_BYTES: the times are launched in batches  *
 * of max(1, LT_SPECTRUM_WORKSPACE_BYTES / (LT_SPECTRUM_BLOCKS planes (n_bins + 2) 8)).                                 *
 *                                                                                                               *
 * Supersampled records.  Called with the fine records (R S, W S) the result divided by S^2 is in output-pixel units,    *
 * as the light curve's first column (image_lens.render_sequence does so).                                            *
 *                                                                                                               *
 * Refusals, in this order: those of the emitter's frame up to and including the disk's q / exposure (lt_shade_hotspot,  *
 * lt_shade_diskmap; lt_disk_spectrum: null hits / metric / disk, the metric, the frame, max_images, q / exposure);       *
 * then LT_ERR_INVALID_ARG for a null spec, the g range, n_bins, n_times, t_start / dt, and a null out.  n_times = 0 is   *
 * LT_OK and writes nothing.  The outputs of a refused call are untouched.                                           *
 * disk.Spectrum / disk.spectrum_bin / disk.disk_spectrum / disk.hotspot_spectrum / disk.diskmap_spectrum (Python)       *
 * state the rule in numpy.                                                                                       *
 *                                                                                                               *
 * Out of scope: any rest-frame shape other than a line (the thermal continuum has its own section), polarized          *
 * spectra, logarithmic grids, per-pixel spectra, lt_render_multi and the multi-process path, adaptive sampling.        */
#define LT_SPECTRUM_MAX_BINS 512
#define LT_SPECTRUM_BLOCKS 256
#define LT_SPECTRUM_WORKSPACE_BYTES (64 << 20)

typedef struct lt_spectrum {
    double g_min, g_max;  /* the grid's ends in g = E_obs / E_rest, 0 < g_min < g_max, finite */
    int32_t n_bins;       /* 1 ... LT_SPECTRUM_MAX_BINS */
    int32_t split_orders; /* nonzero: one plane per stored slot (image order) */
} lt_spectrum;
void lt_default_spectrum(lt_spectrum *spec); /* 0.0625 ... 1.5625, 96 bins, not split */

/* The _dev forms take DEVICE pointers and enqueue on the default stream; the others HOST pointers, staged like the light
 * curves.  out: (n_times, planes, n_bins + 2) float64. */
int lt_disk_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                         const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, double *d_out);
int lt_disk_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                     const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, double *out);
int lt_hotspot_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                            const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_spectrum *spec,
                            double t_start, double dt, int32_t n_times, double *d_out);
int lt_hotspot_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                        const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_spectrum *spec,
                        double t_start, double dt, int32_t n_times, double *out);
int lt_diskmap_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                            const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                            const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *d_out);
int lt_diskmap_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                        const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                        const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *out);

/* ---- visibilities: what an interferometer measures, from the stored hits ------------------------------------ *
 * Every product above lives in the image plane or is a total flux.  An interferometer samples the image's Fourier     *
 * transform on a set of baselines; the photon ring's thin arcs carry almost no flux and dominate the long ones.       *
 * These entry points give the complex visibility of one emitter's light per observer time, image order and baseline:  *
 * a fifth reduction over the records of lt_trace_disk_hits; nothing is traced again.                               *
 *                                                                                                               *
 * The rule.  For a record buffer of R x W pixels (pixel p has ix = p % W, iy = p / W), a baseline b = (u_b, v_b) in     *
 * CYCLES PER PIXEL OF THAT BUFFER and an observer time t,                                                          *
 *     V[t, plane, b] = sum over pixels p and stored slots j of the plane:  w(rec_pj, t) exp(-2 pi i (u_b ix + v_b iy))  *
 * Weight.  w is exactly what a spectrum bins ("energy-resolved light": the disk's, the spot's or the map's unclamped   *
 * exposure g^4 emitter, no colour ramp; with_disk is not looked at).  The stored slots are the re-shades'; a stored    *
 * slot whose g is NaN is skipped.                                                                                  *
 * Planes.  1, or max_images with split_orders != 0: plane j then holds the hits stored in slot j, image order j.       *
 * Without split_orders a pixel's slots are added first, in their order, and the sum takes the pixel's phase.           *
 * Phase, in float64 and in exactly this form:                                                                      *
 *     x = u ix + v iy        both products rounded, then the sum (no fma)                                             *
 *     f = x - rint(x)        exact; |f| <= 1/2                                                                        *
 *     (s, c) = sincospi(2 f)                                                                                        *
 * and the term is (w c, -w s), each component added to its sum with one fused multiply-add.  The reduced argument      *
 * makes the phases at quarter cycles exact (c, s in {0, 1, -1}) and keeps the phase's error, 2 pi (W + H) 2^-53 from   *
 * the roundings of x plus sincospi's own, independent of anything else.  The origin of the phase is pixel (0, 0).     *
 * Limits.  |u|, |v| <= 0.5, the Nyquist limit of the buffer, both finite; 1 <= n_baselines <=                          *
 * LT_VISIBILITY_MAX_BASELINES.  Times as the spectrum's: row i at t_start + i dt (product rounded, then the sum),      *
 * i < n_times <= 65535.                                                                                            *
 *                                                                                                               *
 * Output.  float64 (n_times, planes, n_baselines, 2) holding (re, im); lt_disk_visibility one row (1, planes,         *
 * n_baselines, 2) and no time.  A plane without light is exactly 0 + 0i.  V at (0, 0) is the plane's total flux.       *
 *                                                                                                               *
 * Order of every sum (it depends on R, W, max_images and the records alone; no floating-point atomics anywhere, so a   *
 * result is the same bits run after run, whatever batch of times it is computed in and whatever other baselines are    *
 * asked for with it).  Workgroup k of LT_VISIBILITY_BLOCKS walks the chunks of 256 pixels p = 256 (k + c               *
 * LT_VISIBILITY_BLOCKS) + i, c ascending (the light curve's stride order), and adds to its sum, which starts at 0,    *
 * the terms of the chunk's pixels in ascending i; a pixel whose weights are exactly 0 at every time and plane of its   *
 * batch is left out, which changes no bit.  The final stage adds the LT_VISIBILITY_BLOCKS partial sums, k ascending.    *
 * A workgroup keeps the sums of a batch of times in registers: max(1, LT_VISIBILITY_BATCH_TERMS / planes) times        *
 * (lt_visibility_batch_times).  The partials live in a grow-only workspace of at most LT_VISIBILITY_WORKSPACE_BYTES     *
 * (plus the baselines' 16 KiB): a call's batches go in as few launches as that allows.                                *
 *                                                                                                               *
 * Supersampled records.  Called with the fine records (R S, W S) and the baselines (u / S, v / S), u, v in cycles per  *
 * output pixel, the result divided by S^2 is in output-pixel units; image_lens.render_sequence does so and moves the    *
 * phase's origin to the centre of the output frame (disk.Baselines.recentre).                                        *
 *                                                                                                               *
 * Refusals, in this order: those of the emitter's frame up to and including the disk's q / exposure, as the spectrum's; *
 * then LT_ERR_INVALID_ARG for a null uv, n_baselines, a baseline out of range or not finite, n_times, t_start / dt,     *
 * and a null out.  n_times = 0 is LT_OK and writes nothing, even with a null out.  The outputs of a refused call are   *
 * untouched.  disk.Baselines / disk.visibility_phase / disk.disk_visibility / disk.hotspot_visibility /              *
 * disk.diskmap_visibility (Python) state the rule in numpy.                                                        *
 *                                                                                                               *
 * Out of scope: closure quantities (products of these numbers), baselines beyond Nyquist, noise and the (u, v) tracks  *
 * of real arrays, lt_render_multi and the multi-process path, adaptive sampling.  Polarized visibilities are the next   *
 * section's.                                                                                                       */
#define LT_VISIBILITY_MAX_BASELINES 1024
#define LT_VISIBILITY_BLOCKS 256
#define LT_VISIBILITY_BATCH_TERMS 16 /* times x planes a workgroup accumulates at once, per owned baseline */
#define LT_VISIBILITY_WORKSPACE_BYTES (64 << 20)

/* Times of one batch: max(1, LT_VISIBILITY_BATCH_TERMS / planes).  Needs no device. */
int32_t lt_visibility_batch_times(int32_t max_images, int32_t split_orders);

/* The _dev forms take DEVICE pointers for the records, the texels and the output and enqueue on the default stream; the
 * others HOST pointers, staged like the spectra.  uv is a HOST pointer in both: n_baselines pairs (u, v) of float64,
 * checked on the host and uploaded with the call.  out: (n_times, planes, n_baselines, 2) float64. */
int lt_disk_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                           const lt_metric *metric, const lt_disk *disk, const double *uv, int32_t n_baselines,
                           int32_t split_orders, double *d_out);
int lt_disk_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                       const lt_metric *metric, const lt_disk *disk, const double *uv, int32_t n_baselines,
                       int32_t split_orders, double *out);
int lt_hotspot_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                              const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const double *uv,
                              int32_t n_baselines, int32_t split_orders, double t_start, double dt, int32_t n_times,
                              double *d_out);
int lt_hotspot_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                          const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const double *uv,
                          int32_t n_baselines, int32_t split_orders, double t_start, double dt, int32_t n_times, double *out);
int lt_diskmap_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                              const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                              const double *uv, int32_t n_baselines, int32_t split_orders, double t_start, double dt,
                              int32_t n_times, double *d_out);
int lt_diskmap_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                          const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                          const double *uv, int32_t n_baselines, int32_t split_orders, double t_start, double dt,
                          int32_t n_times, double *out);

/* ---- a disk movie: emissivity tables that change with time, shaded from stored hits --------------------------- *
 * A map ("a rotating emissivity map") is one snapshot that can only turn.  A movie is a sequence of snapshots at      *
 * evenly spaced coordinate times -- a flare that brightens and fades, a clump that forms and shears apart, the        *
 * frames of a simulation -- looked up at each stored slot's own emission time t_obs - dt, so every image order sees   *
 * the movie at its own moment and the photon ring shows a flare again, later.  All five products of the stored hits:  *
 * the frame, the supersampled frame, the light curve, the dynamic spectrum and the visibilities.  Nothing is traced    *
 * again.                                                                                                         *
 *                                                                                                               *
 * The movie.  texels (n_frames, n_r, n_phi) float32, frame-major with phi contiguous, plus lt_diskmap, whose fields    *
 * keep their meaning for every frame, plus lt_diskmovie.  Frame q is the emissivity at coordinate time                *
 * T_q = t0 + q dt_frame.  Texels must be finite and are not checked.                                               *
 *                                                                                                               *
 * Rule.  Per stored slot, in float64 from the float32 record (r, phi, g, dt), in this order:                         *
 *   1. t_em = t_obs - dt;  s = (t_em - t0) / dt_frame;                                                             *
 *   2. LT_MOVIE_HOLD:  q0 = clamp(floor(s), 0, n_frames - 1),  q1 = min(q0 + 1, n_frames - 1),                       *
 *      f_t = clamp(s - q0, 0, 1);  the table indices are k0 = q0, k1 = q1.  Where q1 == q0 -- at or after the last   *
 *      frame, n_frames = 1 -- ONE look-up is made and m = m_q0 exactly; before frame 0 f_t = 0 and m = m_0 exactly    *
 *      as well (finite texels).  A NaN s gives q0 = 0, f_t = 0;                                                     *
 *   3. LT_MOVIE_LOOP:  q0 = floor(s),  q1 = q0 + 1,  f_t = s - q0;  k = q - n_frames floor(q / n_frames), clamped     *
 *      into [0, n_frames - 1]: the last frame blends into frame 0.  Always two look-ups.  A NaN s takes frame 0 with   *
 *      f_t = 0.  Every index is clamped before it is used, whatever the record holds;                               *
 *   4. each frame of the pair is unwound from its OWN epoch by the map's rotation:  T_q = t0 + q dt_frame,            *
 *      psi_q = wrap_2pi(phi - Omega (t_em - T_q)), Omega as in the map's step 1 (the hit's own r for LT_MAP_KEPLERIAN,  *
 *      omega_p for LT_MAP_RIGID);  m_q = the map's steps 3 to 5 (bilinear in r and psi, periodic seam, 0 outside       *
 *      [r_min, r_max]) on frame k_q at psi_q.  So between two snapshots the pattern is carried along by the disk's     *
 *      rotation instead of cross-fading in place; inside the movie the phase Omega (t_em - T_q) is at most            *
 *      Omega dt_frame, however large t_obs is; outside a held movie the end frame keeps turning as a rotating map      *
 *      would.  LT_MAP_RIGID with omega_p = 0 is plain interpolation of lab-frame snapshots;                         *
 *   5. m = (1 - f_t) m_q0 + f_t m_q1;  E = exposure g^4 m ramp(g);  the frame's composition, with_disk, base,        *
 *      channels and the clamp are exactly the map's step 6.                                                        *
 * The rule is continuous in t_em across every floor and clamp: at a whole s the pair (q0 - 1, q0) at f_t -> 1 and the  *
 * pair (q0, q0 + 1) at f_t = 0 both give m_q0 at psi = phi; before frame 0 of a held movie f_t = 0 and past its last    *
 * frame the single look-up is the limit of f_t -> 1; a loop's index wraps where the pair's weights do not change.  A    *
 * rounding of s therefore moves m by the rounding times the slope, never by a jump.  One held frame with t0 = 0 is the  *
 * map, bit for bit.  disk.DiskMovie / disk.sample_movie / disk.movie_emission / disk.shade_diskmovie /               *
 * disk.diskmovie_lightcurve / disk.diskmovie_spectrum / disk.diskmovie_visibility (Python) state the rule in numpy.    *
 *                                                                                                               *
 * Products.  Each is the map's with the movie as the emitter: lt_shade_diskmovie the frame, lt_shade_diskmovie_aa     *
 * the supersampled frame (bit for bit aa.resolve of the fine frame; samples = 1 is lt_shade_diskmovie),              *
 * lt_diskmovie_lightcurve the light curve (n_times, 3), lt_diskmovie_spectrum the dynamic spectrum                  *
 * ("energy-resolved light": the weight is exposure g^4 m) and lt_diskmovie_visibility the visibilities              *
 * ("visibilities", the same weight).  Outputs, limits, batches, the fixed order of every sum and the guarantees are   *
 * the map's; no floating-point atomics are used.                                                                  *
 *                                                                                                               *
 * Refusals, in the map's order.  No GPU: LT_ERR_NO_DEVICE (the _aa forms then refuse samples); null hits / metric /    *
 * disk / map / movie / texels: LT_ERR_INVALID_ARG; a metric that is not LT_METRIC_KERR: LT_ERR_UNSUPPORTED; then        *
 * LT_ERR_INVALID_ARG for a bad metric, an empty frame, max_images, the map's fields in the struct's order, the         *
 * movie's fields in the struct's order (t0, dt_frame, n_frames with the size limit, boundary), the disk's            *
 * q / exposure, and then what the map's entry point of the same product refuses behind them.  The size limit is        *
 * refused before the table is read.  A refused call writes nothing.                                               *
 *                                                                                                               *
 * Out of scope: non-uniform frame times, polarized movies, a movie plus a spot in one call, lt_render_multi and the    *
 * multi-process path, adaptive sampling of sequences, streaming a movie larger than the limit.                     */
#define LT_MOVIE_HOLD 0
#define LT_MOVIE_LOOP 1

typedef struct lt_diskmovie {
    double t0;        /* coordinate time of frame 0, finite */
    double dt_frame;  /* spacing of the frames, finite, > 0 */
    int32_t n_frames; /* >= 1; n_frames n_r n_phi <= 2^28 (and n_r n_phi <= 2^26 as before) */
    int32_t boundary; /* LT_MOVIE_HOLD: the end frames are held; LT_MOVIE_LOOP: the last frame blends into frame 0 */
} lt_diskmovie;
void lt_default_diskmovie(lt_diskmovie *mv); /* t0 0, dt_frame 1, 1 frame, hold */

/* Pointers as the map's: the _dev forms take DEVICE pointers (d_texels too) and enqueue on the default stream, the
 * others HOST pointers; uv is a HOST pointer in both.  texels: (n_frames, n_r, n_phi) float32. */
int lt_shade_diskmovie_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                           const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                           const float *d_texels, double t_obs, const float *d_base, int32_t channels, float *d_rgb,
                           uint8_t *d_rgba);
int lt_shade_diskmovie(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                       const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                       const float *texels, double t_obs, const float *base, int32_t channels, float *out_rgb,
                       uint8_t *out_rgba);
int lt_shade_diskmovie_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                              int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                              const lt_diskmovie *movie, const float *d_texels, double t_obs,
                              const float *d_base /* (R S, W S, channels) or NULL */, int32_t channels,
                              float *d_rgb /* (R, W, channels) */, uint8_t *d_rgba /* (R, W, 4) */);
int lt_shade_diskmovie_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples,
                          int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                          const lt_diskmovie *movie, const float *texels, double t_obs, const float *base, int32_t channels,
                          float *out_rgb, uint8_t *out_rgba);
int lt_diskmovie_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                const float *d_texels, double t_start, double dt, int32_t n_times, double *d_out);
int lt_diskmovie_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                            const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                            const float *texels, double t_start, double dt, int32_t n_times, double *out);
int lt_diskmovie_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                              const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                              const float *d_texels, const lt_spectrum *spec, double t_start, double dt, int32_t n_times,
                              double *d_out);
int lt_diskmovie_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                          const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                          const float *texels, const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *out);
int lt_diskmovie_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                const float *d_texels, const double *uv, int32_t n_baselines, int32_t split_orders,
                                double t_start, double dt, int32_t n_times, double *d_out);
int lt_diskmovie_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                            const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                            const float *texels, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start,
                            double dt, int32_t n_times, double *out);

/* ---- polarized visibilities: Stokes I, Q, U of the stored hits on every baseline ------------------------------ *
 * What polarimetric interferometry measures: the Fourier transforms Q~(u, v) and U~(u, v) of the linearly polarized  *
 * image next to I~(u, v), and from them the fractional polarization m = (Q~ + i U~) / I~ on a baseline.  These entry  *
 * points are lt_disk_visibility / lt_hotspot_visibility ("visibilities") with the polarization records of           *
 * lt_trace_disk_pol ("linear polarization"): pol (R, W, max_images, 4) float32 = (q, u, sin zeta, mu) per stored     *
 * slot, and the field, of which only pol_frac (Pi) enters.  The rule, the phase, the limits, the times, the stored    *
 * slots and the order of every sum are those of "visibilities"; what is new is the Stokes axis.                     *
 *                                                                                                               *
 * Weights.  Per stored slot whose g is not NaN, in float64 from the float32 records and in exactly this order, every   *
 * product rounded:                                                                                               *
 *     w_I                                 the weight of lt_disk_visibility / lt_hotspot_visibility, unchanged          *
 *     w_Q = ((Pi sz sz) q) w_I            sz = sin zeta; Pi sz sz evaluated as (Pi sz) sz                            *
 *     w_U = ((Pi sz sz) u) w_I                                                                                      *
 * A slot whose g is NaN is skipped in all three.  A NaN in the slot's pol record propagates into Q~ and U~: it is the  *
 * record's answer.  Without split_orders a pixel's slots are added in slot order before the phase is applied, once     *
 * per Stokes parameter.                                                                                           *
 *                                                                                                               *
 * Output.  float64 (n_times, planes, 3, n_baselines, 2) holding (re, im), the Stokes axis (I, Q, U);                  *
 * lt_disk_visibility_stokes one row (1, planes, 3, n_baselines, 2) and no time.  planes as lt_*_visibility: 1, or      *
 * max_images with split_orders.  A plane without light is exactly 0 + 0i in all three.                              *
 *                                                                                                               *
 * Batches.  (time, plane) is flattened into a pair index k = time planes + plane over the whole call; a workgroup      *
 * keeps the sums of LT_VISIBILITY_STOKES_BATCH_PAIRS consecutive pairs in registers (three terms each, within         *
 * LT_VISIBILITY_BATCH_TERMS), so a batch may begin and end in the middle of a time.  Workspace, blocks, chunk order     *
 * and final stage are those of "visibilities".                                                                    *
 *                                                                                                               *
 * Guarantees.  The I plane has the bits of lt_disk_visibility / lt_hotspot_visibility for the same arguments.  The     *
 * same bits come out run after run; a row depends neither on its batch nor on its launch; a baseline's result does     *
 * not depend on what other baselines are asked for with it; V(-u, -v) is the bitwise conjugate of V(u, v) in all      *
 * three planes.  No floating-point atomics are used.                                                              *
 *                                                                                                               *
 * Refusals, in this order: everything the unpolarized entry point refuses, with its codes and in its order, through    *
 * the baselines; then LT_ERR_INVALID_ARG for a null pol, a null field and the field's own faults (direction not finite  *
 * or zero, pol_frac outside [0, 1]), as lt_shade_stokes words them; then the times; then a null out.  n_times = 0 is    *
 * LT_OK and writes nothing, even with a null out.  The outputs of a refused call are untouched.  Without a device      *
 * LT_ERR_NO_DEVICE, as everywhere.  disk.disk_visibility_stokes / disk.hotspot_visibility_stokes /                  *
 * disk.fractional_polarization (Python) state the rule in numpy.                                                   *
 *                                                                                                               *
 * Out of scope: the emissivity map (it is not polarized: image_lens.render_sequence refuses a map with a field),      *
 * circular polarization (Stokes V), Faraday rotation and conversion, closure quantities, lt_render_multi.            */
#define LT_VISIBILITY_STOKES_BATCH_PAIRS 5 /* (time, plane) pairs a workgroup accumulates at once: 15 of the 16 terms */

/* LT_VISIBILITY_STOKES_BATCH_PAIRS.  Needs no device. */
int32_t lt_visibility_stokes_batch_pairs(void);

/* Pointers as lt_*_visibility's: the _dev forms take DEVICE pointers for the records (hits, n_hits, pol) and the output
 * and enqueue on the default stream, the others HOST pointers; uv is a HOST pointer in both.
 * out: (n_times, planes, 3, n_baselines, 2) float64. */
int lt_disk_visibility_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                  int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_bfield *field,
                                  const double *uv, int32_t n_baselines, int32_t split_orders, double *d_out);
int lt_disk_visibility_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                              int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_bfield *field,
                              const double *uv, int32_t n_baselines, int32_t split_orders, double *out);
int lt_hotspot_visibility_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                     int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                     const lt_bfield *field, const double *uv, int32_t n_baselines, int32_t split_orders,
                                     double t_start, double dt, int32_t n_times, double *d_out);
int lt_hotspot_visibility_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                 int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                 const lt_bfield *field, const double *uv, int32_t n_baselines, int32_t split_orders,
                                 double t_start, double dt, int32_t n_times, double *out);

/* ---- thermal continuum: a radial flux table, its multi-colour blackbody spectrum and band images ------------------- *
 * Every product above shades the disk with one fixed law, exposure g^4 (r_in / r)^q, and has no frequency.  These      *
 * entry points give the disk a temperature: a radial flux profile F(r) -- Novikov-Thorne's, or any other the caller    *
 * tabulates -- makes every stored hit a blackbody at T = t_max F^(1/4), hardened by a colour-correction factor and     *
 * shifted by the hit's g.  lt_disk_thermal_spectrum is the multi-colour blackbody spectrum the continuum-fitting       *
 * method measures spin from, lt_shade_thermal the image in up to LT_THERMAL_MAX_BANDS narrow bands.  Two more          *
 * reductions over the records of lt_trace_disk_hits; nothing is traced again, and the disk's q and exposure are not    *
 * looked at beyond their refusals.                                                                                     *
 *                                                                                                                      *
 * Emitter.  lt_thermal and a float64 table flux[n_r]: node i sits at r_min + i (r_max - r_min) / (n_r - 1).  The FLUX  *
 * is tabulated and not the temperature: near the ISCO the flux is about quadratic in sqrt(r) - sqrt(r_isco), so linear *
 * interpolation holds, where the temperature has an infinite slope.  t_max is a frequency (k T / h at flux = 1), so    *
 * are the nu below, and 2 h / c^2 = 1.                                                                                 *
 *                                                                                                                      *
 * The rule, per stored slot (the stored slots are the re-shades': the first min(n_hits, max_images), or the leading    *
 * slots whose r is not NaN when n_hits is NULL), in float64 from the stored float32 (r, g), in exactly these steps --  *
 * each is one rounded operation or an explicit fma, whatever the compiler may contract:                                *
 *   1. r = (double)r32, g = (double)g32.  The slot emits nothing if g is NaN or g <= 0, or if r is NaN, r < r_min or r *
 *      > r_max (the float32 value compared exactly against the doubles).                                               *
 *   2. v = (r - r_min) inv_dr, a subtraction and then a product, with inv_dr = (n_r - 1) / (r_max - r_min) computed    *
 *      once on the host;  i0 = min((int)floor(v), n_r - 2);  w = v - i0, a subtraction of the rounded v.               *
 *   3. F = fma(w, flux[i0 + 1] - flux[i0], flux[i0]).  The slot emits nothing where !(F > 0).                          *
 *   4. T = t_max sqrt(sqrt(F));  c = 1.0 / ((g f_col) T).  A = exposure / ((f_col f_col) (f_col f_col)) is the same    *
 *      for every slot and computed once on the host.                                                                   *
 *   5. The observed specific intensity through this slot at frequency nu is nu^3 A / expm1(nu c), nu c rounded: this   *
 *      is exposure g^3 f_col^-4 B_{nu/g}(f_col T) with B_nu(T) = nu^3 / expm1(nu / T), the g^3 of the invariant I_nu / *
 *      nu^3 cancelling against (nu / g)^3; integrated over nu it is (pi^4 / 15) exposure g^4 T^4, the bolometric g^4   *
 *      of the other products.  The factor nu^3 is applied once per sum, not per term: a sum S of quotients becomes     *
 *      ((nu nu) nu) S, three rounded products.                                                                         *
 * expm1 is the only operation whose result the device library may round differently from another statement of the      *
 * rule. Where nu c overflows expm1 the term is +0.                                                                     *
 *                                                                                                                      *
 * Frequencies.  nu is n_freq float64 values, each finite and > 0, in any order.  They are not checked: nu = 0 gives    *
 * NaN where a slot emits (0 times infinity) and +0 elsewhere, a negative nu the formula's value with nu^3 < 0          *
 * (positive, or -0 where nothing emits), a NaN gives NaN.  Nor are the flux values: a NaN or non-positive F emits      *
 * nothing (step 3).                                                                                                    *
 *                                                                                                                      *
 * lt_disk_thermal_spectrum.  out: float64 (planes, n_freq), the flux density summed over all pixels and stored slots;  *
 * planes is 1, or max_images with split_orders: plane j then holds the hits stored in slot j.  n_freq <=               *
 * LT_THERMAL_MAX_FREQS.  A plane without an emitting slot is exactly +0.0. Order of every sum (it depends on R, W,     *
 * max_images and the records alone; no floating-point atomics anywhere, so a result is the same bits run after run,    *
 * whatever other frequencies are asked for with it and in whatever order). Workgroup b of LT_SPECTRUM_BLOCKS walks the *
 * chunks of 256 pixels p = 256 (b + k LT_SPECTRUM_BLOCKS) + i, k ascending (the light curve's stride order), and adds  *
 * to its sum of a plane and frequency, which starts at 0, the quotients A / expm1(nu c) of the chunk's emitting slots  *
 * ordered by wavefront i div 64, then lane i mod 64, then slot -- that is, in ascending i and then slot.  After its    *
 * last chunk it multiplies by nu^3.  The final stage adds the LT_SPECTRUM_BLOCKS partial sums, b ascending.  The       *
 * partials, at most LT_SPECTRUM_BLOCKS x 8 x 1024 x 8 B = 16 MiB, live in the spectra's grow-only workspace, in one    *
 * batch.                                                                                                               *
 *                                                                                                                      *
 * lt_shade_thermal.  out: float32 (n_freq, R, W), plane-major, n_freq <= LT_THERMAL_MAX_BANDS.  Per pixel and band the *
 * quotients of the pixel's emitting slots are added in slot order in float64, the sum is multiplied by nu^3 and        *
 * rounded once to float32.  No base, no clamp, no colour ramp: a pixel without an emitting slot is exactly +0.0.       *
 * split_orders is refused.  The image is linear in the records, so a supersampled image is the S x S mean of the fine  *
 * one per plane (aa.resolve on the host).                                                                              *
 *                                                                                                                      *
 * Refusals, in this order: those of lt_disk_spectrum up to and including the disk's q / exposure; then                 *
 * LT_ERR_INVALID_ARG for a null thermal / flux / nu; the struct's fields in the struct's order (the range, t_max,      *
 * f_col, exposure, n_r; split_orders for lt_shade_thermal); n_freq outside 0 ... the limit; and a null out.  n_freq =  *
 * 0 is LT_OK and writes nothing, even with a null out.  The outputs of a refused call are untouched. disk.ThermalDisk  *
 * / disk.novikov_thorne_flux / disk.thermal_coeffs / disk.thermal_spectrum / disk.shade_thermal (Python) state the     *
 * rule in numpy.                                                                                                       *
 *                                                                                                                      *
 * Out of scope: limb darkening and returning radiation, absolute units and a conversion from an accretion rate to      *
 * t_max, thermal light for the spot, the map and the movie, visibilities per frequency, a fused supersampled form,     *
 * lt_render_multi and the multi-process path, replacing the (r_in / r)^q law in the existing frames.                   */
#define LT_THERMAL_MAX_NODES 65536
#define LT_THERMAL_MAX_FREQS 1024
#define LT_THERMAL_MAX_BANDS 16

typedef struct lt_thermal {
    double r_min, r_max;  /* node i sits at r_min + i (r_max - r_min)/(n_r - 1); 0 < r_min < r_max, finite */
    double t_max;         /* T = t_max * flux^(1/4), as a frequency (kT/h); > 0, finite */
    double f_col;         /* colour-correction (hardening) factor; > 0, finite; default 1 */
    double exposure;      /* >= 0, finite */
    int32_t n_r;          /* 2 ... LT_THERMAL_MAX_NODES */
    int32_t split_orders; /* nonzero: one plane per stored slot (image order); lt_shade_thermal refuses it */
} lt_thermal;
void lt_default_thermal(lt_thermal *thermal); /* 6 ... 20, t_max 1, f_col 1, exposure 1, 2 nodes, not split */

/* The _dev forms take DEVICE pointers for the records, flux, nu and the output and enqueue on the default stream; the
 * others HOST pointers, staged like the spectra.  flux: thermal->n_r float64; nu: n_freq float64.
 * lt_disk_thermal_spectrum: out (planes, n_freq) float64.  lt_shade_thermal: out (n_freq, R, W) float32. */
int lt_disk_thermal_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                 const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                                 const double *d_flux, const double *d_nu, int32_t n_freq, double *d_out);
int lt_disk_thermal_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                             const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *flux,
                             const double *nu, int32_t n_freq, double *out);
int lt_shade_thermal_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                         const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *d_flux,
                         const double *d_nu, int32_t n_freq, float *d_out);
int lt_shade_thermal(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                     const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *flux,
                     const double *nu, int32_t n_freq, float *out);

/* ---- polarized thermal continuum: a scattering atmosphere's limb darkening and its Stokes I, Q, U ----------------- *
 * The thermal continuum above treats every hit as an isotropic, unpolarized blackbody.  A thin disk's surface is a    *
 * scattering atmosphere (Chandrasekhar): its light is limb-darkened and linearly polarized parallel to the surface,   *
 * by up to 11.7 % at grazing emission, and because the hot inner disk's light is swung round by the hole the net      *
 * angle turns with energy -- what X-ray polarimetry measures.  These entry points are lt_disk_thermal_spectrum and    *
 * lt_shade_thermal with a weight per slot and Stokes parameter.  Nothing is traced again, and no record is new.       *
 *                                                                                                                     *
 * Records.  pol: float32 (R, W, max_images, 4), (q, u, sin zeta, mu) per slot as lt_trace_disk_pol writes them,       *
 * TRACED WITH THE FIELD (0, 0, 1): the polarization rule takes the electric vector along k^ x b^, which for a field   *
 * along the disk's normal is k^ x e_(z), the direction perpendicular to the plane of the normal and the ray -- the    *
 * scattering atmosphere's --, and mu = |k^ . e_(z)| is the cosine both tables below depend on.  The call cannot see   *
 * which field was traced: records of another field give that field's angles.  sin zeta and the field's pol_frac play  *
 * no part.                                                                                                            *
 *                                                                                                                     *
 * Atmosphere.  lt_atmosphere and two float64 tables of n_mu nodes, node i at mu_i = i / (n_mu - 1): limb[i], the      *
 * limb-darkening factor h(mu), 1 meaning isotropic, and poldeg[i], the polarization degree delta(mu).  Neither table  *
 * is checked, as flux is not.                                                                                         *
 *                                                                                                                     *
 * The rule, per stored slot.  Steps 1 to 5 of the thermal continuum stay exactly as they are.  After them:            *
 *   6. mu = (double)pol[3].  The slot emits nothing unless mu >= 0 && mu <= 1 (a NaN fails).  v = mu (double)(n_mu -  *
 *      1), one rounded product;  i0 = max(min((int)floor(v), n_mu - 2), 0);  w = v - i0; h = fma(w, limb[i0 + 1] -    *
 *      limb[i0], limb[i0]);  d = fma(w, poldeg[i0 + 1] - poldeg[i0], poldeg[i0]).                                     *
 *   7. w_I = h,  w_Q = (h d) (double)pol[0],  w_U = (h d) (double)pol[1], every product rounded.                      *
 *   8. With t = A / expm1(nu c) as in step 5, each of the three sums takes S = fma(w_X, t, S), an explicit fma, in    *
 *      the order of lt_disk_thermal_spectrum -- chunk, then wavefront, lane and slot --; afterwards ((nu nu) nu) S,   *
 *      and the final stage adds the LT_SPECTRUM_BLOCKS partials, b ascending.                                         *
 * Consequences.  With limb identically 1 (and every stored mu in [0, 1]) the I plane has the bits of                  *
 * lt_disk_thermal_spectrum, because fma(1, t, S) = S + t, and the band images' I plane those of lt_shade_thermal.     *
 * With poldeg identically 0 (and h >= 0) Q and U are exactly +0.0.  A frequency's result does not depend on the other *
 * frequencies or on their order, and the same bits come out run after run: no floating-point atomics anywhere.        *
 *                                                                                                                     *
 * lt_disk_thermal_spectrum_stokes.  out: float64 (planes, 3, n_freq), the Stokes axis (I, Q, U); planes and n_freq as *
 * lt_disk_thermal_spectrum.  A plane without an emitting slot is exactly +0.0 in all three.  The partials, at most    *
 * LT_SPECTRUM_BLOCKS x 8 x 3 x 1024 x 8 B = 48 MiB, live in the spectra's grow-only workspace, in one batch.          *
 *                                                                                                                     *
 * lt_shade_thermal_stokes.  out: float32 (n_freq, 3, R, W), plane-major, n_freq <= LT_THERMAL_MAX_BANDS.  Per pixel,  *
 * band and Stokes parameter the emitting slots' terms are added in slot order in float64 by step 8's fma, the sum is  *
 * multiplied by nu^3 and rounded once to float32, as lt_shade_thermal does.  split_orders is refused.                 *
 *                                                                                                                     *
 * Refusals, in this order: everything lt_disk_thermal_spectrum / lt_shade_thermal refuses up to and including the     *
 * struct's fields (split_orders for the band images), in their order; then LT_ERR_INVALID_ARG for a null pol /        *
 * atmosphere / limb / poldeg; n_mu outside 2 ... LT_ATMOSPHERE_MAX_NODES; n_freq outside 0 ... the limit; and a null  *
 * out.  n_freq = 0 is LT_OK and writes nothing, even with a null out.  The outputs of a refused call are untouched.   *
 * disk.Atmosphere / disk.atmosphere_weights / disk.thermal_spectrum_stokes / disk.shade_thermal_stokes /              *
 * disk.polarization_degree_angle (Python) state the rule in numpy.                                                    *
 *                                                                                                                     *
 * Out of scope: returning radiation, ionised or absorbing atmospheres, Stokes V, the atmosphere for the spot, the map *
 * and the movie, visibilities per frequency, a fused supersampled form, lt_render_multi.                             */
#define LT_ATMOSPHERE_MAX_NODES 4096

typedef struct lt_atmosphere {
    int32_t n_mu;     /* nodes of the two tables, node i at mu = i / (n_mu - 1); 2 ... LT_ATMOSPHERE_MAX_NODES */
    int32_t reserved; /* not looked at */
} lt_atmosphere;

/* The _dev forms take DEVICE pointers for the records, the tables, nu and the output and enqueue on the default stream;
 * the others HOST pointers, staged like lt_disk_thermal_spectrum.  pol: (R, W, max_images, 4) float32; flux:
 * thermal->n_r float64; limb, poldeg: atmosphere->n_mu float64 each; nu: n_freq float64.
 * lt_disk_thermal_spectrum_stokes: out (planes, 3, n_freq) float64.  lt_shade_thermal_stokes: out (n_freq, 3, R, W)
 * float32. */
int lt_disk_thermal_spectrum_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R,
                                        int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                                        const lt_thermal *thermal, const double *d_flux, const lt_atmosphere *atmosphere,
                                        const double *d_limb, const double *d_poldeg, const double *d_nu, int32_t n_freq,
                                        double *d_out);
int lt_disk_thermal_spectrum_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                    int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                                    const lt_thermal *thermal, const double *flux, const lt_atmosphere *atmosphere,
                                    const double *limb, const double *poldeg, const double *nu, int32_t n_freq,
                                    double *out);
int lt_shade_thermal_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                                const double *d_flux, const lt_atmosphere *atmosphere, const double *d_limb,
                                const double *d_poldeg, const double *d_nu, int32_t n_freq, float *d_out);
int lt_shade_thermal_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                            int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                            const double *flux, const lt_atmosphere *atmosphere, const double *limb, const double *poldeg,
                            const double *nu, int32_t n_freq, float *out);

/* ---- reverberation: the disk's response to a flash, a delay-energy transfer function ------------------------------- *
 * Every product above asks what the disk looks like at an observer time.  X-ray timing asks the converse: a compact    *
 * source above the hole flashes once -- when, and at what energy, does the disk's echo arrive?  The answer is the 2-D  *
 * transfer function psi(tau, g): the stored hits binned by the redshift factor g AND by the delay tau between the      *
 * direct flash and the echo through that hit.  Summed over tau it is the broadened line (lt_disk_spectrum's, with the  *
 * emissivity below); summed over g the impulse response.  One more reduction over the records of lt_trace_disk_hits;   *
 * nothing is traced again.  Of lt_disk only `exposure` is used; its q is not looked at beyond its refusal.             *
 *                                                                                                                      *
 * Emitter.  lt_transfer and two float64 tables of n_r nodes, node i at r_min + i (r_max - r_min) / (n_r - 1):          *
 * delay[i], the coordinate time light takes from the source to the disk at that radius, and emis[i], what the disk     *
 * re-emits there per unit of the flash, any non-negative profile.  The physics of the source lives in the tables alone *
 * (disk.lamppost_tables builds them for a point source on the spin axis); t_ref, the direct flash's own arrival time   *
 * at the camera, is subtracted from every delay.                                                                       *
 *                                                                                                                      *
 * The rule, per stored slot (the stored slots are the re-shades': the first min(n_hits, max_images), or the leading    *
 * slots whose r is not NaN when n_hits is NULL), in float64 from the stored float32 (r, g, dt), in exactly these steps *
 * -- each is one rounded operation or an explicit fma, whatever the compiler may contract:                             *
 *   1. r = (double)r32, g = (double)g32, dt = (double)dt32.  The slot contributes nothing if g is NaN or g <= 0, if dt *
 *      is NaN, or if r is off the table, !(r >= r_min && r <= r_max) (a NaN r included).                               *
 *   2. v = (r - r_min) inv_dr, a subtraction and then a rounded product, with inv_dr = (n_r - 1) / (r_max - r_min)     *
 *      computed once on the host;  i0 = min((int)v, n_r - 2);  w = v - i0, a subtraction of the rounded v.             *
 *   3. eps = fma(w, emis[i0 + 1] - emis[i0], emis[i0]).  The slot contributes nothing where !(eps > 0).                *
 *      t_ld = fma(w, delay[i0 + 1] - delay[i0], delay[i0]).                                                            *
 *   4. tau = (t_ld + dt) - t_ref, two rounded operations.  Its bin is the spectrum's rule on the delay grid:           *
 *          inv_dtau = n_tau / (tau_max - tau_min)          (computed once on the host)                                 *
 *          k_tau = tau < tau_min ? 0 : tau >= tau_max ? n_tau + 1                                                      *
 *                                    : 1 + min((int)floor((tau - tau_min) * inv_dtau), n_tau - 1)                      *
 *      a subtraction followed by a multiplication.  Column 0 is the underflow, column n_tau + 1 the overflow, bin      *
 *      k = 1 ... n_tau is half-open.  A NaN tau (a NaN table node) contributes nothing.  The bin of g, k_g, is         *
 *      lt_spectrum's, unchanged ("energy-resolved light"), with its underflow and overflow columns.                    *
 *   5. The weight is (exposure ((g g) (g g))) eps: g^4 bracketed as the disk's own intensity brackets it, then two     *
 *      rounded products from the left.  A weight of exactly 0 is not added.                                            *
 *                                                                                                                      *
 * Output.  float64 (planes, n_tau + 2, n_bins + 2); planes is 1, or max_images with spec->split_orders: plane j then   *
 * holds the hits stored in slot j.  Key = (plane (n_tau + 2) + k_tau) (n_bins + 2) + k_g.  An empty key is exactly     *
 * +0.0.  The keys are capped: planes (n_tau + 2) (n_bins + 2) <= LT_TRANSFER_MAX_KEYS, which makes the                 *
 * LT_SPECTRUM_BLOCKS partials exactly the spectra's workspace of LT_SPECTRUM_WORKSPACE_BYTES, in one batch.  A finer   *
 * grid is several calls on adjacent delay ranges: the bin rule makes them tile exactly -- every tau falls into the     *
 * same bin of the part as of the whole -- when the ranges share inv_dtau, each part's tau_min is the whole's tau_min   *
 * plus a whole number of bins, and tau - tau_min and its product with inv_dtau are exact in both (tau_min = 0 and a    *
 * bin width that is a power of two make it so).  Where the subtraction or the product rounds, a tau within that one    *
 * rounding below an edge between two parts is in the whole's upper bin and in the lower part's last one: the part      *
 * clamps at its end, the whole has no end there.  This is lt_spectrum's rule and as rare as a g on an edge's last bit. *
 *                                                                                                                      *
 * Order of every sum: the spectra's, word for word.  Workgroup b of LT_SPECTRUM_BLOCKS walks the chunks of 256 pixels  *
 * p = 256 (b + c LT_SPECTRUM_BLOCKS) + i, c ascending.  Within a chunk, wavefront w = i div 64 adds, for every slot j, *
 * the weights of a key over its 64 lanes l = i mod 64 with the butterfly l ^ 32, l ^ 16, ... l ^ 1 (lanes without that *
 * key add +0.0, which changes no bit).  The owner of a key adds these sums to the workgroup's accumulator ordered by   *
 * w, then j; the final stage adds the LT_SPECTRUM_BLOCKS partials per key, b ascending.  The order depends on R, W and *
 * max_images alone: not on how the kernel divides the key space among workgroups, nor on which other keys exist, so a  *
 * key's bits are the same in a small grid and inside a large one.  No floating-point atomics anywhere.                 *
 *                                                                                                                      *
 * Supersampled records.  Called with the fine records (R S, W S) the result divided by S^2 is in output-pixel units,   *
 * as the spectra's (image_lens.render_sequence does so).                                                               *
 *                                                                                                                      *
 * Refusals, in this order: those of lt_disk_spectrum up to and including the disk's q / exposure; the grid's (a null   *
 * spec, the g range, n_bins); then LT_ERR_INVALID_ARG for a null transfer; the tau range (finite, tau_min < tau_max);  *
 * n_tau; n_r; the r range (0 < r_min < r_max, finite); a non-finite t_ref; a null delay / emis; the key cap; and a     *
 * null out.  The outputs of a refused call are untouched.  disk.TransferGrid / disk.transfer_bin / disk.disk_transfer  *
 * (Python) state the rule in numpy; disk.Lamppost / disk.lamppost_tables build the tables of a lamp-post corona.       *
 *                                                                                                                      *
 * Out of scope: off-axis or extended coronae, the ionisation state and a rest-frame reflection spectrum other than a   *
 * line, returning radiation, the response of the spot, the map or the movie, polarized or per-pixel responses,         *
 * logarithmic delay grids, lt_render_multi and the multi-process path, adaptive sampling.                              */
#define LT_TRANSFER_MAX_TAU 1024
#define LT_TRANSFER_MAX_KEYS 32768

typedef struct lt_transfer {
    double tau_min, tau_max; /* the delay grid's ends, finite, tau_min < tau_max (tau_min may be negative) */
    int32_t n_tau;           /* 1 ... LT_TRANSFER_MAX_TAU */
    int32_t n_r;             /* nodes of the two tables, 2 ... LT_THERMAL_MAX_NODES */
    double r_min, r_max;     /* node i sits at r_min + i (r_max - r_min)/(n_r - 1); 0 < r_min < r_max, finite */
    double t_ref;            /* subtracted from every delay: the direct flash's own arrival time at the camera; finite */
} lt_transfer;
void lt_default_transfer(lt_transfer *transfer); /* tau 0 ... 256, 64 bins, 2 nodes on 6 ... 20, t_ref 0 */

/* The _dev form takes DEVICE pointers for the records, the two tables and the output and enqueues on the default
 * stream; the other HOST pointers, staged like lt_disk_thermal_spectrum.  delay, emis: transfer->n_r float64 each.
 * out: (planes, n_tau + 2, n_bins + 2) float64. */
int lt_disk_transfer_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                         const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, const lt_transfer *transfer,
                         const double *d_delay, const double *d_emis, double *d_out);
int lt_disk_transfer(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                     const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, const lt_transfer *transfer,
                     const double *delay, const double *emis, double *out);

/* ---- supersampled (anti-aliased) frames, resolved on the GPU ------------------------------------------- *
 * Every frame above is one ray per pixel, taken at the pixel's corner.  These entry points trace S x S rays per       *
 * pixel and write only the resolved pixels: nothing of the S^2 times larger frame crosses PCIe or stays in memory.    *
 *                                                                                                               *
 * Fine frame.  For a camera (W, H, hfov, vfov, psi, r_obs, theta_obs) and samples = S (1 <= S <= LT_AA_MAX_SAMPLES)  *
 * the fine frame is the same camera with width = W S and height = H S.  The camera model uses pixel corners,        *
 * x_cam = (ix - W/2) / fx, so fine pixel (y S + j, x S + i) is sub-sample (j, i) of output pixel (y, x), and          *
 * sub-sample (0, 0) is the ray lt_render traces for that pixel.  There is no new camera arithmetic.                  *
 *                                                                                                               *
 * Modes.  The colour of a fine pixel is the colour an existing entry point gives the fine frame:                     *
 *   LT_AA_PLAIN        lt_render_dev with tb_symmetry = 0 (opts->tb_symmetry is ignored);                              *
 *   LT_AA_DISK         lt_render_disk_dev with `disk`;                                                                *
 *   LT_AA_DISK_IMAGES  lt_render_disk_images_dev with `disk` and aa->max_images.                                      *
 *                                                                                                               *
 * Background.  d_bg is a full FINE-size image (H S, W S, bg_channels), the whole frame on every partition, or NULL      *
 * (the mode's render without a background).  A fine pixel looks its texel up with the fine frame's own W S, H S,      *
 * exactly as the mode's entry point does when it is given the fine camera and this image.                            *
 *                                                                                                               *
 * Resolve.  For every output pixel and channel: take the float32 colour the mode's epilogue writes for each of the    *
 * pixel's S^2 fine pixels; add them in float64 in row-major order -- j outer, i inner -- starting from 0.0; divide    *
 * by (double)(S S); round to float32.  RGBA8 follows from that float32 as everywhere: (x 255) truncated, alpha 255.   *
 * So rgb is, bit for bit, that box filter of the rgb the mode's entry point returns for the fine frame, and with      *
 * samples = 1 it is that entry point's rgb / rgba themselves.                                                         *
 *                                                                                                               *
 * Coverage.  d_cover (R, W, 4) uint8: how many of the pixel's S^2 sub-rays escaped, were captured, were invalid,       *
 * and hit the disk.  LT_AA_DISK: slot 3 counts status LT_STATUS_DISK and the four slots sum to S^2.                   *
 * LT_AA_DISK_IMAGES: slot 3 counts the rays with at least one hit and the first three slots sum to S^2.               *
 * LT_AA_PLAIN: slot 3 is 0.                                                                                          *
 *                                                                                                               *
 * Stats.  Words 0-5, LT_STAT_DISK and LT_STAT_DISK_HITS are the fine frame's (rays = S^2 R W); so are the integrate    *
 * kernel's words 6-9.  Kernel times are summed over the bands.                                                       *
 *                                                                                                               *
 * Partitions.  n_parts, part, row_block and block_owner refer to OUTPUT rows, and outputs are (R, W) compact with     *
 * R = lt_local_rows(H, ...) as everywhere.  A partition's fine rows are the fine frame's partition with row blocks    *
 * of row_block S rows and the same table.                                                                            *
 *                                                                                                               *
 * Bands.  A call renders its rows in bands of aa->band_rows output rows (a multiple of row_block; a partition's rows *
 * in its local order): prologue, the mode's integrate kernel and the resolve epilogue run band after band on the      *
 * stream, so the (device, stream) workspace never holds more than one band's ray records.  band_rows = 0: automatic,  *
 * the largest band whose records (three 4-vectors of the precision per ray of the fine tiles, plus the thin disk's    *
 * slots) fit LT_AA_BAND_BYTES; a band never has more than 65535 fine rows.  Results do not depend on the banding.      *
 * A call of several bands uploads the partition's block list once, like a block_owner table (a wait for the stream   *
 * the first time, none when the same call is repeated), and every band reads its piece of it.  The ray records are   *
 * reused as for lt_render_dev: a one-band call repeated with equal inputs on a stream reuses its own, and whatever   *
 * call follows on the stream sees the key of the last band rendered, which is a fine-frame key.                      *
 *                                                                                                               *
 * Refusals.  samples outside [1, LT_AA_MAX_SAMPLES], an unknown mode, a disk mode with disk = NULL, band_rows < 0 or   *
 * not a multiple of row_block: LT_ERR_INVALID_ARG.  The mode's own refusals apply unchanged (LT_METRIC_SCHWARZSCHILD  *
 * or LT_SCHED_QUEUE with a disk mode: LT_ERR_UNSUPPORTED; the disk's parameters as lt_render_disk_dev); the plain     *
 * mode accepts what lt_render_dev accepts.  No GPU: LT_ERR_NO_DEVICE.                                                 */
#define LT_AA_PLAIN 0
#define LT_AA_DISK 1
#define LT_AA_DISK_IMAGES 2
#define LT_AA_MAX_SAMPLES 8
#define LT_AA_BAND_BYTES ((int64_t)2 << 30) /* 2 GiB: the record budget of an automatic band (a 4096^2 fine frame in
                                               float32 is 0.75 GiB and stays one band; 8192^2 becomes two) */

typedef struct lt_aa {
    int32_t samples;    /* S: S x S rays per pixel, 1 ... LT_AA_MAX_SAMPLES (2) */
    int32_t mode;       /* LT_AA_*                                                */
    int32_t max_images; /* LT_AA_DISK_IMAGES: slots per ray (3)                   */
    int32_t band_rows;  /* output rows per band; 0 = automatic                    */
} lt_aa;
void lt_default_aa(lt_aa *a);

/* DEVICE pointers (any output may be NULL = not wanted), sized for R = the partition's output rows:
 *   d_bg    (H S, W S, bg_channels) float32 or NULL;  bg_channels 1 or 3
 *   d_rgb   (R, W, bg_channels or 3) float32          d_rgba (R, W, 4) uint8
 *   d_cover (R, W, 4) uint8                           d_stats LT_STAT_WORDS uint64, ACCUMULATED into
 * disk: NULL for LT_AA_PLAIN.  Asynchronous on opts->stream; opts->timing as lt_render_dev, one record per band. */
int lt_render_aa_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                     const lt_disk *disk, const float *d_bg, int32_t bg_channels, float *d_rgb, uint8_t *d_rgba,
                     uint8_t *d_cover, uint64_t *d_stats);
/* The same with HOST pointers, staged like lt_render: the fine-size background goes in, only the resolved outputs
 * come back.  stats may be NULL. */
int lt_render_aa(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                 const lt_disk *disk, const float *bg, int32_t bg_channels, float *out_rgb, uint8_t *out_rgba,
                 uint8_t *out_cover, lt_stats *stats);
/* What a call with these arguments would do, from host arithmetic alone (needs no device): returns the bytes of ray
 * records its largest band needs in the (device, stream) workspace, or a negative LT_ERR_* with the call's refusals;
 * *band_rows = output rows per band, *n_bands = bands of this partition (either may be NULL). */
int64_t lt_aa_band_bytes(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                         const lt_disk *disk, int32_t *band_rows, int32_t *n_bands);

/* ---- adaptive supersampling: refine only the pixels on an edge ---------------------------------------- *
 * lt_render_aa traces S x S rays for EVERY pixel; almost everywhere they agree.  These entry points render the frame *
 * at samples_lo, find the pixels that lie on an edge from that pass's own outputs, and trace only those at samples_hi. *
 * No ray is new: every pixel of the result is a pixel of one of two lt_render_aa frames.                             *
 *                                                                                                               *
 * Write LO for what lt_render_aa returns with samples = S_lo and a background of (H S_lo, W S_lo), HI for            *
 * samples = S_hi and a background of (H S_hi, W S_hi); camera, metric, opts, mode and disk are the call's.           *
 *                                                                                                               *
 * Refined pixels.  A pixel p is refined when any of these holds, N(p) being its 3 x 3 neighbourhood clipped to the   *
 * frame, p itself excluded:                                                                                     *
 *   mixed     LO.cover[p] has more than one non-zero slot.  LT_AA_PLAIN and LT_AA_DISK look at slots 0-3;             *
 *             LT_AA_DISK_IMAGES, whose slot 3 overlaps the others, looks at slots 0-2, or flags                      *
 *             0 < LO.cover[p][3] < S_lo^2;                                                                      *
 *   edge      some n in N(p) has LO.cover[n] != LO.cover[p], compared as 4 bytes;                                    *
 *   contrast  contrast >= 0, and some n in N(p) and some channel has fabsf(LO.rgb[p][ch] - LO.rgb[n][ch]) > contrast *
 *             in float32 (a difference equal to contrast does not count).  This finds what cover cannot see: the    *
 *             photon ring, where a 1-hit pixel lies next to a 2-hit pixel, winding-colour seams, a background that   *
 *             aliases.  contrast < 0 switches the test off.                                                      *
 *                                                                                                               *
 * Outputs.  rgb, rgba and cover are HI's at refined pixels and LO's elsewhere, bit for bit.  level (H, W) uint8 is    *
 * S_hi where the pixel was refined and S_lo elsewhere: a pixel's cover slots sum to level^2 (LT_AA_DISK_IMAGES: its   *
 * first three slots do).  With S_lo = 1 every unrefined pixel is exactly the mode's own one-ray pixel.  Nothing       *
 * depends on the order in which refined pixels are found, on band_rows or on chunk_pixels.                           *
 *                                                                                                               *
 * Stats.  Words 0-5, LT_STAT_DISK and LT_STAT_DISK_HITS are the base pass's plus the refined rays', so               *
 * rays = S_lo^2 W H + S_hi^2 N; LT_STAT_AA_REFINED is N, the number of refined pixels.  Kernel times are summed over   *
 * the base pass's bands and the refined pass's chunks; the kernel that applies the three tests counts as prologue.   *
 *                                                                                                               *
 * Passes.  The base pass is lt_render_aa_dev's, in bands of band_rows.  The refined pixels are then traced in chunks *
 * of chunk_pixels pixels (0: automatic, the most pixels whose S_hi^2 ray records each fit LT_AA_BAND_BYTES), each a    *
 * prologue, the mode's integrate kernel and a resolve epilogue that overwrites the listed pixels.  The refined pass  *
 * overwrites the ray records of the (device, stream) workspace: the frame that follows on the stream reuses nothing. *
 *                                                                                                               *
 * Partitions.  The 3 x 3 test reads rows a partition does not own: n_parts != 1 and a block_owner table are refused   *
 * with LT_ERR_UNSUPPORTED.                                                                                      *
 *                                                                                                               *
 * Other refusals.  samples_lo outside [1, 4], samples_hi outside (samples_lo, LT_AA_MAX_SAMPLES], a NaN contrast, a    *
 * negative chunk_pixels, one background without the other, a frame of more than 2^31 - 1 pixels: LT_ERR_INVALID_ARG. *
 * Everything else is refused as lt_render_aa refuses it: the mode's own refusals, band_rows, a disk mode without a    *
 * disk.  No GPU: LT_ERR_NO_DEVICE.                                                                               */
typedef struct lt_aa_adaptive {
    int32_t samples_lo;   /* base pass: S_lo x S_lo rays for every pixel, 1 ... 4   (1) */
    int32_t samples_hi;   /* refined pixels: S_hi x S_hi rays, S_lo < S_hi <= LT_AA_MAX_SAMPLES (4) */
    int32_t mode;         /* LT_AA_*                                                   */
    int32_t max_images;   /* LT_AA_DISK_IMAGES (3)                                      */
    int32_t band_rows;    /* base pass, as lt_aa.band_rows; 0 = automatic              */
    int32_t chunk_pixels; /* refined pass: pixels per chunk; 0 = automatic (records within LT_AA_BAND_BYTES) */
    float   contrast;     /* colour test threshold; < 0: off (default 0.0625f)         */
    int32_t reserved;
} lt_aa_adaptive;
void lt_default_aa_adaptive(lt_aa_adaptive *a);

/* DEVICE pointers (any output may be NULL = not wanted; what the refinement tests read of the base pass -- cover,
 * and rgb when contrast >= 0 -- then lives in the library's own buffers of the stream):
 *   d_bg_lo (H S_lo, W S_lo, bg_channels), d_bg_hi (H S_hi, W S_hi, bg_channels) float32: both NULL or both given
 *   d_rgb (H, W, bg_channels or 3) float32   d_rgba (H, W, 4) uint8   d_cover (H, W, 4) uint8   d_level (H, W) uint8
 *   d_stats LT_STAT_WORDS uint64, ACCUMULATED into
 * Enqueued on opts->stream, but NOT asynchronous: the call waits for its stream ONCE, between the passes, to read the
 * number of refined pixels -- the refined pass's launch sizes need it (so it cannot be captured into a graph); what it
 * enqueues after that is not waited for.  opts->timing as lt_render_dev: one record per band, one for the flag kernel, one
 * per chunk. */
int lt_render_aa_adaptive_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *adaptive,
                              const lt_disk *disk, const float *d_bg_lo, const float *d_bg_hi, int32_t bg_channels,
                              float *d_rgb, uint8_t *d_rgba, uint8_t *d_cover, uint8_t *d_level, uint64_t *d_stats);
/* The same with HOST pointers, staged like lt_render_aa: the two backgrounds go in, only the resolved outputs come
 * back.  stats may be NULL. */
int lt_render_aa_adaptive(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *adaptive,
                          const lt_disk *disk, const float *bg_lo, const float *bg_hi, int32_t bg_channels, float *out_rgb,
                          uint8_t *out_rgba, uint8_t *out_cover, uint8_t *out_level, lt_stats *stats);
/* What a call with these arguments would do, from host arithmetic alone (needs no device): 0, or the call's refusal.
 * *base_band_bytes = bytes of ray records the base pass's largest band needs, *chunk_pixels = refined pixels per chunk
 * (either may be NULL). */
int lt_aa_adaptive_plan(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *adaptive,
                        const lt_disk *disk, int64_t *base_band_bytes, int64_t *chunk_pixels);

/* Sum of HIP-event times (ms) of the prologue / integrate / epilogue kernels over all
 * lt_render_dev calls made with opts->timing != 0 since the last collect; *calls = how many.
 * Synchronises on the recorded events. */
int lt_timing_collect(double *prologue_ms, double *integrate_ms, double *epilogue_ms, int32_t *calls);

/* The ray records the camera prologue writes depend on the camera, the metric, the row partition and the precision
 * only, and stay in the (device, stream) workspace: a frame whose inputs equal those of the frame before it on the same
 * stream reuses them instead of running the prologue again (LT_IC_REUSE=0 in the environment: never).  Every frame still
 * traces and shades every ray.  *hits = frames that reused their records, *misses = frames that ran the prologue, both
 * since the library was loaded, over all devices and streams; either may be NULL.  Needs no device. */
void lt_ic_reuse_counts(uint64_t *hits, uint64_t *misses);

#ifdef __cplusplus
}
#endif
#endif /* LTRACE_H */
