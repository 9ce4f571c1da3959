// lt_api_disk.inc -- included at the end of lt_api.hip.
//
// Host side of the thin accretion disk (include/ltrace.h, "thin Keplerian accretion disk"): parameter checks, the
// launches of the disk kernels of lt_disk.hpp, and the entry points.  The frame plumbing (camera, partitions,
// workspaces, staging, timing) is lt_render's: render_dev_impl / render_host_impl / trace_batch with a DiskParams.

// Bardeen-Press-Teukolsky: the innermost stable circular equatorial orbit of the orbit direction +phi
extern "C" double lt_kerr_isco(double M, double a)
{
    if (!(M > 0.0) || !(fabs(a) <= M)) return NAN;
    const double x = fabs(a) / M;
    const double z1 = 1.0 + cbrt(1.0 - x * x) * (cbrt(1.0 + x) + cbrt(1.0 - x));
    const double z2 = sqrt(3.0 * x * x + z1 * z1);
    const double sgn = a < 0.0 ? -1.0 : 1.0;
    return M * (3.0 + z2 - sgn * sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)));
}

extern "C" void lt_default_disk(lt_disk *d)
{
    memset(d, 0, sizeof(*d));
    d->r_in = 0.0; // the ISCO
    d->r_out = 20.0;
    d->q = 3.0;
    d->exposure = 1.0;
}

// Refusals and the resolved inner edge.  `schedule`: LT_SCHED_* of the call (the queue schedule has no disk variant).
// max_images: NULL for the opaque disk, else the optically thin disk's slots per ray.
static int resolve_disk(const lt_metric *metric, double r_obs, int schedule, const lt_disk *disk, const int32_t *max_images,
                        DiskParams *dp)
{
    if (!metric || !disk) return fail(LT_ERR_INVALID_ARG, "null metric / disk");
    if (metric->kind != LT_METRIC_KERR)
        return fail(LT_ERR_UNSUPPORTED, "the disk needs LT_METRIC_KERR: for a Schwarzschild hole use Kerr with a = 0");
    if (schedule != LT_SCHED_DIRECT) return fail(LT_ERR_UNSUPPORTED, "the disk is traced with the direct schedule only");
    if (!(metric->M > 0.0) || !(fabs(metric->a) <= metric->M)) return fail(LT_ERR_INVALID_ARG, "bad metric (M %g, a %g)", metric->M, metric->a);
    const double isco = lt_kerr_isco(metric->M, metric->a);
    const double r_in = disk->r_in <= 0.0 ? isco : disk->r_in;
    // (the ISCO itself, computed by a caller with another libm, may differ from ours in the last bits)
    if (!(r_in >= isco * (1.0 - 1e-12)))
        return fail(LT_ERR_INVALID_ARG, "disk r_in %g lies inside the ISCO %g", r_in, isco);
    if (!(disk->r_out > r_in) || !(disk->r_out < r_obs))
        return fail(LT_ERR_INVALID_ARG, "disk needs r_in < r_out < r_obs (r_in %g, r_out %g, r_obs %g)", r_in, disk->r_out, r_obs);
    if (!std::isfinite(disk->q) || !(disk->exposure >= 0.0) || !std::isfinite(disk->exposure))
        return fail(LT_ERR_INVALID_ARG, "disk q / exposure must be finite, exposure >= 0");
    dp->r_in = r_in;
    dp->r_out = disk->r_out;
    dp->q = disk->q;
    dp->exposure = disk->exposure;
    dp->d_disk = nullptr;
    if (!max_images) return LT_OK;
    if (*max_images < 1 || *max_images > DISK_MAX_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", (int)*max_images, DISK_MAX_IMAGES);
    dp->max_images = *max_images;
    return LT_OK;
}

// What the disk frame entry points do before the frame plumbing takes over.
static int disk_frame_setup(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                            const int32_t *max_images, DiskParams *dp)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / opts");
    return resolve_disk(metric, cam->r_obs, opts->schedule, disk, max_images, dp);
}

// ... and the batch twins: the disk first, then lt_trace_batch_kerr's set-up on the direct schedule.
static int disk_batch_setup(const lt_metric *m, double r_obs, double theta_obs, int integrator, int precision, const lt_disk *disk,
                            const int32_t *max_images, DiskParams *dp, lt_opts *o, MetricConsts *mc)
{
    int rc = require_device();
    if (rc || (rc = resolve_disk(m, r_obs, LT_SCHED_DIRECT, disk, max_images, dp))) return rc;
    return kerr_batch_setup(m, r_obs, theta_obs, integrator, precision, LT_SCHED_DIRECT, o, mc);
}

// The disk's constants as the integrate kernels get them: the annulus and 1 / r_plus^2 rounded to T.
template <typename T> static DiskConsts<T> make_disk_consts(const MetricConsts &mc, const DiskParams &dp)
{
    return DiskConsts<T>{(T)dp.r_in, (T)dp.r_out, (T)(1.0 / (mc.r_plus * mc.r_plus))};
}

// The integrate launch of both disks: the direct schedule of launch_integrate (launch_direct) with the disk's kernels,
// 64-wide workgroups, no stamps.  dp.max_images > 0: the thin disk, which also gets its records (recs).
template <typename T>
static int launch_integrate_disk(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w, int64_t n_q,
                                 hipStream_t s, uint64_t *kstats, const DiskParams &dp, const DiskRecordsBuf &recs)
{
    const KerrConsts<T> k = make_kerr<T>(mc, lambda_max, o.h_max);
    const DiskConsts<T> d = make_disk_consts<T>(mc, dp);
    if (dp.pol)
        return launch_direct<T, DiskPolKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
            kernel<<<grid, 64, 0, s>>>(k, d, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q, long_iters, kstats, head, recs.img<T>(), recs.hits,
                                       dp.max_images, (T *)recs.tim, (typename Vec2<T>::type *)recs.mom);
        });
    if (dp.timed)
        return launch_direct<T, DiskTimedKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
            kernel<<<grid, 64, 0, s>>>(k, d, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q, long_iters, kstats, head, recs.img<T>(), recs.hits,
                                       dp.max_images, (T *)recs.tim);
        });
    if (dp.max_images)
        return launch_direct<T, DiskImagesKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
            kernel<<<grid, 64, 0, s>>>(k, d, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q, long_iters, kstats, head, recs.img<T>(), recs.hits,
                                       dp.max_images);
        });
    return launch_direct<T, DiskKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
        kernel<<<grid, 64, 0, s>>>(k, d, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n_q, long_iters, kstats, head);
    });
}

static int launch_epilogue_disk(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams &dp)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    launch_epilogue_rows(c, o, fo, [&](auto t, auto bg, dim3 ge) {
        using T = decltype(t);
        k_epilogue_disk<T, decltype(bg)::value><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, w.fin0<T>(), w.fin1<T>(), fo, dp.d_disk);
    });
    // (this epilogue fills no word 7: its destination is the frame path's)
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_DISK, LT_STAT_BG_TILES_GLOBAL);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_render_disk_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                  const float *d_bg, int32_t bg_channels, float *d_fa, uint16_t *d_w, int8_t *d_status,
                                  uint32_t *d_steps, float *d_disk, float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats)
{
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, nullptr, &dp);
    if (rc) return rc;
    dp.d_disk = d_disk;
    return render_dev_impl(cam, metric, opts, d_bg, bg_channels, d_fa, d_w, d_status, d_steps, d_rgb, d_rgba, d_stats,
                           nullptr, &dp);
}

extern "C" int lt_render_disk(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                              const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w, int8_t *out_status,
                              uint32_t *out_steps, float *out_disk, float *out_rgb, uint8_t *out_rgba, lt_stats *stats)
{
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, nullptr, &dp);
    if (rc) return rc;
    return render_host_impl(cam, metric, opts, bg, bg_channels, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba, stats,
                            &dp, out_disk);
}

extern "C" int lt_trace_batch_kerr_disk(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                        double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                        int precision, const lt_disk *disk, int64_t n, double *out_fa, int64_t *out_w,
                                        int8_t *out_status, double *out_disk, uint32_t *out_rhs_evals)
{
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    lt_opts o;
    MetricConsts mc;
    int rc = disk_batch_setup(&m, r_obs, theta_obs, integrator, precision, disk, nullptr, &dp, &o, &mc);
    if (rc) return rc;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp,
                       out_disk);
}

// ---- the disk test block by block (parity probes; they call the functions the disk kernels call) -----------------------------
// The metric and the disk as a disk call resolves them (r_in <= 0: the ISCO; the refusals of resolve_disk).
static int disk_probe_setup(const lt_metric *metric, double r_obs, double r_in, double r_out, MetricConsts *mc, DiskParams *dp)
{
    int rc = require_device();
    if (rc) return rc;
    lt_disk disk;
    lt_default_disk(&disk);
    disk.r_in = r_in;
    disk.r_out = r_out;
    if ((rc = resolve_disk(metric, r_obs, LT_SCHED_DIRECT, &disk, nullptr, dp))) return rc;
    return make_metric(metric, r_obs, M_PI / 2, 0.0, mc);
}

extern "C" int lt_disk_crossing_probe(const lt_metric *metric, double r_in, double r_out, const double *y0, const double *y1,
                                      const double *p_phi, const double *h, const double *t_end, int64_t n, int precision,
                                      uint8_t *out_found, double *out_hit, double *out_tau)
{
    MetricConsts mc;
    DiskParams dp;
    int rc = disk_probe_setup(metric, 50.0, r_in, r_out, &mc, &dp);
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (!y0 || !y1 || !p_phi || !h || !t_end || !out_found || !out_hit || !out_tau) return fail(LT_ERR_INVALID_ARG, "null pointer");
    DevBuf d0, d1, dl, dh, dt, of, oh, ot;
    if ((rc = probe_upload(d0, y0, n * 40)) || (rc = probe_upload(d1, y1, n * 40)) || (rc = probe_upload(dl, p_phi, n * 8)) ||
        (rc = probe_upload(dh, h, n * 8)) || (rc = probe_upload(dt, t_end, n * 8)) || (rc = of.alloc(n)) || (rc = oh.alloc(n * 40)) ||
        (rc = ot.alloc(n * 8))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_disk_crossing_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), make_disk_consts<T>(mc, dp), (const double *)d0.p,
                                                                    (const double *)d1.p, (const double *)dl.p, (const double *)dh.p,
                                                                    (const double *)dt.p, n, (uint8_t *)of.p, (double *)oh.p, (double *)ot.p);
    });
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_found, of, n)) || (rc = probe_download(out_hit, oh, n * 40)) || (rc = probe_download(out_tau, ot, n * 8)))
        return rc;
    return LT_OK;
}

extern "C" int lt_disk_advance_probe(const lt_metric *metric, double r_obs, double lambda_max, double h_max, double r_in, double r_out,
                                     int integrator, int precision, const double *states, const double *p_phi, const uint8_t *refine,
                                     const double *aux, const uint32_t *steps, const uint8_t *act, int64_t n, double *out_state,
                                     double *out_aux, int32_t *out_int, double *out_hit, double *out_on)
{
    MetricConsts mc;
    DiskParams dp;
    int rc = disk_probe_setup(metric, r_obs, r_in, r_out, &mc, &dp);
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (integrator != LT_INTEGRATOR_RK4 && !(integrator == LT_INTEGRATOR_DP45_EXACT && precision == 64))
        return fail(LT_ERR_UNSUPPORTED, "the disk advance probe runs RK4 (float32, float64) and DP45-exact (float64)");
    if (!(h_max > 0.0)) return fail(LT_ERR_INVALID_ARG, "h_max must be positive");
    if (n <= 0) return LT_OK;
    if (!states || !p_phi || !refine || !aux || !steps || !act || !out_state || !out_aux || !out_int || !out_hit || !out_on)
        return fail(LT_ERR_INVALID_ARG, "null pointer");
    DevBuf ds, dl, dr, da, dst, dac, os, oa, oi, oh, oo;
    if ((rc = probe_upload(ds, states, n * 40)) || (rc = probe_upload(dl, p_phi, n * 8)) || (rc = probe_upload(dr, refine, n)) ||
        (rc = probe_upload(da, aux, n * 16)) || (rc = probe_upload(dst, steps, n * 4)) || (rc = probe_upload(dac, act, n)) ||
        (rc = os.alloc(n * 40)) || (rc = oa.alloc(n * 16)) || (rc = oi.alloc(n * 12)) || (rc = oh.alloc(n * 40)) || (rc = oo.alloc(n * 56)))
        return rc;
    auto launch = [&](auto t, auto integ) {
        using T = decltype(t);
        using Integ = decltype(integ);
        k_disk_advance_probe<T, Integ><<<(unsigned)((n + 63) / 64), 64>>>(
            make_kerr<T>(mc, lambda_max, h_max), make_disk_consts<T>(mc, dp), (const double *)ds.p, (const double *)dl.p, (const uint8_t *)dr.p,
            (const double *)da.p, (const uint32_t *)dst.p, (const uint8_t *)dac.p, n, (double *)os.p, (double *)oa.p, (int32_t *)oi.p,
            (double *)oh.p, (double *)oo.p);
    };
    if (integrator == LT_INTEGRATOR_DP45_EXACT) launch(double{}, Dp45<double, true>{});
    else if (precision == 32) launch(float{}, Rk4<float>{});
    else launch(double{}, Rk4<double>{});
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_state, os, n * 40)) || (rc = probe_download(out_aux, oa, n * 16)) || (rc = probe_download(out_int, oi, n * 12)) ||
        (rc = probe_download(out_hit, oh, n * 40)) || (rc = probe_download(out_on, oo, n * 56))) return rc;
    return LT_OK;
}

extern "C" int lt_disk_shade_probe(const lt_metric *metric, double r_in, double q, double exposure, const double *in, int64_t n,
                                   double *out_f64, int64_t *out_half, float *out_f32)
{
    int rc = require_device();
    if (rc) return rc;
    if (!metric || metric->kind != LT_METRIC_KERR || !(metric->M > 0.0) || !(fabs(metric->a) <= metric->M))
        return fail(LT_ERR_INVALID_ARG, "the disk shade probe needs a Kerr metric with M > 0, |a| <= M");
    if (n <= 0) return LT_OK;
    if (!in || !out_f64 || !out_half || !out_f32) return fail(LT_ERR_INVALID_ARG, "null pointer");
    const DiskShade ds{metric->M, metric->a, r_in <= 0.0 ? lt_kerr_isco(metric->M, metric->a) : r_in, q, exposure};
    DevBuf di, o64, oh, o32;
    if ((rc = probe_upload(di, in, n * 32)) || (rc = o64.alloc(n * 40)) || (rc = oh.alloc(n * 8)) || (rc = o32.alloc(n * 16))) return rc;
    k_disk_shade_probe<<<(unsigned)((n + 63) / 64), 64>>>(ds, (const double *)di.p, n, (double *)o64.p, (int64_t *)oh.p, (float *)o32.p);
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_f64, o64, n * 40)) || (rc = probe_download(out_half, oh, n * 8)) || (rc = probe_download(out_f32, o32, n * 16)))
        return rc;
    return LT_OK;
}
