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
static int resolve_disk(const lt_metric *metric, double r_obs, int schedule, const lt_disk *disk, DiskParams *dp)
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
    return LT_OK;
}

// The integrate launch of both disks: the direct schedule of launch_integrate (launch_direct) with the disk's kernels,
// 64-wide workgroups, no stamps.  dp.max_images > 0: the thin disk, which also gets its records (recs).
template <typename T>
static int launch_integrate_disk(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w, int64_t n_q,
                                 hipStream_t s, uint64_t *kstats, const DiskParams &dp, const DiskRecordsBuf &recs)
{
    using V = typename Vec4<T>::type;
    using V2 = typename Vec2<T>::type;
    const KerrConsts<T> k = make_kerr<T>(mc, lambda_max, o.h_max);
    const DiskConsts<T> d{(T)dp.r_in, (T)dp.r_out, (T)(1.0 / (mc.r_plus * mc.r_plus))};
    if (dp.max_images)
        return launch_direct<T, DiskImagesKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
            kernel<<<grid, 64, 0, s>>>(k, d, (const V *)w.ic, (V *)w.fin0, (V *)w.fin1, n_q, long_iters, kstats, head, (V2 *)recs.img,
                                       recs.hits, dp.max_images);
        });
    return launch_direct<T, DiskKernels<T>>(o, w, n_q, s, 64, [&](auto kernel, unsigned grid, uint32_t long_iters, unsigned long long *head) {
        kernel<<<grid, 64, 0, s>>>(k, d, (const V *)w.ic, (V *)w.fin0, (V *)w.fin1, n_q, long_iters, kstats, head);
    });
}

static int launch_epilogue_disk(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams &dp)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    const dim3 ge((unsigned)((c.W + EPILOGUE_BLOCK - 1) / EPILOGUE_BLOCK), (unsigned)c.rows_local);
    if (o.precision == 32) {
        if (has_bg) k_epilogue_disk<float, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, dp.d_disk);
        else k_epilogue_disk<float, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, dp.d_disk);
    } else {
        if (has_bg) k_epilogue_disk<double, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, dp.d_disk);
        else k_epilogue_disk<double, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, dp.d_disk);
    }
    // (this epilogue fills no word 7: its destination is the frame path's)
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_DISK, LT_STAT_BG_TILES_GLOBAL);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_render_disk_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                  const float *d_bg, int32_t bg_channels, float *d_fa, uint16_t *d_w, int8_t *d_status,
                                  uint32_t *d_steps, float *d_disk, float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / opts");
    DiskParams dp;
    if ((rc = resolve_disk(metric, cam->r_obs, opts->schedule, disk, &dp))) return rc;
    dp.d_disk = d_disk;
    return render_dev_impl(cam, metric, opts, d_bg, bg_channels, d_fa, d_w, d_status, d_steps, d_rgb, d_rgba, d_stats,
                           nullptr, &dp);
}

extern "C" int lt_render_disk(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                              const float *bg, int32_t bg_channels, float *out_fa, uint16_t *out_w, int8_t *out_status,
                              uint32_t *out_steps, float *out_disk, float *out_rgb, uint8_t *out_rgba, lt_stats *stats)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / opts");
    DiskParams dp;
    if ((rc = resolve_disk(metric, cam->r_obs, opts->schedule, disk, &dp))) return rc;
    return render_host_impl(cam, metric, opts, bg, bg_channels, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba, stats,
                            &dp, out_disk);
}

extern "C" int lt_trace_batch_kerr_disk(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                        double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                        int precision, const lt_disk *disk, int64_t n, double *out_fa, int64_t *out_w,
                                        int8_t *out_status, double *out_disk, uint32_t *out_rhs_evals)
{
    int rc = require_device();
    if (rc) return rc;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    if ((rc = resolve_disk(&m, r_obs, LT_SCHED_DIRECT, disk, &dp))) return rc;
    lt_opts o;
    lt_default_opts(&o);
    o.integrator = integrator; o.precision = precision; o.schedule = LT_SCHED_DIRECT;
    if ((rc = check_opts(&m, &o))) return rc;
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, theta_obs, 0.0, &mc))) return rc;
    if (integrator != LT_INTEGRATOR_RK4) { mc.evals_fixed = 1; mc.evals_per_step = 6; }
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp,
                       out_disk);
}
