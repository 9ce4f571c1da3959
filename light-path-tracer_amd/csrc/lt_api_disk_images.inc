// lt_api_disk_images.inc -- included at the end of lt_api.hip, after lt_api_disk.inc.
//
// Host side of the optically thin disk (include/ltrace.h, "optically thin disk"): the launches of the kernels of
// lt_disk_images.hpp and the entry points.  Parameter checks are lt_render_disk's (resolve_disk) plus max_images; the
// frame plumbing is render_dev_impl / render_host_impl / trace_batch with a DiskParams whose max_images is > 0.

static int check_max_images(int32_t max_images)
{
    if (max_images < 1 || max_images > DISK_MAX_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", (int)max_images, DISK_MAX_IMAGES);
    return LT_OK;
}

// The integrate kernel's hit records of (current device, stream): Vec2<T> [max_images][n_q], then the counts
// uint32 [n_q].  A buffer of its own, so that the frame workspace keeps its layout; the integrate kernel writes every
// count and the epilogues read only the slots below it, so nothing here is zeroed.  Nothing to do without a thin disk.
static int get_disk_records(hipStream_t s, int64_t n_q, size_t elem, const DiskParams *disk, DiskRecordsBuf *recs)
{
    if (!disk || !disk->max_images) return LT_OK;
    StreamSlot *sl;
    int rc = get_slot(s, &sl);
    if (rc) return rc;
    const size_t img_bytes = (size_t)disk->max_images * (size_t)n_q * 2 * elem;
    if ((rc = grow(sl->disk_img, img_bytes + (size_t)n_q * sizeof(uint32_t), s))) return rc;
    recs->img = sl->disk_img.p;
    recs->hits = (uint32_t *)((char *)sl->disk_img.p + img_bytes);
    return LT_OK;
}

static int launch_epilogue_disk_images(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                       int64_t n_q, const FrameOut &fo, uint64_t *d_stats, hipStream_t s,
                                       const DiskParams &dp, const DiskRecordsBuf &recs)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const DiskImagesOut di{recs.img, recs.hits, n_q, dp.max_images, dp.d_images, dp.d_n_hits};
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    const dim3 ge((unsigned)((c.W + EPILOGUE_BLOCK - 1) / EPILOGUE_BLOCK), (unsigned)c.rows_local);
    if (o.precision == 32) {
        if (has_bg) k_epilogue_disk_images<float, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, di);
        else k_epilogue_disk_images<float, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, di);
    } else {
        if (has_bg) k_epilogue_disk_images<double, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, di);
        else k_epilogue_disk_images<double, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, di);
    }
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_DISK, LT_STAT_DISK_HITS);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_arrays_disk_images(const MetricConsts &mc, const lt_opts &o, const Workspace &w, int64_t n,
                                              int64_t n_q, double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev,
                                              double *d_images, int32_t *d_n_hits, hipStream_t s, const DiskParams &dp,
                                              const DiskRecordsBuf &recs)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const unsigned gn = (unsigned)((n + 255) / 256);
    if (o.precision == 32)
        k_epilogue_arrays_disk_images<float><<<gn, 256, 0, s>>>(mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, n, d_fa, d_w, d_st, d_ev,
                                                                (const float2 *)recs.img, recs.hits, n_q, dp.max_images, d_images, d_n_hits);
    else
        k_epilogue_arrays_disk_images<double><<<gn, 256, 0, s>>>(mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, n, d_fa, d_w, d_st, d_ev,
                                                                 (const double2 *)recs.img, recs.hits, n_q, dp.max_images, d_images, d_n_hits);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_render_disk_images_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts,
                                         const lt_disk *disk, int32_t max_images, const float *d_bg, int32_t bg_channels,
                                         float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps, float *d_images,
                                         uint8_t *d_n_hits, float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / opts");
    DiskParams dp;
    if ((rc = resolve_disk(metric, cam->r_obs, opts->schedule, disk, &dp))) return rc;
    if ((rc = check_max_images(max_images))) return rc;
    dp.max_images = max_images;
    dp.d_images = d_images;
    dp.d_n_hits = d_n_hits;
    return render_dev_impl(cam, metric, opts, d_bg, bg_channels, d_fa, d_w, d_status, d_steps, d_rgb, d_rgba, d_stats,
                           nullptr, &dp);
}

extern "C" int lt_render_disk_images(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts,
                                     const lt_disk *disk, int32_t max_images, const float *bg, int32_t bg_channels,
                                     float *out_fa, uint16_t *out_w, int8_t *out_status, uint32_t *out_steps,
                                     float *out_images, uint8_t *out_n_hits, float *out_rgb, uint8_t *out_rgba,
                                     lt_stats *stats)
{
    int rc = require_device();
    if (rc) return rc;
    if (!cam || !opts) return fail(LT_ERR_INVALID_ARG, "null camera / opts");
    DiskParams dp;
    if ((rc = resolve_disk(metric, cam->r_obs, opts->schedule, disk, &dp))) return rc;
    if ((rc = check_max_images(max_images))) return rc;
    dp.max_images = max_images;
    return render_host_impl(cam, metric, opts, bg, bg_channels, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba, stats,
                            &dp, nullptr, out_images, out_n_hits);
}

extern "C" int lt_trace_batch_kerr_disk_images(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                               double theta_obs, double lambda_max, const uint8_t *axis_refines,
                                               int integrator, int precision, const lt_disk *disk, int32_t max_images,
                                               int64_t n, double *out_fa, int64_t *out_w, int8_t *out_status,
                                               double *out_images, int32_t *out_n_hits, uint32_t *out_rhs_evals)
{
    int rc = require_device();
    if (rc) return rc;
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    if ((rc = resolve_disk(&m, r_obs, LT_SCHED_DIRECT, disk, &dp))) return rc;
    if ((rc = check_max_images(max_images))) return rc;
    dp.max_images = max_images;
    lt_opts o;
    lt_default_opts(&o);
    o.integrator = integrator; o.precision = precision; o.schedule = LT_SCHED_DIRECT;
    if ((rc = check_opts(&m, &o))) return rc;
    MetricConsts mc;
    if ((rc = make_metric(&m, r_obs, theta_obs, 0.0, &mc))) return rc;
    if (integrator != LT_INTEGRATOR_RK4) { mc.evals_fixed = 1; mc.evals_per_step = 6; }
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp,
                       nullptr, out_images, out_n_hits);
}
