// lt_api_disk_images.inc -- included at the end of lt_api.hip, after lt_api_disk.inc.
//
// Host side of the optically thin disk (include/ltrace.h, "optically thin disk"): the launches of the kernels of
// lt_disk_images.hpp and the entry points.  Parameter checks are lt_render_disk's (resolve_disk, which also checks max_images); the
// frame plumbing is render_dev_impl / render_host_impl / trace_batch with a DiskParams whose max_images is > 0.

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
    recs->p = sl->disk_img.p;
    recs->hits = (uint32_t *)((char *)sl->disk_img.p + img_bytes);
    if (disk->timed) {
        if ((rc = grow(sl->disk_time, img_bytes / 2, s))) return rc;
        recs->tim = sl->disk_time.p;
    }
    if (disk->pol) {
        if ((rc = grow(sl->disk_mom, img_bytes, s))) return rc;
        recs->mom = sl->disk_mom.p;
    }
    return LT_OK;
}

// The timed trace's epilogue launches (lt_api_hotspot.inc).
static void launch_epilogue_disk_hits(const CamConsts &c, const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w,
                                      const FrameOut &fo, const DiskImagesOut &di, const DiskRecordsBuf &recs, hipStream_t s);
static void launch_epilogue_arrays_disk_hits(const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w, int64_t n,
                                             double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_hits, int32_t *d_n_hits,
                                             hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs);
// ... and the polarized trace's (lt_api_polarization.inc).
static void launch_epilogue_disk_pol(const CamConsts &c, const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w,
                                     const FrameOut &fo, const DiskImagesOut &di, const DiskRecordsBuf &recs, hipStream_t s,
                                     const DiskParams &dp);
static void launch_epilogue_arrays_disk_pol(const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w, int64_t n,
                                            double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_hits, int32_t *d_n_hits,
                                            hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs);

static int launch_epilogue_disk_images(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                       const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams &dp,
                                       const DiskRecordsBuf &recs)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const DiskImagesOut di{recs.p, recs.hits, (int64_t)w.n_q, dp.max_images, dp.d_images, dp.d_n_hits};
    if (dp.pol) launch_epilogue_disk_pol(c, mc, ds, o, w, fo, di, recs, s, dp);
    else if (dp.timed) launch_epilogue_disk_hits(c, mc, ds, o, w, fo, di, recs, s);
    else launch_epilogue_rows(c, o, fo, [&](auto t, auto bg, dim3 ge) {
        using T = decltype(t);
        k_epilogue_disk_images<T, decltype(bg)::value><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, w.fin0<T>(), w.fin1<T>(), fo, di);
    });
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_DISK, LT_STAT_DISK_HITS);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_arrays_disk_images(const MetricConsts &mc, const lt_opts &o, const Workspace &w, int64_t n,
                                              double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_images,
                                              int32_t *d_n_hits, hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs)
{
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    if (dp.pol) launch_epilogue_arrays_disk_pol(mc, ds, o, w, n, d_fa, d_w, d_st, d_ev, d_images, d_n_hits, s, dp, recs);
    else if (dp.timed) launch_epilogue_arrays_disk_hits(mc, ds, o, w, n, d_fa, d_w, d_st, d_ev, d_images, d_n_hits, s, dp, recs);
    else with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_epilogue_arrays_disk_images<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(mc, ds, w.fin0<T>(), w.fin1<T>(), n, d_fa, d_w, d_st, d_ev,
                                                                                    recs.img<T>(), recs.hits, (int64_t)w.n_q, dp.max_images,
                                                                                    d_images, d_n_hits);
    });
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_render_disk_images_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts,
                                         const lt_disk *disk, int32_t max_images, const float *d_bg, int32_t bg_channels,
                                         float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps, float *d_images,
                                         uint8_t *d_n_hits, float *d_rgb, uint8_t *d_rgba, uint64_t *d_stats)
{
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, &max_images, &dp);
    if (rc) return rc;
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
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, &max_images, &dp);
    if (rc) return rc;
    return render_host_impl(cam, metric, opts, bg, bg_channels, out_fa, out_w, out_status, out_steps, out_rgb, out_rgba, stats,
                            &dp, nullptr, out_images, out_n_hits);
}

extern "C" int lt_trace_batch_kerr_disk_images(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                               double theta_obs, double lambda_max, const uint8_t *axis_refines,
                                               int integrator, int precision, const lt_disk *disk, int32_t max_images,
                                               int64_t n, double *out_fa, int64_t *out_w, int8_t *out_status,
                                               double *out_images, int32_t *out_n_hits, uint32_t *out_rhs_evals)
{
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    lt_opts o;
    MetricConsts mc;
    int rc = disk_batch_setup(&m, r_obs, theta_obs, integrator, precision, disk, &max_images, &dp, &o, &mc);
    if (rc) return rc;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp,
                       nullptr, out_images, out_n_hits);
}
