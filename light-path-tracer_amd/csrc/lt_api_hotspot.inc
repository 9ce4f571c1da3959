// lt_api_hotspot.inc -- included at the end of lt_api.hip, after lt_api_disk_images.inc.
//
// Host side of the hit times and the hot spot (include/ltrace.h, "hit times and an orbiting hot spot"): the timed trace is
// the thin disk's call with DiskParams::timed set (same checks, same frame plumbing, the kernels of lt_hit_time.hpp);
// shading and the light curve (lt_hotspot.hpp) read the caller's hit records and run on the default stream.

static void launch_epilogue_disk_hits(const CamConsts &c, const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w,
                                      const FrameOut &fo, const DiskImagesOut &di, const DiskRecordsBuf &recs, hipStream_t s)
{
    launch_epilogue_rows(c, o, fo, [&](auto t, auto, dim3 ge) {
        using T = decltype(t);
        k_epilogue_disk_hits<T><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, w.fin0<T>(), w.fin1<T>(), fo, di, (const T *)recs.tim);
    });
}

static void launch_epilogue_arrays_disk_hits(const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w, int64_t n,
                                             double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_hits, int32_t *d_n_hits,
                                             hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs)
{
    with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_epilogue_arrays_disk_hits<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(mc, ds, w.fin0<T>(), w.fin1<T>(), n, d_fa, d_w, d_st, d_ev,
                                                                                  recs.img<T>(), recs.hits, (int64_t)w.n_q, dp.max_images,
                                                                                  (const T *)recs.tim, d_hits, d_n_hits);
    });
}

extern "C" int lt_trace_disk_hits_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                      int32_t max_images, float *d_fa, uint16_t *d_w, int8_t *d_status, uint32_t *d_steps,
                                      float *d_hits, uint8_t *d_n_hits, uint64_t *d_stats)
{
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, &max_images, &dp);
    if (rc) return rc;
    dp.timed = true;
    dp.d_images = d_hits;
    dp.d_n_hits = d_n_hits;
    return render_dev_impl(cam, metric, opts, nullptr, 3, d_fa, d_w, d_status, d_steps, nullptr, nullptr, d_stats, nullptr, &dp);
}

extern "C" int lt_trace_disk_hits(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                  int32_t max_images, float *out_fa, uint16_t *out_w, int8_t *out_status, uint32_t *out_steps,
                                  float *out_hits, uint8_t *out_n_hits, lt_stats *stats)
{
    DiskParams dp;
    int rc = disk_frame_setup(cam, metric, opts, disk, &max_images, &dp);
    if (rc) return rc;
    dp.timed = true;
    return render_host_impl(cam, metric, opts, nullptr, 3, out_fa, out_w, out_status, out_steps, nullptr, nullptr, stats, &dp, nullptr,
                            out_hits, out_n_hits);
}

extern "C" int lt_trace_batch_kerr_disk_hits(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                             double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                             int precision, const lt_disk *disk, int32_t max_images, int64_t n, double *out_fa,
                                             int64_t *out_w, int8_t *out_status, double *out_hits, int32_t *out_n_hits,
                                             uint32_t *out_rhs_evals)
{
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    lt_opts o;
    MetricConsts mc;
    int rc = disk_batch_setup(&m, r_obs, theta_obs, integrator, precision, disk, &max_images, &dp, &o, &mc);
    if (rc) return rc;
    dp.timed = true;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp, nullptr,
                       out_hits, out_n_hits);
}

extern "C" int lt_step_time_probe(const lt_metric *metric, const double *p_phi, const double *y0, const double *y1, const double *h,
                                  const double *tau, int64_t n, int precision, double *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (!metric || metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "the step-time probe needs LT_METRIC_KERR");
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (!p_phi || !y0 || !y1 || !h || !tau || !out) return fail(LT_ERR_INVALID_ARG, "null array");
    MetricConsts mc;
    if ((rc = make_metric(metric, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    Staging st;
    const int i_l = st.in(p_phi, n, 8), i_0 = st.in(y0, n, 32), i_1 = st.in(y1, n, 32), i_h = st.in(h, n, 8), i_t = st.in(tau, n, 8);
    const int i_o = st.out(out, n, 8);
    if ((rc = st.commit(nullptr))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_step_time_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), st.dev<const double>(i_l), st.dev<const double>(i_0),
                                                                st.dev<const double>(i_1), st.dev<const double>(i_h), st.dev<const double>(i_t),
                                                                n, st.dev<double>(i_o));
    });
    HIP_TRY(hipGetLastError());
    if ((rc = st.fetch(i_o))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

extern "C" void lt_default_hotspot(lt_hotspot *h)
{
    memset(h, 0, sizeof(*h));
    h->r_spot = 8.0;
    h->sigma = 1.0;
    h->exposure = 1.0;
    h->with_disk = 1;
}

// Refusals, the disk's shading constants (r_in resolved as in resolve_disk) and the spot's.
static int resolve_hotspot(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_hotspot *spot, DiskShade *ds, HotspotShade *hs)
{
    int rc = require_device();
    if (rc) return rc;
    if (!hits || !metric || !disk || !spot) return fail(LT_ERR_INVALID_ARG, "null hits / metric / disk / spot");
    if (metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "the hot spot needs LT_METRIC_KERR");
    if (!(metric->M > 0.0) || !(fabs(metric->a) <= metric->M)) return fail(LT_ERR_INVALID_ARG, "bad metric (M %g, a %g)", metric->M, metric->a);
    if (R <= 0 || W <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", W, R);
    if (max_images < 1 || max_images > DISK_MAX_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", (int)max_images, DISK_MAX_IMAGES);
    if (!(spot->sigma > 0.0) || !std::isfinite(spot->sigma)) return fail(LT_ERR_INVALID_ARG, "hot spot sigma must be positive and finite");
    if (!(spot->r_spot > 0.0) || !std::isfinite(spot->r_spot) || !std::isfinite(spot->phi0) || !(spot->exposure >= 0.0) ||
        !std::isfinite(spot->exposure))
        return fail(LT_ERR_INVALID_ARG, "hot spot needs r_spot > 0, finite phi0, finite exposure >= 0");
    if (!std::isfinite(disk->q) || !(disk->exposure >= 0.0) || !std::isfinite(disk->exposure))
        return fail(LT_ERR_INVALID_ARG, "disk q / exposure must be finite, exposure >= 0");
    const double sM = sqrt(metric->M);
    *ds = DiskShade{metric->M, metric->a, disk->r_in <= 0.0 ? lt_kerr_isco(metric->M, metric->a) : disk->r_in, disk->q, disk->exposure};
    *hs = HotspotShade{spot->r_spot, spot->phi0, sM / (spot->r_spot * sqrt(spot->r_spot) + metric->a * sM),
                       1.0 / (2.0 * spot->sigma * spot->sigma), spot->exposure, spot->with_disk != 0};
    return LT_OK;
}

extern "C" int lt_shade_hotspot_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs,
                                    const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (!std::isfinite(t_obs)) return fail(LT_ERR_INVALID_ARG, "t_obs must be finite");
    const int64_t n_px = (int64_t)R * W;
    k_shade_hotspot<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, n_px, max_images, ds, hs, t_obs, d_base, channels, d_rgb, d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_hotspot(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs, const float *base,
                                int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    const size_t n = (size_t)R * W;
    Staging st;
    const int i_h = st.in(hits, n, (size_t)max_images * 16), i_n = st.in(n_hits, n, 1), i_b = st.in(base, n, (size_t)channels * 4);
    const int i_rgb = st.out(out_rgb, n, (size_t)channels * 4), i_rgba = st.out(out_rgba, n, 4);
    if ((rc = st.commit(nullptr))) return rc;
    if ((rc = lt_shade_hotspot_dev(st.dev<const float>(i_h), st.dev<const uint8_t>(i_n), R, W, max_images, metric, disk, spot, t_obs,
                                   st.dev<const float>(i_b), channels, st.dev<float>(i_rgb), st.dev<uint8_t>(i_rgba))))
        return rc;
    if ((rc = st.fetch(i_rgba)) || (rc = st.fetch(i_rgb))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

extern "C" int lt_hotspot_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                                         int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc) return rc;
    if (n_times < 0 || n_times > 65535) return fail(LT_ERR_INVALID_ARG, "n_times %d not in [0, 65535]", (int)n_times);
    if (!std::isfinite(t_start) || !std::isfinite(dt)) return fail(LT_ERR_INVALID_ARG, "t_start / dt must be finite");
    if (n_times == 0) return LT_OK;
    if (!d_out) return fail(LT_ERR_INVALID_ARG, "null out");
    StreamSlot *sl;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->hotspot, (size_t)n_times * LC_BLOCKS * 3 * sizeof(double), nullptr))) return rc;
    k_lightcurve_partial<<<dim3(LC_BLOCKS, (unsigned)n_times), 256>>>(d_hits, d_n_hits, (int64_t)R * W, W, max_images, hs, t_start, dt,
                                                                      (double *)sl->hotspot.p);
    k_lightcurve_final<<<(unsigned)n_times, 256>>>((const double *)sl->hotspot.p, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_hotspot_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                                     int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc) return rc;
    if (n_times < 0 || n_times > 65535) return fail(LT_ERR_INVALID_ARG, "n_times %d not in [0, 65535]", (int)n_times);
    const size_t n = (size_t)R * W;
    Staging st;
    const int i_h = st.in(hits, n, (size_t)max_images * 16), i_n = st.in(n_hits, n, 1);
    const int i_o = st.out(out, (size_t)n_times, 24);
    if ((rc = st.commit(nullptr))) return rc;
    if ((rc = lt_hotspot_lightcurve_dev(st.dev<const float>(i_h), st.dev<const uint8_t>(i_n), R, W, max_images, metric, disk, spot, t_start, dt,
                                        n_times, st.dev<double>(i_o))))
        return rc;
    if ((rc = st.fetch(i_o))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}
