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

extern "C" int lt_time_rates_probe(const lt_metric *metric, const double *p_phi, const double *y, int64_t n, int precision, double *out)
{
    int rc = require_device();
    if (rc) return rc;
    if (!metric || metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "the time-rates probe needs LT_METRIC_KERR");
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    if (n <= 0) return LT_OK;
    if (!p_phi || !y || !out) return fail(LT_ERR_INVALID_ARG, "null array");
    MetricConsts mc;
    if ((rc = make_metric(metric, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    Staging st;
    const int i_l = st.in(p_phi, n, 8), i_y = st.in(y, n, 32);
    const int i_o = st.out(out, n, 24);
    if ((rc = st.commit(nullptr))) return rc;
    with_precision(precision, [&](auto t) {
        using T = decltype(t);
        k_time_rates_probe<T><<<(unsigned)((n + 63) / 64), 64>>>(make_kerr<T>(mc, 5000.0, 1.0), st.dev<const double>(i_l), st.dev<const double>(i_y),
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

// ---- what the re-shades of stored hits share (the hot spot's here, the Stokes forms of lt_api_polarization.inc, the
// supersampled forms of lt_api_hotspot_aa.inc, the map's of lt_api_diskmap.inc) -----------------------------------------

// The refusals of a re-shade in their order, and the disk's shading constants (r_in resolved as in resolve_disk): no
// device, a null argument (`given`: the emitter's own pointers and hits; `pointers` names them in the message), a metric
// that is not Kerr (`who` needs it), a bad metric, an empty frame, max_images; then the emitter's own refusals and
// constants (`emitter`, called once metric is known to be good); the disk's q / exposure last.
template <typename Emitter>
static int resolve_reshade(const char *who, const char *pointers, bool given, int32_t R, int32_t W, int32_t max_images,
                           const lt_metric *metric, const lt_disk *disk, DiskShade *ds, Emitter emitter)
{
    int rc = require_device();
    if (rc) return rc;
    if (!given || !metric || !disk) return fail(LT_ERR_INVALID_ARG, "null hits / metric / disk / %s", pointers);
    if (metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "the %s needs LT_METRIC_KERR", who);
    if (!(metric->M > 0.0) || !(fabs(metric->a) <= metric->M)) return fail(LT_ERR_INVALID_ARG, "bad metric (M %g, a %g)", metric->M, metric->a);
    if (R <= 0 || W <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", W, R);
    if (max_images < 1 || max_images > DISK_MAX_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", (int)max_images, DISK_MAX_IMAGES);
    if ((rc = emitter())) return rc;
    if (!std::isfinite(disk->q) || !(disk->exposure >= 0.0) || !std::isfinite(disk->exposure))
        return fail(LT_ERR_INVALID_ARG, "disk q / exposure must be finite, exposure >= 0");
    *ds = DiskShade{metric->M, metric->a, disk->r_in <= 0.0 ? lt_kerr_isco(metric->M, metric->a) : disk->r_in, disk->q, disk->exposure};
    return LT_OK;
}

// What a frame refuses behind its resolve: the host-pointer forms the channels (the staged sizes need them), the _dev
// forms the channels and then the time.
static int check_channels(int32_t channels)
{
    return channels == 1 || channels == 3 ? LT_OK : fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
}

static int check_t_obs(double t_obs)
{
    return std::isfinite(t_obs) ? LT_OK : fail(LT_ERR_INVALID_ARG, "t_obs must be finite");
}

static int check_n_times(int32_t n_times)
{
    return n_times >= 0 && n_times <= 65535 ? LT_OK : fail(LT_ERR_INVALID_ARG, "n_times %d not in [0, 65535]", (int)n_times);
}

// A _dev light curve behind its resolve: the refusals of the times and of a null out, the slot's partials, the first
// stage -- first_stage(grid, partial) launches the emitter's kernel -- and k_lightcurve_final.
template <typename FirstStage> static int launch_lightcurve(double t_start, double dt, int32_t n_times, double *d_out, FirstStage first_stage)
{
    int rc = check_n_times(n_times);
    if (rc) return rc;
    if (!std::isfinite(t_start) || !std::isfinite(dt)) return fail(LT_ERR_INVALID_ARG, "t_start / dt must be finite");
    if (n_times == 0) return LT_OK;
    if (!d_out) return fail(LT_ERR_INVALID_ARG, "null out");
    StreamSlot *sl;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->hotspot, (size_t)n_times * LC_BLOCKS * 3 * sizeof(double), nullptr))) return rc;
    first_stage(dim3(LC_BLOCKS, (unsigned)n_times), (double *)sl->hotspot.p);
    k_lightcurve_final<<<(unsigned)n_times, 256>>>((const double *)sl->hotspot.p, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// A host-pointer re-shade through its _dev form on the default stream: the host arrays `ins` and `outs` staged (a null
// one stays null), dev(in, out) called with their device addresses in the order given, the outputs fetched in the order
// given, and the stream waited for.
struct HostArray { const void *host; size_t count, unit; };
template <size_t NI, size_t NO, typename Dev> static int staged_call(const HostArray (&ins)[NI], const HostArray (&outs)[NO], Dev dev)
{
    Staging st;
    int i_in[NI], i_out[NO], rc;
    for (size_t k = 0; k < NI; ++k) i_in[k] = st.in(ins[k].host, ins[k].count, ins[k].unit);
    for (size_t k = 0; k < NO; ++k) i_out[k] = st.out((void *)outs[k].host, outs[k].count, outs[k].unit);
    if ((rc = st.commit(nullptr))) return rc;
    void *d_in[NI], *d_out[NO];
    for (size_t k = 0; k < NI; ++k) d_in[k] = st.dev<void>(i_in[k]);
    for (size_t k = 0; k < NO; ++k) d_out[k] = st.dev<void>(i_out[k]);
    if ((rc = dev(d_in, d_out))) return rc;
    for (size_t k = 0; k < NO; ++k)
        if ((rc = st.fetch(i_out[k]))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

// Refusals, the disk's shading constants and the spot's.
static int resolve_hotspot(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_hotspot *spot, DiskShade *ds, HotspotShade *hs)
{
    return resolve_reshade("hot spot", "spot", hits && spot, R, W, max_images, metric, disk, ds, [&]() {
        if (!(spot->sigma > 0.0) || !std::isfinite(spot->sigma)) return fail(LT_ERR_INVALID_ARG, "hot spot sigma must be positive and finite");
        if (!(spot->r_spot > 0.0) || !std::isfinite(spot->r_spot) || !std::isfinite(spot->phi0) || !(spot->exposure >= 0.0) ||
            !std::isfinite(spot->exposure))
            return fail(LT_ERR_INVALID_ARG, "hot spot needs r_spot > 0, finite phi0, finite exposure >= 0");
        const double sM = sqrt(metric->M);
        *hs = HotspotShade{spot->r_spot, spot->phi0, sM / (spot->r_spot * sqrt(spot->r_spot) + metric->a * sM),
                           1.0 / (2.0 * spot->sigma * spot->sigma), spot->exposure, spot->with_disk != 0};
        return LT_OK;
    });
}

extern "C" int lt_shade_hotspot_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs,
                                    const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = check_channels(channels)) || (rc = check_t_obs(t_obs))) return rc;
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
    if (rc || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W;
    return staged_call({{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}, {base, n, (size_t)channels * 4}},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_hotspot_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spot, t_obs,
                                    (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_hotspot_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                                         int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc) return rc;
    return launch_lightcurve(t_start, dt, n_times, d_out, [&](dim3 grid, double *partial) {
        k_lightcurve_partial<<<grid, 256>>>(d_hits, d_n_hits, (int64_t)R * W, W, max_images, hs, t_start, dt, partial);
    });
}

extern "C" int lt_hotspot_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_start, double dt,
                                     int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = check_n_times(n_times))) return rc;
    const size_t n = (size_t)R * W;
    return staged_call({{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}}, {{out, (size_t)n_times, 24}}, [&](void *const *in, void *const *out_) {
        return lt_hotspot_lightcurve_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spot, t_start, dt,
                                         n_times, (double *)out_[0]);
    });
}
