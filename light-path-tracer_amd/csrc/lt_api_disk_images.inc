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
// count and the epilogues read only the slots below it, so nothing here is zeroed.  The integrate launch and the
// epilogue of one call ask for the same size and get the same pointers.
static int get_disk_records(hipStream_t s, int64_t n_q, size_t elem, int max_images, void **img, uint32_t **hits)
{
    StreamSlot *sl;
    int rc = get_slot(s, &sl);
    if (rc) return rc;
    const size_t img_bytes = (size_t)max_images * (size_t)n_q * 2 * elem;
    if ((rc = grow(sl->disk_img, img_bytes + (size_t)n_q * sizeof(uint32_t), s))) return rc;
    *img = sl->disk_img.p;
    *hits = (uint32_t *)((char *)sl->disk_img.p + img_bytes);
    return LT_OK;
}

template <typename T>
static int launch_integrate_disk_images(const MetricConsts &mc, const lt_opts &o, double lambda_max, const Workspace &w,
                                        int64_t n_q, hipStream_t s, uint64_t *kstats, const DiskParams &dp)
{
    using V = typename Vec4<T>::type;
    using V2 = typename Vec2<T>::type;
    const KerrConsts<T> k = make_kerr<T>(mc, lambda_max, o.h_max);
    const DiskConsts<T> d{(T)dp.r_in, (T)dp.r_out, (T)(1.0 / (mc.r_plus * mc.r_plus))};
    const bool exact = o.integrator == LT_INTEGRATOR_DP45_EXACT;
    const bool dp45 = o.integrator == LT_INTEGRATOR_DP45 || exact;
    if (dp45 && sizeof(T) != 8) return fail(LT_ERR_UNSUPPORTED, "DP45 needs precision 64");
    void *img = nullptr;
    uint32_t *hits = nullptr;
    int rc = get_disk_records(s, n_q, sizeof(T), dp.max_images, &img, &hits);
    if (rc) return rc;
    // grid, tile queue and "long" threshold as launch_integrate_disk
    static const int long_iters = env_int("LT_D_LONG", 384);
    static const int persist = env_int("LT_D_PERSIST", 1);
    unsigned kgrid = (unsigned)((n_q + 63) / 64);
    unsigned long long *head = nullptr;
    auto resident_grid = [&](int slots) {
        if (persist && slots > 0 && (unsigned)slots < kgrid) { kgrid = (unsigned)slots; head = w.head; }
    };
    if constexpr (sizeof(T) == 8) {
        if (dp45 && !exact) {
            resident_grid(resident_slots<k_kerr_disk_images<T, Dp45<T>>>());
            if (head) HIP_TRY(hipMemsetAsync(head, 0, sizeof(unsigned long long), s));
            k_kerr_disk_images<T, Dp45<T>><<<kgrid, 64, 0, s>>>(k, d, (const V *)w.ic, (V *)w.fin0, (V *)w.fin1, n_q, (uint32_t)(long_iters / 3),
                                                                kstats, head, (V2 *)img, hits, dp.max_images);
        }
        if (exact) {
            resident_grid(resident_slots<k_kerr_disk_images<T, Dp45<T, true>>>());
            if (head) HIP_TRY(hipMemsetAsync(head, 0, sizeof(unsigned long long), s));
            k_kerr_disk_images<T, Dp45<T, true>><<<kgrid, 64, 0, s>>>(k, d, (const V *)w.ic, (V *)w.fin0, (V *)w.fin1, n_q,
                                                                      (uint32_t)(long_iters / 3), kstats, head, (V2 *)img, hits,
                                                                      dp.max_images);
        }
    }
    if (!dp45) {
        resident_grid(resident_slots<k_kerr_disk_images<T, Rk4<T>>>());
        if (head) HIP_TRY(hipMemsetAsync(head, 0, sizeof(unsigned long long), s));
        k_kerr_disk_images<T, Rk4<T>><<<kgrid, 64, 0, s>>>(k, d, (const V *)w.ic, (V *)w.fin0, (V *)w.fin1, n_q, (uint32_t)long_iters,
                                                           kstats, head, (V2 *)img, hits, dp.max_images);
    }
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_disk_images(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w,
                                       int64_t n_q, const FrameOut &fo, uint64_t *d_stats, hipStream_t s,
                                       const DiskParams &dp)
{
    const size_t elem = o.precision == 32 ? sizeof(float) : sizeof(double);
    void *img = nullptr;
    uint32_t *hits = nullptr;
    int rc = get_disk_records(s, n_q, elem, dp.max_images, &img, &hits);
    if (rc) return rc;
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const DiskImagesOut di{img, hits, n_q, dp.max_images, dp.d_images, dp.d_n_hits};
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    const dim3 ge((unsigned)((c.W + EPILOGUE_BLOCK - 1) / EPILOGUE_BLOCK), (unsigned)c.rows_local);
    if (o.precision == 32) {
        if (has_bg) k_epilogue_disk_images<float, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, di);
        else k_epilogue_disk_images<float, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, fo, di);
    } else {
        if (has_bg) k_epilogue_disk_images<double, true><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, di);
        else k_epilogue_disk_images<double, false><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, fo, di);
    }
    if (d_stats) k_stats_reduce_disk_images<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_arrays_disk_images(const MetricConsts &mc, const lt_opts &o, const Workspace &w, int64_t n,
                                              int64_t n_q, double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev,
                                              double *d_images, int32_t *d_n_hits, hipStream_t s, const DiskParams &dp)
{
    const size_t elem = o.precision == 32 ? sizeof(float) : sizeof(double);
    void *img = nullptr;
    uint32_t *hits = nullptr;
    int rc = get_disk_records(s, n_q, elem, dp.max_images, &img, &hits);
    if (rc) return rc;
    const DiskShade ds{mc.M, mc.a, dp.r_in, dp.q, dp.exposure};
    const unsigned gn = (unsigned)((n + 255) / 256);
    if (o.precision == 32)
        k_epilogue_arrays_disk_images<float><<<gn, 256, 0, s>>>(mc, ds, (const float4 *)w.fin0, (const float4 *)w.fin1, n, d_fa, d_w, d_st, d_ev,
                                                                (const float2 *)img, hits, n_q, dp.max_images, d_images, d_n_hits);
    else
        k_epilogue_arrays_disk_images<double><<<gn, 256, 0, s>>>(mc, ds, (const double4 *)w.fin0, (const double4 *)w.fin1, n, d_fa, d_w, d_st, d_ev,
                                                                 (const double2 *)img, hits, n_q, dp.max_images, d_images, d_n_hits);
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
