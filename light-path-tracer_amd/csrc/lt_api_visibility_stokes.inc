// lt_api_visibility_stokes.inc -- included at the end of lt_api.hip, after lt_api_visibility.inc.
//
// Host side of the polarized visibilities (include/ltrace.h, "polarized visibilities"): the refusals in the header's order
// -- the unpolarized entry point's through the baselines, then the polarization records and the field, the times and the
// output --, and the batches of (time, plane) pairs a workgroup keeps in registers.  The launcher (launch_visibility: the
// baselines' upload, the workspace, the launches and the final stage) is the unpolarized visibilities'.

static_assert(VIS_STOKES_BATCH_PAIRS == LT_VISIBILITY_STOKES_BATCH_PAIRS, "lt_visibility_stokes.hpp restates the header's constant");
static_assert((size_t)LT_VISIBILITY_BLOCKS * LT_VISIBILITY_STOKES_BATCH_PAIRS * 3 * LT_VISIBILITY_MAX_BASELINES * 16 <=
                  (size_t)LT_VISIBILITY_WORKSPACE_BYTES,
              "the partials of one batch of pairs at the most baselines fit the workspace");

extern "C" int32_t lt_visibility_stokes_batch_pairs(void) { return LT_VISIBILITY_STOKES_BATCH_PAIRS; }

// The records' and the field's refusals (behind the baselines'), worded as lt_shade_stokes words them.
static int resolve_visibility_stokes(const void *pol, const lt_metric *metric, const lt_bfield *field)
{
    if (!pol) return fail(LT_ERR_INVALID_ARG, "null pol");
    PolConsts pc;
    return resolve_bfield(metric, 4.0 * metric->M, M_PI / 2, field, &pc); // (the observer plays no part here)
}

// first_stage(NP, ...) with NP the accumulator pairs for `pairs` (time, plane) pairs, as a compile-time constant.
template <typename F> static void with_visibility_stokes_pairs(int pairs, F f)
{
    if (pairs <= 1) f(std::integral_constant<int, 1>{});
    else if (pairs <= 2) f(std::integral_constant<int, 2>{});
    else if (pairs <= 3) f(std::integral_constant<int, 3>{});
    else f(std::integral_constant<int, 5>{});
}

// The polarized family's units for launch_visibility: a (time, plane) pair is a unit of 3 x n_baselines x 2 doubles,
// `planes` of them per time and LT_VISIBILITY_STOKES_BATCH_PAIRS in a batch, NP from the batch's pairs.
template <typename FirstStage>
static int launch_visibility_pairs(int32_t W, int32_t max_images, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start,
                                   double dt, int32_t n_times, double *d_out, FirstStage first_stage)
{
    const int planes = split_orders ? max_images : 1;
    return launch_visibility(W, planes, uv, n_baselines, t_start, dt, n_times, planes, LT_VISIBILITY_STOKES_BATCH_PAIRS, 3 * n_baselines * 2, d_out,
                             [](int pairs, auto f) { with_visibility_stokes_pairs(pairs, f); }, first_stage);
}

static size_t visibility_stokes_row_bytes(int32_t max_images, int32_t n_baselines, int32_t split_orders)
{
    return 3 * visibility_row_bytes(max_images, n_baselines, split_orders);
}

extern "C" int lt_disk_visibility_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                             int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_bfield *field,
                                             const double *uv, int32_t n_baselines, int32_t split_orders, double *d_out)
{
    DiskShade ds;
    int rc = resolve_disk_visibility(d_hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(d_pol, metric, field))) return rc;
    return launch_visibility_pairs(W, max_images, uv, n_baselines, split_orders, 0.0, 0.0, 1, d_out,
                                   [&](auto np, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NP = decltype(np)::value;
        k_disk_visibility_stokes_partial<NP><<<grid, 256, visibility_lds_bytes(3 * NP)>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images, ds,
                                                                                         field->pol_frac, vg, d_uv, partial);
    });
}

extern "C" int lt_disk_visibility_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_bfield *field, const double *uv,
                                         int32_t n_baselines, int32_t split_orders, double *out)
{
    DiskShade ds;
    int rc = resolve_disk_visibility(hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(pol, metric, field))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{pol, (size_t)R * W, (size_t)max_images * 16}},
                            {out, 1, visibility_stokes_row_bytes(max_images, n_baselines, split_orders)}, [&](void *const *in, void *const *out_) {
        return lt_disk_visibility_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric, disk,
                                             field, uv, n_baselines, split_orders, (double *)out_[0]);
    });
}

extern "C" int lt_hotspot_visibility_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                                int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                                const lt_bfield *field, const double *uv, int32_t n_baselines, int32_t split_orders,
                                                double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(d_pol, metric, field))) return rc;
    return launch_visibility_pairs(W, max_images, uv, n_baselines, split_orders, t_start, dt, n_times, d_out,
                                   [&](auto np, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NP = decltype(np)::value;
        k_hotspot_visibility_stokes_partial<NP><<<grid, 256, visibility_lds_bytes(3 * NP)>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images,
                                                                                            hs, field->pol_frac, vg, t_start, dt, d_uv, partial);
    });
}

extern "C" int lt_hotspot_visibility_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                            int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                            const lt_bfield *field, const double *uv, int32_t n_baselines, int32_t split_orders,
                                            double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(pol, metric, field)) ||
        (rc = check_spectrum_times(t_start, dt, n_times)))
        return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{pol, (size_t)R * W, (size_t)max_images * 16}},
                            {out, (size_t)n_times, visibility_stokes_row_bytes(max_images, n_baselines, split_orders)},
                            [&](void *const *in, void *const *out_) {
        return lt_hotspot_visibility_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric,
                                                disk, spot, field, uv, n_baselines, split_orders, t_start, dt, n_times, (double *)out_[0]);
    });
}
