// lt_api_visibility.inc -- included at the end of lt_api.hip.
//
// Host side of the visibilities (include/ltrace.h, "visibilities"): the refusals in the header's order -- the emitter's own
// resolve first, then the baselines, the times and the output --, the baselines' upload, the batches of times a workgroup
// keeps in registers, the launches that keep the partials within LT_VISIBILITY_WORKSPACE_BYTES, on the default stream.

static_assert(VIS_BLOCKS == LT_VISIBILITY_BLOCKS && VIS_MAX_BASELINES == LT_VISIBILITY_MAX_BASELINES && VIS_BATCH_TERMS == LT_VISIBILITY_BATCH_TERMS,
              "lt_visibility.hpp restates the header's constants");
static_assert((size_t)LT_VISIBILITY_BLOCKS * LT_VISIBILITY_BATCH_TERMS * LT_VISIBILITY_MAX_BASELINES * 16 <= (size_t)LT_VISIBILITY_WORKSPACE_BYTES,
              "the partials of one batch at the most baselines fit the workspace");

// The disk's refusals, shared with its polarized form: resolve_reshade's with no emitter.
static int resolve_disk_visibility(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                                   DiskShade *ds)
{
    return resolve_reshade("disk visibility", "records", hits != nullptr, R, W, max_images, metric, disk, ds, []() { return LT_OK; });
}

// The baselines' refusals (behind the emitter's resolve).
static int resolve_baselines(const double *uv, int32_t n_baselines)
{
    if (!uv) return fail(LT_ERR_INVALID_ARG, "null uv");
    if (n_baselines < 1 || n_baselines > LT_VISIBILITY_MAX_BASELINES)
        return fail(LT_ERR_INVALID_ARG, "n_baselines %d not in [1, %d]", (int)n_baselines, LT_VISIBILITY_MAX_BASELINES);
    for (int32_t b = 0; b < n_baselines; ++b)
        if (!(fabs(uv[2 * b]) <= 0.5) || !(fabs(uv[2 * b + 1]) <= 0.5))
            return fail(LT_ERR_INVALID_ARG, "baseline %d (%g, %g) beyond |u|, |v| <= 0.5 cycles per pixel", (int)b, uv[2 * b], uv[2 * b + 1]);
    return LT_OK;
}

extern "C" int32_t lt_visibility_batch_times(int32_t max_images, int32_t split_orders)
{
    const int planes = split_orders ? std::min(std::max((int)max_images, 1), DISK_MAX_IMAGES) : 1;
    return std::max(1, LT_VISIBILITY_BATCH_TERMS / planes);
}

// first_stage(NT, ...) with NT the power of two from `terms` up, as a compile-time constant.
template <typename F> static void with_visibility_terms(int terms, F f)
{
    if (terms <= 1) f(std::integral_constant<int, 1>{});
    else if (terms <= 2) f(std::integral_constant<int, 2>{});
    else if (terms <= 4) f(std::integral_constant<int, 4>{});
    else if (terms <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, 16>{});
}

// A _dev visibility of either family behind its resolves: the refusals of the times and of a null out, the baselines' upload
// to the head of the slot's workspace, then the call's units -- a unit is a time here and a (time, plane) pair in
// lt_api_visibility_stokes.inc: units_per_time of them per time, at most batch_units in a batch, unit_doubles doubles of
// output each -- in launches whose partials fit the workspace.  with_terms(units, f) calls f(N) with the compile-time
// constant for a batch of `units`; first_stage(N, grid, vg, d_uv, partial) launches the emitter's kernel for the batches of
// vg.units units from vg.first on.  Each launch is followed by k_sum_blocks into its rows.  A row depends neither on its
// batch nor on its launch.
template <typename WithTerms, typename FirstStage>
static int launch_visibility(int32_t W, int planes, const double *uv, int32_t n_baselines, double t_start, double dt, int32_t n_times,
                             int units_per_time, int batch_units, int unit_doubles, double *d_out, WithTerms with_terms, FirstStage first_stage)
{
    int rc = check_times_and_out(t_start, dt, n_times, d_out);
    if (rc || n_times == 0) return rc;
    const int n_units = n_times * units_per_time;                         // <= 65535 x 8
    const int units = std::min(n_units, batch_units);
    const int row = units * unit_doubles;                                 // doubles of a full batch's output
    const size_t per_batch = (size_t)VIS_BLOCKS * row * sizeof(double);
    const int n_batches = (n_units + units - 1) / units;
    const int per_launch = (int)std::min<size_t>((size_t)n_batches, std::max<size_t>(1, (size_t)LT_VISIBILITY_WORKSPACE_BYTES / per_batch));
    const size_t uv_bytes = (size_t)LT_VISIBILITY_MAX_BASELINES * 16;
    StreamSlot *sl;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->visibility, uv_bytes + (size_t)per_launch * per_batch, nullptr))) return rc;
    double *d_uv = (double *)sl->visibility.p, *partial = (double *)((char *)sl->visibility.p + uv_bytes);
    HIP_TRY(hipMemcpyAsync(d_uv, uv, (size_t)n_baselines * 16, hipMemcpyHostToDevice, nullptr));
    with_terms(units, [&](auto nt) {
        for (int first = 0; first < n_units; first += per_launch * units) {
            const int left = n_units - first;
            const unsigned n = (unsigned)std::min(per_launch, (left + units - 1) / units);
            const VisibilityGrid vg{n_baselines, planes, units, n_units, first, W};
            first_stage(nt, dim3(VIS_BLOCKS, n, (unsigned)((n_baselines + 255) / 256)), vg, (const double *)d_uv, partial);
            k_sum_blocks<<<dim3((unsigned)((row + 255) / 256), n), 256>>>(partial, row, (int64_t)std::min<int>(left, (int)n * units) * unit_doubles,
                                                                       d_out + (int64_t)first * unit_doubles);
        }
    });
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// The unpolarized family's units: a time is a unit of planes x n_baselines x 2 doubles, lt_visibility_batch_times of them in a
// batch, NT from the batch's terms.
template <typename FirstStage>
static int launch_visibility_times(int32_t W, int32_t max_images, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start,
                                   double dt, int32_t n_times, double *d_out, FirstStage first_stage)
{
    const int planes = split_orders ? max_images : 1;
    return launch_visibility(W, planes, uv, n_baselines, t_start, dt, n_times, 1, lt_visibility_batch_times(max_images, split_orders),
                             planes * n_baselines * 2, d_out, [&](int times, auto f) { with_visibility_terms(times * planes, f); }, first_stage);
}

static size_t visibility_row_bytes(int32_t max_images, int32_t n_baselines, int32_t split_orders)
{
    return (size_t)(split_orders ? max_images : 1) * n_baselines * 2 * sizeof(double);
}

extern "C" int lt_disk_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                      const lt_metric *metric, const lt_disk *disk, const double *uv, int32_t n_baselines, int32_t split_orders,
                                      double *d_out)
{
    DiskShade ds;
    int rc = resolve_disk_visibility(d_hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_baselines(uv, n_baselines))) return rc;
    return launch_visibility_times(W, max_images, uv, n_baselines, split_orders, 0.0, 0.0, 1, d_out,
                                   [&](auto nt, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NT = decltype(nt)::value;
        k_disk_visibility_partial<NT><<<grid, 256, visibility_lds_bytes(NT)>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, ds, vg, d_uv, partial);
    });
}

extern "C" int lt_disk_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                                  const lt_disk *disk, const double *uv, int32_t n_baselines, int32_t split_orders, double *out)
{
    DiskShade ds;
    int rc = resolve_disk_visibility(hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_baselines(uv, n_baselines))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {}, {out, 1, visibility_row_bytes(max_images, n_baselines, split_orders)},
                            [&](void *const *in, void *const *out_) {
        return lt_disk_visibility_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, uv, n_baselines, split_orders,
                                      (double *)out_[0]);
    });
}

extern "C" int lt_hotspot_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const double *uv,
                                         int32_t n_baselines, int32_t split_orders, double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_baselines(uv, n_baselines))) return rc;
    return launch_visibility_times(W, max_images, uv, n_baselines, split_orders, t_start, dt, n_times, d_out,
                                   [&](auto nt, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NT = decltype(nt)::value;
        k_hotspot_visibility_partial<NT><<<grid, 256, visibility_lds_bytes(NT)>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, hs, vg, t_start, dt,
                                                                                 d_uv, partial);
    });
}

extern "C" int lt_hotspot_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                                     const lt_disk *disk, const lt_hotspot *spot, const double *uv, int32_t n_baselines, int32_t split_orders,
                                     double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {}, {out, (size_t)n_times, visibility_row_bytes(max_images, n_baselines, split_orders)},
                            [&](void *const *in, void *const *out_) {
        return lt_hotspot_visibility_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spot, uv, n_baselines,
                                         split_orders, t_start, dt, n_times, (double *)out_[0]);
    });
}

extern "C" int lt_diskmap_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                         const double *uv, int32_t n_baselines, int32_t split_orders, double t_start, double dt, int32_t n_times,
                                         double *d_out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc || (rc = resolve_baselines(uv, n_baselines))) return rc;
    return launch_visibility_times(W, max_images, uv, n_baselines, split_orders, t_start, dt, n_times, d_out,
                                   [&](auto nt, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NT = decltype(nt)::value;
        k_diskmap_visibility_partial<NT><<<grid, 256, visibility_lds_bytes(NT)>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, dm, d_texels, vg,
                                                                                 t_start, dt, d_uv, partial);
    });
}

extern "C" int lt_diskmap_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                                     const lt_disk *disk, const lt_diskmap *map, const float *texels, const double *uv, int32_t n_baselines,
                                     int32_t split_orders, double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{texels, (size_t)map->n_r * map->n_phi, 4}},
                            {out, (size_t)n_times, visibility_row_bytes(max_images, n_baselines, split_orders)}, [&](void *const *in, void *const *out_) {
        return lt_diskmap_visibility_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, (const float *)in[2], uv,
                                         n_baselines, split_orders, t_start, dt, n_times, (double *)out_[0]);
    });
}
