// lt_api_visibility_stokes.inc -- included at the end of lt_api.hip, after lt_api_visibility.inc.
//
// Host side of the polarized visibilities (include/ltrace.h, "polarized visibilities"): the refusals in the header's order
// -- the unpolarized entry point's through the baselines, then the polarization records and the field, the times and the
// output --, the batches of (time, plane) pairs a workgroup keeps in registers, the launches that keep the partials within
// LT_VISIBILITY_WORKSPACE_BYTES, on the default stream.  The baselines' upload, the workspace and the final stage are the
// unpolarized visibilities'.

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

// A _dev polarized visibility behind its resolves, as launch_visibility: the refusals of the times and of a null out, the
// baselines' upload, then the pairs in launches whose partials fit the workspace -- first_stage(NP, grid, lds, vg, d_uv,
// partial) launches the emitter's kernel for the batches of vg.pairs pairs from vg.first on -- each followed by
// k_visibility_final into its rows.  A row depends neither on its batch nor on its launch.
template <typename FirstStage>
static int launch_visibility_stokes(int32_t W, int32_t max_images, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start,
                                    double dt, int32_t n_times, double *d_out, FirstStage first_stage)
{
    int rc = check_spectrum_times(t_start, dt, n_times);
    if (rc) return rc;
    if (n_times == 0) return LT_OK;
    if (!d_out) return fail(LT_ERR_INVALID_ARG, "null out");
    const int planes = split_orders ? max_images : 1;
    const int n_pairs = n_times * planes;                                 // <= 65535 x 8
    const int pairs = std::min<int>(n_pairs, LT_VISIBILITY_STOKES_BATCH_PAIRS);
    const int row = pairs * 3 * n_baselines * 2;                          // doubles of a full batch's output
    const size_t per_batch = (size_t)VIS_BLOCKS * row * sizeof(double);
    const int n_batches = (n_pairs + pairs - 1) / pairs;
    const int per_launch = (int)std::min<size_t>((size_t)n_batches, std::max<size_t>(1, (size_t)LT_VISIBILITY_WORKSPACE_BYTES / per_batch));
    const size_t uv_bytes = (size_t)LT_VISIBILITY_MAX_BASELINES * 16;
    StreamSlot *sl;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->visibility, uv_bytes + (size_t)per_launch * per_batch, nullptr))) return rc;
    double *d_uv = (double *)sl->visibility.p, *partial = (double *)((char *)sl->visibility.p + uv_bytes);
    HIP_TRY(hipMemcpyAsync(d_uv, uv, (size_t)n_baselines * 16, hipMemcpyHostToDevice, nullptr));
    const int64_t out_pair = (int64_t)3 * n_baselines * 2;                // doubles of one (time, plane)
    with_visibility_stokes_pairs(pairs, [&](auto np) {
        for (int first = 0; first < n_pairs; first += per_launch * pairs) {
            const int left = n_pairs - first;
            const unsigned n = (unsigned)std::min(per_launch, (left + pairs - 1) / pairs);
            const VisibilityStokesGrid vg{n_baselines, planes, pairs, n_pairs, first, W};
            first_stage(np, dim3(VIS_BLOCKS, n, (unsigned)((n_baselines + 255) / 256)), visibility_lds_bytes(3 * decltype(np)::value), vg,
                        (const double *)d_uv, partial);
            k_visibility_final<<<dim3((unsigned)((row + 255) / 256), n), 256>>>(partial, row, (int64_t)std::min<int>(left, (int)n * pairs) * out_pair,
                                                                             d_out + (int64_t)first * out_pair);
        }
    });
    HIP_TRY(hipGetLastError());
    return LT_OK;
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
    int rc = resolve_reshade("disk visibility", "records", d_hits != nullptr, R, W, max_images, metric, disk, &ds, []() { return LT_OK; });
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(d_pol, metric, field))) return rc;
    return launch_visibility_stokes(W, max_images, uv, n_baselines, split_orders, 0.0, 0.0, 1, d_out,
                                    [&](auto np, dim3 grid, size_t lds, const VisibilityStokesGrid &vg, const double *d_uv, double *partial) {
        k_disk_visibility_stokes_partial<decltype(np)::value><<<grid, 256, lds>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images, ds,
                                                                                 field->pol_frac, vg, d_uv, partial);
    });
}

extern "C" int lt_disk_visibility_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_bfield *field, const double *uv,
                                         int32_t n_baselines, int32_t split_orders, double *out)
{
    DiskShade ds;
    int rc = resolve_reshade("disk visibility", "records", hits != nullptr, R, W, max_images, metric, disk, &ds, []() { return LT_OK; });
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = resolve_visibility_stokes(pol, metric, field))) return rc;
    const size_t n = (size_t)R * W, rec = (size_t)max_images * 16;
    return staged_call({{hits, n, rec}, {n_hits, n, 1}, {pol, n, rec}}, {{out, 1, visibility_stokes_row_bytes(max_images, n_baselines, split_orders)}},
                       [&](void *const *in, void *const *out_) {
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
    return launch_visibility_stokes(W, max_images, uv, n_baselines, split_orders, t_start, dt, n_times, d_out,
                                    [&](auto np, dim3 grid, size_t lds, const VisibilityStokesGrid &vg, const double *d_uv, double *partial) {
        k_hotspot_visibility_stokes_partial<decltype(np)::value><<<grid, 256, lds>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images, hs,
                                                                                    field->pol_frac, vg, t_start, dt, d_uv, partial);
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
    const size_t n = (size_t)R * W, rec = (size_t)max_images * 16;
    return staged_call({{hits, n, rec}, {n_hits, n, 1}, {pol, n, rec}},
                       {{out, (size_t)n_times, visibility_stokes_row_bytes(max_images, n_baselines, split_orders)}},
                       [&](void *const *in, void *const *out_) {
        return lt_hotspot_visibility_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric,
                                                disk, spot, field, uv, n_baselines, split_orders, t_start, dt, n_times, (double *)out_[0]);
    });
}
