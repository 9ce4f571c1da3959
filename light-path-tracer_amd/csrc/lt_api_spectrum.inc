// lt_api_spectrum.inc -- included at the end of lt_api.hip.
//
// Host side of the energy-resolved light (include/ltrace.h, "energy-resolved light"): the refusals in the header's order
// -- the emitter's own resolve first, then the grid, the times and the output --, the batches of times that keep the
// partials within LT_SPECTRUM_WORKSPACE_BYTES, and the launches of lt_spectrum.hpp on the default stream.

static_assert(SP_BLOCKS == LT_SPECTRUM_BLOCKS && SP_MAX_BINS == LT_SPECTRUM_MAX_BINS, "lt_spectrum.hpp restates the header's constants");

extern "C" void lt_default_spectrum(lt_spectrum *s)
{
    memset(s, 0, sizeof(*s));
    s->g_min = 0.0625;
    s->g_max = 1.5625;
    s->n_bins = 96;
}

// The grid's refusals (behind the emitter's resolve) and its constants.
static int resolve_spectrum(const lt_spectrum *spec, int32_t max_images, SpectrumGrid *sg)
{
    if (!spec) return fail(LT_ERR_INVALID_ARG, "null spec");
    if (!(spec->g_min > 0.0) || !(spec->g_max > spec->g_min) || !std::isfinite(spec->g_max))
        return fail(LT_ERR_INVALID_ARG, "spectrum needs 0 < g_min < g_max, both finite");
    if (spec->n_bins < 1 || spec->n_bins > LT_SPECTRUM_MAX_BINS)
        return fail(LT_ERR_INVALID_ARG, "spectrum n_bins %d not in [1, %d]", (int)spec->n_bins, LT_SPECTRUM_MAX_BINS);
    *sg = SpectrumGrid{spec->g_min, spec->g_max, (double)spec->n_bins / (spec->g_max - spec->g_min), spec->n_bins,
                       spec->split_orders ? max_images : 1};
    return LT_OK;
}

static int check_spectrum_times(double t_start, double dt, int32_t n_times)
{
    int rc = check_n_times(n_times);
    if (rc) return rc;
    if (!std::isfinite(t_start) || !std::isfinite(dt)) return fail(LT_ERR_INVALID_ARG, "t_start / dt must be finite");
    return LT_OK;
}

// What a two-stage reduction of the stored hits (a spectrum, a visibility) refuses behind its resolves, in this order: the
// times, then a null out unless there is no time, which is no error and no work.
static int check_times_and_out(double t_start, double dt, int32_t n_times, const void *d_out)
{
    const int rc = check_spectrum_times(t_start, dt, n_times);
    if (rc || n_times == 0) return rc;
    return d_out ? LT_OK : fail(LT_ERR_INVALID_ARG, "null out");
}

// A host-pointer reduction through its _dev form (staged_call): the records, their counts and the further inputs `more` --
// none to five: the polarization records, the map's texels, the thermal, the atmosphere's and the transfer tables (a null
// array stays null and takes no room) -- staged as in[0], in[1], in[2] ... in[6], and the rows of `out` fetched.
template <typename Dev>
static int staged_hits_call(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                            std::initializer_list<HostArray> more, const HostArray &out, Dev dev)
{
    const size_t n = (size_t)R * W;
    HostArray ins[7] = {{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}};
    std::copy(more.begin(), more.end(), ins + 2);
    return staged_call(ins, {out}, dev);
}

// The two stages of a reduction whose partials are (batch, block, row) in the slot's spectra workspace, on the default
// stream: the workspace grown to batches x SP_BLOCKS x row doubles, first_stage(partial) -- the caller's launch --, then
// k_sum_blocks of the batches' rows into d_out.
template <typename FirstStage> static int launch_two_stage(unsigned batches, int row, double *d_out, FirstStage first_stage)
{
    StreamSlot *sl;
    int rc;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->spectrum, (size_t)batches * SP_BLOCKS * row * sizeof(double), nullptr))) return rc;
    double *partial = (double *)sl->spectrum.p;
    first_stage(partial);
    k_sum_blocks<<<dim3((unsigned)((row + 255) / 256), batches), 256>>>(partial, row, (int64_t)batches * row, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

// A _dev spectrum behind its resolves: the refusals of the times and of a null out, then the times in batches whose
// partials fit the slot's bounded workspace (the first batch is the largest, so the workspace grows once) --
// first_stage(grid, lds, first, partial) launches the emitter's kernel for the times first ... first + grid.y - 1 -- each
// followed by k_sum_blocks into its rows.  A row does not depend on its batch.
template <typename FirstStage>
static int launch_spectrum(const SpectrumGrid &sg, int32_t max_images, double t_start, double dt, int32_t n_times, double *d_out,
                           FirstStage first_stage)
{
    int rc = check_times_and_out(t_start, dt, n_times, d_out);
    if (rc || n_times == 0) return rc;
    const int n_keys = (sg.n_bins + 2) * sg.planes;
    const size_t per_time = (size_t)SP_BLOCKS * n_keys * sizeof(double);
    const int32_t batch = (int32_t)std::min<size_t>((size_t)n_times, std::max<size_t>(1, (size_t)LT_SPECTRUM_WORKSPACE_BYTES / per_time));
    for (int32_t first = 0; first < n_times && !rc; first += batch) {
        const unsigned n = (unsigned)std::min(batch, n_times - first);
        rc = launch_two_stage(n, n_keys, d_out + (int64_t)first * n_keys, [&](double *partial) {
            first_stage(dim3(SP_BLOCKS, n), spectrum_lds_bytes(n_keys, max_images), (int)first, partial);
        });
    }
    return rc;
}

static size_t spectrum_row_bytes(const SpectrumGrid &sg) { return (size_t)(sg.n_bins + 2) * sg.planes * sizeof(double); }

// The disk's refusals: resolve_reshade's with no emitter.
static int resolve_disk_spectrum(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                                 DiskShade *ds)
{
    return resolve_reshade("disk spectrum", "records", hits != nullptr, R, W, max_images, metric, disk, ds, []() { return LT_OK; });
}

extern "C" int lt_disk_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, double *d_out)
{
    DiskShade ds;
    SpectrumGrid sg;
    int rc = resolve_disk_spectrum(d_hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg))) return rc;
    return launch_spectrum(sg, max_images, 0.0, 0.0, 1, d_out, [&](dim3 grid, size_t lds, int, double *partial) {
        k_disk_spectrum_partial<<<grid, 256, lds>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, ds, sg, partial);
    });
}

extern "C" int lt_disk_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, double *out)
{
    DiskShade ds;
    SpectrumGrid sg;
    int rc = resolve_disk_spectrum(hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {}, {out, 1, spectrum_row_bytes(sg)}, [&](void *const *in, void *const *out_) {
        return lt_disk_spectrum_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spec, (double *)out_[0]);
    });
}

extern "C" int lt_hotspot_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                       const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_spectrum *spec,
                                       double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    SpectrumGrid sg;
    int rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg))) return rc;
    return launch_spectrum(sg, max_images, t_start, dt, n_times, d_out, [&](dim3 grid, size_t lds, int first, double *partial) {
        k_hotspot_spectrum_partial<<<grid, 256, lds>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, hs, sg, t_start, dt, first, partial);
    });
}

extern "C" int lt_hotspot_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                   const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_spectrum *spec,
                                   double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    SpectrumGrid sg;
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {}, {out, (size_t)n_times, spectrum_row_bytes(sg)},
                            [&](void *const *in, void *const *out_) {
        return lt_hotspot_spectrum_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spot, spec, t_start, dt,
                                       n_times, (double *)out_[0]);
    });
}

extern "C" int lt_diskmap_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                       const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                       const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    DiskMapShade dm;
    SpectrumGrid sg;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg))) return rc;
    return launch_spectrum(sg, max_images, t_start, dt, n_times, d_out, [&](dim3 grid, size_t lds, int first, double *partial) {
        k_diskmap_spectrum_partial<<<grid, 256, lds>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, dm, d_texels, sg, t_start, dt, first, partial);
    });
}

extern "C" int lt_diskmap_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                   const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                                   const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    DiskMapShade dm;
    SpectrumGrid sg;
    int rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{texels, (size_t)map->n_r * map->n_phi, 4}},
                            {out, (size_t)n_times, spectrum_row_bytes(sg)}, [&](void *const *in, void *const *out_) {
        return lt_diskmap_spectrum_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, (const float *)in[2],
                                       spec, t_start, dt, n_times, (double *)out_[0]);
    });
}
