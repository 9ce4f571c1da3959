// lt_api_thermal.inc -- included at the end of lt_api.hip, after lt_api_visibility.inc.
//
// Host side of the thermal continuum (include/ltrace.h, "thermal continuum"): the refusals in the header's order -- the
// disk spectrum's resolve first, then the emitter's pointers, the struct's fields in their order, n_freq and the output --,
// the shading constants the host computes once, and the launches of lt_thermal.hpp on the default stream.  The refusals
// (resolve_thermal) and the spectrum's launcher (launch_thermal_spectrum) also serve lt_api_thermal_stokes.inc.

static_assert(TH_MAX_NODES == LT_THERMAL_MAX_NODES && TH_MAX_FREQS == LT_THERMAL_MAX_FREQS && TH_MAX_BANDS == LT_THERMAL_MAX_BANDS,
              "lt_thermal.hpp restates the header's constants");
static_assert((size_t)LT_SPECTRUM_BLOCKS * LT_DISK_MAX_IMAGES * LT_THERMAL_MAX_FREQS * sizeof(double) <= (size_t)LT_SPECTRUM_WORKSPACE_BYTES,
              "the partials of the most planes and frequencies fit the spectra's workspace in one batch");

extern "C" void lt_default_thermal(lt_thermal *t)
{
    memset(t, 0, sizeof(*t));
    t->r_min = 6.0;
    t->r_max = 20.0;
    t->t_max = 1.0;
    t->f_col = 1.0;
    t->exposure = 1.0;
    t->n_r = 2;
}

// Every refusal of an entry point of the thermal families, in the header's order: the disk spectrum's, then the emitter's
// pointers and fields (`bands`: the band images, which take no split_orders and at most LT_THERMAL_MAX_BANDS frequencies),
// then the family's own -- more(): none here (no_more), resolve_atmosphere in lt_api_thermal_stokes.inc --, then n_freq and a null
// out unless there is no frequency, which is no error and no work: the callers return behind `rc || n_freq == 0`.  With
// them the constants of the header's steps 2 and 4 that are computed once.
template <typename More>
static int resolve_thermal(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_thermal *th, const double *flux, const double *nu, bool bands, int32_t n_freq, const void *out,
                           ThermalShade *ts, More more)
{
    DiskShade ds;
    int rc = resolve_disk_spectrum(hits, R, W, max_images, metric, disk, &ds);
    if (rc) return rc;
    if (!th || !flux || !nu) return fail(LT_ERR_INVALID_ARG, "null thermal / flux / nu");
    if (!(th->r_min > 0.0) || !(th->r_max > th->r_min) || !std::isfinite(th->r_max))
        return fail(LT_ERR_INVALID_ARG, "thermal needs 0 < r_min < r_max, both finite");
    if (!(th->t_max > 0.0) || !std::isfinite(th->t_max)) return fail(LT_ERR_INVALID_ARG, "thermal t_max must be positive and finite");
    if (!(th->f_col > 0.0) || !std::isfinite(th->f_col)) return fail(LT_ERR_INVALID_ARG, "thermal f_col must be positive and finite");
    if (!(th->exposure >= 0.0) || !std::isfinite(th->exposure)) return fail(LT_ERR_INVALID_ARG, "thermal exposure must be finite, >= 0");
    if (th->n_r < 2 || th->n_r > LT_THERMAL_MAX_NODES)
        return fail(LT_ERR_INVALID_ARG, "thermal n_r %d not in [2, %d]", (int)th->n_r, LT_THERMAL_MAX_NODES);
    if (bands && th->split_orders) return fail(LT_ERR_INVALID_ARG, "a band image has one plane per band: split_orders must be 0");
    const double f2 = th->f_col * th->f_col;
    *ts = ThermalShade{th->r_min, th->r_max, (double)(th->n_r - 1) / (th->r_max - th->r_min), th->t_max, th->f_col, th->exposure / (f2 * f2),
                       th->n_r};
    if ((rc = more())) return rc;
    const int limit = bands ? LT_THERMAL_MAX_BANDS : LT_THERMAL_MAX_FREQS;
    if (n_freq < 0 || n_freq > limit) return fail(LT_ERR_INVALID_ARG, "n_freq %d not in [0, %d]", (int)n_freq, limit);
    return n_freq == 0 || out ? LT_OK : fail(LT_ERR_INVALID_ARG, "null out");
}

static int no_more() { return LT_OK; }

// The spectrum's two stages for both families, behind the refusals: `stokes` sums a plane (1 or 3) and `lds` bytes the
// first stage, first_stage(NP, grid, planes, partial), which launches the family's kernel with NP planes a work-item -- 1, or
// DISK_MAX_IMAGES with split_orders -- on one pass of the grid per 256 frequencies.
template <typename FirstStage>
static int launch_thermal_spectrum(const lt_thermal *thermal, int32_t max_images, int32_t n_freq, int stokes, double *d_out,
                                   FirstStage first_stage)
{
    const int planes = thermal->split_orders ? max_images : 1;
    const dim3 grid(SP_BLOCKS, 1, (unsigned)((n_freq + 255) / 256));
    return launch_two_stage(1, planes * stokes * n_freq, d_out, [&](double *partial) {
        if (planes > 1)
            first_stage(std::integral_constant<int, DISK_MAX_IMAGES>(), grid, planes, partial);
        else
            first_stage(std::integral_constant<int, 1>(), grid, planes, partial);
    });
}

extern "C" int lt_disk_thermal_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                            const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *d_flux,
                                            const double *d_nu, int32_t n_freq, double *d_out)
{
    ThermalShade ts;
    const int rc = resolve_thermal(d_hits, R, W, max_images, metric, disk, thermal, d_flux, d_nu, false, n_freq, d_out, &ts, no_more);
    if (rc || n_freq == 0) return rc;
    const size_t lds = thermal_lds_bytes(max_images);
    return launch_thermal_spectrum(thermal, max_images, n_freq, 1, d_out, [&](auto np, dim3 grid, int planes, double *partial) {
        k_thermal_spectrum_partial<decltype(np)::value><<<grid, 256, lds>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, ts, d_flux, d_nu, n_freq,
                                                                          planes, partial);
    });
}

extern "C" int lt_disk_thermal_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                        const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *flux,
                                        const double *nu, int32_t n_freq, double *out)
{
    ThermalShade ts;
    const int rc = resolve_thermal(hits, R, W, max_images, metric, disk, thermal, flux, nu, false, n_freq, out, &ts, no_more);
    if (rc || n_freq == 0) return rc;
    const size_t planes = thermal->split_orders ? (size_t)max_images : 1;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{flux, (size_t)thermal->n_r, 8}, {nu, (size_t)n_freq, 8}},
                            {out, planes * (size_t)n_freq, 8}, [&](void *const *in, void *const *out_) {
        return lt_disk_thermal_spectrum_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, thermal,
                                            (const double *)in[2], (const double *)in[3], n_freq, (double *)out_[0]);
    });
}

extern "C" int lt_shade_thermal_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *d_flux,
                                    const double *d_nu, int32_t n_freq, float *d_out)
{
    ThermalShade ts;
    const int rc = resolve_thermal(d_hits, R, W, max_images, metric, disk, thermal, d_flux, d_nu, true, n_freq, d_out, &ts, no_more);
    if (rc || n_freq == 0) return rc;
    const int64_t n_px = (int64_t)R * W;
    k_shade_thermal<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, n_px, max_images, ts, d_flux, d_nu, n_freq, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_thermal(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                                const lt_disk *disk, const lt_thermal *thermal, const double *flux, const double *nu, int32_t n_freq,
                                float *out)
{
    ThermalShade ts;
    const int rc = resolve_thermal(hits, R, W, max_images, metric, disk, thermal, flux, nu, true, n_freq, out, &ts, no_more);
    if (rc || n_freq == 0) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{flux, (size_t)thermal->n_r, 8}, {nu, (size_t)n_freq, 8}},
                            {out, (size_t)n_freq * (size_t)R * W, 4}, [&](void *const *in, void *const *out_) {
        return lt_shade_thermal_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, thermal,
                                    (const double *)in[2], (const double *)in[3], n_freq, (float *)out_[0]);
    });
}
