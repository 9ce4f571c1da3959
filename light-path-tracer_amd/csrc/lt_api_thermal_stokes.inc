// lt_api_thermal_stokes.inc -- included at the end of lt_api.hip, after lt_api_thermal.inc.
//
// Host side of the polarized thermal continuum (include/ltrace.h, "polarized thermal continuum"): the refusals in the
// header's order -- the thermal continuum's through its struct, then the polarization records and the atmosphere's
// pointers, n_mu, n_freq and the output: resolve_thermal with resolve_atmosphere in its middle --, and the launches of
// lt_thermal_stokes.hpp on the default stream.  The host forms stage seven inputs through staged_hits_call, the polarization
// records first among the further ones, as in lt_api_visibility_stokes.inc: in[0] ... in[6] are hits, n_hits, pol, flux,
// limb, poldeg, nu.

#include "lt_thermal_stokes.hpp"

static_assert(ATM_MAX_NODES == LT_ATMOSPHERE_MAX_NODES, "lt_thermal_stokes.hpp restates the header's constant");
static_assert((size_t)LT_SPECTRUM_BLOCKS * LT_DISK_MAX_IMAGES * 3 * LT_THERMAL_MAX_FREQS * sizeof(double) <= (size_t)LT_SPECTRUM_WORKSPACE_BYTES,
              "the partials of the most planes, three Stokes parameters and the most frequencies fit the spectra's workspace in one batch");

// The refusals behind resolve_thermal's own and before the frequencies': the pointers, then n_mu.
static int resolve_atmosphere(const void *pol, const lt_atmosphere *atm, const double *limb, const double *poldeg, AtmosphereShade *as)
{
    if (!pol || !atm || !limb || !poldeg) return fail(LT_ERR_INVALID_ARG, "null pol / atmosphere / limb / poldeg");
    if (atm->n_mu < 2 || atm->n_mu > LT_ATMOSPHERE_MAX_NODES)
        return fail(LT_ERR_INVALID_ARG, "atmosphere n_mu %d not in [2, %d]", (int)atm->n_mu, LT_ATMOSPHERE_MAX_NODES);
    *as = AtmosphereShade{limb, poldeg, atm->n_mu};
    return LT_OK;
}

extern "C" int lt_disk_thermal_spectrum_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                                   int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                                                   const double *d_flux, const lt_atmosphere *atmosphere, const double *d_limb,
                                                   const double *d_poldeg, const double *d_nu, int32_t n_freq, double *d_out)
{
    ThermalShade ts;
    AtmosphereShade as;
    const int rc = resolve_thermal(d_hits, R, W, max_images, metric, disk, thermal, d_flux, d_nu, false, n_freq, d_out, &ts,
                                   [&]() { return resolve_atmosphere(d_pol, atmosphere, d_limb, d_poldeg, &as); });
    if (rc || n_freq == 0) return rc;
    const size_t lds = thermal_stokes_lds_bytes(max_images);
    return launch_thermal_spectrum(thermal, max_images, n_freq, 3, d_out, [&](auto np, dim3 grid, int planes, double *partial) {
        k_thermal_spectrum_stokes_partial<decltype(np)::value><<<grid, 256, lds>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images, ts, d_flux,
                                                                                 as, d_nu, n_freq, planes, partial);
    });
}

extern "C" int lt_disk_thermal_spectrum_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                               int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                                               const double *flux, const lt_atmosphere *atmosphere, const double *limb, const double *poldeg,
                                               const double *nu, int32_t n_freq, double *out)
{
    ThermalShade ts;
    AtmosphereShade as;
    const int rc = resolve_thermal(hits, R, W, max_images, metric, disk, thermal, flux, nu, false, n_freq, out, &ts,
                                   [&]() { return resolve_atmosphere(pol, atmosphere, limb, poldeg, &as); });
    if (rc || n_freq == 0) return rc;
    const size_t planes = thermal->split_orders ? (size_t)max_images : 1, n_mu = (size_t)atmosphere->n_mu;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{pol, (size_t)R * W, (size_t)max_images * 16}, {flux, (size_t)thermal->n_r, 8},
                            {limb, n_mu, 8}, {poldeg, n_mu, 8}, {nu, (size_t)n_freq, 8}}, {out, planes * 3 * (size_t)n_freq, 8},
                            [&](void *const *in, void *const *out_) {
        return lt_disk_thermal_spectrum_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric,
                                                   disk, thermal, (const double *)in[3], atmosphere, (const double *)in[4],
                                                   (const double *)in[5], (const double *)in[6], n_freq, (double *)out_[0]);
    });
}

extern "C" int lt_shade_thermal_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                           int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal,
                                           const double *d_flux, const lt_atmosphere *atmosphere, const double *d_limb, const double *d_poldeg,
                                           const double *d_nu, int32_t n_freq, float *d_out)
{
    ThermalShade ts;
    AtmosphereShade as;
    const int rc = resolve_thermal(d_hits, R, W, max_images, metric, disk, thermal, d_flux, d_nu, true, n_freq, d_out, &ts,
                                   [&]() { return resolve_atmosphere(d_pol, atmosphere, d_limb, d_poldeg, &as); });
    if (rc || n_freq == 0) return rc;
    const int64_t n_px = (int64_t)R * W;
    k_shade_thermal_stokes<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, d_pol, n_px, max_images, ts, d_flux, as, d_nu, n_freq, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_thermal_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t max_images,
                                       const lt_metric *metric, const lt_disk *disk, const lt_thermal *thermal, const double *flux,
                                       const lt_atmosphere *atmosphere, const double *limb, const double *poldeg, const double *nu,
                                       int32_t n_freq, float *out)
{
    ThermalShade ts;
    AtmosphereShade as;
    const int rc = resolve_thermal(hits, R, W, max_images, metric, disk, thermal, flux, nu, true, n_freq, out, &ts,
                                   [&]() { return resolve_atmosphere(pol, atmosphere, limb, poldeg, &as); });
    if (rc || n_freq == 0) return rc;
    const size_t n_mu = (size_t)atmosphere->n_mu;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{pol, (size_t)R * W, (size_t)max_images * 16}, {flux, (size_t)thermal->n_r, 8},
                            {limb, n_mu, 8}, {poldeg, n_mu, 8}, {nu, (size_t)n_freq, 8}}, {out, (size_t)n_freq * 3 * (size_t)R * W, 4},
                            [&](void *const *in, void *const *out_) {
        return lt_shade_thermal_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric, disk,
                                           thermal, (const double *)in[3], atmosphere, (const double *)in[4], (const double *)in[5],
                                           (const double *)in[6], n_freq, (float *)out_[0]);
    });
}
