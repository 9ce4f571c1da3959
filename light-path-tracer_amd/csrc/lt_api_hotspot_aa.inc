// lt_api_hotspot_aa.inc -- included at the end of lt_api.hip, after lt_api_polarization.inc.
//
// Host side of the supersampled hot-spot and Stokes frames (include/ltrace.h, "supersampled hot-spot and Stokes frames"):
// the refusals of the one-sample entry points in their order behind the one of `samples`, and the launches of
// lt_hotspot_aa.hpp on the default stream.  R, W are OUTPUT rows and columns; the records are the fine frame's.

// No device, then samples outside [1, LT_AA_MAX_SAMPLES]; what the one-sample entry point refuses comes after.
static int resolve_hotspot_aa(int32_t samples)
{
    int rc = require_device();
    if (rc) return rc;
    if (samples < 1 || samples > AA_MAX_SAMPLES) return fail(LT_ERR_INVALID_ARG, "samples %d not in [1, %d]", (int)samples, AA_MAX_SAMPLES);
    return LT_OK;
}

// Workgroups of P = AA_BLOCK / S^2 output pixels over the R W of them (a 1-D grid).
static int hotspot_aa_grid(int32_t R, int32_t W, int32_t samples, unsigned *blocks)
{
    const int64_t P = AA_BLOCK / (samples * samples), n = ((int64_t)R * W + P - 1) / P;
    if (n > 0x7fffffff) return fail(LT_ERR_INVALID_ARG, "frame %dx%d at %d samples: too many workgroups", W, R, (int)samples);
    *blocks = (unsigned)n;
    return LT_OK;
}

extern "C" int lt_shade_hotspot_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                                       int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                       double t_obs, const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskShade ds;
    HotspotShade hs;
    unsigned blocks;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_hotspot(d_hits, R, W, max_images, metric, disk, spot, &ds, &hs)) || (rc = check_channels(channels)) ||
        (rc = check_t_obs(t_obs)) || (rc = hotspot_aa_grid(R, W, samples, &blocks)))
        return rc;
    k_shade_hotspot_aa<<<blocks, AA_BLOCK>>>(d_hits, d_n_hits, (int64_t)R * W, W, samples, max_images, ds, hs, t_obs, d_base, channels, d_rgb,
                                             d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_hotspot_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples, int32_t max_images,
                                   const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, double t_obs, const float *base,
                                   int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, &ds, &hs)) || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W, n_fine = n * (size_t)(samples * samples);
    return staged_call({{hits, n_fine, (size_t)max_images * 16}, {n_hits, n_fine, 1}, {base, n_fine, (size_t)channels * 4}},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_hotspot_aa_dev((const float *)in[0], (const uint8_t *)in[1], R, W, samples, max_images, metric, disk, spot, t_obs,
                                       (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_shade_stokes_aa_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                      int32_t samples, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                                      const lt_hotspot *spot, const lt_bfield *field, double t_obs, float *d_iqu)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_stokes(d_hits, d_pol, R, W, max_images, metric, disk, spot, field, &ds, &hs)) || (rc = check_t_obs(t_obs))) return rc;
    if (!d_iqu) return fail(LT_ERR_INVALID_ARG, "null out");
    unsigned blocks;
    if ((rc = hotspot_aa_grid(R, W, samples, &blocks))) return rc;
    k_shade_stokes_aa<<<blocks, AA_BLOCK>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, W, samples, max_images, ds, hs, field->pol_frac, t_obs,
                                            d_iqu);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_stokes_aa(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t samples,
                                  int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                  const lt_bfield *field, double t_obs, float *out_iqu)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_stokes(hits, pol, R, W, max_images, metric, disk, spot, field, &ds, &hs))) return rc;
    const size_t n = (size_t)R * W, n_fine = n * (size_t)(samples * samples), rec = (size_t)max_images * 16;
    return staged_call({{hits, n_fine, rec}, {n_hits, n_fine, 1}, {pol, n_fine, rec}}, {{out_iqu, n, 12}}, [&](void *const *in, void *const *out) {
        return lt_shade_stokes_aa_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, samples, max_images, metric,
                                      disk, spot, field, t_obs, (float *)out[0]);
    });
}
