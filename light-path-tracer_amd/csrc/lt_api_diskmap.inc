// lt_api_diskmap.inc -- included at the end of lt_api.hip, after lt_api_hotspot_aa.inc.
//
// Host side of the rotating emissivity map (include/ltrace.h, "a rotating emissivity map"): the refusals in the header's
// order, the map's shading constants, and the launches of lt_diskmap.hpp on the default stream.  The entry points are the
// hot spot's (lt_api_hotspot.inc, lt_api_hotspot_aa.inc) with (map, texels) in the spot's place.

extern "C" void lt_default_diskmap(lt_diskmap *m)
{
    memset(m, 0, sizeof(*m));
    m->r_min = 6.0;
    m->r_max = 20.0;
    m->exposure = 1.0;
    m->n_r = 1;
    m->n_phi = 1;
    m->rotation = LT_MAP_KEPLERIAN;
    m->with_disk = 1;
}

// The refusals of the map's fields, in the struct's order, and its shading constants; the movie's resolve
// (lt_api_diskmovie.inc) goes through them too.
static int resolve_diskmap_fields(const lt_metric *metric, const lt_diskmap *map, DiskMapShade *dm)
{
    if (!(map->r_min > 0.0) || !(map->r_max > map->r_min) || !std::isfinite(map->r_max))
        return fail(LT_ERR_INVALID_ARG, "disk map needs 0 < r_min < r_max, both finite");
    if (map->rotation != LT_MAP_KEPLERIAN && !std::isfinite(map->omega_p)) return fail(LT_ERR_INVALID_ARG, "disk map omega_p must be finite");
    if (!(map->exposure >= 0.0) || !std::isfinite(map->exposure)) return fail(LT_ERR_INVALID_ARG, "disk map exposure must be finite, >= 0");
    if (map->n_r < 1 || map->n_phi < 1 || (int64_t)map->n_r * map->n_phi > ((int64_t)1 << 26))
        return fail(LT_ERR_INVALID_ARG, "disk map of %d x %d texels: n_r, n_phi >= 1 and n_r n_phi <= 2^26", (int)map->n_r, (int)map->n_phi);
    if (map->rotation != LT_MAP_KEPLERIAN && map->rotation != LT_MAP_RIGID)
        return fail(LT_ERR_INVALID_ARG, "disk map rotation %d is neither LT_MAP_KEPLERIAN nor LT_MAP_RIGID", (int)map->rotation);
    const double sM = sqrt(metric->M);
    *dm = DiskMapShade{map->r_min, map->r_max, map->omega_p, sM, metric->a * sM, (double)map->n_phi / 6.283185307179586, map->exposure,
                       map->n_r, map->n_phi, map->rotation == LT_MAP_RIGID, map->with_disk != 0};
    return LT_OK;
}

// Refusals, the disk's shading constants and the map's.
static int resolve_diskmap(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_diskmap *map, const float *texels, DiskShade *ds, DiskMapShade *dm)
{
    return resolve_reshade("disk map", "map / texels", hits && map && texels, R, W, max_images, metric, disk, ds,
                           [&]() { return resolve_diskmap_fields(metric, map, dm); });
}

extern "C" int lt_shade_diskmap_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                    double t_obs, const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc || (rc = check_channels(channels)) || (rc = check_t_obs(t_obs))) return rc;
    const int64_t n_px = (int64_t)R * W;
    k_shade_diskmap<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, n_px, max_images, ds, dm, d_texels, t_obs, d_base, channels,
                                                             d_rgb, d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_diskmap(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels, double t_obs,
                                const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm);
    if (rc || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W;
    return staged_call({{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}, {base, n, (size_t)channels * 4},
                        {texels, (size_t)map->n_r * map->n_phi, 4}},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_diskmap_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, (const float *)in[3],
                                    t_obs, (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_shade_diskmap_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                                       int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                                       const float *d_texels, double t_obs, const float *d_base, int32_t channels, float *d_rgb,
                                       uint8_t *d_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    unsigned blocks;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm)) || (rc = check_channels(channels)) ||
        (rc = check_t_obs(t_obs)) || (rc = hotspot_aa_grid(R, W, samples, &blocks)))
        return rc;
    k_shade_diskmap_aa<<<blocks, AA_BLOCK>>>(d_hits, d_n_hits, (int64_t)R * W, W, samples, max_images, ds, dm, d_texels, t_obs, d_base,
                                             channels, d_rgb, d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_diskmap_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples, int32_t max_images,
                                   const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels, double t_obs,
                                   const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm)) || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W, n_fine = n * (size_t)(samples * samples);
    return staged_call({{hits, n_fine, (size_t)max_images * 16}, {n_hits, n_fine, 1}, {base, n_fine, (size_t)channels * 4},
                        {texels, (size_t)map->n_r * map->n_phi, 4}},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_diskmap_aa_dev((const float *)in[0], (const uint8_t *)in[1], R, W, samples, max_images, metric, disk, map,
                                       (const float *)in[3], t_obs, (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_diskmap_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                         double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc) return rc;
    return launch_lightcurve(t_start, dt, n_times, d_out, [&](dim3 grid, double *partial) {
        k_diskmap_lightcurve_partial<<<grid, 256>>>(d_hits, d_n_hits, (int64_t)R * W, W, max_images, dm, d_texels, t_start, dt, partial);
    });
}

extern "C" int lt_diskmap_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                                     double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm);
    if (rc || (rc = check_n_times(n_times))) return rc;
    const size_t n = (size_t)R * W;
    return staged_call({{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}, {texels, (size_t)map->n_r * map->n_phi, 4}},
                       {{out, (size_t)n_times, 24}}, [&](void *const *in, void *const *out_) {
        return lt_diskmap_lightcurve_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map,
                                         (const float *)in[2], t_start, dt, n_times, (double *)out_[0]);
    });
}
