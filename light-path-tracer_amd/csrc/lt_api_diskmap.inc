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

// Refusals, the disk's shading constants (r_in resolved as in resolve_disk) and the map's.
static int resolve_diskmap(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                           const lt_diskmap *map, const float *texels, DiskShade *ds, DiskMapShade *dm)
{
    int rc = require_device();
    if (rc) return rc;
    if (!hits || !metric || !disk || !map || !texels) return fail(LT_ERR_INVALID_ARG, "null hits / metric / disk / map / texels");
    if (metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "the disk map needs LT_METRIC_KERR");
    if (!(metric->M > 0.0) || !(fabs(metric->a) <= metric->M)) return fail(LT_ERR_INVALID_ARG, "bad metric (M %g, a %g)", metric->M, metric->a);
    if (R <= 0 || W <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", W, R);
    if (max_images < 1 || max_images > DISK_MAX_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", (int)max_images, DISK_MAX_IMAGES);
    if (!(map->r_min > 0.0) || !(map->r_max > map->r_min) || !std::isfinite(map->r_max))
        return fail(LT_ERR_INVALID_ARG, "disk map needs 0 < r_min < r_max, both finite");
    if (map->rotation != LT_MAP_KEPLERIAN && !std::isfinite(map->omega_p)) return fail(LT_ERR_INVALID_ARG, "disk map omega_p must be finite");
    if (!(map->exposure >= 0.0) || !std::isfinite(map->exposure)) return fail(LT_ERR_INVALID_ARG, "disk map exposure must be finite, >= 0");
    if (map->n_r < 1 || map->n_phi < 1 || (int64_t)map->n_r * map->n_phi > ((int64_t)1 << 26))
        return fail(LT_ERR_INVALID_ARG, "disk map of %d x %d texels: n_r, n_phi >= 1 and n_r n_phi <= 2^26", (int)map->n_r, (int)map->n_phi);
    if (map->rotation != LT_MAP_KEPLERIAN && map->rotation != LT_MAP_RIGID)
        return fail(LT_ERR_INVALID_ARG, "disk map rotation %d is neither LT_MAP_KEPLERIAN nor LT_MAP_RIGID", (int)map->rotation);
    if (!std::isfinite(disk->q) || !(disk->exposure >= 0.0) || !std::isfinite(disk->exposure))
        return fail(LT_ERR_INVALID_ARG, "disk q / exposure must be finite, exposure >= 0");
    const double sM = sqrt(metric->M);
    *ds = DiskShade{metric->M, metric->a, disk->r_in <= 0.0 ? lt_kerr_isco(metric->M, metric->a) : disk->r_in, disk->q, disk->exposure};
    *dm = DiskMapShade{map->r_min, map->r_max, map->omega_p, sM, metric->a * sM, (double)map->n_phi / 6.283185307179586, map->exposure,
                       map->n_r, map->n_phi, map->rotation == LT_MAP_RIGID, map->with_disk != 0};
    return LT_OK;
}

extern "C" int lt_shade_diskmap_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                    double t_obs, const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (!std::isfinite(t_obs)) return fail(LT_ERR_INVALID_ARG, "t_obs must be finite");
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
    if (rc) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    const size_t n = (size_t)R * W;
    Staging st;
    const int i_h = st.in(hits, n, (size_t)max_images * 16), i_n = st.in(n_hits, n, 1), i_b = st.in(base, n, (size_t)channels * 4);
    const int i_t = st.in(texels, (size_t)map->n_r * map->n_phi, 4);
    const int i_rgb = st.out(out_rgb, n, (size_t)channels * 4), i_rgba = st.out(out_rgba, n, 4);
    if ((rc = st.commit(nullptr))) return rc;
    if ((rc = lt_shade_diskmap_dev(st.dev<const float>(i_h), st.dev<const uint8_t>(i_n), R, W, max_images, metric, disk, map,
                                   st.dev<const float>(i_t), t_obs, st.dev<const float>(i_b), channels, st.dev<float>(i_rgb),
                                   st.dev<uint8_t>(i_rgba))))
        return rc;
    if ((rc = st.fetch(i_rgba)) || (rc = st.fetch(i_rgb))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

extern "C" int lt_shade_diskmap_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                                       int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                                       const float *d_texels, double t_obs, const float *d_base, int32_t channels, float *d_rgb,
                                       uint8_t *d_rgba)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm))) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (!std::isfinite(t_obs)) return fail(LT_ERR_INVALID_ARG, "t_obs must be finite");
    unsigned blocks;
    if ((rc = hotspot_aa_grid(R, W, samples, &blocks))) return rc;
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
    if (rc || (rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm))) return rc;
    if (channels != 1 && channels != 3) return fail(LT_ERR_INVALID_ARG, "channels must be 1 or 3");
    const size_t n = (size_t)R * W, n_fine = n * (size_t)(samples * samples);
    Staging st;
    const int i_h = st.in(hits, n_fine, (size_t)max_images * 16), i_n = st.in(n_hits, n_fine, 1), i_b = st.in(base, n_fine, (size_t)channels * 4);
    const int i_t = st.in(texels, (size_t)map->n_r * map->n_phi, 4);
    const int i_rgb = st.out(out_rgb, n, (size_t)channels * 4), i_rgba = st.out(out_rgba, n, 4);
    if ((rc = st.commit(nullptr))) return rc;
    if ((rc = lt_shade_diskmap_aa_dev(st.dev<const float>(i_h), st.dev<const uint8_t>(i_n), R, W, samples, max_images, metric, disk, map,
                                      st.dev<const float>(i_t), t_obs, st.dev<const float>(i_b), channels, st.dev<float>(i_rgb),
                                      st.dev<uint8_t>(i_rgba))))
        return rc;
    if ((rc = st.fetch(i_rgba)) || (rc = st.fetch(i_rgb))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

extern "C" int lt_diskmap_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *d_texels,
                                         double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(d_hits, R, W, max_images, metric, disk, map, d_texels, &ds, &dm);
    if (rc) return rc;
    if (n_times < 0 || n_times > 65535) return fail(LT_ERR_INVALID_ARG, "n_times %d not in [0, 65535]", (int)n_times);
    if (!std::isfinite(t_start) || !std::isfinite(dt)) return fail(LT_ERR_INVALID_ARG, "t_start / dt must be finite");
    if (n_times == 0) return LT_OK;
    if (!d_out) return fail(LT_ERR_INVALID_ARG, "null out");
    StreamSlot *sl;
    if ((rc = get_slot(nullptr, &sl)) || (rc = grow(sl->hotspot, (size_t)n_times * LC_BLOCKS * 3 * sizeof(double), nullptr))) return rc;
    k_diskmap_lightcurve_partial<<<dim3(LC_BLOCKS, (unsigned)n_times), 256>>>(d_hits, d_n_hits, (int64_t)R * W, W, max_images, dm, d_texels,
                                                                              t_start, dt, (double *)sl->hotspot.p);
    k_lightcurve_final<<<(unsigned)n_times, 256>>>((const double *)sl->hotspot.p, d_out);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_diskmap_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const float *texels,
                                     double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    DiskMapShade dm;
    int rc = resolve_diskmap(hits, R, W, max_images, metric, disk, map, texels, &ds, &dm);
    if (rc) return rc;
    if (n_times < 0 || n_times > 65535) return fail(LT_ERR_INVALID_ARG, "n_times %d not in [0, 65535]", (int)n_times);
    const size_t n = (size_t)R * W;
    Staging st;
    const int i_h = st.in(hits, n, (size_t)max_images * 16), i_n = st.in(n_hits, n, 1);
    const int i_t = st.in(texels, (size_t)map->n_r * map->n_phi, 4);
    const int i_o = st.out(out, (size_t)n_times, 24);
    if ((rc = st.commit(nullptr))) return rc;
    if ((rc = lt_diskmap_lightcurve_dev(st.dev<const float>(i_h), st.dev<const uint8_t>(i_n), R, W, max_images, metric, disk, map,
                                        st.dev<const float>(i_t), t_start, dt, n_times, st.dev<double>(i_o))))
        return rc;
    if ((rc = st.fetch(i_o))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}
