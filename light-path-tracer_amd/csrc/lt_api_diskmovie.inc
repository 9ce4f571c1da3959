// lt_api_diskmovie.inc -- included at the end of lt_api.hip, after lt_api_visibility.inc.
//
// Host side of the disk movie (include/ltrace.h, "a disk movie"): the refusals in the header's order -- the map's, with the
// movie's fields behind the map's --, the movie's shading constants, and the launches of lt_diskmovie.hpp on the default
// stream through the map's launchers.  The entry points are the map's (lt_api_diskmap.inc, lt_api_spectrum.inc,
// lt_api_visibility.inc) with `movie` after `map` and texels of n_frames tables.

extern "C" void lt_default_diskmovie(lt_diskmovie *mv)
{
    memset(mv, 0, sizeof(*mv));
    mv->dt_frame = 1.0;
    mv->n_frames = 1;
    mv->boundary = LT_MOVIE_HOLD;
}

// What a movie's call resolves to: the disk's, the map's and the movie's shading constants.
struct DiskMovieCall {
    DiskShade ds;
    DiskMapShade dm;
    DiskMovieShade mv;
};

static int resolve_diskmovie(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                             const lt_diskmap *map, const lt_diskmovie *movie, const float *texels, DiskMovieCall *c)
{
    return resolve_reshade("disk movie", "map / movie / texels", hits && map && movie && texels, R, W, max_images, metric, disk, &c->ds, [&]() {
        const int rc = resolve_diskmap_fields(metric, map, &c->dm);
        if (rc) return rc;
        if (!std::isfinite(movie->t0)) return fail(LT_ERR_INVALID_ARG, "disk movie t0 must be finite");
        if (!(movie->dt_frame > 0.0) || !std::isfinite(movie->dt_frame)) return fail(LT_ERR_INVALID_ARG, "disk movie dt_frame must be finite, > 0");
        const int64_t frame_texels = (int64_t)map->n_r * map->n_phi;
        if (movie->n_frames < 1 || (int64_t)movie->n_frames > ((int64_t)1 << 28) / frame_texels)
            return fail(LT_ERR_INVALID_ARG, "disk movie of %d frames of %d x %d texels: n_frames >= 1 and n_frames n_r n_phi <= 2^28",
                        (int)movie->n_frames, (int)map->n_r, (int)map->n_phi);
        if (movie->boundary != LT_MOVIE_HOLD && movie->boundary != LT_MOVIE_LOOP)
            return fail(LT_ERR_INVALID_ARG, "disk movie boundary %d is neither LT_MOVIE_HOLD nor LT_MOVIE_LOOP", (int)movie->boundary);
        c->mv = DiskMovieShade{movie->t0, movie->dt_frame, frame_texels, movie->n_frames, movie->boundary == LT_MOVIE_LOOP};
        return (int)LT_OK;
    });
}

// The movie's texels as a staged input (behind resolve_diskmovie: the product is at most 2^28).
static HostArray movie_texels(const float *texels, const lt_diskmap *map, const lt_diskmovie *movie)
{
    return {texels, (size_t)movie->n_frames * map->n_r * map->n_phi, 4};
}

extern "C" int lt_shade_diskmovie_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                      const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                      const float *d_texels, double t_obs, const float *d_base, int32_t channels, float *d_rgb, uint8_t *d_rgba)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(d_hits, R, W, max_images, metric, disk, map, movie, d_texels, &c);
    if (rc || (rc = check_channels(channels)) || (rc = check_t_obs(t_obs))) return rc;
    const int64_t n_px = (int64_t)R * W;
    k_shade_diskmovie<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, n_px, max_images, c.ds, c.dm, c.mv, d_texels, t_obs, d_base,
                                                               channels, d_rgb, d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_diskmovie(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                  const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                  const float *texels, double t_obs, const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(hits, R, W, max_images, metric, disk, map, movie, texels, &c);
    if (rc || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W;
    return staged_call({{hits, n, (size_t)max_images * 16}, {n_hits, n, 1}, {base, n, (size_t)channels * 4}, movie_texels(texels, map, movie)},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_diskmovie_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, movie,
                                      (const float *)in[3], t_obs, (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_shade_diskmovie_aa_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t samples,
                                         int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map,
                                         const lt_diskmovie *movie, const float *d_texels, double t_obs, const float *d_base, int32_t channels,
                                         float *d_rgb, uint8_t *d_rgba)
{
    DiskMovieCall c;
    unsigned blocks;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_diskmovie(d_hits, R, W, max_images, metric, disk, map, movie, d_texels, &c)) || (rc = check_channels(channels)) ||
        (rc = check_t_obs(t_obs)) || (rc = hotspot_aa_grid(R, W, samples, &blocks)))
        return rc;
    k_shade_diskmovie_aa<<<blocks, AA_BLOCK>>>(d_hits, d_n_hits, (int64_t)R * W, W, samples, max_images, c.ds, c.dm, c.mv, d_texels, t_obs,
                                               d_base, channels, d_rgb, d_rgba);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_diskmovie_aa(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t samples, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                     const float *texels, double t_obs, const float *base, int32_t channels, float *out_rgb, uint8_t *out_rgba)
{
    DiskMovieCall c;
    int rc = resolve_hotspot_aa(samples);
    if (rc || (rc = resolve_diskmovie(hits, R, W, max_images, metric, disk, map, movie, texels, &c)) || (rc = check_channels(channels))) return rc;
    const size_t n = (size_t)R * W, n_fine = n * (size_t)(samples * samples);
    return staged_call({{hits, n_fine, (size_t)max_images * 16}, {n_hits, n_fine, 1}, {base, n_fine, (size_t)channels * 4},
                        movie_texels(texels, map, movie)},
                       {{out_rgba, n, 4}, {out_rgb, n, (size_t)channels * 4}}, [&](void *const *in, void *const *out) {
        return lt_shade_diskmovie_aa_dev((const float *)in[0], (const uint8_t *)in[1], R, W, samples, max_images, metric, disk, map, movie,
                                         (const float *)in[3], t_obs, (const float *)in[2], channels, (float *)out[1], (uint8_t *)out[0]);
    });
}

extern "C" int lt_diskmovie_lightcurve_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                           const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                           const float *d_texels, double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(d_hits, R, W, max_images, metric, disk, map, movie, d_texels, &c);
    if (rc) return rc;
    return launch_lightcurve(t_start, dt, n_times, d_out, [&](dim3 grid, double *partial) {
        k_diskmovie_lightcurve_partial<<<grid, 256>>>(d_hits, d_n_hits, (int64_t)R * W, W, max_images, c.dm, c.mv, d_texels, t_start, dt, partial);
    });
}

extern "C" int lt_diskmovie_lightcurve(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                       const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                       const float *texels, double t_start, double dt, int32_t n_times, double *out)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(hits, R, W, max_images, metric, disk, map, movie, texels, &c);
    if (rc || (rc = check_n_times(n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {movie_texels(texels, map, movie)}, {out, (size_t)n_times, 24},
                            [&](void *const *in, void *const *out_) {
        return lt_diskmovie_lightcurve_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, movie,
                                           (const float *)in[2], t_start, dt, n_times, (double *)out_[0]);
    });
}

extern "C" int lt_diskmovie_spectrum_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                         const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                         const float *d_texels, const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskMovieCall c;
    SpectrumGrid sg;
    int rc = resolve_diskmovie(d_hits, R, W, max_images, metric, disk, map, movie, d_texels, &c);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg))) return rc;
    return launch_spectrum(sg, max_images, t_start, dt, n_times, d_out, [&](dim3 grid, size_t lds, int first, double *partial) {
        k_diskmovie_spectrum_partial<<<grid, 256, lds>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, c.dm, c.mv, d_texels, sg, t_start, dt, first,
                                                         partial);
    });
}

extern "C" int lt_diskmovie_spectrum(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                     const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                     const float *texels, const lt_spectrum *spec, double t_start, double dt, int32_t n_times, double *out)
{
    DiskMovieCall c;
    SpectrumGrid sg;
    int rc = resolve_diskmovie(hits, R, W, max_images, metric, disk, map, movie, texels, &c);
    if (rc || (rc = resolve_spectrum(spec, max_images, &sg)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {movie_texels(texels, map, movie)}, {out, (size_t)n_times, spectrum_row_bytes(sg)},
                            [&](void *const *in, void *const *out_) {
        return lt_diskmovie_spectrum_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, movie,
                                         (const float *)in[2], spec, t_start, dt, n_times, (double *)out_[0]);
    });
}

extern "C" int lt_diskmovie_visibility_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                           const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                           const float *d_texels, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start,
                                           double dt, int32_t n_times, double *d_out)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(d_hits, R, W, max_images, metric, disk, map, movie, d_texels, &c);
    if (rc || (rc = resolve_baselines(uv, n_baselines))) return rc;
    return launch_visibility_times(W, max_images, uv, n_baselines, split_orders, t_start, dt, n_times, d_out,
                                   [&](auto nt, dim3 grid, const VisibilityGrid &vg, const double *d_uv, double *partial) {
        constexpr int NT = decltype(nt)::value;
        k_diskmovie_visibility_partial<NT><<<grid, 256, visibility_lds_bytes(NT)>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, c.dm, c.mv,
                                                                                   d_texels, vg, t_start, dt, d_uv, partial);
    });
}

extern "C" int lt_diskmovie_visibility(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images,
                                       const lt_metric *metric, const lt_disk *disk, const lt_diskmap *map, const lt_diskmovie *movie,
                                       const float *texels, const double *uv, int32_t n_baselines, int32_t split_orders, double t_start, double dt,
                                       int32_t n_times, double *out)
{
    DiskMovieCall c;
    int rc = resolve_diskmovie(hits, R, W, max_images, metric, disk, map, movie, texels, &c);
    if (rc || (rc = resolve_baselines(uv, n_baselines)) || (rc = check_spectrum_times(t_start, dt, n_times))) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {movie_texels(texels, map, movie)},
                            {out, (size_t)n_times, visibility_row_bytes(max_images, n_baselines, split_orders)}, [&](void *const *in, void *const *out_) {
        return lt_diskmovie_visibility_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, map, movie,
                                           (const float *)in[2], uv, n_baselines, split_orders, t_start, dt, n_times, (double *)out_[0]);
    });
}
