// lt_diskmovie.hpp -- a disk movie: emissivity tables that change with time, shaded from the stored hits of
// lt_trace_disk_hits (include/ltrace.h, "a disk movie").  The map's products -- the frame (k_shade_diskmovie), the
// supersampled frame (k_shade_diskmovie_aa), the light curve (k_diskmovie_lightcurve_partial), the dynamic spectrum
// (k_diskmovie_spectrum_partial) and the visibilities (k_diskmovie_visibility_partial) -- with the table looked up in the
// two frames that bracket each slot's own emission time, each unwound from its own epoch by the map's rotation, and blended.
//
// The tables are read where they lie, eight gathers per slot (four where one frame is held): texels (n_frames, n_r, n_phi),
// frame-major, so both frames of a pair keep the map's locality in phi; a movie of many frames does not fit one XCD's L2
// and the gathers then come from the Infinity Cache.  No LDS tile of it, no floating-point atomics.
//
// The kernels are the stored-hit kernels (reshade_pixel, store_pixel, lightcurve_partial, lc_add_centroid of lt_hotspot.hpp;
// the two phases of lt_hotspot_aa.hpp; spectrum_partial of lt_spectrum.hpp; visibility_partial of lt_visibility.hpp) with
// diskmovie_intensity / diskmovie_emission as the emitter.
#pragma once
#include "lt_diskmap.hpp"
#include "lt_spectrum.hpp"
#include "lt_visibility.hpp"

namespace lt {

struct DiskMovieShade {
    double t0, dt_frame;    // coordinate time of frame 0, spacing of the frames
    int64_t frame_texels;   // n_r n_phi: the offset from one frame to the next
    int n_frames, loop;
};

// exposure g^4 m of one stored hit: m the blend of the two frames about the slot's emission time (the header's steps 1 to
// 5).  Every frame index is clamped before it is used, whatever the record holds.
__device__ __forceinline__ double diskmovie_intensity(const DiskMapShade &dm, const DiskMovieShade &mv, const float *__restrict__ texels,
                                                      double t_obs, const float *rec)
{
    const double r = (double)rec[0], ph = (double)rec[1], g = (double)rec[2], dt = (double)rec[3];
    double m = 0.0;
    if (r >= dm.r_min && r <= dm.r_max) {
        const double t_em = t_obs - dt;
        const double om = diskmap_omega(dm, r);
        const double s = (t_em - mv.t0) / mv.dt_frame;
        const double last = (double)(mv.n_frames - 1);
        double q0, q1, f_t, k0, k1;
        if (mv.loop) {
            const bool ok = s == s;
            q0 = ok ? floor(s) : 0.0;
            q1 = q0 + 1.0;
            f_t = ok ? s - q0 : 0.0;
            const double n = (double)mv.n_frames;
            k0 = fmin(fmax(q0 - n * floor(q0 / n), 0.0), last);          // (a NaN index, of an infinite s, gives 0)
            k1 = fmin(fmax(q1 - n * floor(q1 / n), 0.0), last);
        } else {
            q0 = fmin(fmax(floor(s), 0.0), last);                          // (a NaN s gives 0)
            q1 = fmin(q0 + 1.0, last);
            f_t = fmin(fmax(s - q0, 0.0), 1.0);
            k0 = q0;
            k1 = q1;
        }
        const double T0 = mv.t0 + q0 * mv.dt_frame;
        m = diskmap_bilinear(dm, texels + (int64_t)k0 * mv.frame_texels, r, wrap_2pi(ph - om * (t_em - T0)));
        if (mv.loop || q1 != q0) {
            const double T1 = mv.t0 + q1 * mv.dt_frame;
            const double m1 = diskmap_bilinear(dm, texels + (int64_t)k1 * mv.frame_texels, r, wrap_2pi(ph - om * (t_em - T1)));
            m = (1.0 - f_t) * m + f_t * m1;
        }
    }
    const double g2 = g * g;
    return dm.exposure * (g2 * g2) * m;
}

__device__ __forceinline__ void diskmovie_emission(const DiskMapShade &dm, const DiskMovieShade &mv, const float *__restrict__ texels,
                                                   double t_obs, const float *rec, double *e)
{
    const double g = (double)rec[2];
    const double I = diskmovie_intensity(dm, mv, texels, t_obs, rec);
    for (int i = 0; i < 3; ++i) e[i] = I * fmin(fmax(2.0 * g - 0.5 * i, 0.0), 1.0);
}

// One pixel per work-item, k_shade_diskmap with the movie as the emitter.
__global__ void __launch_bounds__(256) k_shade_diskmovie(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                         int max_images, DiskShade ds, DiskMapShade dm, DiskMovieShade mv,
                                                         const float *__restrict__ texels, double t_obs, const float *__restrict__ base,
                                                         int nch, float *__restrict__ out_rgb, uint8_t *__restrict__ out_rgba)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    float rgb[3];
    reshade_pixel(hits, n_hits, p, max_images, ds, dm.with_disk, base, nch,
                  [&](const float *rec, double *e) { diskmovie_emission(dm, mv, texels, t_obs, rec, e); }, rgb);
    store_pixel(p, rgb, nch, out_rgb, out_rgba);
}

// The two phases of k_shade_diskmap_aa: hits, n_hits, base are the FINE buffers, out_rgb / out_rgba the (R, W) output.
__global__ void __launch_bounds__(AA_BLOCK) k_shade_diskmovie_aa(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                 int64_t n_out, int W, int samples, int max_images, DiskShade ds,
                                                                 DiskMapShade dm, DiskMovieShade mv, const float *__restrict__ texels,
                                                                 double t_obs, const float *__restrict__ base, int nch,
                                                                 float *__restrict__ out_rgb, uint8_t *__restrict__ out_rgba)
{
    __shared__ float sh_rgb[AA_BLOCK][3];
    const HotspotAaSlots sl(samples, n_out, W);
    const int t = (int)threadIdx.x;
    const int64_t p = sl.fine_pixel(t);
    if (p >= 0) {
        float rgb[3];
        reshade_pixel(hits, n_hits, p, max_images, ds, dm.with_disk, base, nch,
                      [&](const float *rec, double *e) { diskmovie_emission(dm, mv, texels, t_obs, rec, e); }, rgb);
        sh_rgb[t][0] = rgb[0]; sh_rgb[t][1] = rgb[1]; sh_rgb[t][2] = rgb[2];
    }
    __syncthreads();
    const int64_t po = sl.out_pixel(t);
    if (po >= 0) {
        float rgb[3];
        hotspot_aa_mean(sh_rgb, t, sl.S2, rgb);
        store_pixel(po, rgb, nch, out_rgb, out_rgba);
    }
}

// The light curve's first stage, k_diskmap_lightcurve_partial with the movie as the emitter.
__global__ void __launch_bounds__(256) k_diskmovie_lightcurve_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                      int64_t n_px, int W, int max_images, DiskMapShade dm, DiskMovieShade mv,
                                                                      const float *__restrict__ texels, double t_start, double dt,
                                                                      double *__restrict__ partial)
{
    const double t_obs = t_start + dt * (double)blockIdx.y;
    lightcurve_partial(n_px, partial, [&](int64_t p, double *v) {
        lc_add_centroid(hits, n_hits, p, W, max_images, [&](const float *rec, double *e) { diskmovie_emission(dm, mv, texels, t_obs, rec, e); }, v);
    });
}

// The spectrum's and the visibilities' first stages, k_diskmap_spectrum_partial and k_diskmap_visibility_partial with the
// movie as the emitter.
__global__ void __launch_bounds__(256) k_diskmovie_spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                    int64_t n_px, int max_images, DiskMapShade dm, DiskMovieShade mv,
                                                                    const float *__restrict__ texels, SpectrumGrid sg, double t_start,
                                                                    double dt, int first, double *__restrict__ partial)
{
    const double t_obs = spectrum_time(t_start, dt, first + (int)blockIdx.y);
    spectrum_partial(hits, n_hits, n_px, max_images, sg, partial, [&](const float *rec) { return diskmovie_intensity(dm, mv, texels, t_obs, rec); });
}

template <int NT>
__global__ void __launch_bounds__(256) k_diskmovie_visibility_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                      int64_t n_px, int max_images, DiskMapShade dm, DiskMovieShade mv,
                                                                      const float *__restrict__ texels, VisibilityGrid vg, double t_start,
                                                                      double dt, const double *__restrict__ uv, double *__restrict__ partial)
{
    visibility_partial<NT>(hits, n_hits, n_px, max_images, vg, t_start, dt, uv, partial,
                           [&](const float *rec, double t_obs) { return diskmovie_intensity(dm, mv, texels, t_obs, rec); });
}

} // namespace lt
