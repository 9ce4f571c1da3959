// lt_hotspot.hpp -- an orbiting hot spot re-shaded from the stored hits of lt_trace_disk_hits (include/ltrace.h, "hot
// spot"): the frame at one observer time (k_shade_hotspot) and the light curve over many (k_lightcurve_partial,
// k_lightcurve_final).  Both read the callers' own (R, W, max_images, 4) float32 records (r, phi, g, elapsed time) and
// evaluate in float64, so that a frame is a function of what is stored.
#pragma once
#include "lt_disk.hpp"

namespace lt {

struct HotspotShade {
    double r_spot, phi0, omega; // the spot's orbit: phi_s(t) = phi0 + omega t, omega the Keplerian rate at r_spot
    double inv_2s2;             // 1 / (2 sigma^2)
    double exposure;
    int with_disk;
};

// Light of the spot seen through one stored hit, unclamped: E = exposure g^4 w ramp(g), w = exp(-d^2 / 2 sigma^2) with d the
// distance in the disk's plane between the hit and the spot at the time the light left, t_obs - dt.
__device__ __forceinline__ double hotspot_intensity(const HotspotShade &hs, double t_obs, const float *rec)
{
    const double r = (double)rec[0], ph = (double)rec[1], g = (double)rec[2], dt = (double)rec[3];
    const double phi_s = hs.phi0 + hs.omega * (t_obs - dt);
    const double d2 = r * r + hs.r_spot * hs.r_spot - 2.0 * r * hs.r_spot * cos(ph - phi_s);
    const double g2 = g * g;
    return hs.exposure * (g2 * g2) * exp(-d2 * hs.inv_2s2);
}

__device__ __forceinline__ void hotspot_emission(const HotspotShade &hs, double t_obs, const float *rec, double *e)
{
    const double g = (double)rec[2];
    const double I = hotspot_intensity(hs, t_obs, rec); // exposure g^4 w, what a spectrum bins (lt_spectrum.hpp)
    for (int i = 0; i < 3; ++i) e[i] = I * fmin(fmax(2.0 * g - 0.5 * i, 0.0), 1.0);
}

// Slots of a pixel that hold a hit: min(n_hits, max_images), or without n_hits the leading slots whose r is not NaN.
__device__ __forceinline__ int stored_slots(const float *rec, const uint8_t *n_hits, int64_t p, int max_images)
{
    if (n_hits) return n_hits[p] < max_images ? (int)n_hits[p] : max_images;
    int ns = 0;
    while (ns < max_images && rec[ns * 4] == rec[ns * 4]) ++ns;
    return ns;
}

// One pixel of a re-shaded frame: rgb = clamp(base + sum_j (with_disk E_j^disk + E_j^emit), 0, 1), summed in float64, base
// first (0 without one), then per slot the disk's light and the emitter's.  A pixel without a stored hit keeps base.
// emit(rec, e): the emitter's unclamped light through one stored hit (hotspot_emission; diskmap_emission of lt_diskmap.hpp).
// The body of every frame kernel of the family, one-sample and supersampled: they agree bit for bit because it is one.
template <typename Emit>
__device__ __forceinline__ void reshade_pixel(const float *hits, const uint8_t *n_hits, int64_t p, int max_images, const DiskShade &ds,
                                              int with_disk, const float *base, int nch, Emit emit, float *rgb)
{
    const float *rec = hits + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (base) for (int ch = 0; ch < nch; ++ch) rgb[ch] = base[p * nch + ch];
    double sum[3] = {(double)rgb[0], (double)rgb[1], (double)rgb[2]};
    for (int j = 0; j < ns; ++j) {
        double e[3];
        if (with_disk) {
            disk_emission(ds, rec[j * 4], rec[j * 4 + 2], e);
            if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
            else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
        }
        emit(rec + j * 4, e);
        if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
        else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
    }
    if (ns > 0) for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)fmin(fmax(sum[ch], 0.0), 1.0);
}

// The frame kernels' tail: pixel p of the float32 frame (nch channels) and of the RGBA8 frame, whichever is asked for.
__device__ __forceinline__ void store_pixel(int64_t p, const float *rgb, int nch, float *out_rgb, uint8_t *out_rgba)
{
    if (out_rgb) for (int ch = 0; ch < nch; ++ch) out_rgb[p * nch + ch] = rgb[ch];
    if (out_rgba) {
        FrameOut o{};
        o.rgba = out_rgba;
        store_rgba(o, p, rgb, nch);
    }
}

// One pixel per work-item.
__global__ void __launch_bounds__(256) k_shade_hotspot(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                       int max_images, DiskShade ds, HotspotShade hs, double t_obs,
                                                       const float *__restrict__ base, int nch, float *__restrict__ out_rgb,
                                                       uint8_t *__restrict__ out_rgba)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    float rgb[3];
    reshade_pixel(hits, n_hits, p, max_images, ds, hs.with_disk, base, nch,
                  [&](const float *rec, double *e) { hotspot_emission(hs, t_obs, rec, e); }, rgb);
    store_pixel(p, rgb, nch, out_rgb, out_rgba);
}

// The light curve: per time, sum of e, e ix and e iy over all pixels and stored slots, e the mean of the spot's three
// channels.  Two stages in a fixed order and no floating-point atomics, so a result is the same bits run after run:
// workgroup (b, t) sums the pixels p = b 256 + i + k 256 LC_BLOCKS (k ascending) of time t per work-item i, folds its
// 256 sums with a tree in LDS and writes one partial; k_lightcurve_final adds a time's LC_BLOCKS partials in order.
constexpr int LC_BLOCKS = 256;

__device__ __forceinline__ void lc_tree(double (*sh)[3], double *v)
{
    const int i = (int)threadIdx.x;
    for (int c = 0; c < 3; ++c) sh[i][c] = v[c];
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (i < half) for (int c = 0; c < 3; ++c) sh[i][c] += sh[i + half][c];
        __syncthreads();
    }
}

// The first stage: the stride loop of work-item i of workgroup (b, t), the tree and the partial's store.  pixel(p, v) adds
// pixel p's three columns to v.
template <typename Pixel> __device__ __forceinline__ void lightcurve_partial(int64_t n_px, double *partial, Pixel pixel)
{
    __shared__ double sh[256][3];
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_px; p += (int64_t)256 * LC_BLOCKS) pixel(p, v);
    lc_tree(sh, v);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partial[((int64_t)blockIdx.y * LC_BLOCKS + blockIdx.x) * 3 + c] = sh[0][c];
}

// The columns of an emitter's light curve (the spot's, the map's): (e, e ix, e iy) of pixel p, e the mean of the three
// channels of emit(rec, e) summed over the pixel's stored slots.
template <typename Emit>
__device__ __forceinline__ void lc_add_centroid(const float *hits, const uint8_t *n_hits, int64_t p, int W, int max_images, Emit emit, double *v)
{
    const float *rec = hits + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    double e_px = 0.0;
    for (int j = 0; j < ns; ++j) {
        double e[3];
        emit(rec + j * 4, e);
        e_px += (e[0] + e[1] + e[2]) / 3.0;
    }
    v[0] += e_px; v[1] += e_px * (double)(p % W); v[2] += e_px * (double)(p / W);
}

__global__ void __launch_bounds__(256) k_lightcurve_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                            int W, int max_images, HotspotShade hs, double t_start, double dt,
                                                            double *__restrict__ partial)
{
    const double t_obs = t_start + dt * (double)blockIdx.y;
    lightcurve_partial(n_px, partial, [&](int64_t p, double *v) {
        lc_add_centroid(hits, n_hits, p, W, max_images, [&](const float *rec, double *e) { hotspot_emission(hs, t_obs, rec, e); }, v);
    });
}

__global__ void __launch_bounds__(256) k_lightcurve_final(const double *__restrict__ partial, double *__restrict__ out)
{
    __shared__ double sh[256][3];
    double v[3];
    for (int c = 0; c < 3; ++c) v[c] = partial[((int64_t)blockIdx.x * LC_BLOCKS + threadIdx.x) * 3 + c];
    lc_tree(sh, v);
    if (threadIdx.x == 0) for (int c = 0; c < 3; ++c) out[(int64_t)blockIdx.x * 3 + c] = sh[0][c];
}

} // namespace lt
