// lt_hotspot_aa.hpp -- supersampled hot-spot and Stokes frames (include/ltrace.h, "supersampled hot-spot and Stokes
// frames"): the re-shade of lt_hotspot.hpp / lt_polarization.hpp on the FINE records (R S, W S, max_images, 4) and the
// resolve of lt_aa.hpp in one kernel each, k_shade_hotspot_aa and k_shade_stokes_aa.  Only the (R, W) output is written.
//
// The two phases of aa_resolve.  A workgroup of AA_BLOCK holds P = AA_BLOCK / S^2 output pixels ("slots", numbered over
// all R W output pixels: slot n is pixel (n / W, n mod W), so a workgroup's slots may straddle output rows); work-item t
// is sub-sample k = t mod S^2 of the workgroup's slot t / S^2, the work-items past P S^2 idle.  Phase 1: the work-item
// evaluates fine pixel (y S + j, x S + i), k = j S + i, and parks its three float32 values in LDS -- the S sub-samples of
// a fine row read S max_images 16 contiguous bytes.  Phase 2, after the barrier every work-item reaches: work-item
// t < P adds its slot's S^2 triples in order (j outer, i inner) in float64 from 0.0, divides by (double)(S S) and writes
// the output pixel.
//
// Phase 1 is the one-sample kernels' own pixel body (reshade_pixel of lt_hotspot.hpp, stokes_pixel of
// lt_polarization.hpp) on the fine records, so S = 1 is the one-sample frame bit for bit.  No floating-point atomics;
// nothing depends on the launch geometry: a fine pixel's value is a function of its records, a sum's order is the
// definition's.
#pragma once
#include "lt_aa.hpp"
#include "lt_polarization.hpp"

namespace lt {

// Slot arithmetic of one work-item, both phases.
struct HotspotAaSlots {
    int S, S2, P;
    int64_t n_out; // R W
    int W;         // output width
    __device__ __forceinline__ HotspotAaSlots(int samples, int64_t n_out_, int W_)
        : S(samples), S2(samples * samples), P(AA_BLOCK / (samples * samples)), n_out(n_out_), W(W_) {}
    // phase 1: the fine pixel work-item t evaluates, or -1 (an idle lane, a slot past the frame)
    __device__ __forceinline__ int64_t fine_pixel(int t) const
    {
        const int pl = t / S2, k = t - pl * S2;
        const int64_t n = (int64_t)blockIdx.x * P + pl;
        if (pl >= P || n >= n_out) return -1;
        const int64_t y = n / W, x = n - y * W;
        const int j = k / S, i = k - j * S;
        return (y * S + j) * ((int64_t)W * S) + (x * S + i);
    }
    // phase 2: the output pixel work-item t resolves, or -1
    __device__ __forceinline__ int64_t out_pixel(int t) const
    {
        const int64_t n = (int64_t)blockIdx.x * P + t;
        return (t < P && n < n_out) ? n : -1;
    }
};

// Phase 2's sum: the S^2 parked triples of slot t in order, float64 from 0.0, the mean rounded to float32.
__device__ __forceinline__ void hotspot_aa_mean(const float (*sh)[3], int t, int S2, float *mean)
{
    double sum[3] = {0.0, 0.0, 0.0};
    for (int s = t * S2; s < (t + 1) * S2; ++s) {
        sum[0] += (double)sh[s][0]; sum[1] += (double)sh[s][1]; sum[2] += (double)sh[s][2];
    }
    const double s2 = (double)S2;
    for (int c = 0; c < 3; ++c) mean[c] = (float)(sum[c] / s2);
}

// hits, n_hits, base: the FINE buffers ((R S) (W S) pixels); out_rgb / out_rgba: (R, W) pixels.  grid = ceil(R W / P).
__global__ void __launch_bounds__(AA_BLOCK) k_shade_hotspot_aa(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                               int64_t n_out, int W, int samples, int max_images, DiskShade ds,
                                                               HotspotShade hs, double t_obs, const float *__restrict__ base, int nch,
                                                               float *__restrict__ out_rgb, uint8_t *__restrict__ out_rgba)
{
    __shared__ float sh_rgb[AA_BLOCK][3];
    const HotspotAaSlots sl(samples, n_out, W);
    const int t = (int)threadIdx.x;
    const int64_t p = sl.fine_pixel(t);
    if (p >= 0) {
        float rgb[3];
        reshade_pixel(hits, n_hits, p, max_images, ds, hs.with_disk, base, nch,
                      [&](const float *rec, double *e) { hotspot_emission(hs, t_obs, rec, e); }, rgb);
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

// hits, n_hits, pol: the FINE buffers; out: (R, W, 3) float32 (I, Q, U).  grid = ceil(R W / P).
__global__ void __launch_bounds__(AA_BLOCK) k_shade_stokes_aa(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                              const float *__restrict__ pol, int64_t n_out, int W, int samples,
                                                              int max_images, DiskShade ds, HotspotShade hs, double pol_frac,
                                                              double t_obs, float *__restrict__ out)
{
    __shared__ float sh_iqu[AA_BLOCK][3];
    const HotspotAaSlots sl(samples, n_out, W);
    const int t = (int)threadIdx.x;
    const int64_t p = sl.fine_pixel(t);
    if (p >= 0) {
        double sum[3];
        stokes_pixel(hits, n_hits, pol, p, max_images, ds, hs, pol_frac, t_obs, sum);
        for (int c = 0; c < 3; ++c) sh_iqu[t][c] = (float)sum[c];
    }
    __syncthreads();
    const int64_t po = sl.out_pixel(t);
    if (po >= 0) {
        float iqu[3];
        hotspot_aa_mean(sh_iqu, t, sl.S2, iqu);
        for (int c = 0; c < 3; ++c) out[po * 3 + c] = iqu[c];
    }
}

} // namespace lt
