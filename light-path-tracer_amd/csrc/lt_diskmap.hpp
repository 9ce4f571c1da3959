// lt_diskmap.hpp -- a rotating emissivity map on the disk, shaded from the stored hits of lt_trace_disk_hits
// (include/ltrace.h, "a rotating emissivity map"): the frame at one observer time (k_shade_diskmap), the supersampled
// frame resolved in the same kernel (k_shade_diskmap_aa) and the light curve over many times
// (k_diskmap_lightcurve_partial, then k_lightcurve_final itself).  The hot spot's kernels with the Gaussian replaced by
// a bilinear look-up in the caller's (n_r, n_phi) float32 table, unwound by the rotation since t = 0.
//
// The table is read where it lies, four gathers per slot: rows have phi contiguous, so the neighbouring pixels of a
// wavefront touch neighbouring texels, and a 256 x 1024 table is 1 MB of L2.  No LDS tile of it (VERDICT weak #4).
//
// The per-pixel bodies of k_shade_hotspot, k_shade_hotspot_aa and k_lightcurve_partial are RESTATED here, statement for
// statement, through the same device functions (stored_slots, disk_emission, store_rgba, lc_tree, HotspotAaSlots,
// hotspot_aa_mean), with diskmap_emission in hotspot_emission's place: those kernels' source is not touched, and
// their code is held byte-identical (tools/kernel_diff.sh).
#pragma once
#include "lt_hotspot_aa.hpp"

namespace lt {

struct DiskMapShade {
    double r_min, r_max;   // the annulus the table covers
    double omega_p;        // LT_MAP_RIGID: the pattern speed
    double sM, a_sM;       // LT_MAP_KEPLERIAN: Omega(r) = sM / (r^1.5 + a_sM), sM = sqrt(M)
    double phi_scale;      // n_phi / 2 pi
    double exposure;
    int n_r, n_phi;
    int rigid, with_disk;
};

// Light of the map seen through one stored hit, unclamped: E = exposure g^4 m ramp(g), m the table's bilinear value at
// the hit's radius and at its azimuth unwound to t = 0, psi = wrap_2pi(phi - Omega (t_obs - dt)); constant extrapolation
// over the outer half texels in r, periodic in psi; m = 0 outside [r_min, r_max] and for a NaN r (the comparisons are
// false).  Every index is clamped before it is used, whatever the record holds.
__device__ __forceinline__ void diskmap_emission(const DiskMapShade &dm, const float *__restrict__ texels, double t_obs, const float *rec,
                                                 double *e)
{
    const double r = (double)rec[0], ph = (double)rec[1], g = (double)rec[2], dt = (double)rec[3];
    double m = 0.0;
    if (r >= dm.r_min && r <= dm.r_max) {
        const double t_em = t_obs - dt;
        const double om = dm.rigid ? dm.omega_p : dm.sM / (r * sqrt(r) + dm.a_sM);
        const double psi = wrap_2pi(ph - om * t_em);
        const int top = dm.n_r - 1;
        const double v = fmin(fmax((r - dm.r_min) / (dm.r_max - dm.r_min) * (double)dm.n_r - 0.5, 0.0), (double)top);
        const int i0 = min((int)floor(v), top), i1 = min(i0 + 1, top);
        const double f_r = v - (double)i0;
        const double u = psi * dm.phi_scale - 0.5;
        const double fl = floor(u);
        int k0 = (int)fmin(fmax(fl, -1.0), (double)dm.n_phi); // psi in [0, 2 pi): floor(u) in [-1, n_phi]; a NaN gives -1
        if (k0 < 0) k0 += dm.n_phi;
        if (k0 >= dm.n_phi) k0 -= dm.n_phi;
        const int k1 = k0 + 1 < dm.n_phi ? k0 + 1 : 0;
        const double f_p = u - fl;
        const float *row0 = texels + (int64_t)i0 * dm.n_phi, *row1 = texels + (int64_t)i1 * dm.n_phi;
        const double t00 = (double)row0[k0], t01 = (double)row0[k1], t10 = (double)row1[k0], t11 = (double)row1[k1];
        m = (1.0 - f_r) * ((1.0 - f_p) * t00 + f_p * t01) + f_r * ((1.0 - f_p) * t10 + f_p * t11);
    }
    const double g2 = g * g;
    const double I = dm.exposure * (g2 * g2) * m;
    for (int i = 0; i < 3; ++i) e[i] = I * fmin(fmax(2.0 * g - 0.5 * i, 0.0), 1.0);
}

// One pixel per work-item, k_shade_hotspot's shape: rgb = clamp(base + sum_j (with_disk E_j^disk + E_j^map), 0, 1), summed
// in float64, base first (0 without one), then per slot the disk's light and the map's.  A pixel without a stored hit
// keeps base.
__global__ void __launch_bounds__(256) k_shade_diskmap(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                       int max_images, DiskShade ds, DiskMapShade dm, const float *__restrict__ texels,
                                                       double t_obs, const float *__restrict__ base, int nch, float *__restrict__ out_rgb,
                                                       uint8_t *__restrict__ out_rgba)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    const float *rec = hits + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    if (base) for (int ch = 0; ch < nch; ++ch) rgb[ch] = base[p * nch + ch];
    double sum[3] = {(double)rgb[0], (double)rgb[1], (double)rgb[2]};
    for (int j = 0; j < ns; ++j) {
        double e[3];
        if (dm.with_disk) {
            disk_emission(ds, rec[j * 4], rec[j * 4 + 2], e);
            if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
            else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
        }
        diskmap_emission(dm, texels, t_obs, rec + j * 4, e);
        if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
        else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
    }
    if (ns > 0) for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)fmin(fmax(sum[ch], 0.0), 1.0);
    if (out_rgb) for (int ch = 0; ch < nch; ++ch) out_rgb[p * nch + ch] = rgb[ch];
    if (out_rgba) {
        FrameOut o{};
        o.rgba = out_rgba;
        store_rgba(o, p, rgb, nch);
    }
}

// The two phases of k_shade_hotspot_aa (lt_hotspot_aa.hpp): hits, n_hits, base are the FINE buffers ((R S) (W S) pixels),
// out_rgb / out_rgba the (R, W) output.  grid = ceil(R W / P), P = AA_BLOCK / S^2.
__global__ void __launch_bounds__(AA_BLOCK) k_shade_diskmap_aa(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                               int64_t n_out, int W, int samples, int max_images, DiskShade ds,
                                                               DiskMapShade dm, const float *__restrict__ texels, double t_obs,
                                                               const float *__restrict__ base, int nch, float *__restrict__ out_rgb,
                                                               uint8_t *__restrict__ out_rgba)
{
    __shared__ float sh_rgb[AA_BLOCK][3];
    const HotspotAaSlots sl(samples, n_out, W);
    const int t = (int)threadIdx.x;
    const int64_t p = sl.fine_pixel(t);
    if (p >= 0) {
        // k_shade_diskmap's body for fine pixel p
        const float *rec = hits + p * max_images * 4;
        const int ns = stored_slots(rec, n_hits, p, max_images);
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        if (base) for (int ch = 0; ch < nch; ++ch) rgb[ch] = base[p * nch + ch];
        double sum[3] = {(double)rgb[0], (double)rgb[1], (double)rgb[2]};
        for (int j = 0; j < ns; ++j) {
            double e[3];
            if (dm.with_disk) {
                disk_emission(ds, rec[j * 4], rec[j * 4 + 2], e);
                if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
                else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
            }
            diskmap_emission(dm, texels, t_obs, rec + j * 4, e);
            if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
            else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
        }
        if (ns > 0) for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)fmin(fmax(sum[ch], 0.0), 1.0);
        sh_rgb[t][0] = rgb[0]; sh_rgb[t][1] = rgb[1]; sh_rgb[t][2] = rgb[2];
    }
    __syncthreads();
    const int64_t po = sl.out_pixel(t);
    if (po >= 0) {
        float rgb[3];
        hotspot_aa_mean(sh_rgb, t, sl.S2, rgb);
        if (out_rgb) for (int ch = 0; ch < nch; ++ch) out_rgb[po * nch + ch] = rgb[ch];
        if (out_rgba) {
            FrameOut o{};
            o.rgba = out_rgba;
            store_rgba(o, po, rgb, nch);
        }
    }
}

// The light curve's first stage: k_lightcurve_partial's grid (LC_BLOCKS, n_times), stride, order and tree, e the mean of
// the map's three channels.  k_lightcurve_final adds a time's LC_BLOCKS partials.
__global__ void __launch_bounds__(256) k_diskmap_lightcurve_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                    int64_t n_px, int W, int max_images, DiskMapShade dm,
                                                                    const float *__restrict__ texels, double t_start, double dt,
                                                                    double *__restrict__ partial)
{
    __shared__ double sh[256][3];
    const double t_obs = t_start + dt * (double)blockIdx.y;
    double v[3] = {0.0, 0.0, 0.0};
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n_px; p += (int64_t)256 * LC_BLOCKS) {
        const float *rec = hits + p * max_images * 4;
        const int ns = stored_slots(rec, n_hits, p, max_images);
        double e_px = 0.0;
        for (int j = 0; j < ns; ++j) {
            double e[3];
            diskmap_emission(dm, texels, t_obs, rec + j * 4, e);
            e_px += (e[0] + e[1] + e[2]) / 3.0;
        }
        v[0] += e_px; v[1] += e_px * (double)(p % W); v[2] += e_px * (double)(p / W);
    }
    lc_tree(sh, v);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partial[((int64_t)blockIdx.y * LC_BLOCKS + blockIdx.x) * 3 + c] = sh[0][c];
}

} // namespace lt
