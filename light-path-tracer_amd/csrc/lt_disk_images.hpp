// lt_disk_images.hpp -- the optically thin disk of lt_render_disk_images (include/ltrace.h): the hooks into the shared
// tile loop (DiskImagesStep; direct_tiles, lt_kernels.hpp) that record every crossing of the annulus and let the ray go
// on, the kernel k_kerr_disk_images, and its epilogues.  K1 is the frame path's prologue.
//
// Same disk as lt_disk.hpp (same crossing test, same refinement on the step's cubic Hermite, same redshift), but a hit
// changes neither the ray's state nor its event: the lane writes (r, phi) of the crossing into slot j of a slot-major
// (max_images, n_q) buffer and counts it.  Every ray therefore ends exactly as in k_kerr_direct, and the records are
// independent of max_images (a hit beyond the last slot is only counted).  Each ray stores its count once, where it
// stores its final record, so neither buffer needs zero-filling; the epilogues read slots below min(count, max_images).
#pragma once
#include "lt_disk.hpp"

namespace lt {

template <typename T> struct Vec2;
template <> struct Vec2<float> { using type = float2; };
template <> struct Vec2<double> { using type = double2; };

constexpr int DISK_MAX_IMAGES = 8; // LT_DISK_MAX_IMAGES

// The thin disk's hooks into the tile loop (direct_tiles, lt_kernels.hpp): DiskStep's streak gate (its proof is per step:
// it never needed the ray to stop) and disk test, with the crossing recorded instead of taking the ray's place.  A hit
// goes to img[n * n_q + q] for n < max_images and is counted in n, the lane's hit count for the tile's ray; only a real
// lane records (a ghost lane is a bitwise twin of the lead ray, whose hits are the lead's own, written by the lead).
// hits[q]: the ray's hit count, stored with its final record.
template <typename T, typename Integ> struct DiskImagesStep : DiskStep<T, Integ> {
    typename Vec2<T>::type *img;
    uint32_t *hits;
    int64_t n_q;
    int max_images;
    struct Lane : DiskStep<T, Integ>::Lane {
        uint32_t n; // hits of the tile's ray so far
    };
    __device__ __forceinline__ void begin_tile(Lane &l, const KerrConsts<T> &k) { DiskStep<T, Integ>::begin_tile(l, k); l.n = 0; }
    __device__ __forceinline__ int advance(Lane &l, const KerrConsts<T> &k, const RayConsts<T> &rc, typename Integ::State &st, int64_t q, bool real)
    {
        return disk_advance<T, Integ>(k, this->d, rc, l.vmax2, st, real, [&](typename Integ::State &, const State5<T> &hit, int ev) {
            if (l.n < (uint32_t)max_images) {
                typename Vec2<T>::type v;
                v.x = hit.r; v.y = hit.ph;
                img[(int64_t)l.n * n_q + q] = v;
            }
            ++l.n;
            return ev;
        });
    }
    __device__ __forceinline__ void stored(Lane &l, int64_t q) { hits[q] = l.n; }
};

template <typename T, typename Integ>
__global__ void __launch_bounds__(256, Integ::MIN_WAVES_PER_SIMD) k_kerr_disk_images(KerrConsts<T> k_in, DiskConsts<T> d,
                                                       const typename Vec4<T>::type *__restrict__ ic,
                                                       typename Vec4<T>::type *__restrict__ fin0,
                                                       typename Vec4<T>::type *__restrict__ fin1, int64_t n_q,
                                                       uint32_t long_iters, uint64_t *__restrict__ kstats,
                                                       unsigned long long *__restrict__ head,
                                                       typename Vec2<T>::type *__restrict__ img, uint32_t *__restrict__ hits,
                                                       int max_images)
{
    DiskImagesStep<T, Integ> step;
    step.d = d;
    step.img = img; step.hits = hits; step.n_q = n_q; step.max_images = max_images;
    direct_tiles<T, Integ>(k_in, step, ic, fin0, fin1, n_q, long_iters, nullptr, kstats, head);
}

// ---- K3 ---------------------------------------------------------------------------------------------------------------
// Outputs of the images epilogue beyond FrameOut: images (R, W, max_images, 3) float32 (r_hit, phi_hit in [0, 2 pi), g),
// NaN in unused slots; n_hits (R, W) saturating at 255.  Either may be NULL.
struct DiskImagesOut {
    const void *img;     // the integrate kernel's slot buffer: Vec2<T> [max_images][n_q]
    const uint32_t *hits; // [n_q]
    int64_t n_q;
    int max_images;
    float *images;
    uint8_t *n_hits;
};

// One pixel per work-item, as k_epilogue_disk.  Every non-image output is k_epilogue_frame's (load_result / shade of
// the ray's own end); the colour adds the light of the stored hits: rgb = clamp(base + sum_j E_j, 0, 1), summed in
// float64, base first (0 without a background), then the slots in order.  A pixel without a stored hit keeps base.
template <typename T, bool HAS_BG>
__global__ void __launch_bounds__(EPILOGUE_BLOCK) k_epilogue_disk_images(CamConsts c, MetricConsts m, DiskShade ds,
                                                                         const typename Vec4<T>::type *__restrict__ fin0,
                                                                         const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                                         DiskImagesOut di)
{
    const int lrow = (int)blockIdx.y, ix = (int)(blockIdx.x * EPILOGUE_BLOCK + threadIdx.x);
    const int64_t p = (int64_t)lrow * c.W + ix;
    StatAcc acc;
    uint32_t nh = 0;
    if (ix < c.W) {
        const int64_t q = pixel_to_q(c, ix, lrow);
        RayResult res;
        load_result<T>(m, fin0, fin1, q, res);
        acc.add(res);
        nh = di.hits[q];
        const int ns = (int)(nh < (uint32_t)di.max_images ? nh : (uint32_t)di.max_images);
        const double xi = (double)fin1[q].y;
        const typename Vec2<T>::type *img = (const typename Vec2<T>::type *)di.img;
        const float fa32 = (res.status == 1) ? (float)res.fa : __builtin_nanf("");
        const long long wl = res.n_half < 0 ? 0 : (res.n_half > 65535 ? 65535 : res.n_half);
        if (o.fa) o.fa[p] = fa32;
        if (o.w) o.w[p] = (uint16_t)wl;
        if (o.status) o.status[p] = (int8_t)res.status;
        if (o.steps) o.steps[p] = res.steps;
        if (di.n_hits) di.n_hits[p] = (uint8_t)(nh > 255u ? 255u : nh);
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        int nch = (HAS_BG && o.bg) ? o.bg_c : 3;
        if (HAS_BG && o.bg && (o.rgb || o.rgba)) shade<HAS_BG>(c, o, ix, local_to_global_row(c, lrow), fa32, (int)wl, rgb, nch);
        double sum[3] = {(double)rgb[0], (double)rgb[1], (double)rgb[2]};
        for (int j = 0; j < di.max_images; ++j) {
            const float NaNf = __builtin_nanf("");
            float r3[3] = {NaNf, NaNf, NaNf};
            if (j < ns) {
                const typename Vec2<T>::type v = img[(int64_t)j * di.n_q + q];
                r3[0] = (float)v.x;
                r3[1] = (float)wrap_2pi((double)v.y);
                r3[2] = (float)disk_redshift(ds.M, ds.a, (double)v.x, xi);
                double e[3];
                disk_emission(ds, r3[0], r3[2], e);
                if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
                else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
            }
            if (di.images) {
                float *dst = di.images + (p * di.max_images + j) * 3;
                dst[0] = r3[0]; dst[1] = r3[1]; dst[2] = r3[2];
            }
        }
        if (ns > 0) for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)fmin(fmax(sum[ch], 0.0), 1.0);
        if (o.rgb) for (int ch = 0; ch < nch; ++ch) o.rgb[p * nch + ch] = rgb[ch];
        if (o.rgba) store_rgba(o, p, rgb, nch);
    }
    // words 6, 7: the rays with at least one hit and all hits (-> LT_STAT_DISK, LT_STAT_DISK_HITS)
    flush_stats<8>(o.stats, acc, m, nh > 0, nh);
}

// Epilogue of lt_trace_batch_kerr_disk_images: k_epilogue_arrays plus out_images (n, max_images, 3) float64
// (r_hit, phi_hit in [0, 2 pi), g), NaN in unused slots, and out_n_hits (n) int32 (every hit of the ray).
template <typename T>
__global__ void __launch_bounds__(256) k_epilogue_arrays_disk_images(MetricConsts m, DiskShade ds,
                                                                     const typename Vec4<T>::type *__restrict__ fin0,
                                                                     const typename Vec4<T>::type *__restrict__ fin1, int64_t n,
                                                                     double *__restrict__ out_fa, int64_t *__restrict__ out_w,
                                                                     int8_t *__restrict__ out_status, uint32_t *__restrict__ out_evals,
                                                                     const typename Vec2<T>::type *__restrict__ img,
                                                                     const uint32_t *__restrict__ hits, int64_t n_q, int max_images,
                                                                     double *__restrict__ out_images, int32_t *__restrict__ out_n_hits)
{
    int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    RayResult res;
    load_result<T>(m, fin0, fin1, q, res);
    const double NaN = __builtin_nan("");
    out_fa[q] = (res.status == 1) ? res.fa : NaN;
    out_w[q] = res.n_half;
    if (out_status) out_status[q] = (int8_t)res.status;
    if (out_evals) out_evals[q] = res.evals;
    const uint32_t nh = hits[q];
    if (out_n_hits) out_n_hits[q] = (int32_t)nh;
    if (!out_images) return;
    const double xi = (double)fin1[q].y;
    for (int j = 0; j < max_images; ++j) {
        double d3[3] = {NaN, NaN, NaN};
        if ((uint32_t)j < nh) {
            const typename Vec2<T>::type v = img[(int64_t)j * n_q + q];
            d3[0] = (double)v.x;
            d3[1] = wrap_2pi((double)v.y);
            d3[2] = disk_redshift(ds.M, ds.a, (double)v.x, xi);
        }
        double *dst = out_images + (q * max_images + j) * 3;
        dst[0] = d3[0]; dst[1] = d3[1]; dst[2] = d3[2];
    }
}

} // namespace lt
