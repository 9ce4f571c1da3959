// lt_aa_adaptive.hpp -- the kernels of the adaptively supersampled frame (include/ltrace.h, "adaptive supersampling")
// around the integrate kernels, which do not know about pixels: they take n_q initial records in wavefronts of 64 and a
// ray's result does not depend on its wave mates.
//
//   k_aa_flag              reads the base pass's cover and float32 rgb (S_lo x S_lo rays per pixel, lt_render_aa's), applies
//                          the three tests of the definition to every pixel, writes `level` and appends the flagged pixels
//                          to a device list;
//   k_prologue_aa_list     the initial records of the S_hi x S_hi sub-samples of a chunk of that list: ray q = k S_hi^2 + t
//                          is sub-sample (t / S_hi, t % S_hi) of list pixel k = (y, x), which is fine pixel
//                          (x S_hi + i, y S_hi + j) of the S_hi fine camera -- k_prologue_camera's store_camera_ray;
//   k_epilogue_aa_list     the resolve of lt_aa.hpp (aa_resolve) over list entries instead of a row segment, overwriting
//                          rgb / rgba / cover at the listed pixels.
//
// One ray per work-item everywhere, as in lt_aa.hpp and for its reason.  Nothing depends on the order of the list: each
// entry's rays are a function of the entry alone and its outputs go to the entry's own pixel.
#pragma once
#include "lt_aa.hpp"

namespace lt {

constexpr int AA_FLAG_BLOCK = 256;

// More than one of the slots the mode's classes exclude each other in is non-zero, or (thin disk, whose slot 3 overlaps
// the others) some but not all sub-rays have a hit.
__device__ __forceinline__ bool aa_cover_mixed(uchar4 cv, int mode, int s2_lo)
{
    int n = (cv.x != 0) + (cv.y != 0) + (cv.z != 0);
    if (mode == AA_DISK_IMAGES) return n > 1 || (cv.w > 0 && (int)cv.w < s2_lo);
    return n + (cv.w != 0) > 1;
}

// cover (H, W, 4) and rgb (H, W, nch) float32 of the base pass; rgb is read only when contrast >= 0.  level (H, W) or
// NULL.  list: room for H W pixel indices (y W + x); *count: 0 on entry, the pixels appended on exit.  grid = (segments of
// AA_FLAG_BLOCK pixels, rows from y0 on).  The append is aggregated per wavefront -- a ballot, the lane's prefix in it, ONE atomic on
// the count per wavefront that flagged something (same-address atomics cost ~6 ns each) -- so the list's order
// is whatever order the wavefronts' atomics arrived in.
__global__ void __launch_bounds__(AA_FLAG_BLOCK) k_aa_flag(const uchar4 *__restrict__ cover, const float *__restrict__ rgb, int nch,
                                                           int W, int H, int y0, int s_lo, int s_hi, int mode, float contrast,
                                                           uint8_t *__restrict__ level, uint32_t *__restrict__ list,
                                                           unsigned int *__restrict__ count)
{
    const int y = y0 + (int)blockIdx.y, x = (int)(blockIdx.x * AA_FLAG_BLOCK + threadIdx.x);
    bool flag = false;
    if (x < W) {
        const int64_t p = (int64_t)y * W + x;
        const uchar4 cp = cover[p];
        flag = aa_cover_mixed(cp, mode, s_lo * s_lo);
        const bool colour = contrast >= 0.0f;
        float cp_rgb[3] = {0.0f, 0.0f, 0.0f};
        if (colour) for (int ch = 0; ch < nch; ++ch) cp_rgb[ch] = rgb[p * nch + ch];
        for (int dy = -1; dy <= 1; ++dy) {
            const int ny = y + dy;
            if (ny < 0 || ny >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int nx = x + dx;
                if (nx < 0 || nx >= W || (dx == 0 && dy == 0)) continue;
                const int64_t n = (int64_t)ny * W + nx;
                const uchar4 cn = cover[n];
                flag |= cn.x != cp.x || cn.y != cp.y || cn.z != cp.z || cn.w != cp.w;
                if (colour) for (int ch = 0; ch < nch; ++ch) flag |= fabsf(cp_rgb[ch] - rgb[n * nch + ch]) > contrast;
            }
        }
        if (level) level[p] = (uint8_t)(flag ? s_hi : s_lo);
    }
    // every work-item of the wavefront is here (no early return above)
    const unsigned long long ballot = __builtin_amdgcn_ballot_w64(flag);
    const unsigned int n_wave = (unsigned int)__popcll(ballot);
    if (n_wave == 0) return; // (wave-uniform)
    const unsigned int prefix = __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
    unsigned int base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(count, n_wave);
    base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
    if (flag) list[base + prefix] = (uint32_t)(y * W + x); // (the host refuses a frame of 2^31 pixels or more)
}

// The refined pixels of a call, into its counters (LT_STAT_AA_REFINED), on the stream like everything else.
__global__ void k_aa_count_to_stats(const unsigned int *__restrict__ count, unsigned long long *__restrict__ stats, int word)
{
    if (threadIdx.x == 0 && blockIdx.x == 0 && *count) atomicAdd(&stats[word], (unsigned long long)*count);
}

// c: the S_hi fine camera as one partition of the whole frame (n_parts = 1, no block list: local rows are global rows).
// list: the chunk's n entries; n_q = n S^2 rounded up to whole wavefronts (< 2^31); records past the chunk's end are pads.
template <typename T>
__global__ void __launch_bounds__(256) k_prologue_aa_list(CamConsts c, MetricConsts m, const uint32_t *__restrict__ list, int n,
                                                          int S, int W, typename Vec4<T>::type *__restrict__ ic, int64_t n_q)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_q) return;
    const uint32_t S2 = (uint32_t)(S * S), k = (uint32_t)q / S2, t = (uint32_t)q - k * S2;
    if (k >= (uint32_t)n) { store_ic<T>(ic, q, 0, 0, 0, FLAG_PAD); return; }
    const uint32_t p = list[k], y = p / (uint32_t)W, x = p - y * (uint32_t)W;
    const uint32_t j = t / (uint32_t)S, i = t - j * (uint32_t)S;
    const int ix = (int)(x * (uint32_t)S + i), grow = (int)(y * (uint32_t)S + j);
    store_camera_ray<T>(c, m, ic, q, ix, grow);
}

// List addressing of the resolve (AaOut of lt_aa.hpp is the other): slot e of the launch is the chunk's entry e, its
// sub-sample k is record e S^2 + k, and the result overwrites the entry's pixel of the WHOLE output frame.
struct AaListOut {
    int samples;          // S_hi
    int W;                // output width
    uint8_t *cover;       // (H, W, 4) of the whole frame, or NULL
    const uint32_t *list; // the chunk's entries: output pixel y W + x
    int n;                // ... and how many
    __device__ __forceinline__ bool live(int e) const { return e < n; }
    __device__ __forceinline__ void pixel(int e, int &x, int &y) const
    {
        const uint32_t p = list[e], py = p / (uint32_t)W;
        y = (int)py; x = (int)(p - py * (uint32_t)W);
    }
    __device__ __forceinline__ int64_t record(const CamConsts &, int e, int k, int, int) const { return (int64_t)e * (samples * samples) + k; }
    __device__ __forceinline__ int64_t out(int e) const { return (int64_t)list[e]; }
};

// c, o: as k_prologue_aa_list's camera and k_epilogue_aa's FrameOut (the background at S_hi fine size; rgb / rgba the
// WHOLE output frame).  grid = groups of P = AA_BLOCK / S^2 list entries.
template <typename T, int MODE, bool HAS_BG>
__global__ void __launch_bounds__(AA_BLOCK) k_epilogue_aa_list(CamConsts c, MetricConsts m, DiskShade ds,
                                                               const typename Vec4<T>::type *__restrict__ fin0,
                                                               const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                               DiskImagesOut di, AaListOut aa)
{
    aa_resolve<T, MODE, HAS_BG>(c, m, ds, fin0, fin1, o, di, aa);
}

} // namespace lt
