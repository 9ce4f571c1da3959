// lt_visibility.hpp -- complex visibilities of the stored hits of lt_trace_disk_hits (include/ltrace.h, "visibilities"):
// per observer time, plane and baseline b = (u, v) the sum of w exp(-2 pi i (u ix + v iy)) over the stored slots, w the
// weight a spectrum bins.  A skinny matrix product whose operands are made on the fly: the weights depend on (pixel,
// slot, time) and not on the baseline, the phases on (pixel, baseline) and not on the time or the slot.  So a workgroup
// evaluates each once and combines them from LDS and registers; no floating-point atomics anywhere.
//
// First stage (visibility_partial<NT>; grid (VIS_BLOCKS, batches of times, passes of 256 baselines), 256 work-items).
// A batch is `times` observer times with times x planes <= VIS_BATCH_TERMS terms; NT, the power of two from that count
// up, is the number of complex accumulators a work-item keeps in registers (2 NT doubles, 64 VGPRs at NT = 16).  A
// workgroup walks its pixels in chunks of 256 in the light curve's stride order.
//   Phase one: work-item i evaluates its pixel's weight for every term of the batch -- per time, per plane; without
//   split_orders the slots added in their order -- into LDS, term-major (sh_w[term][i]: neighbouring lanes write
//   neighbouring doubles, no bank conflict), with the pixel's (ix, iy) as doubles.  A pixel whose weights are all exactly 0
//   -- most of a frame has no hit -- is left out: each wavefront ballots and lists the lanes it keeps, in lane order.
//   Phase two: work-item k owns baseline pass 256 + k.  It walks the four lists in order; all lanes read the same
//   addresses (broadcasts: ds_read_b64 of one address is conflict-free whatever the layout), take ONE sincospi per kept
//   pixel and add the NT terms with two fused multiply-adds each.  A wavefront whose 64 baselines lie beyond n_baselines
//   skips the phase.
// After its last chunk the work-item writes its sums: one partial per (batch, block, term, baseline).
// Final stage (k_sum_blocks, lt_spectrum.hpp, with row = the terms x n_baselines x 2 doubles of a full batch): one work-item
// per (term, baseline, re / im) adds the VIS_BLOCKS partials in ascending block order.
//
// Why the passes are a grid dimension and the weights are evaluated again per pass: owning baselines k, k + 256, ... in one
// workgroup needs 2 NT doubles of accumulators per owned baseline -- 256 VGPRs at four -- or their round trip through
// memory per chunk.  A pass costs the weights of its pixels once more, terms x slots evaluations per pixel against 256
// sincospi and 512 NT multiply-adds per kept pixel (DESIGN.md 10j has the count and what both phases were measured at).
//
// LDS is sized by the launch (visibility_lds_bytes): NT x 256 x 8 (weights) + 2 x 256 x 8 (ix, iy) + 256 x 2 (lists) + 16
// (counts) = 37 392 B at NT = 16, so four workgroups could share a CU's 160 KiB at the largest configuration, and 6 672 B
// at NT = 1.  The registers bound the occupancy before that: at NT = 16 the map's kernel takes 143 VGPRs, the disk's 207
// and the spot's 208 (no scratch), three and two workgroups per CU.
#pragma once
#include "lt_spectrum.hpp"

namespace lt {

constexpr int VIS_BLOCKS = 256;          // LT_VISIBILITY_BLOCKS
constexpr int VIS_MAX_BASELINES = 1024;  // LT_VISIBILITY_MAX_BASELINES
constexpr int VIS_BATCH_TERMS = 16;      // LT_VISIBILITY_BATCH_TERMS
static_assert(VIS_BLOCKS == SP_BLOCKS, "k_sum_blocks (lt_spectrum.hpp) adds SP_BLOCKS partials per output");

extern __shared__ __attribute__((aligned(16))) unsigned char vis_lds[];
inline size_t visibility_lds_bytes(int nt) { return (size_t)nt * 256 * 8 + 2 * 256 * 8 + 256 * 2 + 16; }
static_assert((VIS_BATCH_TERMS * 256 * 8 + 2 * 256 * 8 + 256 * 2 + 16) * 4 <= 160 * 1024, "four workgroups of the largest batch share a CU");

// A unit is an observer time here and a (time, plane) pair in lt_visibility_stokes.hpp.
struct VisibilityGrid {
    int n_baselines, planes; // planes: 1, or max_images with split_orders
    int units;               // units of a batch: times x planes <= VIS_BATCH_TERMS, pairs <= VIS_STOKES_BATCH_PAIRS
    int n_units, first;      // the call's units, and the index of this launch's first one
    int W;                   // the record buffer's width: pixel p is (p % W, p / W)
};

// The phase of pixel (ix, iy) on baseline (u, v) as the header states it: x = u ix + v iy with both products rounded
// before the sum, f = x - rint(x) (exact, |f| <= 1/2), (s, c) = sincospi(2 f).  The term is (w c, -w s).
// The library is built with -ffp-contract=fast, under which the backend fuses a product into a sum whatever a pragma
// says (the listing showed v_mul, v_fmac here): the empty asm makes the two rounded products opaque, and costs nothing.
__device__ __forceinline__ void visibility_phase(double u, double v, double ix, double iy, double *s, double *c)
{
#pragma clang fp contract(off)
    double a = u * ix, b = v * iy;
    asm("" : "+v"(a), "+v"(b));
    const double x = a + b;
    const double f = x - rint(x);
    sincospi(2.0 * f, s, c);
}

// The walk both first stages share (lt_visibility_stokes.hpp has the other): the LDS carve-up, the ownership of the
// baselines, the chunks in stride order, the lists, phase two and the write of the partial.  NT: the complex accumulators.
// stride_terms: the terms of a full batch, the partial's stride; terms <= NT: those of this batch.  phase_one(p, sh_w, t)
// writes the weights of pixel p (which may lie beyond n_px) to sh_w[term * 256 + t] for the batch's terms and returns
// whether any of them is not exactly 0.  partial: this launch's (batch, block, term, baseline) complex sums.
// The callers' lambdas capture by value: capturing by reference the spot's kernels here took 7 % longer over phase one than
// the bodies this walk replaced, by value they compile to those bodies' sizes and registers (profiles/visibility_fold_check.txt).
template <int NT, typename PhaseOne>
__device__ __forceinline__ void visibility_walk(int64_t n_px, int W, int n_baselines, const double *__restrict__ uv,
                                                double *__restrict__ partial, int stride_terms, int terms, PhaseOne phase_one)
{
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    double *sh_w = (double *)vis_lds, *sh_x = sh_w + NT * 256, *sh_y = sh_x + 256;
    uint16_t *sh_list = (uint16_t *)(sh_y + 256);
    int *sh_cnt = (int *)(sh_list + 256);
    const int b = (int)blockIdx.z * 256 + t;
    const bool owner = b < n_baselines;
    const bool wave_owns = (int)blockIdx.z * 256 + wave * 64 < n_baselines;
    const double u = owner ? uv[2 * b] : 0.0, v = owner ? uv[2 * b + 1] : 0.0;
    double re[NT], im[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        re[i] = im[i] = 0.0;
        sh_w[i * 256 + t] = 0.0; // (the terms beyond `terms` stay 0)
    }
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_px; base += (int64_t)256 * VIS_BLOCKS) {
        // phase one: this pixel's weights, term-major, and the list of the pixels that hold light
        const int64_t p = base + t;
        const bool has = phase_one(p, sh_w, t);
        sh_x[t] = (double)(p % W);
        sh_y[t] = (double)(p / W);
        const uint64_t kept = __ballot(has);
        if (has) sh_list[wave * 64 + __popcll(kept & (((uint64_t)1 << lane) - 1))] = (uint16_t)t;
        if (lane == 0) sh_cnt[wave] = __popcll(kept);
        __syncthreads();
        // phase two: one sincospi per kept pixel and owned baseline, the batch's terms from LDS
        if (wave_owns) {
            for (int s = 0; s < 4; ++s) {
                const int n = sh_cnt[s];
                for (int e = 0; e < n; ++e) {
                    const int q = sh_list[s * 64 + e];
                    double sn, cs;
                    visibility_phase(u, v, sh_x[q], sh_y[q], &sn, &cs);
#pragma unroll
                    for (int i = 0; i < NT; ++i) {
                        const double w = sh_w[i * 256 + q];
                        re[i] = fma(w, cs, re[i]);
                        im[i] = fma(-w, sn, im[i]);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!owner) return;
    double *mine = partial + (((int64_t)blockIdx.y * VIS_BLOCKS + blockIdx.x) * stride_terms * n_baselines + b) * 2;
#pragma unroll
    for (int i = 0; i < NT; ++i)
        if (i < terms) {
            mine[(int64_t)i * n_baselines * 2] = re[i];
            mine[(int64_t)i * n_baselines * 2 + 1] = im[i];
        }
}

// The first stage.  weight(rec, t_obs): the emitter's unclamped intensity through one stored hit.  A unit is a time,
// term = time of the batch x planes + plane.
template <int NT, typename Weight>
__device__ __forceinline__ void visibility_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                   int max_images, const VisibilityGrid &vg, double t_start, double dt,
                                                   const double *__restrict__ uv, double *__restrict__ partial, Weight weight)
{
    const int first = vg.first + (int)blockIdx.y * vg.units;             // this batch's first time
    const int times = min(vg.units, vg.n_units - first);                 // (the call's last batch may hold fewer)
    visibility_walk<NT>(n_px, vg.W, vg.n_baselines, uv, partial, vg.units * vg.planes, times * vg.planes, [=](int64_t p, double *sh_w, int t) {
        const float *rec = hits + (p < n_px ? p : 0) * max_images * 4;
        const int ns = p < n_px ? stored_slots(rec, n_hits, p, max_images) : 0;
        bool has = false;
        for (int tt = 0; tt < times; ++tt) {
            const double t_obs = spectrum_time(t_start, dt, first + tt);
            double sum = 0.0;
            for (int j = 0; j < max_images; ++j) {
                double w = 0.0;
                if (j < ns && rec[j * 4 + 2] == rec[j * 4 + 2]) w = weight(rec + j * 4, t_obs); // (a slot whose g is NaN is skipped)
                if (vg.planes > 1) {
                    sh_w[(tt * vg.planes + j) * 256 + t] = w;
                    has |= !(w == 0.0); // (a NaN weight is kept: it is the emitter's answer)
                } else if (j < ns) {
                    sum += w;
                }
            }
            if (vg.planes == 1) {
                sh_w[tt * 256 + t] = sum;
                has |= !(sum == 0.0);
            }
        }
        return has;
    });
}

// The three emitters (the disk has one row and no time).
template <int NT>
__global__ void __launch_bounds__(256) k_disk_visibility_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                                 int max_images, DiskShade ds, VisibilityGrid vg, const double *__restrict__ uv,
                                                                 double *__restrict__ partial)
{
    visibility_partial<NT>(hits, n_hits, n_px, max_images, vg, 0.0, 0.0, uv, partial,
                           [&](const float *rec, double) { return disk_intensity(ds, ds.r_in / (double)rec[0], (double)rec[2]); });
}

template <int NT>
__global__ void __launch_bounds__(256) k_hotspot_visibility_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                    int64_t n_px, int max_images, HotspotShade hs, VisibilityGrid vg,
                                                                    double t_start, double dt, const double *__restrict__ uv,
                                                                    double *__restrict__ partial)
{
    visibility_partial<NT>(hits, n_hits, n_px, max_images, vg, t_start, dt, uv, partial,
                           [&](const float *rec, double t_obs) { return hotspot_intensity(hs, t_obs, rec); });
}

template <int NT>
__global__ void __launch_bounds__(256) k_diskmap_visibility_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                    int64_t n_px, int max_images, DiskMapShade dm,
                                                                    const float *__restrict__ texels, VisibilityGrid vg, double t_start,
                                                                    double dt, const double *__restrict__ uv, double *__restrict__ partial)
{
    visibility_partial<NT>(hits, n_hits, n_px, max_images, vg, t_start, dt, uv, partial,
                           [&](const float *rec, double t_obs) { return diskmap_intensity(dm, texels, t_obs, rec); });
}

} // namespace lt
