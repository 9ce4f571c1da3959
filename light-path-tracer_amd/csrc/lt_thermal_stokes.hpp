// lt_thermal_stokes.hpp -- the thermal continuum of a scattering atmosphere (include/ltrace.h, "polarized thermal
// continuum"): lt_thermal.hpp's two products with a weight per stored slot and Stokes parameter.  The records of
// lt_trace_disk_pol for the field (0, 0, 1) hold the electric vector's (q, u) along k^ x e_(z) and mu = |k^ . e_(z)|; two
// tables on mu, the limb-darkening factor h and the polarization degree delta, make a slot's light
// (w_I, w_Q, w_U) A / expm1(nu c) with w_I = h, w_Q = (h delta) q, w_U = (h delta) u (atmosphere_weights: the header's
// steps 6 and 7, every operation rounded as stated there).  c, A, the term and the nu^3 are lt_thermal.hpp's functions,
// called and not restated; its kernels are not touched.
//
// First stage (k_thermal_spectrum_stokes_partial<NP>; grid (SP_BLOCKS, 1, passes of 256 frequencies), 256 work-items; NP
// = 1, or DISK_MAX_IMAGES with split_orders: a work-item keeps 3 NP accumulators).  The walk is
// k_thermal_spectrum_partial's: chunks of 256 pixels in the light curve's stride order, phase one lists the emitting
// slots per wavefront in the order lane, slot by ballots, phase two gives every work-item one frequency and walks the
// lists by broadcast reads.  What differs:
//   Phase one: a slot emits only if its mu lies in [0, 1] as well; the lanes keep c of their slots through the ballots,
//   as there, and evaluate the three weights while they write their entries, so no weight waits in a register.  An entry
//   is (c, w_I, w_Q, w_U, slot), 33 bytes, as five arrays.
//   Phase two: per entry one product, one expm1 and one division as there, then three explicit fmas, S = fma(w, t, S),
//   into the accumulators of the entry's plane, reached by a scalar branch on the wave-uniform slot (the unpolarized kernel
//   selects among eight additions; three times as many selects cost more than the branch).  With h = 1 the first fma is
//   S + t, the unpolarized kernel's addition.
// After its last chunk the owner writes nu^3 times its sums: one partial per (block, plane, Stokes, frequency).
// Final stage (k_sum_blocks with row = planes x 3 x n_freq).
//
// LDS, the decision.  At 33 bytes an entry, the four lists of a chunk take 4 x 64 max_images x 33 + 16 bytes: 25 360 B at
// three images, 33 808 B at four and 67 600 B at eight, which would leave two workgroups to a CU's 160 KiB where the
// unpolarized kernel has four -- and lie above the 64 KiB a launch may ask for without further ado.  Phase two is bound
// by float64 issue with long dependent chains (expm1, the division), which is what more resident wavefronts hide, so
// the occupancy is kept: above THS_WHOLE_IMAGES = 4 images a chunk's lists are walked in two halves, wavefronts 0 and 1,
// then 2 and 3, through two segments (33 808 B at eight images again).  Every wavefront still evaluates its phase one
// once per chunk, before the first half; a half costs two more barriers per chunk.  The order of addition is the header's
// in either case -- chunk, wavefront, lane, slot -- because the halves are taken in wavefront order.  Up to four images,
// the shipped frames' three among them, the walk is lt_thermal.hpp's with one pair of barriers per chunk.  DESIGN.md 10o
// has the registers (95 VGPRs at NP = 1; 128 at NP = 8, where the launch bound holds them to four wavefronts per SIMD, which
// is four workgroups per CU, at the price of five spilled) and what was measured.
#pragma once
#include "lt_thermal.hpp"

namespace lt {

constexpr int ATM_MAX_NODES = 4096;  // LT_ATMOSPHERE_MAX_NODES
constexpr int THS_WHOLE_IMAGES = 4;  // up to this many images a chunk's four lists are in LDS at once, above it two at a time

// The lists (one per wavefront) that are in LDS at once, and the launch's LDS: that many segments of 64 max_images entries
// of 4 x 8 + 1 bytes, and four counts.
__host__ __device__ inline int thermal_stokes_lists(int max_images) { return max_images > THS_WHOLE_IMAGES ? 2 : 4; }
inline size_t thermal_stokes_lds_bytes(int max_images) { return (size_t)thermal_stokes_lists(max_images) * 64 * max_images * 33 + 16; }
static_assert((4 * 64 * THS_WHOLE_IMAGES * 33 + 16) * 4 <= 160 * 1024 && (2 * 64 * DISK_MAX_IMAGES * 33 + 16) * 4 <= 160 * 1024,
              "four workgroups of the longest lists share a CU, walked whole or in halves");

struct AtmosphereShade {
    const double *limb, *poldeg; // n_mu nodes each, node i at mu = i / (n_mu - 1)
    int n_mu;
};

// The first half of the header's step 6: whether the slot's mu lets it emit (a NaN fails both comparisons).
__device__ __forceinline__ bool atmosphere_emits(const float *prec)
{
    const double mu = (double)prec[3];
    return mu >= 0.0 && mu <= 1.0;
}

// The header's steps 6 and 7 for a slot that emits: (w_I, w_Q, w_U) = (h, (h d) q, (h d) u).  As in thermal_coeff, v is
// kept a rounded product before the subtraction that makes the interpolation weight, the interpolations are explicit
// fmas, and h d, its products with q and u and h itself are rounded before phase two's fmas see them (the empty asm, as in
// visibility_stokes_weights: the library is built with -ffp-contract=fast).  The index is clamped before it is used.
__device__ __forceinline__ void atmosphere_weights(const AtmosphereShade &at, const float *prec, double *w)
{
    double v = (double)prec[3] * (double)(at.n_mu - 1);
    asm("" : "+v"(v));
    const int i0 = max(min((int)floor(v), at.n_mu - 2), 0);
    const double wt = v - (double)i0;
    const double l0 = at.limb[i0], l1 = at.limb[i0 + 1], p0 = at.poldeg[i0], p1 = at.poldeg[i0 + 1];
    double h = fma(wt, l1 - l0, l0);
    const double d = fma(wt, p1 - p0, p0);
    double hd = h * d;
    asm("" : "+v"(h), "+v"(hd));
    double w_q = hd * (double)prec[0], w_u = hd * (double)prec[1];
    asm("" : "+v"(w_q), "+v"(w_u));
    w[0] = h; w[1] = w_q; w[2] = w_u;
}

// (__launch_bounds__' second argument holds the registers to four wavefronts per SIMD, 128 VGPRs: four workgroups per CU.)
template <int NP>
__global__ void __launch_bounds__(256, 4) k_thermal_spectrum_stokes_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                            const float *__restrict__ pol, int64_t n_px, int max_images,
                                                                            ThermalShade th, const double *__restrict__ flux,
                                                                            AtmosphereShade at, const double *__restrict__ nu, int n_freq,
                                                                            int planes, double *__restrict__ partial)
{
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    const int seg = 64 * max_images;                     // entries of one wavefront's segment: at most one per lane and slot
    const int lists = thermal_stokes_lists(max_images);  // segments in LDS: the lists walked between two barriers
    double *sh_c = (double *)th_lds, *sh_w = sh_c + lists * seg; // c, then w_I, w_Q, w_U: lists x seg doubles each
    uint8_t *sh_j = (uint8_t *)(sh_c + 4 * lists * seg);
    int *sh_cnt = (int *)(sh_j + lists * seg);
    const int k = (int)blockIdx.z * 256 + t;
    const bool owner = k < n_freq;
    const bool wave_owns = (int)blockIdx.z * 256 + wave * 64 < n_freq;
    const double my_nu = owner ? nu[k] : 1.0;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    static_assert(NP <= DISK_MAX_IMAGES && DISK_MAX_IMAGES == 8, "phase two names the eight planes");
    double acc[3 * NP];
#pragma unroll
    for (int i = 0; i < 3 * NP; ++i) acc[i] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_px; base += (int64_t)256 * SP_BLOCKS) {
        // phase one: which of this pixel's slots emit, their c, and where the lane's entries begin in its wavefront's list
        const int64_t p = base + t;
        const float *rec = hits + (p < n_px ? p : 0) * max_images * 4, *prec = pol + (p < n_px ? p : 0) * max_images * 4;
        const int ns = p < n_px ? stored_slots(rec, n_hits, p, max_images) : 0;
        double pc[DISK_MAX_IMAGES];
        int before = 0, mine = 0;
#pragma unroll
        for (int j = 0; j < DISK_MAX_IMAGES; ++j) {
            const bool emits = j < ns && atmosphere_emits(prec + j * 4) && thermal_coeff(th, flux, rec + j * 4, &pc[j]);
            if (emits) mine |= 1 << j;
            before += __popcll(__ballot(emits) & below);
        }
        const int total = __shfl(before + __popc(mine), 63);
        for (int first = 0; first < 4; first += lists) { // the wavefronts first ... first + lists - 1 list, then all walk
            if (wave >= first && wave < first + lists) {
                int e = (wave - first) * seg + before;
#pragma unroll
                for (int j = 0; j < DISK_MAX_IMAGES; ++j)
                    if (mine >> j & 1) {
                        double w[3];
                        atmosphere_weights(at, prec + j * 4, w);
                        sh_c[e] = pc[j];
                        sh_w[e] = w[0];
                        sh_w[lists * seg + e] = w[1];
                        sh_w[2 * lists * seg + e] = w[2];
                        sh_j[e] = (uint8_t)j;
                        ++e;
                    }
                if (lane == 0) sh_cnt[wave - first] = total;
            }
            __syncthreads();
            // phase two: one expm1, one division and three fmas per entry and owned frequency
            if (wave_owns) {
                for (int s = 0; s < lists; ++s) {
                    const int n = __builtin_amdgcn_readfirstlane(sh_cnt[s]);
                    for (int e = s * seg; e < s * seg + n; ++e) {
                        const double q = thermal_term(my_nu, th.amp, sh_c[e]);
                        const double w_i = sh_w[e], w_q = sh_w[lists * seg + e], w_u = sh_w[2 * lists * seg + e];
                        const auto add = [&](int i) {
                            acc[3 * i] = fma(w_i, q, acc[3 * i]);
                            acc[3 * i + 1] = fma(w_q, q, acc[3 * i + 1]);
                            acc[3 * i + 2] = fma(w_u, q, acc[3 * i + 2]);
                        };
                        if (NP == 1) {
                            add(0);
                        } else {
                            // The slot is wave-uniform, so this is a scalar branch to the plane's three fmas.  The empty
                            // volatile asm keeps it one: left alone, the compiler converts eight guarded updates into 24
                            // fmas and as many selects per entry.
                            const int j = __builtin_amdgcn_readfirstlane((int)sh_j[e]);
#define LT_THS_PLANE(i) case i: if (i < NP) { asm volatile(""); add(i); } break;
                            switch (j) { LT_THS_PLANE(0) LT_THS_PLANE(1) LT_THS_PLANE(2) LT_THS_PLANE(3)
                                         LT_THS_PLANE(4) LT_THS_PLANE(5) LT_THS_PLANE(6) LT_THS_PLANE(7) }
#undef LT_THS_PLANE
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
    if (!owner) return;
    double *out = partial + (int64_t)blockIdx.x * planes * 3 * n_freq + k;
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (i < planes) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out[(int64_t)(i * 3 + c) * n_freq] = thermal_scale(my_nu, acc[3 * i + c]);
        }
}

// The band images: one pixel per work-item, c and the weights of its slots once, then per band the slots' terms added in
// slot order in float64 by the same fmas, scaled by nu^3 and rounded once to float32.  out: (n_bands, 3, n_px).
__global__ void __launch_bounds__(256) k_shade_thermal_stokes(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                              const float *__restrict__ pol, int64_t n_px, int max_images, ThermalShade th,
                                                              const double *__restrict__ flux, AtmosphereShade at,
                                                              const double *__restrict__ nu, int n_bands, float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    const float *rec = hits + p * max_images * 4, *prec = pol + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    double c[DISK_MAX_IMAGES], w[DISK_MAX_IMAGES][3];
    int emits = 0;
#pragma unroll
    for (int j = 0; j < DISK_MAX_IMAGES; ++j)
        if (j < ns && atmosphere_emits(prec + j * 4) && thermal_coeff(th, flux, rec + j * 4, &c[j])) {
            atmosphere_weights(at, prec + j * 4, w[j]);
            emits |= 1 << j;
        }
    for (int b = 0; b < n_bands; ++b) {
        const double f = nu[b];
        double sum[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < DISK_MAX_IMAGES; ++j)
            if (emits >> j & 1) {
                const double q = thermal_term(f, th.amp, c[j]);
                sum[0] = fma(w[j][0], q, sum[0]);
                sum[1] = fma(w[j][1], q, sum[1]);
                sum[2] = fma(w[j][2], q, sum[2]);
            }
#pragma unroll
        for (int s = 0; s < 3; ++s) out[((int64_t)b * 3 + s) * n_px + p] = (float)thermal_scale(f, sum[s]);
    }
}

} // namespace lt
