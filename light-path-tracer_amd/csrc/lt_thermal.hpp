// lt_thermal.hpp -- the disk's thermal continuum from the stored hits of lt_trace_disk_hits (include/ltrace.h, "thermal
// continuum"): a radial flux table F(r) and a temperature scale make every stored hit a blackbody at T = t_max F^(1/4),
// hardened by f_col and shifted by the hit's g.  Two products: the spectrum, the flux density at up to TH_MAX_FREQS
// frequencies summed over all pixels and slots (k_thermal_spectrum_partial, then k_sum_blocks of lt_spectrum.hpp), and
// the band images, up to TH_MAX_BANDS float32 planes (k_shade_thermal).
//
// A hit's light at frequency nu is nu^3 A / expm1(nu c): A is the call's, c depends on the hit alone (thermal_coeff: the
// header's steps 1 to 4, every operation rounded as stated there), the frequency enters through one product and one expm1.  The
// spectrum is therefore a skinny dense product whose operands are made on the fly, the visibilities' shape with an expm1
// and a division where they have a sincospi, and its walk is theirs (lt_visibility.hpp).
//
// First stage (k_thermal_spectrum_partial<NP>; grid (SP_BLOCKS, 1, passes of 256 frequencies), 256 work-items; NP = 1,
// or DISK_MAX_IMAGES with split_orders: the accumulators a work-item keeps in registers).  A workgroup walks its pixels in
// chunks of 256 in the light curve's stride order.
//   Phase one: work-item i evaluates c of its pixel's stored slots.  Each wavefront lists the slots that emit, in the
//   order lane, slot, packed: the ballots of the slots give every lane the count of the entries before its own, so the
//   list has no holes and needs no scan.  An entry is (c, slot) in the wavefront's segment of LDS.  The slots are
//   unrolled to DISK_MAX_IMAGES so that a lane's c wait in registers for the last ballot.
//   Phase two: work-item k owns frequency pass 256 + k.  It walks the four lists in order; all lanes read the same
//   addresses (broadcasts: conflict-free whatever the layout), take one product, one expm1 and one division per entry and
//   add the quotient to the accumulator of the entry's plane.  The slot is wave-uniform, so picking the accumulator is
//   scalar control flow and the accumulators stay in registers.  A wavefront whose 64 frequencies lie beyond n_freq skips
//   the phase.
// After its last chunk the owner writes nu^3 times its sums: one partial per (block, plane, frequency).
// Final stage (k_sum_blocks with row = planes x n_freq): one work-item per (plane, frequency) adds the SP_BLOCKS partials
// in ascending block order.
//
// Why the passes are a grid dimension: as the visibilities', a pass costs the c of its pixels once more -- two square
// roots and a division per slot -- against 256 expm1 and divisions per entry.
//
// LDS is sized by the launch (thermal_lds_bytes): 4 x 64 max_images entries of 8 + 1 bytes and the four counts, 18 448 B
// at eight images and 6 928 B at three.  DESIGN.md 10m has the registers and what was measured.
#pragma once
#include "lt_visibility.hpp"

namespace lt {

constexpr int TH_MAX_NODES = 65536; // LT_THERMAL_MAX_NODES
constexpr int TH_MAX_FREQS = 1024;  // LT_THERMAL_MAX_FREQS
constexpr int TH_MAX_BANDS = 16;    // LT_THERMAL_MAX_BANDS

extern __shared__ __attribute__((aligned(16))) unsigned char th_lds[];
inline size_t thermal_lds_bytes(int max_images) { return (size_t)4 * 64 * max_images * 9 + 16; }
static_assert((4 * 64 * DISK_MAX_IMAGES * 9 + 16) * 4 <= 160 * 1024, "four workgroups of the longest lists share a CU");

struct ThermalShade {
    double r_min, r_max, inv_dr; // inv_dr = (n_r - 1) / (r_max - r_min), from the host
    double t_max, f_col;
    double amp;                  // A = exposure / ((f_col f_col) (f_col f_col)), from the host
    int n_r;
};

// The header's steps 1 to 4 for one stored slot: whether it emits, and then its c.  Every operation is rounded as the
// header states it: the library is built with -ffp-contract=fast, under which v's product would fuse into the subtraction
// that makes w (the empty asm keeps it a rounded product, as in visibility_phase), the interpolation is an explicit fma,
// and the rest are products, quotients and square roots with nothing to contract.  The index is clamped before it is used,
// whatever r holds.
__device__ __forceinline__ bool thermal_coeff(const ThermalShade &th, const double *__restrict__ flux, const float *rec, double *c)
{
    const double r = (double)rec[0], g = (double)rec[2];
    if (!(g > 0.0) || !(r >= th.r_min) || !(r <= th.r_max)) return false; // (a NaN fails every comparison)
    double v = (r - th.r_min) * th.inv_dr;
    asm("" : "+v"(v));
    const int i0 = max(min((int)floor(v), th.n_r - 2), 0);
    const double w = v - (double)i0;
    const double f0 = flux[i0], f1 = flux[i0 + 1];
    const double F = fma(w, f1 - f0, f0);
    if (!(F > 0.0)) return false;
    const double T = th.t_max * sqrt(sqrt(F));
    *c = 1.0 / ((g * th.f_col) * T);
    return true;
}

// Step 5 without its nu^3: A / expm1(nu c), the product rounded before expm1 sees it (inlined, its first operations could
// otherwise fuse with it).
__device__ __forceinline__ double thermal_term(double nu, double A, double c)
{
    double x = nu * c;
    asm("" : "+v"(x));
    return A / expm1(x);
}

// nu^3 sum with its three products rounded: (nu nu) nu, then the sum's.
__device__ __forceinline__ double thermal_scale(double nu, double sum) { return ((nu * nu) * nu) * sum; }

template <int NP>
__global__ void __launch_bounds__(256) k_thermal_spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                  int64_t n_px, int max_images, ThermalShade th,
                                                                  const double *__restrict__ flux, const double *__restrict__ nu,
                                                                  int n_freq, int planes, double *__restrict__ partial)
{
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    const int seg = 64 * max_images; // entries of one wavefront's segment: at most one per lane and slot
    double *sh_c = (double *)th_lds;
    uint8_t *sh_j = (uint8_t *)(sh_c + 4 * seg);
    int *sh_cnt = (int *)(sh_j + 4 * seg);
    const int k = (int)blockIdx.z * 256 + t;
    const bool owner = k < n_freq;
    const bool wave_owns = (int)blockIdx.z * 256 + wave * 64 < n_freq;
    const double my_nu = owner ? nu[k] : 1.0;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    double acc[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) acc[i] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_px; base += (int64_t)256 * SP_BLOCKS) {
        // phase one: this wavefront's list of the slots that emit, in the order lane, slot
        const int64_t p = base + t;
        const float *rec = hits + (p < n_px ? p : 0) * max_images * 4;
        const int ns = p < n_px ? stored_slots(rec, n_hits, p, max_images) : 0;
        double pc[DISK_MAX_IMAGES];
        int before = 0, mine = 0; // entries of the lanes below this one, and this lane's emitting slots
#pragma unroll
        for (int j = 0; j < DISK_MAX_IMAGES; ++j) {
            const bool emits = j < ns && thermal_coeff(th, flux, rec + j * 4, &pc[j]);
            if (emits) mine |= 1 << j;
            before += __popcll(__ballot(emits) & below);
        }
        const int total = __shfl(before + __popc(mine), 63);
        int at = wave * seg + before;
#pragma unroll
        for (int j = 0; j < DISK_MAX_IMAGES; ++j)
            if (mine >> j & 1) {
                sh_c[at] = pc[j];
                sh_j[at] = (uint8_t)j;
                ++at;
            }
        if (lane == 0) sh_cnt[wave] = total;
        __syncthreads();
        // phase two: one expm1 and one division per entry and owned frequency
        if (wave_owns) {
            for (int s = 0; s < 4; ++s) {
                const int n = __builtin_amdgcn_readfirstlane(sh_cnt[s]);
                for (int e = s * seg; e < s * seg + n; ++e) {
                    const double q = thermal_term(my_nu, th.amp, sh_c[e]);
                    if (NP == 1) {
                        acc[0] += q;
                    } else {
                        const int j = __builtin_amdgcn_readfirstlane((int)sh_j[e]);
#pragma unroll
                        for (int i = 0; i < NP; ++i)
                            if (j == i) acc[i] += q;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!owner) return;
    double *out = partial + (int64_t)blockIdx.x * planes * n_freq + k;
#pragma unroll
    for (int i = 0; i < NP; ++i)
        if (i < planes) out[(int64_t)i * n_freq] = thermal_scale(my_nu, acc[i]);
}

// The band images: one pixel per work-item, c of its slots once, then per band the slots' quotients added in slot
// order in float64, scaled by nu^3 and rounded once to float32.  out: (n_bands, n_px), plane-major.
__global__ void __launch_bounds__(256) k_shade_thermal(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                       int max_images, ThermalShade th, const double *__restrict__ flux,
                                                       const double *__restrict__ nu, int n_bands, float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    const float *rec = hits + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    double c[DISK_MAX_IMAGES];
    int emits = 0;
#pragma unroll
    for (int j = 0; j < DISK_MAX_IMAGES; ++j)
        if (j < ns && thermal_coeff(th, flux, rec + j * 4, &c[j])) emits |= 1 << j;
    for (int b = 0; b < n_bands; ++b) {
        const double f = nu[b];
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < DISK_MAX_IMAGES; ++j)
            if (emits >> j & 1) sum += thermal_term(f, th.amp, c[j]);
        out[(int64_t)b * n_px + p] = (float)thermal_scale(f, sum);
    }
}

} // namespace lt
