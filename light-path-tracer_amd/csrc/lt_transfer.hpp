// lt_transfer.hpp -- the disk's reverberation response from the stored hits of lt_trace_disk_hits (include/ltrace.h,
// "reverberation"): a histogram of float64 weights over the keys (image order, bin of the delay tau, bin of g), the
// 2-D transfer function of a flash above the disk.  The spectra's reduction (lt_spectrum.hpp) over a key space eight
// times the one spectrum_partial keeps in LDS: up to TR_MAX_KEYS = 32 768 keys against SP_MAX_KEYS = 4 112.
//
// First stage (k_disk_transfer_partial; grid (SP_BLOCKS, key tiles), 256 work-items).  Tile T owns the keys
// [TR_TILE T, TR_TILE (T + 1)).  A workgroup evaluates the header's steps 1 to 5 for every stored slot of its chunks -- a
// table interpolation and four products, repeated once per tile -- and hands the slot's key and weight to the spectra's
// walk (histogram_walk of lt_spectrum.hpp), which keeps the slots whose key lies in the tile, runs its two phases on them
// and writes the accumulators into the workgroup's partial, at the tile's place.
// Final stage: k_sum_blocks of lt_spectrum.hpp as it is, row = the keys of the call.
//
// Why a key's bits do not depend on the tiling: a slot's keys outside the tile are absent lanes of the walk's butterfly, as
// they are for every other key of the slot inside the tile, and a key is merged whole in the one workgroup that owns it
// (the walk's comment has the argument).
//
// LDS is sized by the launch (transfer_lds_bytes): TR_TILE x 8 (accumulators) + 4 x 64 max_images x (8 + 4) (entries)
// + 16 = 57 360 B at eight images, 42 000 B at three: two workgroups share a CU's 160 KiB at eight images, three at
// three.  The entries' keys start 16-byte aligned (TR_TILE x 8 and 4 x 64 max_images x 8 are multiples of 16) and every
// segment is 256 max_images bytes long.  The two tables are read through __restrict__ global pointers: at most
// 65 536 x 16 B, they stay in L2.
#pragma once
#include "lt_spectrum.hpp"
#include "lt_thermal.hpp"

namespace lt {

constexpr int TR_MAX_TAU = 1024;   // LT_TRANSFER_MAX_TAU
constexpr int TR_MAX_KEYS = 32768; // LT_TRANSFER_MAX_KEYS
constexpr int TR_TILE = 4096;      // keys one workgroup accumulates

inline size_t transfer_lds_bytes(int max_images) { return (size_t)TR_TILE * 8 + (size_t)4 * 64 * max_images * 12 + 16; }
static_assert((TR_TILE * 8 + 4 * 64 * DISK_MAX_IMAGES * 12 + 16) * 2 <= 160 * 1024, "two workgroups share a CU at eight images");
static_assert(TR_TILE % 256 == 0 && TR_MAX_KEYS % TR_TILE == 0, "an owner's keys are those = its index (mod 256) in every tile");

struct TransferShade {
    double tau_min, tau_max, inv_dtau; // inv_dtau = n_tau / (tau_max - tau_min), from the host
    double r_min, r_max, inv_dr;       // inv_dr = (n_r - 1) / (r_max - r_min), from the host
    double t_ref, exposure;
    int n_tau, n_r;
};

// Step 4's delay, (t_ld + dt) - t_ref: two rounded operations (t_ld comes from an explicit fma, which nothing here may
// absorb).
__device__ __forceinline__ double transfer_delay(double t_ld, double dt, double t_ref)
{
#pragma clang fp contract(off)
    const double arrival = t_ld + dt;
    return arrival - t_ref;
}

// Column of a delay: 0 the underflow, n_tau + 1 the overflow, else the half-open bin; spectrum_bin's rule on the delay
// grid.  A subtraction and then a multiplication: nothing to contract.  tau is not NaN here.
__device__ __forceinline__ int transfer_bin(const TransferShade &tr, double tau)
{
    if (tau < tr.tau_min) return 0;
    if (tau >= tr.tau_max) return tr.n_tau + 1;
    const int k = (int)floor((tau - tr.tau_min) * tr.inv_dtau);
    return 1 + max(min(k, tr.n_tau - 1), 0);
}

// The header's steps 1 to 5 for one stored slot: whether it contributes, and then its columns and its weight.  Every
// operation is rounded as the header states it: v's product is kept from fusing into the subtraction that makes w (the
// empty asm, as in thermal_coeff), the interpolations are explicit fmas, the weight is products alone.  The index is
// clamped before it is used, whatever r holds.
__device__ __forceinline__ bool transfer_slot(const TransferShade &tr, const SpectrumGrid &sg, const double *__restrict__ delay,
                                              const double *__restrict__ emis, const float *rec, int *k_tau, int *k_g, double *weight)
{
    const double r = (double)rec[0], g = (double)rec[2], dt = (double)rec[3];
    if (!(g > 0.0) || dt != dt || !(r >= tr.r_min) || !(r <= tr.r_max)) return false; // (a NaN fails every comparison)
    double v = (r - tr.r_min) * tr.inv_dr;
    asm("" : "+v"(v));
    const int i0 = max(min((int)v, tr.n_r - 2), 0);
    const double w = v - (double)i0;
    const double e0 = emis[i0], e1 = emis[i0 + 1];
    const double eps = fma(w, e1 - e0, e0);
    if (!(eps > 0.0)) return false;
    const double d0 = delay[i0], d1 = delay[i0 + 1];
    const double tau = transfer_delay(fma(w, d1 - d0, d0), dt, tr.t_ref);
    if (tau != tau) return false;
    *k_tau = transfer_bin(tr, tau);
    *k_g = spectrum_bin(sg, rec[2]);
    const double g2 = g * g;
    *weight = tr.exposure * (g2 * g2) * eps; // (exposure ((g g) (g g))) eps: disk_intensity's bracketing
    return true;
}

__global__ void __launch_bounds__(256) k_disk_transfer_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                               int max_images, TransferShade tr, SpectrumGrid sg,
                                                               const double *__restrict__ delay, const double *__restrict__ emis,
                                                               int n_keys, double *__restrict__ partial)
{
    const int cols = sg.n_bins + 2, rows = tr.n_tau + 2;
    const int first = (int)blockIdx.y * TR_TILE; // this tile's keys: first ... first + TR_TILE - 1
    histogram_walk<true>(hits, n_hits, n_px, max_images, TR_TILE, first,
                         [=](const float *rec, int j, int *key, double *w) {
        int k_tau, k_g;
        if (transfer_slot(tr, sg, delay, emis, rec, &k_tau, &k_g, w)) // (which leaves w alone where it returns false)
            *key = min(((sg.planes > 1 ? j * rows : 0) + k_tau) * cols + k_g, n_keys - 1);
    }, [=](int *n_out) { *n_out = min(TR_TILE, n_keys - first); return partial + (int64_t)blockIdx.x * n_keys + first; });
}

} // namespace lt
