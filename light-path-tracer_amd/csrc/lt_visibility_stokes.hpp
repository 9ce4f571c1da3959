// lt_visibility_stokes.hpp -- polarized visibilities of the stored hits (include/ltrace.h, "polarized visibilities"): per
// observer time, plane, Stokes parameter (I, Q, U) and baseline the sum of w exp(-2 pi i (u ix + v iy)) over the stored
// slots, w_I the weight lt_*_visibility adds and w_Q, w_U = ((Pi sz sz) q) w_I, ((Pi sz sz) u) w_I from the records of
// lt_trace_disk_pol.  A second phase one for visibility_walk (lt_visibility.hpp), whose phase two, LDS layout, lists, chunk
// order, block count and final stage (k_sum_blocks) it calls: the phases depend on (pixel, baseline) alone, so I, Q and U
// of a hit are three terms of one batch and share the one sincospi.
//
// Batches.  (time, plane) is flattened into a pair index k = time x planes + plane over the whole call; a batch is a run of
// up to VIS_STOKES_BATCH_PAIRS = 5 consecutive pairs, term = pair of the batch x 3 + stokes: 15 of VIS_BATCH_TERMS.  A
// batch may begin and end in the middle of a time.  With the Stokes index innermost a batch's output rows are contiguous
// in (n_times, planes, 3, n_baselines, 2), which is what k_sum_blocks writes.  NP, the pairs a work-item keeps
// accumulators for (1, 2, 3 or 5; 6 NP doubles), is the call's pair count where that is below 5.
//
// Phase one evaluates w_I once per (pair's time, slot) with the unpolarized kernel's lambda and derives w_Q and w_U from it
// as rounded products.  The I terms are the unpolarized kernel's numbers added in its order, so the I plane has its bits:
// a pixel that is kept here and not there (or the other way round) has weights of exactly 0 in the I terms, and
// fma(0, c, re) = re.
//
// Shared, not restated: everything but phase one is visibility_walk, the one text both families compile, so the guarantees
// above hold by construction (profiles/visibility_fold_check.txt has the fold's check against the restated sibling).
#pragma once
#include "lt_polarization.hpp"
#include "lt_visibility.hpp"

namespace lt {

constexpr int VIS_STOKES_BATCH_PAIRS = 5; // LT_VISIBILITY_STOKES_BATCH_PAIRS
static_assert(VIS_STOKES_BATCH_PAIRS * 3 <= VIS_BATCH_TERMS, "a batch of pairs lives within the unpolarized batch's terms");

// (w_I, w_Q, w_U) of one slot that is not skipped, in stokes_weight's order: ((Pi sz) sz) q) w_I, every product rounded.
// The empty asm keeps the products from being fused into the sum over a pixel's slots (-ffp-contract=fast, see
// visibility_phase), and w_I's last product with them.
__device__ __forceinline__ void visibility_stokes_weights(double pol_frac, const float *prec, double w_i, double *w)
{
    asm("" : "+v"(w_i));
    const double pw = stokes_weight(pol_frac, prec);
    double w_q = pw * (double)prec[0] * w_i, w_u = pw * (double)prec[1] * w_i;
    asm("" : "+v"(w_q), "+v"(w_u));
    w[0] = w_i; w[1] = w_q; w[2] = w_u;
}

// The first stage.  weight(rec, t_obs): the emitter's unclamped intensity through one stored hit, as visibility_partial's.
// A unit of the grid is a (time, plane) pair, term = pair of the batch x 3 + stokes.
template <int NP, typename Weight>
__device__ __forceinline__ void visibility_stokes_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                          const float *__restrict__ pol, int64_t n_px, int max_images,
                                                          const VisibilityGrid &vg, double pol_frac, double t_start, double dt,
                                                          const double *__restrict__ uv, double *__restrict__ partial, Weight weight)
{
    const int first = vg.first + (int)blockIdx.y * vg.units;             // this batch's first pair
    const int pairs = min(min(vg.units, NP), vg.n_units - first);        // (the call's last batch may hold fewer)
    visibility_walk<3 * NP>(n_px, vg.W, vg.n_baselines, uv, partial, vg.units * 3, pairs * 3, [=](int64_t p, double *sh_w, int t) {
        const float *rec = hits + (p < n_px ? p : 0) * max_images * 4, *prec = pol + (p < n_px ? p : 0) * max_images * 4;
        const int ns = p < n_px ? stored_slots(rec, n_hits, p, max_images) : 0;
        bool has = false;
        for (int i = 0; i < min(pairs, NP); ++i) { // (pairs <= NP already: the bound restated where the compiler sees it, 2 % at NP = 1)
            const int k = first + i, tt = k / vg.planes, plane = k - tt * vg.planes;
            const double t_obs = spectrum_time(t_start, dt, tt);
            double sum[3] = {0.0, 0.0, 0.0};
            if (vg.planes > 1) {
                if (plane < ns && rec[plane * 4 + 2] == rec[plane * 4 + 2])   // (a slot whose g is NaN is skipped)
                    visibility_stokes_weights(pol_frac, prec + plane * 4, weight(rec + plane * 4, t_obs), sum);
            } else {
                for (int j = 0; j < ns; ++j) {
                    double w[3] = {0.0, 0.0, 0.0};
                    if (rec[j * 4 + 2] == rec[j * 4 + 2]) visibility_stokes_weights(pol_frac, prec + j * 4, weight(rec + j * 4, t_obs), w);
                    sum[0] += w[0]; sum[1] += w[1]; sum[2] += w[2];
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                sh_w[(i * 3 + c) * 256 + t] = sum[c];
                has |= !(sum[c] == 0.0); // (a NaN weight is kept: it is the emitter's, or the record's, answer)
            }
        }
        return has;
    });
}

// The two emitters (the disk has one row and no time).
template <int NP>
__global__ void __launch_bounds__(256) k_disk_visibility_stokes_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                        const float *__restrict__ pol, int64_t n_px, int max_images,
                                                                        DiskShade ds, double pol_frac, VisibilityGrid vg,
                                                                        const double *__restrict__ uv, double *__restrict__ partial)
{
    visibility_stokes_partial<NP>(hits, n_hits, pol, n_px, max_images, vg, pol_frac, 0.0, 0.0, uv, partial,
                                  [&](const float *rec, double) { return disk_intensity(ds, ds.r_in / (double)rec[0], (double)rec[2]); });
}

template <int NP>
__global__ void __launch_bounds__(256) k_hotspot_visibility_stokes_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                           const float *__restrict__ pol, int64_t n_px, int max_images,
                                                                           HotspotShade hs, double pol_frac, VisibilityGrid vg,
                                                                           double t_start, double dt, const double *__restrict__ uv,
                                                                           double *__restrict__ partial)
{
    visibility_stokes_partial<NP>(hits, n_hits, pol, n_px, max_images, vg, pol_frac, t_start, dt, uv, partial,
                                  [&](const float *rec, double t_obs) { return hotspot_intensity(hs, t_obs, rec); });
}

} // namespace lt
