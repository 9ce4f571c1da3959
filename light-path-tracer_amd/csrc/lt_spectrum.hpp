// lt_spectrum.hpp -- line profiles and dynamic spectra binned from the stored hits of lt_trace_disk_hits
// (include/ltrace.h, "energy-resolved light"): per observer time a histogram of float64 weights over the keys
// (image order, bin of g), for the stationary disk, the hot spot and the disk map.  The light curve's evaluation with a
// reduction to up to SP_MAX_KEYS numbers in place of three, in a fixed order and without floating-point atomics.
//
// First stage (spectrum_partial over histogram_walk, the walk lt_transfer.hpp shares; grid (SP_BLOCKS, times of this
// batch), 256 work-items).  A workgroup walks its pixels in chunks of 256 in the light curve's stride order.  Phase one: every work-item evaluates (key, weight) of its pixel's
// stored slots; slot by slot its wavefront adds the non-zero weights of every key the slot holds with a butterfly over the
// lanes (absent lanes add +0.0: a bracketing fixed by the lane indices) and appends one entry (key, sum) per key to the
// wavefront's segment of LDS.  The 64 neighbouring pixels of a row share a few bins, so this leaves a few entries where
// there were up to 64; an entry per hit made phase two, one dependent read-modify-write per entry in the owner's
// wavefront, twenty times the evaluation.  Phase two: the accumulators live in LDS as well, work-item i
// alone owns the keys = i (mod 256); every work-item scans the four segments in order -- all lanes read the same entry,
// a broadcast -- and adds the entries it owns, an unshared read-modify-write.  After the last chunk the workgroup
// writes its accumulators as one partial.
// Final stage (k_sum_blocks): one work-item per key adds a time's SP_BLOCKS partials in ascending block order.
//
// LDS is sized by the launch (spectrum_lds_bytes): at most 4112 x 8 (accumulators) + 2048 x (8 + 4) (entries) + 16 =
// 57 488 B per workgroup, so two workgroups share a CU's 160 KiB even then; the default grid with three images takes
// 10 016 B and the registers bound the occupancy.  The scan reads four keys per ds_read_b128.
#pragma once
#include "lt_diskmap.hpp"

namespace lt {

constexpr int SP_BLOCKS = 256;                                // LT_SPECTRUM_BLOCKS
constexpr int SP_MAX_BINS = 512;                              // LT_SPECTRUM_MAX_BINS
constexpr int SP_MAX_KEYS = (SP_MAX_BINS + 2) * DISK_MAX_IMAGES; // 4112

// The first stage's LDS, sized by the launch: accumulators (n_keys doubles, an even count so that the keys below stay
// 16-byte aligned) | the entries' sums (4 x 64 max_images doubles) | their keys (as many int) | the four segments' counts.
extern __shared__ __attribute__((aligned(16))) unsigned char sp_lds[];
inline size_t spectrum_lds_bytes(int n_keys, int max_images)
{
    return (size_t)((n_keys + 1) & ~1) * 8 + (size_t)4 * 64 * max_images * 12 + 16;
}
static_assert((SP_MAX_KEYS * 8 + 4 * 64 * DISK_MAX_IMAGES * 12 + 16) * 2 <= 160 * 1024, "two workgroups of the largest grid share a CU");

struct SpectrumGrid {
    double g_min, g_max, inv_dg; // inv_dg = n_bins / (g_max - g_min), from the host
    int n_bins, planes;          // planes: 1, or max_images with split_orders
};

// Column of the stored float32 g: 0 the underflow, n_bins + 1 the overflow, else the half-open bin.  A subtraction and
// then a multiplication: nothing to contract.  The result is in [0, n_bins + 1] whatever g holds (a NaN never gets here).
__device__ __forceinline__ int spectrum_bin(const SpectrumGrid &sg, float g32)
{
    const double x = (double)g32;
    if (x < sg.g_min) return 0;
    if (x >= sg.g_max) return sg.n_bins + 1;
    const int k = (int)floor((x - sg.g_min) * sg.inv_dg);
    return 1 + max(min(k, sg.n_bins - 1), 0);
}

// t_start + i dt with the product rounded before the sum, so that a row's time does not depend on how an expression
// around it was contracted: the time computed alone on the host (t_start + i * dt in float64) is this one.
__device__ __forceinline__ double spectrum_time(double t_start, double dt, int i)
{
#pragma clang fp contract(off)
    const double step = dt * (double)i;
    return t_start + step;
}

// The sum of v over the 64 lanes of a wavefront, in every lane: the butterfly over lane ^ 32, ^ 16, ... ^ 1, a bracketing
// fixed by the lane indices (both partners add the same two numbers, so all lanes hold the same bits).
__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The first stage of a keyed histogram, for the spectra below and the transfer function (lt_transfer.hpp): the LDS carve-up,
// the chunks in stride order, both phases and the write of the partial.  The workgroup keeps n_acc accumulators, for the keys
// first ... first + n_acc - 1.  slot(rec, j, &key, &w) gives the key and the weight of stored slot j of a pixel, and leaves w
// as it is, 0.0, where the slot does not contribute.  mine_at(&n_out) gives where this workgroup's partial starts and how
// many of the accumulators it writes there; it is asked after the last chunk.  Tiled: other workgroups own other keys.
// Both callables are shaped by measurement (profiles/histogram_fold_check.txt): a flag returned by slot and tested here cost
// every kernel a compare and a select per slot, and the partial's address computed before the walk moved the loops by one
// instruction and made the spectra of 4096 x 4096 records 0.4 to 0.8 % slower; as they are, the four spectrum kernels
// have the registers, spills and code sizes of the bodies this walk replaced.  The lambdas capture by value, which
// compiles here as capturing by reference does.
// A slot contributes unless its weight is exactly 0 (a NaN weight is kept: it is the emitter's answer).  A key of another
// tile is another workgroup's and an absent lane here, not an entry dropped after its butterfly: the butterfly for a key
// adds the weights of the lanes that hold this key and +0.0 for every other lane, whatever those lanes hold, so the merge
// of a key is complete -- all of a wavefront's lanes with that key in one butterfly, in the one workgroup that owns the
// key -- and its entries reach the owner in the order (wavefront, slot) in every tiling.  What must not happen is a key
// merged in parts (two entries of one wavefront and slot for one key): the sum of the parts brackets differently.  The
// loop takes the leader's key and removes every lane with that key from `todo`.
template <bool Tiled, typename Slot, typename Mine>
__device__ __forceinline__ void histogram_walk(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                               int max_images, int n_acc, int first, Slot slot, Mine mine_at)
{
    const int t = (int)threadIdx.x, wave = t >> 6, lane = t & 63;
    const int seg = 64 * max_images; // entries of one wavefront's segment: at most one per lane and slot
    double *sh_acc = (double *)sp_lds, *sh_w = sh_acc + ((n_acc + 1) & ~1);
    int *sh_key = (int *)(sh_w + 4 * seg), *sh_cnt = sh_key + 4 * seg;
    for (int k = t; k < n_acc; k += 256) sh_acc[k] = 0.0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n_px; base += (int64_t)256 * SP_BLOCKS) {
        // phase one: this wavefront's entries (key - first, sum), slot by slot, one per key
        const int64_t p = base + t;
        const float *rec = hits + (p < n_px ? p : 0) * max_images * 4;
        const int ns = p < n_px ? stored_slots(rec, n_hits, p, max_images) : 0;
        int cnt = 0;
        for (int j = 0; j < max_images; ++j) {
            double w = 0.0;
            int key = first;
            if (j < ns) slot(rec + j * 4, j, &key, &w);
            key -= first;
            const bool has = !(w == 0.0) && (!Tiled || (key >= 0 && key < n_acc));
            // one entry per key this slot holds in this wavefront: the neighbouring pixels of a row share a few bins
            for (uint64_t todo = __ballot(has); todo;) {
                const int leader = __ffsll((unsigned long long)todo) - 1;
                const int k = __shfl(key, leader);
                const bool same = has && key == k;
                const double sum = wave_sum(same ? w : 0.0);
                if (lane == leader) {
                    sh_key[wave * seg + cnt] = k;
                    sh_w[wave * seg + cnt] = sum;
                }
                ++cnt;
                todo &= ~__ballot(same);
            }
        }
        if (lane == 0) sh_cnt[wave] = cnt;
        __syncthreads();
        // phase two: the owner of a key adds its entries in order
        for (int s = 0; s < 4; ++s) {
            const int n = sh_cnt[s];
            const int *kk = sh_key + s * seg;
            const double *ww = sh_w + s * seg;
            for (int e = 0; e < n; e += 4) {
                const int4 k4 = *(const int4 *)(kk + e);
                if ((k4.x & 255) == t) sh_acc[k4.x] += ww[e]; // (e < n)
                if (e + 1 < n && (k4.y & 255) == t) sh_acc[k4.y] += ww[e + 1];
                if (e + 2 < n && (k4.z & 255) == t) sh_acc[k4.z] += ww[e + 2];
                if (e + 3 < n && (k4.w & 255) == t) sh_acc[k4.w] += ww[e + 3];
            }
        }
        __syncthreads();
    }
    __syncthreads(); // (a workgroup without a chunk: the zeroes above)
    int n_out;
    double *mine = mine_at(&n_out);
    for (int k = t; k < n_out; k += 256) mine[k] = sh_acc[k];
}

// The spectra's first stage: one workgroup keeps every key.  weight(rec): the emitter's unclamped intensity through one
// stored hit.  partial: this batch's (time, block, key) sums.
template <typename Weight>
__device__ __forceinline__ void spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                 int max_images, const SpectrumGrid &sg, double *__restrict__ partial, Weight weight)
{
    const int cols = sg.n_bins + 2;
    const int n_keys = min(cols * sg.planes, SP_MAX_KEYS);
    histogram_walk<false>(hits, n_hits, n_px, max_images, n_keys, 0,
                          [=](const float *rec, int j, int *key, double *w) {
        const float g32 = rec[2];
        if (!(g32 == g32)) return; // (a NaN g has no bin)
        *w = weight(rec);
        *key = min((sg.planes > 1 ? j * cols : 0) + spectrum_bin(sg, g32), n_keys - 1);
    }, [=](int *n_out) { *n_out = n_keys; return partial + ((int64_t)blockIdx.y * SP_BLOCKS + blockIdx.x) * n_keys; });
}

// The three emitters.  first: the index of this batch's first time (the disk has one row and no time).
__global__ void __launch_bounds__(256) k_disk_spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits, int64_t n_px,
                                                               int max_images, DiskShade ds, SpectrumGrid sg, double *__restrict__ partial)
{
    spectrum_partial(hits, n_hits, n_px, max_images, sg, partial,
                     [&](const float *rec) { return disk_intensity(ds, ds.r_in / (double)rec[0], (double)rec[2]); });
}

__global__ void __launch_bounds__(256) k_hotspot_spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                  int64_t n_px, int max_images, HotspotShade hs, SpectrumGrid sg,
                                                                  double t_start, double dt, int first, double *__restrict__ partial)
{
    const double t_obs = spectrum_time(t_start, dt, first + (int)blockIdx.y);
    spectrum_partial(hits, n_hits, n_px, max_images, sg, partial, [&](const float *rec) { return hotspot_intensity(hs, t_obs, rec); });
}

__global__ void __launch_bounds__(256) k_diskmap_spectrum_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                  int64_t n_px, int max_images, DiskMapShade dm,
                                                                  const float *__restrict__ texels, SpectrumGrid sg, double t_start,
                                                                  double dt, int first, double *__restrict__ partial)
{
    const double t_obs = spectrum_time(t_start, dt, first + (int)blockIdx.y);
    spectrum_partial(hits, n_hits, n_px, max_images, sg, partial, [&](const float *rec) { return diskmap_intensity(dm, texels, t_obs, rec); });
}

// The final stage of the two-stage reductions whose partials are (batch, block, row): the spectra's (a batch is a time, row
// = n_keys) and the visibilities' (lt_visibility.hpp; VIS_BLOCKS == SP_BLOCKS is asserted there).  grid (ceil(row / 256),
// batches of this launch); n_rows: the doubles this launch writes in all (its last batch may hold less than a row).  out: the
// first row of this launch.  One work-item per double adds its SP_BLOCKS partials in ascending block order.
__global__ void __launch_bounds__(256) k_sum_blocks(const double *__restrict__ partial, int row, int64_t n_rows, double *__restrict__ out)
{
    const int k = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int64_t at = (int64_t)blockIdx.y * row + k;
    if (k >= row || at >= n_rows) return;
    const double *p = partial + (int64_t)blockIdx.y * SP_BLOCKS * row + k;
    double sum = 0.0;
    for (int b = 0; b < SP_BLOCKS; ++b) sum += p[(int64_t)b * row];
    out[at] = sum;
}

} // namespace lt
