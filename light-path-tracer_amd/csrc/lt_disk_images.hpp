// lt_disk_images.hpp -- the optically thin disk of lt_render_disk_images (include/ltrace.h): the integrate kernel that
// records every crossing of the annulus and lets the ray go on, and its epilogues.  K1 is the frame path's prologue.
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

// Where the lane's hits go: img[j * n_q + q] for slot j < max_images.  Wave-uniform but for q.
template <typename T> struct DiskRecords {
    typename Vec2<T>::type *img;
    int64_t n_q;
    int max_images;
};

// disk_advance with the crossing recorded instead of taking the ray's place.  `rec`: this lane writes records (false
// on a ghost lane: a bitwise twin of the lead ray, whose hits are the lead's own).  `n`: the lane's hit count.
template <typename T, typename Integ>
__device__ __forceinline__ int disk_advance_images(const KerrConsts<T> &k, const DiskConsts<T> &d, const RayConsts<T> &rc,
                                                   T vmax2, typename Integ::State &s, const DiskRecords<T> &out,
                                                   int64_t q, bool rec, uint32_t &n)
{
    const T HALF_PI = T(1.5707963267948966);
    const typename Integ::State before = s;
    const int ev = Integ::advance(k, rc, s);
    const T z0 = before.y.th - HALF_PI, z1 = s.y.th - HALF_PI;
    const bool cross = ((z0 < T(0)) & (z1 >= T(0))) | ((z0 > T(0)) & (z1 <= T(0)));
    const T pad = DiskStepLen<Integ>::bound(rc, before) * vmax2;
    const bool near = (M<T>::min(before.y.r, s.y.r) <= d.r_out + pad) & (M<T>::max(before.y.r, s.y.r) >= d.r_in - pad);
    const bool cand = cross & near;
    if (__builtin_expect(wave_any(cand), 0)) {
        if (cand) {
            // (as disk_advance: a step that ends the ray by capture / escape is searched up to where the ray ended)
            const T h = DiskStepLen<Integ>::h(k, rc, before);
            State5<T> y1 = s.y, hit;
            T t_end = T(1);
            if (ev == EV_CAPTURED || ev == EV_ESCAPED) {
                y1 = kerr_rk4_step(k, rc, before.y, h);
                const T target = ev == EV_CAPTURED ? k.r_capture : k.r_escape;
                const T denom = y1.r - before.y.r;
                t_end = denom == T(0) ? T(1) : M<T>::min(M<T>::max((target - before.y.r) / denom, T(0)), T(1));
            }
            if (disk_crossing(k, d, rc, before.y, y1, h, t_end, hit) & rec) {
                if (n < (uint32_t)out.max_images) {
                    typename Vec2<T>::type v;
                    v.x = hit.r; v.y = hit.ph;
                    out.img[(int64_t)n * out.n_q + q] = v;
                }
                ++n;
            }
        }
    }
    return ev;
}

// k_kerr_disk with disk_advance_images: the same tile queue, streak gate (its proof is per step: it never needed the
// ray to stop) and ghost-lane phase.  hits[q]: the ray's hit count, stored with its final record.
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
    KerrConsts<T> k = k_in;
    pin_consts(k);
    const DiskRecords<T> out{img, n_q, max_images};
    const int lane = (int)(threadIdx.x & 63u);
    int64_t tile = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (;;) {
    if (head) {
        unsigned long long w = 0;
        if (lane == 0) w = atomicAdd(head, 1ull);
        tile = (int64_t)(((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(w >> 32)) << 32) |
                         (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)w));
    }
    const int64_t q = tile * 64 + lane;
    if (q >= n_q) return;
    WaveMeter meter;
    meter.begin(kstats, tile);
    typename Vec4<T>::type rec = ic[q];
    int flags = (int)rec.w;
    typename Integ::State st;
    st.y.r = k.r_obs; st.y.th = k.theta_obs; st.y.ph = T(0); st.y.pr = rec.x; st.y.pth = rec.y;
    st.steps = 0;
    int ev = (flags & FLAG_PAD) ? EV_PAD : EV_INVALID;
    uint32_t wave_iters = 0, n = 0;
    bool raised = false;
    RayConsts<T> rc = make_ray_consts(k, rec.z, (flags & FLAG_REFINE) != 0);
    T vmax2 = T(2) * disk_vmax(k, d, rc);
    KerrConsts<T> kg = k; // the streak's constants: rc4 raised to the gate radius
    kg.rc4 = M<T>::max(k.rc4, M<T>::fma(T(2) * rc.hb, vmax2, d.r_out));
    if (flags & FLAG_OK) {
        Integ::start(k, rc, st, rec.x, rec.y);
        uint32_t it = 0;
        do {
            it += Integ::streak(kg, rc, st, 64u);
            ev = disk_advance_images<T, Integ>(k, d, rc, vmax2, st, out, q, true, n);
            ++it;
            if (Integ::GHOST_LANES) {
                if (it >= long_iters) break;
            } else if (it >= long_iters && !raised) {
                __builtin_amdgcn_s_setprio(3);
                raised = true;
            }
        } while (ev == EV_RUNNING);
        wave_iters = it;
    }
    uint32_t steps = st.steps;
    bool real = ev == EV_RUNNING;
    if (Integ::GHOST_LANES && wave_any(real)) {
        __builtin_amdgcn_s_setprio(3);
        raised = true;
        if (!real) {
            store_fin<T>(fin0, fin1, q, st.y.r, st.y.th, st.y.ph, st.y.pr, st.y.pth, rec.z, ev, steps);
            hits[q] = n;
        }
        uint32_t lead = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(real));
        uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)wave_iters, (int)lead);
        bool sync = true;
        for (;;) {
            if (sync) {
                lead = (uint32_t)__builtin_ctzll(__builtin_amdgcn_ballot_w64(real));
                take_from_lane(st, lead, !real);
                take_from_lane(rc, lead, !real);
                vmax2 = T(2) * disk_vmax(k, d, rc);
                kg.rc4 = M<T>::max(k.rc4, M<T>::fma(T(2) * rc.hb, vmax2, d.r_out));
                sync = false;
            }
            it += Integ::streak_lone(kg, rc, st, 64u);
            // only a real lane records: a ghost's hits are its lead's, written by the lead
            int e = disk_advance_images<T, Integ>(k, d, rc, vmax2, st, out, q, real, n);
            ++it;
            if (wave_any(e != EV_RUNNING)) {
                if (real & (e != EV_RUNNING)) {
                    steps = st.steps;
                    store_fin<T>(fin0, fin1, q, st.y.r, st.y.th, st.y.ph, st.y.pr, st.y.pth, rec.z, e, steps);
                    hits[q] = n;
                    real = false;
                }
                if (!wave_any(real)) break;
                sync = true;
            }
        }
        wave_iters = it;
    } else {
        store_fin<T>(fin0, fin1, q, st.y.r, st.y.th, st.y.ph, st.y.pr, st.y.pth, rec.z, ev, steps);
        hits[q] = n;
    }
    meter.end(kstats, wave_iters);
    if (!head) return;
    if (__builtin_amdgcn_ballot_w64(raised)) __builtin_amdgcn_s_setprio(0);
    }
}

// ---- K3 ---------------------------------------------------------------------------------------------------------------
// Light of one stored hit, unclamped: E = exposure g^4 (r_in / r)^q ramp(s), s = g (r_in / r)^(3/4), float64 from the
// float32 (r, g) the caller gets -- disk_shade's arithmetic without its clamp to [0, 1].
__device__ __forceinline__ void disk_emission(const DiskShade &ds, float r32, float g32, double *e)
{
    const double r = (double)r32, g = (double)g32;
    const double x = ds.r_in / r, g2 = g * g;
    const double I = ds.exposure * (g2 * g2) * pow(x, ds.q);
    const double s = g * pow(x, 0.75);
    for (int i = 0; i < 3; ++i) e[i] = I * fmin(fmax(2.0 * s - 0.5 * i, 0.0), 1.0);
}

// Counters of the images epilogue: the frame path's six, the rays with at least one hit (word 6) and all hits
// (word 7) of the workgroup's partial set; k_stats_reduce_disk_images moves them to LT_STAT_DISK / LT_STAT_DISK_HITS.
__device__ __forceinline__ void flush_stats_disk_images(uint64_t *stats, const StatAcc &a, uint32_t hits, const MetricConsts &m)
{
    if (!stats) return;
    __shared__ unsigned long long sh[8];
    if (threadIdx.x < 8) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t st = a.counted ? a.steps : 0u, nh = a.counted ? hits : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        st += __shfl_xor(st, off, 64);
        nh += __shfl_xor(nh, off, 64);
    }
    const unsigned long long rays = (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(a.counted));
    const unsigned long long v[8] = {rays, st, rays * (unsigned long long)m.evals_fixed + (unsigned long long)st * (unsigned long long)m.evals_per_step,
                                     (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(a.esc)),
                                     (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(a.cap)),
                                     (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(a.inv)),
                                     (unsigned long long)__popcll(__builtin_amdgcn_ballot_w64(a.counted && hits > 0)),
                                     (unsigned long long)nh};
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < 8; ++i) if (v[i]) atomicAdd(&sh[i], v[i]);
    __syncthreads();
    unsigned long long *set = (unsigned long long *)stats + (size_t)((blockIdx.x + blockIdx.y * gridDim.x) % STAT_SLOTS) * 8;
    if (threadIdx.x < 8 && sh[threadIdx.x]) atomicAdd(&set[threadIdx.x], sh[threadIdx.x]);
}

#ifndef LT_KERNEL_TEMPLATES_ONLY
// k_stats_reduce with word 6 going to LT_STAT_DISK and word 7 to LT_STAT_DISK_HITS
__global__ void __launch_bounds__(STAT_SLOTS) k_stats_reduce_disk_images(unsigned long long *__restrict__ partials,
                                                                         unsigned long long *__restrict__ stats)
{
    unsigned long long *set = partials + (size_t)threadIdx.x * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        unsigned long long v = wave_sum(set[i]);
        set[i] = 0;
        const int dst = i < 6 ? i : (i == 6 ? 12 : 13);
        if (threadIdx.x == 0 && v) atomicAdd(&stats[dst], v);
    }
}
#endif

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
        if (o.rgba) {
            uchar4 px;
            px.x = (uint8_t)(rgb[0] * 255.0f);
            px.y = (uint8_t)(rgb[nch == 1 ? 0 : 1] * 255.0f);
            px.z = (uint8_t)(rgb[nch == 1 ? 0 : 2] * 255.0f);
            px.w = 255;
            reinterpret_cast<uchar4 *>(o.rgba)[p] = px;
        }
    }
    flush_stats_disk_images(o.stats, acc, nh, m);
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
