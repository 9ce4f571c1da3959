// lt_hit_time.hpp -- coordinate time along a ray and the timed trace of lt_trace_disk_hits (include/ltrace.h, "hit
// times"): the quadrature of dt/dlambda over the accepted steps (step_time), the hooks into the shared tile loop that
// carry it (DiskTimedStep; direct_tiles, lt_kernels.hpp), the kernel k_kerr_disk_timed, its epilogues and the probe of
// the step rule.
//
// Time does not feed back into the ray's state: the timed trace takes the steps of k_kerr_disk_images and looks at the
// two ends of each.  With E = 1, L = p_phi:
//   dt/dlambda = [ (r^2 + a^2) P / Delta + a (L - a sin^2 theta) ] / Sigma,   P = r^2 + a^2 - a L.
// An accepted step y0 -> y1 of length h adds h/6 (t'(y0) + 4 t'(y_m) + t'(y1)), y_m the step's cubic Hermite in (r, theta)
// at 1/2, built from r' = Delta p_r / Sigma and theta' = p_theta / Sigma at both ends: Simpson on the interpolant, local
// error O(h^5) like the RK4 step itself.  A hit at the fraction tau of a step applies the same rule to [0, tau], with
// the cubic's states at tau / 2 and tau.
#pragma once
#include "lt_disk_images.hpp"

namespace lt {

// dt/dlambda, dr/dlambda and dtheta/dlambda at one state (outside the horizon: Sigma, Delta > 0).  t = tx * ts: the two
// factors travel with it for the one place that adds t' to a sum (step_time), which writes that multiply-add as the fma it is
// to be.  Left to -ffp-contract=fast, the compiler fused the product into the sum in one kernel and not in another: the step
// rule of k_step_time_probe and that of the timed kernels differed in the last bit on 2 % of whole steps
// (tests/test_gpu_hit_blocks.py).  A lane carries t, r, th alone: the factors are dead once the step that made them is added.
template <typename T> struct TimeRates { T t, r, th, tx, ts; };

template <typename T> __device__ __forceinline__ void time_rate_parts(const KerrConsts<T> &k, const RayConsts<T> &rc, T r, T th, T &tx, T &iS, T &Delta)
{
    T s, c;
    M<T>::sincos(th, s, c);
    const T s2 = s * s;
    const T ra = M<T>::fma(r, r, k.a2);
    const T Sigma = M<T>::fma(-k.a2, s2, ra);
    Delta = M<T>::fma(-k.two_M, r, ra);
    const T inv = M<T>::rcp_pos(Sigma * Delta);
    iS = Delta * inv;
    const T P = M<T>::fma(r, r, rc.c_P);
    tx = M<T>::fma(ra * P, Sigma * inv, k.a * M<T>::fma(-k.a, s2, rc.L));
}
template <typename T> __device__ __forceinline__ TimeRates<T> time_rates(const KerrConsts<T> &k, const RayConsts<T> &rc, const State5<T> &y)
{
    T Delta;
    TimeRates<T> o;
    time_rate_parts(k, rc, y.r, y.th, o.tx, o.ts, Delta);
    o.t = o.tx * o.ts;
    o.r = Delta * y.pr * o.ts;
    o.th = y.pth * o.ts;
    return o;
}

// The rule on [0, tau] of the step y0 -> y1 of length h (d0, d1: the rates at its ends).  tau = 1: the whole step.
template <typename T>
__device__ __forceinline__ T step_time(const KerrConsts<T> &k, const RayConsts<T> &rc, const State5<T> &y0, const TimeRates<T> &d0,
                                       const State5<T> &y1, const TimeRates<T> &d1, T h, T tau)
{
    const T hr0 = h * d0.r, hr1 = h * d1.r, hth0 = h * d0.th, hth1 = h * d1.th;
    T Delta, xm, sm, xe = d1.tx, se = d1.ts;
    const T tm = T(0.5) * tau;
    time_rate_parts(k, rc, hermite(y0.r, hr0, y1.r, hr1, tm), hermite(y0.th, hth0, y1.th, hth1, tm), xm, sm, Delta);
    if (tau != T(1)) time_rate_parts(k, rc, hermite(y0.r, hr0, y1.r, hr1, tau), hermite(y0.th, hth0, y1.th, hth1, tau), xe, se, Delta);
    // d0.t + 4 t'(mid) + t'(end), the start's rate as the lane carries it (rounded), the other two fused into the sum.  The
    // result is rounded HERE (fma with +0: the product, and no bare product for the caller's next add to absorb -- the stored
    // time t_hi + (t_lo + part) took `part` unrounded into its inner add, one stored time in ~250 a last bit off that sequence)
    return M<T>::fma((tau * h) * T(1.0 / 6.0), M<T>::fma(xe, se, M<T>::fma(T(4) * xm, sm, d0.t)), T(0));
}

// The thin disk's hooks (DiskImagesStep) plus the elapsed coordinate time of the lane's ray: a compensated (two-term)
// sum, so that float32 keeps the ~1000 M of a ray's travel time to better than its steps' own error.  Every step has to
// show both of its ends, so the far-field streak -- up to 64 steps inside one call -- is off: streak_consts hands it an
// infinite rc4, its entry test fails and every step goes through advance().  The streak's steps are the general
// iteration's arithmetic (lt_device.hpp), so the states, the hits and every counter but LT_STAT_WAVE_ITERS and
// LT_STAT_EQ_ITERS are those of k_kerr_disk_images, bit for bit.  tim[n * n_q + q]: the time of hit n, next to img.
// A ghost lane's sum is meaningless (its state is resynchronised, its sum is not) and is never stored.
template <typename T, typename Integ> struct DiskTimedStep : DiskImagesStep<T, Integ> {
    T *tim;
    struct Lane : DiskImagesStep<T, Integ>::Lane {
        T t_hi, t_lo;    // elapsed time from the camera, t_hi + t_lo
        TimeRates<T> rate; // the rates at the current state: a step's end values are the next step's start values
        bool have;       // rate is set
    };
    __device__ __forceinline__ void begin_tile(Lane &l, const KerrConsts<T> &k)
    {
        DiskImagesStep<T, Integ>::begin_tile(l, k);
        l.kg.rc4 = __builtin_inf();
        l.t_hi = l.t_lo = T(0);
        l.have = false;
    }
    __device__ __forceinline__ void bind(Lane &l, const KerrConsts<T> &k, const RayConsts<T> &rc) { l.vmax2 = T(2) * disk_vmax(k, this->d, rc); }
    __device__ __forceinline__ int advance(Lane &l, const KerrConsts<T> &k, const RayConsts<T> &rc, typename Integ::State &st, int64_t q, bool real)
    {
        const State5<T> y0 = st.y;
        const T lam0 = st.lam;
        const T h_try = DiskStepLen<Integ>::h(k, rc, st);
        if (!l.have) { l.rate = time_rates(k, rc, y0); l.have = true; }
        const TimeRates<T> d0 = l.rate;
        DiskHitStep<T> on;
        const int ev = disk_advance<T, Integ>(k, this->d, rc, l.vmax2, st, real, [&](typename Integ::State &, const State5<T> &hit, int e) {
            if (l.n < (uint32_t)this->max_images) {
                typename Vec2<T>::type v;
                v.x = hit.r; v.y = hit.ph;
                this->img[(int64_t)l.n * this->n_q + q] = v;
                const T part = step_time(k, rc, y0, d0, on.y1, time_rates(k, rc, on.y1), on.h, on.tau);
                tim[(int64_t)l.n * this->n_q + q] = l.t_hi + (l.t_lo + part);
            }
            ++l.n;
            return e;
        }, &on);
        // an attempt that was rejected, retried or ended the ray leaves lambda where it was and adds nothing
        const T h = st.lam != lam0 ? h_try : T(0);
        l.rate = time_rates(k, rc, st.y);
        const T dt = h != T(0) ? step_time(k, rc, y0, d0, st.y, l.rate, h, T(1)) : T(0);
        const T sum = l.t_hi + dt, bb = sum - l.t_hi;
        l.t_lo += (l.t_hi - (sum - bb)) + (dt - bb);
        l.t_hi = sum;
        return ev;
    }
};

template <typename T, typename Integ>
__global__ void __launch_bounds__(256, Integ::MIN_WAVES_PER_SIMD) k_kerr_disk_timed(KerrConsts<T> k_in, DiskConsts<T> d,
                                                       const typename Vec4<T>::type *__restrict__ ic,
                                                       typename Vec4<T>::type *__restrict__ fin0,
                                                       typename Vec4<T>::type *__restrict__ fin1, int64_t n_q,
                                                       uint32_t long_iters, uint64_t *__restrict__ kstats,
                                                       unsigned long long *__restrict__ head,
                                                       typename Vec2<T>::type *__restrict__ img, uint32_t *__restrict__ hits,
                                                       int max_images, T *__restrict__ tim)
{
    DiskTimedStep<T, Integ> step;
    step.d = d;
    step.img = img; step.hits = hits; step.n_q = n_q; step.max_images = max_images; step.tim = tim;
    direct_tiles<T, Integ>(k_in, step, ic, fin0, fin1, n_q, long_iters, nullptr, kstats, head);
}

// ---- K3 ---------------------------------------------------------------------------------------------------------------
// The hit records of one ray as the callers get them: slot j -> (r_hit, phi_hit in [0, 2 pi), g, elapsed time), NaN in
// an unused slot.  Out is float (frames) or double (the batch twin).
template <typename T, typename Out>
__device__ __forceinline__ void store_hits(const DiskShade &ds, const typename Vec2<T>::type *__restrict__ img, const T *__restrict__ tim,
                                           int64_t n_q, int max_images, int64_t q, uint32_t nh, double xi, Out *__restrict__ dst)
{
    for (int j = 0; j < max_images; ++j) {
        Out v4[4];
        v4[0] = v4[1] = v4[2] = v4[3] = (Out)__builtin_nan("");
        if ((uint32_t)j < nh) {
            const typename Vec2<T>::type v = img[(int64_t)j * n_q + q];
            v4[0] = (Out)v.x;
            v4[1] = (Out)wrap_2pi((double)v.y);
            v4[2] = (Out)disk_redshift(ds.M, ds.a, (double)v.x, xi);
            v4[3] = (Out)tim[(int64_t)j * n_q + q];
        }
        for (int i = 0; i < 4; ++i) dst[j * 4 + i] = v4[i];
    }
}

// Epilogue of lt_trace_disk_hits_dev: k_epilogue_disk_images without the colour; hits (R, W, max_images, 4) float32.
template <typename T>
__global__ void __launch_bounds__(EPILOGUE_BLOCK) k_epilogue_disk_hits(CamConsts c, MetricConsts m, DiskShade ds,
                                                                       const typename Vec4<T>::type *__restrict__ fin0,
                                                                       const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                                       DiskImagesOut di, const T *__restrict__ tim)
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
        const long long wl = res.n_half < 0 ? 0 : (res.n_half > 65535 ? 65535 : res.n_half);
        if (o.fa) o.fa[p] = (res.status == 1) ? (float)res.fa : __builtin_nanf("");
        if (o.w) o.w[p] = (uint16_t)wl;
        if (o.status) o.status[p] = (int8_t)res.status;
        if (o.steps) o.steps[p] = res.steps;
        if (di.n_hits) di.n_hits[p] = (uint8_t)(nh > 255u ? 255u : nh);
        if (di.images)
            store_hits<T, float>(ds, (const typename Vec2<T>::type *)di.img, tim, di.n_q, di.max_images, q, nh, (double)fin1[q].y,
                                 di.images + p * di.max_images * 4);
    }
    flush_stats<8>(o.stats, acc, m, nh > 0, nh);
}

// Epilogue of lt_trace_batch_kerr_disk_hits: k_epilogue_arrays_disk_images with out_hits (n, max_images, 4) float64.
template <typename T>
__global__ void __launch_bounds__(256) k_epilogue_arrays_disk_hits(MetricConsts m, DiskShade ds,
                                                                   const typename Vec4<T>::type *__restrict__ fin0,
                                                                   const typename Vec4<T>::type *__restrict__ fin1, int64_t n,
                                                                   double *__restrict__ out_fa, int64_t *__restrict__ out_w,
                                                                   int8_t *__restrict__ out_status, uint32_t *__restrict__ out_evals,
                                                                   const typename Vec2<T>::type *__restrict__ img,
                                                                   const uint32_t *__restrict__ hits, int64_t n_q, int max_images,
                                                                   const T *__restrict__ tim, double *__restrict__ out_hits,
                                                                   int32_t *__restrict__ out_n_hits)
{
    int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    RayResult res;
    load_result<T>(m, fin0, fin1, q, res);
    out_fa[q] = (res.status == 1) ? res.fa : __builtin_nan("");
    out_w[q] = res.n_half;
    if (out_status) out_status[q] = (int8_t)res.status;
    if (out_evals) out_evals[q] = res.evals;
    const uint32_t nh = hits[q];
    if (out_n_hits) out_n_hits[q] = (int32_t)nh;
    if (out_hits) store_hits<T, double>(ds, img, tim, n_q, max_images, q, nh, (double)fin1[q].y, out_hits + q * max_images * 4);
}

// lt_step_time_probe: the rule above on n steps given by their ends (r, theta, p_r, p_theta), each with its own p_phi.
template <typename T>
__global__ void k_step_time_probe(KerrConsts<T> k, const double *__restrict__ p_phi, const double *__restrict__ y0,
                                  const double *__restrict__ y1, const double *__restrict__ h, const double *__restrict__ tau,
                                  int64_t n, double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RayConsts<T> rc = make_ray_consts(k, (T)p_phi[i], false);
    State5<T> a, b;
    a.r = (T)y0[i * 4]; a.th = (T)y0[i * 4 + 1]; a.ph = T(0); a.pr = (T)y0[i * 4 + 2]; a.pth = (T)y0[i * 4 + 3];
    b.r = (T)y1[i * 4]; b.th = (T)y1[i * 4 + 1]; b.ph = T(0); b.pr = (T)y1[i * 4 + 2]; b.pth = (T)y1[i * 4 + 3];
    out[i] = (double)step_time(k, rc, a, time_rates(k, rc, a), b, time_rates(k, rc, b), (T)h[i], (T)tau[i]);
}

// lt_time_rates_probe: time_rates on n states (r, theta, p_r, p_theta) -- what a lane carries from one step to the next.
template <typename T>
__global__ void k_time_rates_probe(KerrConsts<T> k, const double *__restrict__ p_phi, const double *__restrict__ y, int64_t n,
                                   double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    RayConsts<T> rc = make_ray_consts(k, (T)p_phi[i], false);
    State5<T> a;
    a.r = (T)y[i * 4]; a.th = (T)y[i * 4 + 1]; a.ph = T(0); a.pr = (T)y[i * 4 + 2]; a.pth = (T)y[i * 4 + 3];
    const TimeRates<T> d = time_rates(k, rc, a);
    out[i * 3] = (double)d.t; out[i * 3 + 1] = (double)d.r; out[i * 3 + 2] = (double)d.th;
}

} // namespace lt
