// lt_polarization.hpp -- linear polarization of the thin disk's images (include/ltrace.h, "linear polarization"): the
// hooks that keep a hit's momenta (DiskPolStep), the kernel k_kerr_disk_pol, the float64 transport of the electric vector
// from the hit to the camera by the Walker-Penrose constant (pol_camera, pol_record), the epilogues that write it, the
// probe of the rule, and the Stokes siblings of the hot spot's kernels (k_shade_stokes, k_lightcurve_stokes_partial).
//
// No ODE is added: kappa = (A - i B)(r - i a cos theta) of (k, f) is conserved along a null geodesic of Kerr, so f at
// the camera follows from the state at the hit and the state at the camera in closed form.  The trace is the timed
// trace's (lt_hit_time.hpp) with one more record per stored hit, (p_r, p_theta), next to (r, phi) and the time.
#pragma once
#include "lt_hit_time.hpp"
#include "lt_hotspot.hpp"

namespace lt {

// ---- K2 ---------------------------------------------------------------------------------------------------------------
// DiskTimedStep plus mom[n * n_q + q] = (p_r, p_theta) of hit n, slot-major like img and tim and stored where they are:
// by a real lane only, below max_images.  advance() is DiskTimedStep's, statement by statement, with that one store added
// (a hook inside DiskTimedStep::advance would have changed k_kerr_disk_timed's code: tools/kernel_diff.sh).
template <typename T, typename Integ> struct DiskPolStep : DiskTimedStep<T, Integ> {
    typename Vec2<T>::type *mom;
    using Lane = typename DiskTimedStep<T, Integ>::Lane;
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
                const int64_t slot = (int64_t)l.n * this->n_q + q;
                typename Vec2<T>::type v, p;
                v.x = hit.r; v.y = hit.ph;
                p.x = hit.pr; p.y = hit.pth;
                this->img[slot] = v;
                mom[slot] = p;
                const T part = step_time(k, rc, y0, d0, on.y1, time_rates(k, rc, on.y1), on.h, on.tau);
                this->tim[slot] = l.t_hi + (l.t_lo + part);
            }
            ++l.n;
            return e;
        }, &on);
        const T h = st.lam != lam0 ? h_try : T(0);
        l.rate = time_rates(k, rc, st.y);
        const T dt = h != T(0) ? step_time(k, rc, y0, d0, st.y, l.rate, h, T(1)) : T(0);
        const T sum = l.t_hi + dt, bb = sum - l.t_hi;
        l.t_lo += (l.t_hi - (sum - bb)) + (dt - bb);
        l.t_hi = sum;
        return ev;
    }
};

// (A kernel of its own, as k_kerr_disk_timed is: every other kernel keeps its code and name.)
template <typename T, typename Integ>
__global__ void __launch_bounds__(256, Integ::MIN_WAVES_PER_SIMD) k_kerr_disk_pol(KerrConsts<T> k_in, DiskConsts<T> d,
                                                       const typename Vec4<T>::type *__restrict__ ic,
                                                       typename Vec4<T>::type *__restrict__ fin0,
                                                       typename Vec4<T>::type *__restrict__ fin1, int64_t n_q,
                                                       uint32_t long_iters, uint64_t *__restrict__ kstats,
                                                       unsigned long long *__restrict__ head,
                                                       typename Vec2<T>::type *__restrict__ img, uint32_t *__restrict__ hits,
                                                       int max_images, T *__restrict__ tim,
                                                       typename Vec2<T>::type *__restrict__ mom)
{
    DiskPolStep<T, Integ> step;
    step.d = d;
    step.img = img; step.hits = hits; step.n_q = n_q; step.max_images = max_images; step.tim = tim; step.mom = mom;
    direct_tiles<T, Integ>(k_in, step, ic, fin0, fin1, n_q, long_iters, nullptr, kstats, head);
}

// ---- the rule, float64 ----------------------------------------------------------------------------------------------------
// disk.polarization (Python) states it.  Every multiply-add is written as the fma it is to be, and no product is left beside
// an add: under -ffp-contract=fast the compiler otherwise decides per kernel which of them to fuse, and the epilogues and the
// probe, which evaluate this on the same record, differed in the last bits of (q, u) on most records
// (tests/test_gpu_hit_blocks.py; disk_redshift, lt_disk.hpp, had the same).  Now they agree in every bit; against numpy the
// rule differs by rounding (tests/test_gpu_polarization.py bounds it by float64's own error on the same records).
#define LT_FMA __builtin_fma
struct PolConsts {
    double M, a;
    double r_obs, s_obs, c_obs; // the static observer: r, sin theta, cos theta
    double b[3];                // unit field on (e_r, e_phi, e_z) of the emitter
};

// Contravariant components of the covector k at (r, theta); s = sin theta, c = cos theta.
__device__ __forceinline__ void pol_raise(double M_, double a, double r, double s, double c, const double *k, double *out)
{
    const double s2 = s * s;
    const double sigma = LT_FMA(r, r, a * a * c * c);
    const double delta = LT_FMA(a, a, LT_FMA(-(2.0 * M_), r, r * r));
    const double sd = sigma * delta;
    const double x = LT_FMA(r, r, a * a);
    const double gtt = -LT_FMA(-(a * a * delta), s2, x * x) / sd;
    const double gtp = -2.0 * M_ * a * r / sd;
    const double gpp = LT_FMA(-(a * a), s2, delta) / (sd * s2);
    out[0] = LT_FMA(gtt, k[0], gtp * k[3]);
    out[1] = delta / sigma * k[1];
    out[2] = k[2] / sigma;
    out[3] = LT_FMA(gtp, k[0], gpp * k[3]);
}

// kappa = (A - i B)(r - i a cos theta) of contravariant k, f: one function for both ends, so that a sign or conjugation
// convention cancels.
__device__ __forceinline__ void walker_penrose(double a, double r, double s, double c, const double *k, const double *f, double &re, double &im)
{
    const double A = LT_FMA(a * s * s, LT_FMA(k[1], f[3], -(k[3] * f[1])), LT_FMA(k[0], f[1], -(k[1] * f[0])));
    const double B = LT_FMA(LT_FMA(r, r, a * a), LT_FMA(k[3], f[2], -(k[2] * f[3])), -(a * LT_FMA(k[0], f[2], -(k[2] * f[0])))) * s;
    re = LT_FMA(A, r, -(B * a * c));
    im = -LT_FMA(A * a, c, B * r);
}

// The camera end of one ray: kappa of the two screen vectors.  North e_2 ~ -e_theta + n^theta n, e_1 = e_2 x n in the
// right-handed static tetrad (r, theta, phi); pr, pth: the backward ray's momenta at the camera (its ic record).
struct PolCamera { double k1re, k1im, k2re, k2im; };
__device__ __forceinline__ PolCamera pol_camera(const PolConsts &pc, double L, double pr, double pth)
{
    const double M_ = pc.M, a = pc.a, r = pc.r_obs, s = pc.s_obs, c = pc.c_obs;
    const double sigma = LT_FMA(r, r, a * a * c * c);
    const double delta = LT_FMA(a, a, LT_FMA(-(2.0 * M_), r, r * r));
    const double g_tt = -(1.0 - 2.0 * M_ * r / sigma);
    const double g_tp = -2.0 * M_ * a * r * s * s / sigma;
    const double g_pp = (LT_FMA(r, r, a * a) + 2.0 * M_ * a * a * r * s * s / sigma) * s * s;
    const double w = -g_tp / g_tt;
    const double n_phi = sqrt(g_pp - g_tp * g_tp / g_tt);
    const double e_r = sqrt(delta / sigma), e_th = 1.0 / sqrt(sigma);
    double n[3] = {-e_r * pr, -e_th * pth, (L - w) / n_phi};
    const double nn = sqrt(LT_FMA(n[2], n[2], LT_FMA(n[1], n[1], n[0] * n[0])));
    for (int i = 0; i < 3; ++i) n[i] = n[i] / nn;
    double e2[3] = {n[1] * n[0], LT_FMA(n[1], n[1], -1.0), n[1] * n[2]};
    const double en = sqrt(LT_FMA(e2[2], e2[2], LT_FMA(e2[1], e2[1], e2[0] * e2[0])));
    for (int i = 0; i < 3; ++i) e2[i] = e2[i] / en;
    const double e1[3] = {LT_FMA(e2[1], n[2], -(e2[2] * n[1])), LT_FMA(e2[2], n[0], -(e2[0] * n[2])), LT_FMA(e2[0], n[1], -(e2[1] * n[0]))};
    const double f1[4] = {e1[2] * w / n_phi, e1[0] * e_r, e1[1] * e_th, e1[2] / n_phi};
    const double f2[4] = {e2[2] * w / n_phi, e2[0] * e_r, e2[1] * e_th, e2[2] / n_phi};
    const double kc[4] = {-1.0, -pr, -pth, L};
    double k[4];
    pol_raise(M_, a, r, s, c, kc, k);
    PolCamera o;
    walker_penrose(a, r, s, c, k, f1, o.k1re, o.k1im);
    walker_penrose(a, r, s, c, k, f2, o.k2re, o.k2im);
    return o;
}

// The record of one hit (r, p_r, p_theta of the backward ray at theta = pi / 2): out = (q, u, sin zeta, mu).
__device__ __forceinline__ void pol_record(const PolConsts &pc, const PolCamera &cam, double L, double r, double pr, double pth, double *out)
{
    const double M_ = pc.M, a = pc.a;
    // the emitter's frame: e_(r) = (0, sqrt(Delta) / r, 0, 0), e_(z) = -d_theta / r, e_(phi) = (ept, 0, 0, epp)
    const double delta = LT_FMA(a, a, LT_FMA(-(2.0 * M_), r, r * r));
    const double g_tt = -(1.0 - 2.0 * M_ / r), g_tp = -2.0 * M_ * a / r, g_pp = LT_FMA(r, r, a * a) + 2.0 * M_ * a * a / r;
    const double sM = sqrt(M_), sr = sqrt(r);
    const double r15 = r * sr;
    const double den = LT_FMA(a, sM, r15);
    const double om = sM / den;
    const double ut = den / (sqrt(r15) * sqrt(LT_FMA(2.0 * a, sM, LT_FMA(-(3.0 * M_), sr, r15))));
    const double u_t = ut * LT_FMA(g_tp, om, g_tt), u_p = ut * LT_FMA(g_pp, om, g_tp);
    const double nrm = sqrt(LT_FMA(g_pp * u_t, u_t, LT_FMA(-(2.0 * g_tp * u_p), u_t, g_tt * u_p * u_p)));
    const double er = sqrt(delta) / r, ept = u_p / nrm, epp = -u_t / nrm;
    // the received photon k = (-1, -p_r, -p_theta, L) on the triad, and f = (k^ x b^) / sin zeta
    double kr = -er * pr, kp = LT_FMA(epp, L, -ept), kz = pth / r;
    const double kn = sqrt(LT_FMA(kz, kz, LT_FMA(kp, kp, kr * kr)));
    kr = kr / kn; kp = kp / kn; kz = kz / kn;
    const double cr = LT_FMA(kp, pc.b[2], -(kz * pc.b[1])), cp = LT_FMA(kz, pc.b[0], -(kr * pc.b[2])), cz = LT_FMA(kr, pc.b[1], -(kp * pc.b[0]));
    const double s2 = LT_FMA(cz, cz, LT_FMA(cp, cp, cr * cr));
    out[3] = fabs(kz);
    if (s2 < 1e-24) { out[0] = out[1] = out[2] = 0.0; return; }
    const double inv = 1.0 / sqrt(s2);
    const double fr = cr * inv, fp = cp * inv, fz = cz * inv;
    const double kc[4] = {-1.0, -pr, -pth, L};
    double k[4];
    pol_raise(M_, a, r, 1.0, 0.0, kc, k);
    const double f[4] = {fp * ept, fr * er, -fz / r, fp * epp};
    double hre, him;
    walker_penrose(a, r, 1.0, 0.0, k, f, hre, him);
    // real (x, y) with x kappa(e_1) + y kappa(e_2) = kappa_hit
    const double det = LT_FMA(cam.k1re, cam.k2im, -(cam.k2re * cam.k1im));
    const double x = LT_FMA(hre, cam.k2im, -(cam.k2re * him)) / det;
    const double y = LT_FMA(cam.k1re, him, -(hre * cam.k1im)) / det;
    const double n2 = LT_FMA(y, y, x * x);
    out[0] = LT_FMA(x, x, -(y * y)) / n2;
    out[1] = 2.0 * x * y / n2;
    out[2] = sqrt(s2);
}

#undef LT_FMA

// ---- K3 ---------------------------------------------------------------------------------------------------------------
// The polarization records of one ray: slot j -> (q, u, sin zeta, mu), NaN in an unused slot.  Out: float or double.
template <typename T, typename Out>
__device__ __forceinline__ void store_pol(const PolConsts &pc, const typename Vec4<T>::type *__restrict__ ic,
                                          const typename Vec2<T>::type *__restrict__ img, const typename Vec2<T>::type *__restrict__ mom,
                                          int64_t n_q, int max_images, int64_t q, uint32_t nh, double L, Out *__restrict__ dst)
{
    PolCamera cam{};
    if (nh > 0) {
        const typename Vec4<T>::type rec = ic[q];
        cam = pol_camera(pc, L, (double)rec.x, (double)rec.y);
    }
    for (int j = 0; j < max_images; ++j) {
        double v4[4];
        v4[0] = v4[1] = v4[2] = v4[3] = __builtin_nan("");
        if ((uint32_t)j < nh) {
            const typename Vec2<T>::type p = mom[(int64_t)j * n_q + q];
            pol_record(pc, cam, L, (double)img[(int64_t)j * n_q + q].x, (double)p.x, (double)p.y, v4);
        }
        for (int i = 0; i < 4; ++i) dst[j * 4 + i] = (Out)v4[i];
    }
}

// Epilogue of lt_trace_disk_pol_dev: k_epilogue_disk_hits plus pol (R, W, max_images, 4) float32.
template <typename T>
__global__ void __launch_bounds__(EPILOGUE_BLOCK) k_epilogue_disk_pol(CamConsts c, MetricConsts m, DiskShade ds, PolConsts pc,
                                                                      const typename Vec4<T>::type *__restrict__ ic,
                                                                      const typename Vec4<T>::type *__restrict__ fin0,
                                                                      const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                                      DiskImagesOut di, const T *__restrict__ tim,
                                                                      const typename Vec2<T>::type *__restrict__ mom, float *__restrict__ pol)
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
        const typename Vec2<T>::type *img = (const typename Vec2<T>::type *)di.img;
        const double xi = (double)fin1[q].y;
        if (di.images) store_hits<T, float>(ds, img, tim, di.n_q, di.max_images, q, nh, xi, di.images + p * di.max_images * 4);
        if (pol) store_pol<T, float>(pc, ic, img, mom, di.n_q, di.max_images, q, nh, xi, pol + p * di.max_images * 4);
    }
    flush_stats<8>(o.stats, acc, m, nh > 0, nh);
}

// Epilogue of lt_trace_batch_kerr_disk_pol: k_epilogue_arrays_disk_hits plus out_pol (n, max_images, 4) float64.
template <typename T>
__global__ void __launch_bounds__(256) k_epilogue_arrays_disk_pol(MetricConsts m, DiskShade ds, PolConsts pc,
                                                                  const typename Vec4<T>::type *__restrict__ ic,
                                                                  const typename Vec4<T>::type *__restrict__ fin0,
                                                                  const typename Vec4<T>::type *__restrict__ fin1, int64_t n,
                                                                  double *__restrict__ out_fa, int64_t *__restrict__ out_w,
                                                                  int8_t *__restrict__ out_status, uint32_t *__restrict__ out_evals,
                                                                  const typename Vec2<T>::type *__restrict__ img,
                                                                  const uint32_t *__restrict__ hits, int64_t n_q, int max_images,
                                                                  const T *__restrict__ tim, const typename Vec2<T>::type *__restrict__ mom,
                                                                  double *__restrict__ out_hits, int32_t *__restrict__ out_n_hits,
                                                                  double *__restrict__ out_pol)
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
    const double xi = (double)fin1[q].y;
    if (out_hits) store_hits<T, double>(ds, img, tim, n_q, max_images, q, nh, xi, out_hits + q * max_images * 4);
    if (out_pol) store_pol<T, double>(pc, ic, img, mom, n_q, max_images, q, nh, xi, out_pol + q * max_images * 4);
}

// lt_polarization_probe: the rule on n records given as hit (r, p_r, p_theta), camera (p_r, p_theta) and L.
__global__ void k_polarization_probe(PolConsts pc, const double *__restrict__ L, const double *__restrict__ hit,
                                     const double *__restrict__ cam, int64_t n, double *__restrict__ out)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PolCamera pcam = pol_camera(pc, L[i], cam[i * 2], cam[i * 2 + 1]);
    double v4[4];
    pol_record(pc, pcam, L[i], hit[i * 3], hit[i * 3 + 1], hit[i * 3 + 2], v4);
    for (int c = 0; c < 4; ++c) out[i * 4 + c] = v4[c];
}

// ---- the timed lane block by block (lt_disk_timed_advance_probe) -------------------------------------------------------------
// Step::advance of the timed (POL = false) or the polarized (POL = true) trace up to `iters` times per row, by the calls
// direct_tiles makes: begin_tile, bind, advance.  Blocks of 64: rows 64 b ... 64 b + 63 share a wavefront; a lane leaves the
// loop at its first event other than EV_RUNNING.  What a lane carries goes in and comes out, so that N launches of one
// iteration resume exactly: the integrator's state (states, aux, steps as k_disk_advance_probe; DP45's k1 and [sin, cos],
// computed from the state where null), the elapsed time and the rates (lane (n,5): t_hi, t_lo, rate.t, rate.r, rate.th;
// lane_int (n,2): have, n).  The records are the policy's own buffers of T (w_img, w_tim, w_mom: slot-major, n_q = n), filled
// with NaN by the lane that owns them and handed out as float64.  trace (iters, n, 7), where given: after each iteration
// r, theta, p_r, p_theta, the h counted (0 where the attempt added nothing), the dt added and the hits counted so far.  h and dt
// are the probe's OWN evaluation of advance()'s two statements on the values advance() used (the step's ends, the rates the lane
// carried in and carries out), not a read-out of advance(): they are tied to the lane by the carried (t_hi, t_lo), which is the
// TwoSum of these terms in every bit or the test that replays it fails.
struct TimedProbeIo {
    const double *states, *p_phi, *aux, *k1, *sc0, *lane;
    const uint8_t *refine, *act;
    const uint32_t *steps;
    const int32_t *lane_int;
    int64_t n;
    int max_images, iters;
    void *w_img, *w_tim, *w_mom;
    double *out_state, *out_aux, *out_k1, *out_sc, *out_lane, *out_img, *out_tim, *out_mom, *trace;
    int32_t *out_int, *out_lane_int;
};

template <typename T, typename Integ, bool POL> struct TimedProbeStep {
    using type = DiskTimedStep<T, Integ>;
    static __device__ __forceinline__ void set_mom(type &, void *) {}
};
template <typename T, typename Integ> struct TimedProbeStep<T, Integ, true> {
    using type = DiskPolStep<T, Integ>;
    static __device__ __forceinline__ void set_mom(type &s, void *p) { s.mom = (typename Vec2<T>::type *)p; }
};

template <typename T>
__device__ __forceinline__ void timed_probe_state(const KerrConsts<T> &k, const RayConsts<T> &rc, const TimedProbeIo &io, int64_t i, RayState<T> &s)
{
    disk_probe_state(k, rc, io.states, io.aux, io.steps, i, s);
}
__device__ __forceinline__ void timed_probe_state(const KerrConsts<double> &k, const RayConsts<double> &rc, const TimedProbeIo &io, int64_t i,
                                                  Dp45State<double> &s)
{
    s = dp45_probe_state(k, rc, io.states, io.k1, io.sc0, i);
    s.lam = io.aux[i * 2 + 0]; s.h = io.aux[i * 2 + 1];
    s.steps = io.steps[i];
}
template <typename T> __device__ __forceinline__ void timed_probe_carry(const RayState<T> &, double *k1, double *sc)
{
    for (int j = 0; j < 5; ++j) k1[j] = __builtin_nan("");
    sc[0] = sc[1] = __builtin_nan("");
}
template <typename T> __device__ __forceinline__ void timed_probe_carry(const Dp45State<T> &s, double *k1, double *sc)
{
    for (int j = 0; j < 5; ++j) k1[j] = (double)s.k1[j];
    sc[0] = (double)s.s0; sc[1] = (double)s.c0;
}

template <typename T, typename Integ, bool POL>
__global__ void __launch_bounds__(64) k_disk_timed_advance_probe(KerrConsts<T> k_in, DiskConsts<T> d, TimedProbeIo io)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= io.n) return;
    using Sel = TimedProbeStep<T, Integ, POL>;
    using V2 = typename Vec2<T>::type;
    KerrConsts<T> k = k_in;
    pin_consts(k);
    const RayConsts<T> rc = make_ray_consts(k, (T)io.p_phi[i], io.refine[i] != 0);
    typename Integ::State s;
    timed_probe_state(k, rc, io, i, s);
    const T nan = (T)__builtin_nan("");
    V2 *w_img = (V2 *)io.w_img, *w_mom = (V2 *)io.w_mom;
    T *w_tim = (T *)io.w_tim;
    for (int j = 0; j < io.max_images; ++j) {
        V2 v;
        v.x = v.y = nan;
        w_img[(int64_t)j * io.n + i] = v;
        w_mom[(int64_t)j * io.n + i] = v;
        w_tim[(int64_t)j * io.n + i] = nan;
    }
    typename Sel::type step;
    step.d = d;
    step.img = w_img; step.hits = nullptr; step.n_q = io.n; step.max_images = io.max_images; step.tim = w_tim;
    Sel::set_mom(step, io.w_mom);
    typename Sel::type::Lane l;
    step.begin_tile(l, k);
    step.bind(l, k, rc);
    l.t_hi = (T)io.lane[i * 5 + 0]; l.t_lo = (T)io.lane[i * 5 + 1];
    l.rate.t = (T)io.lane[i * 5 + 2]; l.rate.r = (T)io.lane[i * 5 + 3]; l.rate.th = (T)io.lane[i * 5 + 4];
    l.rate.tx = l.rate.ts = nan; // (the factors of a carried rate are dead: step_time reads them of the step's END alone)
    l.have = io.lane_int[i * 2 + 0] != 0;
    l.n = (uint32_t)io.lane_int[i * 2 + 1];
    const bool act = io.act[i] != 0;
    int ev = EV_RUNNING, made = 0;
    while (made < io.iters) {
        const State5<T> y0 = s.y;
        const T lam0 = s.lam;
        const T h_try = DiskStepLen<Integ>::h(k, rc, s);
        const TimeRates<T> d0 = l.have ? l.rate : time_rates(k, rc, y0);
        ev = step.advance(l, k, rc, s, i, act);
        if (io.trace) {
            const T h = s.lam != lam0 ? h_try : T(0);
            const T dt = h != T(0) ? step_time(k, rc, y0, d0, s.y, l.rate, h, T(1)) : T(0);
            double *tr = io.trace + ((int64_t)made * io.n + i) * 7;
            tr[0] = (double)s.y.r; tr[1] = (double)s.y.th; tr[2] = (double)s.y.pr; tr[3] = (double)s.y.pth;
            tr[4] = (double)h; tr[5] = (double)dt; tr[6] = (double)l.n;
        }
        ++made;
        if (ev != EV_RUNNING) break;
    }
    io.out_state[i * 5 + 0] = (double)s.y.r; io.out_state[i * 5 + 1] = (double)s.y.th; io.out_state[i * 5 + 2] = (double)s.y.ph;
    io.out_state[i * 5 + 3] = (double)s.y.pr; io.out_state[i * 5 + 4] = (double)s.y.pth;
    io.out_aux[i * 2 + 0] = (double)s.lam; io.out_aux[i * 2 + 1] = (double)disk_probe_aux1(s);
    timed_probe_carry(s, io.out_k1 + i * 5, io.out_sc + i * 2);
    io.out_int[i * 3 + 0] = ev; io.out_int[i * 3 + 1] = (int32_t)s.steps; io.out_int[i * 3 + 2] = made;
    io.out_lane[i * 5 + 0] = (double)l.t_hi; io.out_lane[i * 5 + 1] = (double)l.t_lo;
    io.out_lane[i * 5 + 2] = (double)l.rate.t; io.out_lane[i * 5 + 3] = (double)l.rate.r; io.out_lane[i * 5 + 4] = (double)l.rate.th;
    io.out_lane_int[i * 2 + 0] = l.have ? 1 : 0; io.out_lane_int[i * 2 + 1] = (int32_t)l.n;
    for (int j = 0; j < io.max_images; ++j) {
        const int64_t slot = (int64_t)j * io.n + i;
        io.out_img[slot * 2 + 0] = (double)w_img[slot].x; io.out_img[slot * 2 + 1] = (double)w_img[slot].y;
        io.out_mom[slot * 2 + 0] = (double)w_mom[slot].x; io.out_mom[slot * 2 + 1] = (double)w_mom[slot].y;
        io.out_tim[slot] = (double)w_tim[slot];
    }
}

// ---- Stokes siblings of the hot spot's kernels ---------------------------------------------------------------------------
// Per stored slot, e the mean of the three channels of the slot's light: I += e, Q += w e q, U += w e u with
// w = Pi sin^2 zeta, from the float32 records (pol: (q, u, sin zeta, mu) per slot), in float64.  No clamp, no base.
__device__ __forceinline__ double stokes_weight(double pol_frac, const float *prec)
{
    return pol_frac * (double)prec[2] * (double)prec[2];
}

// (I, Q, U) of pixel p at t_obs, unrounded; the light is the disk's (with_disk) plus the spot's.  The body of k_shade_stokes
// and of phase 1 of k_shade_stokes_aa (lt_hotspot_aa.hpp).
__device__ __forceinline__ void stokes_pixel(const float *hits, const uint8_t *n_hits, const float *pol, int64_t p, int max_images,
                                             const DiskShade &ds, const HotspotShade &hs, double pol_frac, double t_obs, double *sum)
{
    const float *rec = hits + p * max_images * 4, *prec = pol + p * max_images * 4;
    const int ns = stored_slots(rec, n_hits, p, max_images);
    sum[0] = sum[1] = sum[2] = 0.0;
    for (int j = 0; j < ns; ++j) {
        double e[3], m;
        hotspot_emission(hs, t_obs, rec + j * 4, e);
        m = (e[0] + e[1] + e[2]) / 3.0;
        if (hs.with_disk) {
            disk_emission(ds, rec[j * 4], rec[j * 4 + 2], e);
            m = (e[0] + e[1] + e[2]) / 3.0 + m;
        }
        const double w = stokes_weight(pol_frac, prec + j * 4);
        sum[0] += m; sum[1] += w * (double)prec[j * 4] * m; sum[2] += w * (double)prec[j * 4 + 1] * m;
    }
}

// One pixel per work-item: out (R, W, 3) float32 = (I, Q, U) at t_obs.
__global__ void __launch_bounds__(256) k_shade_stokes(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                      const float *__restrict__ pol, int64_t n_px, int max_images, DiskShade ds,
                                                      HotspotShade hs, double pol_frac, double t_obs, float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_px) return;
    double sum[3];
    stokes_pixel(hits, n_hits, pol, p, max_images, ds, hs, pol_frac, t_obs, sum);
    for (int c = 0; c < 3; ++c) out[p * 3 + c] = (float)sum[c];
}

// The Stokes light curve of the spot: k_lightcurve_partial's first stage (lightcurve_partial) with (I, Q, U) in place of
// (e, e ix, e iy); the I column is summed exactly as that kernel's column 0, so it has its bits.
__global__ void __launch_bounds__(256) k_lightcurve_stokes_partial(const float *__restrict__ hits, const uint8_t *__restrict__ n_hits,
                                                                   const float *__restrict__ pol, int64_t n_px, int max_images,
                                                                   HotspotShade hs, double pol_frac, double t_start, double dt,
                                                                   double *__restrict__ partial)
{
    const double t_obs = t_start + dt * (double)blockIdx.y;
    lightcurve_partial(n_px, partial, [&](int64_t p, double *v) {
        const float *rec = hits + p * max_images * 4, *prec = pol + p * max_images * 4;
        const int ns = stored_slots(rec, n_hits, p, max_images);
        double e_px = 0.0, q_px = 0.0, u_px = 0.0;
        for (int j = 0; j < ns; ++j) {
            double e[3];
            hotspot_emission(hs, t_obs, rec + j * 4, e);
            const double m = (e[0] + e[1] + e[2]) / 3.0;
            const double w = stokes_weight(pol_frac, prec + j * 4);
            e_px += m; q_px += w * (double)prec[j * 4] * m; u_px += w * (double)prec[j * 4 + 1] * m;
        }
        v[0] += e_px; v[1] += q_px; v[2] += u_px;
    });
}
// (The second stage is k_lightcurve_final itself: it adds three columns of partials whatever they mean.)

} // namespace lt
