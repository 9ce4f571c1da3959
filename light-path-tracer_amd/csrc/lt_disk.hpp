// lt_disk.hpp -- the thin Keplerian accretion disk of lt_render_disk (include/ltrace.h): the disk test behind an
// integrator's iteration (disk_advance), the disk's hooks into the tile loop of the direct schedule (DiskStep; the loop
// itself is direct_tiles, lt_kernels.hpp, shared with the plain frame path), the kernel k_kerr_disk (K2) and its
// epilogues (K3).  K1 is the frame path's prologue, unchanged.
//
// The disk lies in the equatorial plane between r_in and r_out.  A ray (traced backward from the camera) hits it at the
// first strict sign change of theta - pi/2 between two consecutive accepted states whose crossing point has
// r_in <= r <= r_out; crossings outside the annulus do not stop it.  The crossing point is found on the cubic Hermite
// interpolant of the step in lambda, with the derivatives from the Kerr right-hand side at both ends (two extra
// evaluations, once per hit ray), and replaces the ray's final state; the event is EV_DISK.
//
// Nothing here changes a step: the disk's hooks call the integrators' own advance() and streak(), and only look at the
// states they produce.  A lane's arithmetic never depends on which rays share its wavefront (lt_device.hpp), so a ray
// that misses the disk ends with the same bits as in k_kerr_direct, and its pixel is the frame path's pixel.
// Disk parameters travel as a kernel argument of their own (DiskConsts), not in KerrConsts.
#pragma once
#include "lt_kernels.hpp"

namespace lt {

enum : int { EV_DISK = 5 };
constexpr int STATUS_DISK = 2; // LT_STATUS_DISK

template <typename T> struct DiskConsts {
    T r_in, r_out;
    T inv_rp2; // 1 / r_plus^2: bound on the radial speed, disk_vmax
};

// Upper bound on |dr/dlambda| of the ray anywhere outside the horizon.  With E = 1, Sigma^2 (dr/dlambda)^2 = R(r) =
// P^2 - Delta K with K >= 0 (Carter) and Delta > 0, so |dr/dlambda| <= |P| / Sigma <= (r^2 + a^2 + |a L|) / r^2
// <= 1 + (a^2 + |a L|) / r_plus^2.  Per ray (it depends on L); the callers double it for the drift off the null shell.
template <typename T> __device__ __forceinline__ T disk_vmax(const KerrConsts<T> &k, const DiskConsts<T> &d, const RayConsts<T> &rc)
{
    return M<T>::fma(M<T>::fma(M<T>::abs(k.a), M<T>::abs(rc.L), k.a2), d.inv_rp2, T(1));
}

// The step length of the attempt advance() is about to make, per integrator (the same value advance() computes; needed
// only on a lane that crossed the plane) and an upper bound on it.
template <typename Integ> struct DiskStepLen;
template <typename T> struct DiskStepLen<Rk4<T>> {
    static __device__ __forceinline__ T h(const KerrConsts<T> &k, const RayConsts<T> &rc, const RayState<T> &s)
    {
        T h = kerr_rk4_h(k, rc, s.y.r, k.lambda_max - s.lam);
        return s.h_retry > T(0) ? s.h_retry : h;
    }
    static __device__ __forceinline__ T bound(const RayConsts<T> &rc, const RayState<T> &) { return rc.hb; }
};
template <typename T, bool E> struct DiskStepLen<Dp45<T, E>> {
    static __device__ __forceinline__ T h(const KerrConsts<T> &k, const RayConsts<T> &, const Dp45State<T> &s)
    {
        return M<T>::min(s.h, k.lambda_max - s.lam);
    }
    static __device__ __forceinline__ T bound(const RayConsts<T> &, const Dp45State<T> &s) { return s.h; }
};

// Cubic Hermite on the step [0, 1] (lambda = lam0 + t h): value and d/dt from the end values and h * derivatives.
template <typename T> __device__ __forceinline__ T hermite(T y0, T hd0, T y1, T hd1, T t)
{
    const T t2 = t * t, t3 = t2 * t;
    const T h01 = M<T>::fma(T(-2), t3, T(3) * t2), h10 = t3 - T(2) * t2 + t, h11 = t3 - t2;
    return y0 + h01 * (y1 - y0) + h10 * hd0 + h11 * hd1; // h00 y0 + h01 y1 with h00 = 1 - h01
}
template <typename T> __device__ __forceinline__ T hermite_dt(T y0, T hd0, T y1, T hd1, T t)
{
    const T t2 = t * t;
    return (T(6) * t - T(6) * t2) * (y1 - y0) + (T(3) * t2 - T(4) * t + T(1)) * hd0 + (T(3) * t2 - T(2) * t) * hd1;
}

// The crossing of the plane on the step y0 -> y1 of length h, searched on [0, t_end] (t_end < 1: the step was cut at a
// capture / escape radius, the ray ended at t_end).  True, and the crossing state in `hit`, if the crossing point lies
// in the annulus.  Per lane; runs only on lanes whose states straddle the plane near the annulus.
// `tau`, if given, receives the crossing's fraction of the step (the timed trace of lt_hit_time.hpp integrates up to it).
template <typename T>
__device__ __forceinline__ bool disk_crossing(const KerrConsts<T> &k, const DiskConsts<T> &d, const RayConsts<T> &rc,
                                           const State5<T> &y0, const State5<T> &y1, T h, T t_end, State5<T> &hit,
                                           T *tau = nullptr)
{
    const T HALF_PI = T(1.5707963267948966);
    T f0[5], f1[5];
    kerr_rhs(k, rc, y0.r, y0.th, y0.pr, y0.pth, f0[0], f0[1], f0[2], f0[3], f0[4]);
    kerr_rhs(k, rc, y1.r, y1.th, y1.pr, y1.pth, f1[0], f1[1], f1[2], f1[3], f1[4]);
    for (int i = 0; i < 5; ++i) { f0[i] *= h; f1[i] *= h; }
    auto g = [&](T t) { return hermite(y0.th, f0[1], y1.th, f1[1], t) - HALF_PI; };
    T lo = T(0), hi = t_end;
    T glo = y0.th - HALF_PI, ghi = g(hi);
    if (!((glo < T(0) && ghi >= T(0)) || (glo > T(0) && ghi <= T(0)))) return false; // the cubic does not cross on [0, t_end]
    // Newton from the chord's root, kept inside the bracket (bisection where a Newton step leaves it)
    T t = ghi == T(0) ? hi : lo + (hi - lo) * (glo / (glo - ghi));
    for (int it = 0; it < 12; ++it) {
        const T gt = g(t);
        if (gt == T(0)) break;
        if ((gt < T(0)) == (glo < T(0))) { lo = t; glo = gt; } else { hi = t; }
        const T dg = hermite_dt(y0.th, f0[1], y1.th, f1[1], t);
        T tn = t - gt / dg;
        if (!(tn > lo && tn < hi)) tn = T(0.5) * (lo + hi);
        if (M<T>::abs(tn - t) <= T(sizeof(T) == 4 ? 4.8e-7 : 8.9e-16)) { t = tn; break; }
        t = tn;
    }
    hit.r = hermite(y0.r, f0[0], y1.r, f1[0], t);
    hit.th = HALF_PI;
    hit.ph = hermite(y0.ph, f0[2], y1.ph, f1[2], t);
    hit.pr = hermite(y0.pr, f0[3], y1.pr, f1[3], t);
    hit.pth = hermite(y0.pth, f0[4], y1.pth, f1[4], t);
    if (tau) *tau = t;
    return (hit.r >= d.r_in) & (hit.r <= d.r_out);
}

// One iteration of Integ with the disk test behind it.  The common path adds a sign test of theta - pi/2 on both states,
// a min / max of their radii against the annulus widened by the largest radial move of the step, and ONE wave-uniform
// branch.  `vmax2`: twice disk_vmax of the ray.  A crossing inside the annulus, on a lane with `act` set, goes to
// `on_hit(s, hit, ev)`, which returns the iteration's event: the opaque disk ends the ray there, the thin one records
// the point and lets the ray go on.  `on`, if given, is filled before on_hit runs: the step the hit lies on.
template <typename T> struct DiskHitStep {
    State5<T> y1; // the step's end state (a terminal step: the retaken full step's)
    T h, tau;     // its length and the crossing's fraction of it
};
template <typename T, typename Integ, typename OnHit>
__device__ __forceinline__ int disk_advance(const KerrConsts<T> &k, const DiskConsts<T> &d, const RayConsts<T> &rc,
                                            T vmax2, typename Integ::State &s, bool act, OnHit on_hit,
                                            DiskHitStep<T> *on = nullptr)
{
    const T HALF_PI = T(1.5707963267948966);
    const typename Integ::State before = s;
    int ev = Integ::advance(k, rc, s);
    const T z0 = before.y.th - HALF_PI, z1 = s.y.th - HALF_PI;
    // (a state that did not move -- retry, range end, failure -- has z1 == z0: no sign change)
    const bool cross = ((z0 < T(0)) & (z1 >= T(0))) | ((z0 > T(0)) & (z1 <= T(0)));
    // the crossing point of a step lies within (step length) x (largest radial speed) of both ends
    const T pad = DiskStepLen<Integ>::bound(rc, before) * vmax2;
    const bool near = (M<T>::min(before.y.r, s.y.r) <= d.r_out + pad) & (M<T>::max(before.y.r, s.y.r) >= d.r_in - pad);
    const bool cand = cross & near;
    if (__builtin_expect(wave_any(cand), 0)) {
        if (cand) {
            const T h = DiskStepLen<Integ>::h(k, rc, before);
            State5<T> y1 = s.y, hit;
            T t_end = T(1);
            if (ev == EV_CAPTURED || ev == EV_ESCAPED) {
                // the integrator ended the ray on the chord of this step at the capture / escape radius: retake the full
                // step (for RK4 the same step; for DP45 an RK4 step of the same length stands in, DP45's own end state
                // being gone) and search up to the fraction at which that step's chord in r meets the radius.  Rare, not
                // absent: at a = 0.998 (r_isco = 1.237, capture at 1.074) an h = 0.1 capture step can cross the annulus
                y1 = kerr_rk4_step(k, rc, before.y, h);
                const T target = ev == EV_CAPTURED ? k.r_capture : k.r_escape;
                const T denom = y1.r - before.y.r;
                t_end = denom == T(0) ? T(1) : M<T>::min(M<T>::max((target - before.y.r) / denom, T(0)), T(1));
            }
            if (disk_crossing(k, d, rc, before.y, y1, h, t_end, hit, on ? &on->tau : nullptr) & act) {
                if (on) { on->y1 = y1; on->h = h; }
                ev = on_hit(s, hit, ev);
            }
        }
    }
    return ev;
}

// The disk's hooks into the tile loop of the direct schedule (direct_tiles, lt_kernels.hpp): disk_advance in place of
// Integ::advance, with the crossing point taking the ray's place, and the far-field streak gated.
//
// The streak gate.  kerr_rk4_streak takes up to 64 steps with no test but r >= rc4 at the end of each; here it runs with
// rc4 raised, per lane, to r_gate = r_out + 2 h_base vmax2.  Every step it takes then starts and ends at r >= r_gate,
// and within one step of length h_base the ray (and the Hermite cubic of the step, whose excursion beyond its ends is
// at most 0.15 h (|r'_0| + |r'_1|)) stays within h_base vmax2 of either end: above r_out, so no streak step can hold a
// hit.  Wherever the gate fails the ray steps through disk_advance.  The streak's steps are the general iteration's
// arithmetic (lt_device.hpp), so the gate changes no bit of any state.
template <typename T, typename Integ> struct DiskStep {
    DiskConsts<T> d;
    struct Lane {
        T vmax2;          // twice disk_vmax of the lane's ray
        KerrConsts<T> kg; // the streak's constants: rc4 raised to the gate radius
    };
    __device__ __forceinline__ void begin_tile(Lane &l, const KerrConsts<T> &k) { l.kg = k; }
    __device__ __forceinline__ void bind(Lane &l, const KerrConsts<T> &k, const RayConsts<T> &rc)
    {
        l.vmax2 = T(2) * disk_vmax(k, d, rc);
        l.kg.rc4 = M<T>::max(k.rc4, M<T>::fma(T(2) * rc.hb, l.vmax2, d.r_out));
    }
    __device__ __forceinline__ const KerrConsts<T> &streak_consts(const Lane &l, const KerrConsts<T> &) const { return l.kg; }
    __device__ __forceinline__ int advance(Lane &l, const KerrConsts<T> &k, const RayConsts<T> &rc, typename Integ::State &st, int64_t, bool)
    {
        return disk_advance<T, Integ>(k, d, rc, l.vmax2, st, true, [](typename Integ::State &s, const State5<T> &hit, int) {
            s.y = hit;
            return (int)EV_DISK;
        });
    }
    __device__ __forceinline__ void stored(Lane &, int64_t) {}
};

// (A kernel of its own rather than a template parameter of k_kerr_direct: that kernel's code and name stay what they were.)
template <typename T, typename Integ>
__global__ void __launch_bounds__(256, Integ::MIN_WAVES_PER_SIMD) k_kerr_disk(KerrConsts<T> k_in, DiskConsts<T> d,
                                                       const typename Vec4<T>::type *__restrict__ ic,
                                                       typename Vec4<T>::type *__restrict__ fin0,
                                                       typename Vec4<T>::type *__restrict__ fin1, int64_t n_q,
                                                       uint32_t long_iters, uint64_t *__restrict__ kstats,
                                                       unsigned long long *__restrict__ head)
{
    DiskStep<T, Integ> step;
    step.d = d;
    direct_tiles<T, Integ>(k_in, step, ic, fin0, fin1, n_q, long_iters, nullptr, kstats, head);
}

// ---- K3 ---------------------------------------------------------------------------------------------------------------
// Shading constants of the disk (float64; r_in is the resolved inner edge).
struct DiskShade {
    double M, a, r_in, q, exposure;
};

// g = nu_obs / nu_em = 1 / (u^t (1 - Omega xi)) for the circular equatorial geodesic at r orbiting in +phi:
// Omega = sqrt(M) / (r^1.5 + a sqrt(M)), u^t = (r^1.5 + a sqrt(M)) / (r^0.75 sqrt(r^1.5 - 3 M r^0.5 + 2 a sqrt(M))).
// Every multiply-add is written as the fma it is to be: under -ffp-contract=fast the compiler otherwise decides per kernel
// which of them to fuse, and the kernels that evaluate this on the same hit (opaque disk, images, timed hits, supersampled
// frames) differed by up to 5 ulp -- 1 - Omega xi cancels -- where tests/test_gpu_disk_images.py allows 4.  Now they agree
// in every bit.
__device__ __forceinline__ double disk_redshift(double M_, double a, double r, double xi)
{
    const double sM = sqrt(M_), sr = sqrt(r), r15 = r * sr;
    const double asM = a * sM;
    const double num = __builtin_fma(a, sM, r15);
    const double omega = sM / num;
    const double ut = num / (sqrt(r15) * sqrt(__builtin_fma(2.0, asM, __builtin_fma(-3.0 * M_, sr, r15))));
    return 1.0 / (ut * __builtin_fma(-omega, xi, 1.0));
}

// Light of one point of the disk, unclamped: E = I ramp(s) with I = exposure g^4 (r_in / r)^q, s = g (r_in / r)^(3/4),
// ramp(s) = (clamp(2s, 0, 1), clamp(2s - 0.5, 0, 1), clamp(2s - 1, 0, 1)).  Evaluated in float64 from the float32 (r, g)
// the caller gets in d_disk / d_images, so that the colour is a function of what is stored.
// I of it alone, x = r_in / r: what a spectrum bins (lt_spectrum.hpp).
__device__ __forceinline__ double disk_intensity(const DiskShade &ds, double x, double g)
{
    const double g2 = g * g;
    return ds.exposure * (g2 * g2) * pow(x, ds.q);
}

__device__ __forceinline__ void disk_emission(const DiskShade &ds, float r32, float g32, double *e)
{
    const double r = (double)r32, g = (double)g32;
    const double x = ds.r_in / r;
    const double I = disk_intensity(ds, x, g);
    const double s = g * pow(x, 0.75);
    for (int i = 0; i < 3; ++i) e[i] = I * fmin(fmax(2.0 * s - 0.5 * i, 0.0), 1.0);
}

// Colour of a pixel of the opaque disk: rgb = clamp(E, 0, 1); one channel: the mean of the three.
__device__ __forceinline__ void disk_shade(const DiskShade &ds, float r32, float g32, int nch, float *rgb)
{
    double c[3];
    disk_emission(ds, r32, g32, c);
    for (int i = 0; i < 3; ++i) c[i] = fmin(fmax(c[i], 0.0), 1.0);
    if (nch == 1) rgb[0] = (float)((c[0] + c[1] + c[2]) / 3.0);
    else { rgb[0] = (float)c[0]; rgb[1] = (float)c[1]; rgb[2] = (float)c[2]; }
}

// phi wrapped to [0, 2 pi)
__device__ __forceinline__ double wrap_2pi(double ph)
{
    const double TWO_PI = 6.283185307179586;
    double w = ph - TWO_PI * floor(ph * (1.0 / TWO_PI));
    return (w >= TWO_PI || w < 0.0) ? 0.0 : w;
}

// One pixel per work-item, as k_epilogue_frame (global-gather background sampling).  EV_DISK records get the redshift
// and the disk colour; every other record goes through load_result / shade exactly as there.  disk_out (R, W, 3) float32
// (r_hit, phi_hit in [0, 2 pi), g), NaN where the ray missed the disk; may be NULL.
template <typename T, bool HAS_BG>
__global__ void __launch_bounds__(EPILOGUE_BLOCK) k_epilogue_disk(CamConsts c, MetricConsts m, DiskShade ds,
                                                                  const typename Vec4<T>::type *__restrict__ fin0,
                                                                  const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                                  float *__restrict__ disk_out)
{
    const int lrow = (int)blockIdx.y, ix = (int)(blockIdx.x * EPILOGUE_BLOCK + threadIdx.x);
    const int64_t p = (int64_t)lrow * c.W + ix;
    StatAcc acc;
    bool on_disk = false;
    if (ix < c.W) {
        const int64_t q = pixel_to_q(c, ix, lrow);
        const typename Vec4<T>::type v0 = fin0[q], v1 = fin1[q];
        RayResult res;
        float rgb[3];
        int nch = (HAS_BG && o.bg) ? o.bg_c : 3;
        float d3[3] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        long long wl;
        if ((int)v1.z == EV_DISK) {
            on_disk = true;
            const double ph = (double)v0.z;
            res.status = STATUS_DISK;
            res.fa = __builtin_nan("");
            res.n_half = half_orbits(ph);
            res.steps = (uint32_t)v1.w;
            d3[0] = (float)v0.x;
            d3[1] = (float)wrap_2pi(ph);
            d3[2] = (float)disk_redshift(ds.M, ds.a, (double)v0.x, (double)v1.y);
            disk_shade(ds, d3[0], d3[2], nch, rgb);
        } else {
            load_result<T>(m, fin0, fin1, q, res);
        }
        acc.add(res);
        const float fa32 = (res.status == 1) ? (float)res.fa : __builtin_nanf("");
        wl = res.n_half < 0 ? 0 : (res.n_half > 65535 ? 65535 : res.n_half);
        if (o.fa) o.fa[p] = fa32;
        if (o.w) o.w[p] = (uint16_t)wl;
        if (o.status) o.status[p] = (int8_t)res.status;
        if (o.steps) o.steps[p] = res.steps;
        if (disk_out) { disk_out[p * 3] = d3[0]; disk_out[p * 3 + 1] = d3[1]; disk_out[p * 3 + 2] = d3[2]; }
        if (o.rgb || o.rgba) {
            if (!on_disk) shade<HAS_BG>(c, o, ix, local_to_global_row(c, lrow), fa32, (int)wl, rgb, nch);
            if (o.rgb) for (int ch = 0; ch < nch; ++ch) o.rgb[p * nch + ch] = rgb[ch];
            if (o.rgba) store_rgba(o, p, rgb, nch);
        }
    }
    flush_stats<7>(o.stats, acc, m, on_disk); // word 6: the rays that ended on the disk (-> LT_STAT_DISK)
}

// Epilogue of lt_trace_batch_kerr_disk: k_epilogue_arrays plus out_disk (n, 3) float64 (r_hit, phi_hit, g), NaN off the disk.
template <typename T>
__global__ void __launch_bounds__(256) k_epilogue_arrays_disk(MetricConsts m, DiskShade ds, const typename Vec4<T>::type *__restrict__ fin0,
                                                              const typename Vec4<T>::type *__restrict__ fin1, int64_t n,
                                                              double *__restrict__ out_fa, int64_t *__restrict__ out_w,
                                                              int8_t *__restrict__ out_status, double *__restrict__ out_disk,
                                                              uint32_t *__restrict__ out_evals)
{
    int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const typename Vec4<T>::type v0 = fin0[q], v1 = fin1[q];
    RayResult res;
    const double NaN = __builtin_nan("");
    double d3[3] = {NaN, NaN, NaN};
    if ((int)v1.z == EV_DISK) {
        res.status = STATUS_DISK;
        res.fa = NaN;
        res.n_half = half_orbits((double)v0.z);
        res.steps = (uint32_t)v1.w;
        res.evals = (uint32_t)m.evals_fixed + res.steps * (uint32_t)m.evals_per_step;
        d3[0] = (double)v0.x;
        d3[1] = wrap_2pi((double)v0.z);
        d3[2] = disk_redshift(ds.M, ds.a, (double)v0.x, (double)v1.y);
    } else {
        load_result<T>(m, fin0, fin1, q, res);
    }
    out_fa[q] = (res.status == 1) ? res.fa : NaN;
    out_w[q] = res.n_half;
    if (out_status) out_status[q] = (int8_t)res.status;
    if (out_disk) { out_disk[q * 3] = d3[0]; out_disk[q * 3 + 1] = d3[1]; out_disk[q * 3 + 2] = d3[2]; }
    if (out_evals) out_evals[q] = res.evals;
}

// ---- the disk test block by block (lt_disk_crossing_probe, lt_disk_advance_probe, lt_disk_shade_probe) -------------------
// disk_crossing<T> once per row, on the step y0 -> y1 of length h searched up to t_end.  out_hit (n,5), out_tau (n): what
// the call left in `hit` and `tau` (NaN where it returned before setting them); out_found (n).
template <typename T>
__global__ void __launch_bounds__(64) k_disk_crossing_probe(KerrConsts<T> k_in, DiskConsts<T> d, const double *__restrict__ y0,
                                                            const double *__restrict__ y1, const double *__restrict__ p_phi,
                                                            const double *__restrict__ h, const double *__restrict__ t_end,
                                                            int64_t n, uint8_t *__restrict__ out_found,
                                                            double *__restrict__ out_hit, double *__restrict__ out_tau)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    KerrConsts<T> k = k_in;
    pin_consts(k);
    const RayConsts<T> rc = make_ray_consts(k, (T)p_phi[i], false);
    State5<T> a, b, hit;
    a.r = (T)y0[i * 5 + 0]; a.th = (T)y0[i * 5 + 1]; a.ph = (T)y0[i * 5 + 2]; a.pr = (T)y0[i * 5 + 3]; a.pth = (T)y0[i * 5 + 4];
    b.r = (T)y1[i * 5 + 0]; b.th = (T)y1[i * 5 + 1]; b.ph = (T)y1[i * 5 + 2]; b.pr = (T)y1[i * 5 + 3]; b.pth = (T)y1[i * 5 + 4];
    const T nan = (T)__builtin_nan("");
    hit.r = hit.th = hit.ph = hit.pr = hit.pth = nan;
    T tau = nan;
    const bool found = disk_crossing(k, d, rc, a, b, (T)h[i], (T)t_end[i], hit, &tau);
    out_found[i] = found ? 1 : 0;
    out_hit[i * 5 + 0] = (double)hit.r; out_hit[i * 5 + 1] = (double)hit.th; out_hit[i * 5 + 2] = (double)hit.ph;
    out_hit[i * 5 + 3] = (double)hit.pr; out_hit[i * 5 + 4] = (double)hit.pth;
    out_tau[i] = (double)tau;
}

// A row's integrator state, in the layouts of k_rk4_advance_probe and k_dp45_advance_probe (lt_kernels.hpp).
// aux (n,2): RK4 lam, h_retry; DP45 lam, h (the carried derivative and sincos are computed from the state, as at a start).
template <typename T>
__device__ __forceinline__ void disk_probe_state(const KerrConsts<T> &, const RayConsts<T> &, const double *__restrict__ states,
                                                 const double *__restrict__ aux, const uint32_t *__restrict__ steps, int64_t i,
                                                 RayState<T> &s)
{
    s.y.r = (T)states[i * 5 + 0]; s.y.th = (T)states[i * 5 + 1]; s.y.ph = (T)states[i * 5 + 2];
    s.y.pr = (T)states[i * 5 + 3]; s.y.pth = (T)states[i * 5 + 4];
    s.lam = (T)aux[i * 2 + 0]; s.h_retry = (T)aux[i * 2 + 1];
    s.steps = steps[i];
}
__device__ __forceinline__ void disk_probe_state(const KerrConsts<double> &k, const RayConsts<double> &rc,
                                                 const double *__restrict__ states, const double *__restrict__ aux,
                                                 const uint32_t *__restrict__ steps, int64_t i, Dp45State<double> &s)
{
    s = dp45_probe_state(k, rc, states, nullptr, nullptr, i);
    s.lam = aux[i * 2 + 0]; s.h = aux[i * 2 + 1];
    s.steps = steps[i];
}
template <typename T> __device__ __forceinline__ T disk_probe_aux1(const RayState<T> &s) { return s.h_retry; }
template <typename T> __device__ __forceinline__ T disk_probe_aux1(const Dp45State<T> &s) { return s.h; }

// disk_advance<T, Integ> once per row, with an on_hit that records the hit and returns EV_DISK (the state is left as
// Integ::advance left it) and with `on` given.  Blocks of 64: rows 64 b ... 64 b + 63 share a wavefront.  act (n): the
// lane's `act`.  out_state (n,5), out_aux (n,2) as aux, out_int (n,3): the event, steps, 1 if on_hit ran; out_hit (n,5) and
// out_on (n,7): on.y1 (5), on.h, on.tau -- NaN where nothing wrote them.
template <typename T, typename Integ>
__global__ void __launch_bounds__(64) k_disk_advance_probe(KerrConsts<T> k_in, DiskConsts<T> d, const double *__restrict__ states,
                                                           const double *__restrict__ p_phi, const uint8_t *__restrict__ refine,
                                                           const double *__restrict__ aux, const uint32_t *__restrict__ steps,
                                                           const uint8_t *__restrict__ act, int64_t n,
                                                           double *__restrict__ out_state, double *__restrict__ out_aux,
                                                           int32_t *__restrict__ out_int, double *__restrict__ out_hit,
                                                           double *__restrict__ out_on)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    KerrConsts<T> k = k_in;
    pin_consts(k);
    const RayConsts<T> rc = make_ray_consts(k, (T)p_phi[i], refine[i] != 0);
    typename Integ::State s;
    disk_probe_state(k, rc, states, aux, steps, i, s);
    const T nan = (T)__builtin_nan("");
    State5<T> rec;
    rec.r = rec.th = rec.ph = rec.pr = rec.pth = nan;
    DiskHitStep<T> on;
    on.y1 = rec; on.h = nan; on.tau = nan;
    int was_hit = 0;
    const T vmax2 = T(2) * disk_vmax(k, d, rc);
    const int ev = disk_advance<T, Integ>(k, d, rc, vmax2, s, act[i] != 0, [&](typename Integ::State &, const State5<T> &hit, int) {
        rec = hit;
        was_hit = 1;
        return (int)EV_DISK;
    }, &on);
    out_state[i * 5 + 0] = (double)s.y.r; out_state[i * 5 + 1] = (double)s.y.th; out_state[i * 5 + 2] = (double)s.y.ph;
    out_state[i * 5 + 3] = (double)s.y.pr; out_state[i * 5 + 4] = (double)s.y.pth;
    out_aux[i * 2 + 0] = (double)s.lam; out_aux[i * 2 + 1] = (double)disk_probe_aux1(s);
    out_int[i * 3 + 0] = ev; out_int[i * 3 + 1] = (int32_t)s.steps; out_int[i * 3 + 2] = was_hit;
    out_hit[i * 5 + 0] = (double)rec.r; out_hit[i * 5 + 1] = (double)rec.th; out_hit[i * 5 + 2] = (double)rec.ph;
    out_hit[i * 5 + 3] = (double)rec.pr; out_hit[i * 5 + 4] = (double)rec.pth;
    out_on[i * 7 + 0] = (double)on.y1.r; out_on[i * 7 + 1] = (double)on.y1.th; out_on[i * 7 + 2] = (double)on.y1.ph;
    out_on[i * 7 + 3] = (double)on.y1.pr; out_on[i * 7 + 4] = (double)on.y1.pth;
    out_on[i * 7 + 5] = (double)on.h; out_on[i * 7 + 6] = (double)on.tau;
}

// The closed forms a hit goes through (k_epilogue_disk's statements): in (n,4) r, phi (unwrapped), xi, g_given.  out_f64
// (n,5): g = disk_redshift(r, xi), wrap_2pi(phi), then disk_emission (3) from the float32-rounded (r, g) -- of g_given where
// that is not NaN, so that a test can place s on the ramp's knees; out_half (n): half_orbits(phi); out_f32 (n,4): disk_shade
// of the same float32 (r, g) with 1 channel, then with 3.
__global__ void __launch_bounds__(64) k_disk_shade_probe(DiskShade ds, const double *__restrict__ in, int64_t n,
                                                         double *__restrict__ out_f64, int64_t *__restrict__ out_half,
                                                         float *__restrict__ out_f32)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const double r = in[i * 4 + 0], ph = in[i * 4 + 1], xi = in[i * 4 + 2], g_given = in[i * 4 + 3];
    const double g = disk_redshift(ds.M, ds.a, r, xi);
    const float r32 = (float)r, g32 = (float)(g_given == g_given ? g_given : g);
    out_f64[i * 5 + 0] = g;
    out_f64[i * 5 + 1] = wrap_2pi(ph);
    disk_emission(ds, r32, g32, out_f64 + i * 5 + 2);
    out_half[i] = (int64_t)half_orbits(ph);
    disk_shade(ds, r32, g32, 1, out_f32 + i * 4);
    disk_shade(ds, r32, g32, 3, out_f32 + i * 4 + 1);
}

} // namespace lt
