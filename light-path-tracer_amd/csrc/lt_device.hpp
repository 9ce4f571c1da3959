// lt_device.hpp -- __device__ building blocks of the gfx950 ray integrators.
//
// Written for CDNA4 wave64: everything a ray needs lives in registers, the metric terms are
// inlined, there is no LDS and no cross-lane traffic in the hot loop.
//
// What each block computes is fixed by the reference (cited per function); HOW it is computed is
// not a transcription.  The integrate kernel is VALU-issue bound, and on gfx950 (measured with
// tools/issue_probe.py) every VALU instruction costs ~2.1 issue cycles per wave
// when FMA-class and "second pipe" instructions (min/max/cmp/cvt/select, anything with an SGPR
// operand) are mixed, a transcendental (v_rcp_f32 ...) costs ~13, and a packed v_pk_* costs two
// plain ones.  So the design rule is: fewest instructions, fewest reciprocals.  The Kerr
// right-hand side is re-derived from the separable form of the Hamiltonian (one merged reciprocal,
// ~75 instructions instead of the reference's 186 flops + 14 divides) while remaining the exact
// gradient of the same H, so it agrees with the reference for any state, on- or off-shell
// (tests/test_gpu_parity.py::test_kerr_rhs_probe_matches_reference).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// functions a stand-alone host program can call as well (tools/scratch/eq_sincos_check.hip)
#define LT_HD __host__ __device__ __forceinline__

namespace lt {

// true if the predicate holds in any active lane: the wave-uniform test behind every fast path.  The builtin
// reads the compare's lane mask directly (HIP's __ballot(int) first materialises the bool in a VGPR and
// compares it again: two extra VALU instructions per test).
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0ull; }
// true if the predicate holds in every ACTIVE lane.  (Written on the predicate itself, not as !wave_any(!p): when p is
// also used for per-lane selects the compiler keeps its lane mask, and negating it first costs a 0/1 materialisation
// and a compare -- two VALU instructions per test.)
__device__ __forceinline__ bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(p) == __builtin_amdgcn_ballot_w64(true); }
// A predicate as the wave's lane mask, and a wave-uniform lane mask as each lane's predicate again.  Several tests
// that only ever meet in one wave-uniform branch are cheapest as one mask each, combined on the scalar unit: ANDed as
// bools they are turned into a 0/1 VGPR and compared again to feed the ballot.  lane_pred costs no instruction: the
// mask IS the condition register of the selects that use it.
__device__ __forceinline__ uint64_t lane_mask(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool lane_pred(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }


// ---------------------------------------------------------------------------------------
// scalar math wrappers
// ---------------------------------------------------------------------------------------
template <typename T> struct M;

template <> struct M<float> {
    // 1/x: hardware reciprocal (1 ulp) + one Newton step
    static __device__ __forceinline__ float rcp(float x)
    {
        float y = __builtin_amdgcn_rcpf(x);
        float e = __builtin_fmaf(-x, y, 1.0f);
        return __builtin_fmaf(y, e, y);
    }
    // 1/x for positive normal x WITHOUT the transcendental unit.  Measured on gfx950 (lt_piece_probe):
    // one v_rcp_f32 inside this kernel's FMA-dense stream costs ~70 SIMD cycles, whatever the
    // occupancy and whether or not anything depends on it, against ~13 for six FMA-class instructions.
    // Bit trick seed (relative error <= 5.1 %), one cubic and one quadratic Newton step: error 1.7e-8
    // before rounding, i.e. within 1 ulp like rcp + Newton (every float32 in [2^-100, 2^100] against float64: 0.775 ulp,
    // tests/test_gpu_step_blocks.py).
    static __device__ __forceinline__ float rcp_pos(float x)
    {
        float y = __uint_as_float(0x7EF311C0u - __float_as_uint(x));
        float e = __builtin_fmaf(-x, y, 1.0f);
        y = __builtin_fmaf(y, __builtin_fmaf(e, e, e), y);
        e = __builtin_fmaf(-x, y, 1.0f);
        return __builtin_fmaf(y, e, y);
    }
    static __device__ __forceinline__ float fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
    static __device__ __forceinline__ float abs(float x) { return __builtin_fabsf(x); }
    static __device__ __forceinline__ float max(float a, float b) { return __builtin_fmaxf(a, b); }
    static __device__ __forceinline__ float min(float a, float b) { return __builtin_fminf(a, b); }
    // sin^2 floored at 1e-15 (metrics.py:236-237): below float resolution unless sin^2 < 1e-8, so an
    // add does the job of the max without leaving the FMA pipe.  (Within 1e-4 rad of the axis the two differ: at the
    // float32 next to pi, sin^2 = 7.6e-15 becomes 8.6e-15.  Only the L / sin^2 terms see it, and a ray that close to the
    // axis has |L| < 1e-4 r sin theta.)
    static __device__ __forceinline__ float sin2_floor(float s) { return __builtin_fmaf(s, s, 1e-15f); }
    // pi/2 split for the Cody-Waite reduction: 8 + 11 + 24 significant bits
    static constexpr float PIO2_1 = 1.5703125f, PIO2_2 = 4.837512969970703125e-4f, PIO2_3 = 7.54978995489188e-8f;
    // sin and cos of a reduced angle: single-precision minimax polynomials on [-pi/4, pi/4]
    static LT_HD void sincos_reduced(float y, float &sy, float &cy)
    {
        float z = y * y;
        float ps = __builtin_fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f);
        ps = __builtin_fmaf(ps, z, -1.6666654611e-1f);
        sy = __builtin_fmaf(ps * z, y, y);
        float pc = __builtin_fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f);
        pc = __builtin_fmaf(pc, z, 4.166664568298827e-2f);
        cy = __builtin_fmaf(pc * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    }
    // sin and cos of an angle of modest size (|x| < ~1e4; the polar angle of a ray stays within a
    // few pi).  Cody-Waite reduction by pi/2 in three pieces, the polynomials above, quadrant fix-up
    // with integer ops: ~25 VALU ops for both values.  ABSOLUTE error <= 1.56 u (u = 2^-24, half an ulp of 1) over every
    // float32 |x| <= 1e4 (tests/test_gpu_step_blocks.py) -- about an ulp of a result near 1, not a relative figure: next
    // to a zero of the function the reduced angle carries the argument's rounding of pi/2's third piece, 5.8 ulp of the
    // result at |x| = 3 pi/2, 3 pi.
    static LT_HD void sincos(float x, float &s, float &c)
    {
        const float TWO_OVER_PI = 0.636619772367581343f;
        float kf = __builtin_rintf(x * TWO_OVER_PI);
        float y = __builtin_fmaf(-kf, PIO2_1, x);
        y = __builtin_fmaf(-kf, PIO2_2, y);
        y = __builtin_fmaf(-kf, PIO2_3, y);
        int k = (int)kf;
        float sy, cy;
        sincos_reduced(y, sy, cy);
        bool swap = k & 1;
        float ss = swap ? cy : sy;
        float cc = swap ? sy : cy;
        // sign: sin flips for k = 2,3 (mod 4), cos for k = 1,2
        uint32_t sbit = ((uint32_t)k << 30) & 0x80000000u;
        uint32_t cbit = ((uint32_t)(k + 1) << 30) & 0x80000000u;
        s = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, ss) ^ sbit);
        c = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, cc) ^ cbit);
    }
    // The same for an angle known to reduce to the quadrant k = 1 (x within pi/4 of pi/2; callers keep it inside
    // [EQ_BAND_LO, EQ_BAND_HI]): no multiply by 2/pi, no rint, no quadrant logic -- 14 instructions for 28.  Bit-identical
    // to sincos there: fma(-1, P, x) is x - P rounded once, k = 1 swaps the two polynomials, leaves the sine's sign and
    // flips the cosine's (tools/scratch/eq_sincos_check.hip and tests/test_gpu_eq_streak.py compare every float32 of the band).
    static constexpr float EQ_BAND_LO = 0.80f, EQ_BAND_HI = 2.34f; // strictly inside (pi/4, 3 pi/4) = (0.7854, 2.3562)
    static LT_HD void sincos_q1(float x, float &s, float &c)
    {
        float y = ((x - PIO2_1) - PIO2_2) - PIO2_3;
        float sy, cy;
        sincos_reduced(y, sy, cy);
        s = cy;
        c = -sy;
    }
    // sin and cos of a SMALL angle (|d| <= 0.25): Taylor, 7 FMA-class instructions; truncation error < 1.3e-8, and with
    // the rounding of the operations, over every float32 of the range: cosine within 0.53 u absolute, sine within 1.32 ulp
    // of the result (0.33 u)
    static __device__ __forceinline__ void sincos_small(float d, float &s, float &c)
    {
        float z = d * d;
        float ps = __builtin_fmaf(z, 8.3333333333e-3f, -1.6666666667e-1f);
        s = __builtin_fmaf(ps * z, d, d);
        float pc = __builtin_fmaf(z, -1.3888888889e-3f, 4.1666666667e-2f);
        pc = __builtin_fmaf(pc, z, -0.5f);
        c = __builtin_fmaf(pc, z, 1.0f);
    }
    // true unless x is NaN or +-inf
    static __device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }
    static constexpr float LARGEST = __FLT_MAX__;
};

// sin and cos of a float64 angle of modest size without libm's generic range reduction: Cody-Waite
// by pi/2 (fdlibm's pio2_1 + pio2_1t split, a double-double remainder y0 + y1 good to |x| ~ 1e5) and
// the fdlibm kernel polynomials on [-pi/4, pi/4].  Error < 1 ulp of the result plus the reduction's: pi/2 is carried to
// 86 bits, so the reduced angle of x = k pi/2 + y is off by up to 1.4e-26 |k| -- next to a multiple of pi/2, where one of
// the two results is tiny, that is many ulps OF THAT RESULT and nothing beside the argument's own rounding.  ~45 float64
// FMA-class instructions, no branches, no scratch -- OCML's sincos carries a Payne-Hanek path and costs registers and time.
__device__ __forceinline__ void sincos_f64(double x, double &s, double &c)
{
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double P1 = 1.57079632673412561417e+00, P1T = 6.07710050650619224932e-11;
    double kf = __builtin_rint(x * TWO_OVER_PI);
    double r = __builtin_fma(-kf, P1, x);
    double w = kf * P1T;
    double y0 = r - w;
    double y1 = (r - y0) - w;
    int k = (int)kf;
    double z = y0 * y0;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    double ps = __builtin_fma(z, S6, S5);
    ps = __builtin_fma(z, ps, S4);
    ps = __builtin_fma(z, ps, S3);
    ps = __builtin_fma(z, ps, S2);
    ps = __builtin_fma(z, ps, S1);
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    double pc = __builtin_fma(z, C6, C5);
    pc = __builtin_fma(z, pc, C4);
    pc = __builtin_fma(z, pc, C3);
    pc = __builtin_fma(z, pc, C2);
    pc = __builtin_fma(z, pc, C1);
    // Each value is (large part) + (everything small), summed last, so that it carries ONE rounding of its own size:
    // sin = y0 + (y0 z ps + y1 cos), cos = w + ((1 - w) - z/2 + z^2 pc - y1 y0) with w = 1 - z/2 rounded and (1 - w) - z/2
    // its rounding error, exact (z/2 <= 0.31: 1 - w is exact, fdlibm's __kernel_cos).  The low word y1 enters to first
    // order.  Measured against mpmath over |x| <= 1e5: 0.78 ulp (tests/test_gpu_step_blocks.py); with the polynomial, the
    // 1 - z/2 and the y1 term rounded one after the other, as this function did at first, 1.52.
    const double hz = 0.5 * z;
    const double w1 = 1.0 - hz;
    const double cl = __builtin_fma(z * z, pc, (1.0 - w1) - hz);
    double sr = y0 + __builtin_fma(z * y0, ps, y1 * w1), cr = w1 + __builtin_fma(-y1, y0, cl);
    bool swap = k & 1;
    double ss = swap ? cr : sr, cc = swap ? sr : cr;
    s = (k & 2) ? -ss : ss;
    c = ((k + 1) & 2) ? -cc : cc;
}

// x, hidden from the optimiser.  A product passed through it is rounded on its own: it cannot be fused into the sum it feeds
// (-ffp-contract=fast fuses whatever it can, a function's `fp contract(off)` notwithstanding, and which product of a sum of
// products it picks differs from one kernel to the next).
__device__ __forceinline__ double unfused(double x)
{
    asm volatile("" : "+v"(x));
    return x;
}
__device__ __forceinline__ float unfused(float x)
{
    asm("" : "+v"(x));
    return x;
}

// sin and cos of a float64 angle of a few radians, correctly rounded (against mpmath: every one of 40 000 arguments; glibc's
// own differ from them on 1 in 1000): for what runs once per ray and has to give the reference's bits -- the prologue, whose
// Theta and p_r^2 cancel completely on some rays, where the reference's value is the rounding of its own sin(alpha) and
// only the same sine gives it.  pi/2 is carried to 141 bits (P1 + P1T + P1TT, the product kf P1T exactly), the reduced
// angle is a double-double, the first four terms of either Taylor series are summed in double-double arithmetic and the
// rest (below 2^-21 of the result) in float64.  ~400 float64 operations: not for the integrators, which keep sincos_f64.
struct DD { double hi, lo; };
__device__ __forceinline__ DD dd_two_sum(double a, double b) { double s = a + b, bb = s - a; return {s, (a - (s - bb)) + (b - bb)}; }
__device__ __forceinline__ DD dd_quick_two_sum(double a, double b) { double s = a + b; return {s, b - (s - a)}; }
// (the product is hidden from the compiler: fused into the sum it later feeds, that sum would no longer be the rounded sum of
// its two float64 operands that dd_two_sum's error term is the error of)
__device__ __forceinline__ DD dd_two_prod(double a, double b) { double p = unfused(a * b); return {p, __builtin_fma(a, b, -p)}; }
__device__ __forceinline__ DD dd_add(DD a, DD b)
{
    DD s = dd_two_sum(a.hi, b.hi);
    return dd_quick_two_sum(s.hi, s.lo + (a.lo + b.lo));
}
__device__ __forceinline__ DD dd_mul(DD a, DD b)
{
    DD p = dd_two_prod(a.hi, b.hi);
    return dd_quick_two_sum(p.hi, p.lo + __builtin_fma(a.hi, b.lo, a.lo * b.hi));
}
__device__ __forceinline__ void sincos_f64_exact(double x, double &s, double &c)
{
    // (-1)^k / (2k+1)! and (-1)^k / (2k)!, k = 1 ... 13, as unevaluated sums of two float64
    constexpr double DD_S[13][2] = {{-0.16666666666666666, -9.25185853854297e-18}, {0.008333333333333333, 1.1564823173178714e-19}, {-0.0001984126984126984, -1.7209558293420705e-22}, {2.7557319223985893e-06, -1.858393274046472e-22}, {-2.505210838544172e-08, 1.448814070935912e-24}, {1.6059043836821613e-10, 1.2585294588752098e-26}, {-7.647163731819816e-13, -7.03872877733453e-30}, {2.8114572543455206e-15, 1.6508842730861433e-31}, {-8.22063524662433e-18, -2.2141894119604265e-34}, {1.9572941063391263e-20, -1.3643503830087908e-36}, {-3.868170170630684e-23, 8.843177655482344e-40}, {6.446950284384474e-26, -1.9330404233703465e-42}, {-9.183689863795546e-29, -1.4303150396787322e-45}};
    constexpr double DD_C[13][2] = {{-0.5, 0.0}, {0.041666666666666664, 2.3129646346357427e-18}, {-0.001388888888888889, 5.300543954373577e-20}, {2.48015873015873e-05, 2.1511947866775882e-23}, {-2.755731922398589e-07, -2.3767714622250297e-23}, {2.08767569878681e-09, -1.20734505911326e-25}, {-1.1470745597729725e-11, -2.0655512752830745e-28}, {4.779477332387385e-14, 4.399205485834081e-31}, {-1.5619206968586225e-16, -1.1910679660273754e-32}, {4.110317623312165e-19, 1.4412973378659527e-36}, {-8.896791392450574e-22, 7.911402614872376e-38}, {1.6117375710961184e-24, -3.6846573564509766e-41}, {-2.4795962632247976e-27, 1.2953730964765229e-43}};
    const double TWO_OVER_PI = 6.36619772367581382433e-01;
    const double P1 = 1.57079632673412561417e+00, P1T = 6.07710050650619224932e-11, P1TT = 3.5215598651832003884e-27;
    const double kf = __builtin_rint(x * TWO_OVER_PI);
    const double r = __builtin_fma(-kf, P1, x); // exact
    const DD w = dd_two_prod(kf, P1T);
    DD y = dd_two_sum(r, -w.hi);
    y = dd_quick_two_sum(y.hi, y.lo + __builtin_fma(-kf, P1TT, -w.lo));
    const DD z = dd_mul(y, y);
    double qs = DD_S[12][0], qc = DD_C[12][0];
#pragma unroll
    for (int i = 11; i >= 4; --i) { qs = __builtin_fma(qs, z.hi, DD_S[i][0]); qc = __builtin_fma(qc, z.hi, DD_C[i][0]); }
    DD ps = {qs, 0.0}, pc = {qc, 0.0};
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        ps = dd_add(dd_mul(ps, z), DD{DD_S[i][0], DD_S[i][1]});
        pc = dd_add(dd_mul(pc, z), DD{DD_C[i][0], DD_C[i][1]});
    }
    const DD sn = dd_add(y, dd_mul(dd_mul(ps, z), y)), cn = dd_add(DD{1.0, 0.0}, dd_mul(pc, z));
    const double sr = sn.hi + sn.lo, cr = cn.hi + cn.lo;
    const int k = (int)kf;
    const bool swap = k & 1;
    const double ss = swap ? cr : sr, cc = swap ? sr : cr;
    s = (k & 2) ? -ss : ss;
    c = ((k + 1) & 2) ? -cc : cc;
}

template <> struct M<double> {
    static __device__ __forceinline__ double rcp(double x) { return 1.0 / x; }
    // 1/x for positive normal x: the hardware seed and two Newton steps -- the core of the compiler's IEEE division
    // (~12 instructions) without its scaling, residual correction and special-case fix-up; within an ulp
    static __device__ __forceinline__ double rcp_pos(double x)
    {
        double y = __builtin_amdgcn_rcp(x);
        double e = __builtin_fma(-x, y, 1.0);
        y = __builtin_fma(y, e, y);
        e = __builtin_fma(-x, y, 1.0);
        return __builtin_fma(y, e, y);
    }
    static __device__ __forceinline__ double fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
    static __device__ __forceinline__ double abs(double x) { return __builtin_fabs(x); }
    static __device__ __forceinline__ double max(double a, double b) { return __builtin_fmax(a, b); }
    static __device__ __forceinline__ double min(double a, double b) { return __builtin_fmin(a, b); }
    static __device__ __forceinline__ double sin2_floor(double s) { return __builtin_fmax(s * s, 1e-15); }
    static __device__ __forceinline__ void sincos(double x, double &s, double &c) { sincos_f64(x, s, c); }
    // (float64 has no fixed-quadrant form: its streak never asks for one)
    static __device__ __forceinline__ void sincos_q1(double x, double &s, double &c) { sincos_f64(x, s, c); }
    // |d| <= 0.25: Taylor to d^11 / d^12, truncation error < 3e-18; with the rounding of the operations 0.58 ulp
    static __device__ __forceinline__ void sincos_small(double d, double &s, double &c)
    {
        double z = d * d;
        double ps = __builtin_fma(z, -2.50521083854417188e-08, 2.75573192239858907e-06);
        ps = __builtin_fma(ps, z, -1.98412698412698413e-04);
        ps = __builtin_fma(ps, z, 8.33333333333333333e-03);
        ps = __builtin_fma(ps, z, -1.66666666666666667e-01);
        s = __builtin_fma(ps * z, d, d);
        double pc = __builtin_fma(z, 2.08767569878680990e-09, -2.75573192239858907e-07);
        pc = __builtin_fma(pc, z, 2.48015873015873016e-05);
        pc = __builtin_fma(pc, z, -1.38888888888888889e-03);
        pc = __builtin_fma(pc, z, 4.16666666666666667e-02);
        pc = __builtin_fma(pc, z, -0.5);
        c = __builtin_fma(pc, z, 1.0);
    }
    static __device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }
    static constexpr double LARGEST = __DBL_MAX__;
};

// ---------------------------------------------------------------------------------------
// Kerr
// ---------------------------------------------------------------------------------------
// Wave-uniform constants of one render (kernel argument -> SGPRs).
template <typename T> struct KerrConsts {
    T M, a, a2;
    T two_M;
    T r_cut;       // 1.001 r_plus: RHS returns zero at or inside (metrics.py:228-231)
    T r_capture;   // 1.01 r_plus  (metrics.py:579)
    T r_escape;    // 2 r_obs      (metrics.py:580)
    T r_obs, theta_obs;
    T lambda_max;
    T h_max;       // 1.0 (metrics.py:677)
    T rc4, rc2, rc12; // r_capture * 4, * 2, * 1.2 (metrics.py:606-611)
    T eq_lo, eq_hi;   // polar-angle band of the float32 streak's fixed-quadrant loop (kerr_rk4_streak); lo >= hi: never taken
    T unit_lam;       // lambda_max - 1, the range limit of that loop's unit-step form (kerr_rk4_streak); -inf: never taken
};

// A stream of nothing but VALU instructions with an SGPR source runs on the half-rate pipe on gfx950 (v_fma_f32 with
// an SGPR operand: 4.1 issue cycles against 2.2; tools/issue_probe.py), which is why the constants the right-hand
// side multiplies with are copied into VGPRs once per kernel; the empty asm makes the compiler forget that they are
// wave-uniform.  Interleaved one by one among plain FMAs the same instructions issue at full rate, and the SIMD holds
// a higher clock than on three-register FMAs alone: measured in k_kerr_direct<float, Rk4<float>> (48 v_fma_f32 and
// 16 v_fmac_f32 of its 521-instruction loop read a, a^2 or 2M), leaving all three in SGPRs is 1.2 % faster than
// copying them, a^2 alone 0.9 %, a 0.2 % and 2M 0.3 % (profiles/const_operands_ab.txt).
// Which of the three a kernel copies is therefore its own choice, one bit per constant: pin_consts<PIN_A | PIN_2M>
// leaves a^2 in its SGPR.  Every kernel pins all three (the default) unless it says otherwise where it calls this;
// the one that does is the plain float32 RK4 frame kernel (DirectPin, lt_kernels.hpp), the one that was measured.
enum : unsigned { PIN_NONE = 0u, PIN_A = 1u, PIN_A2 = 2u, PIN_2M = 4u, PIN_ALL = 7u };
template <unsigned PIN = PIN_ALL, typename T> __device__ __forceinline__ void pin_consts(KerrConsts<T> &k)
{
    // (all three in ONE statement, as before the mask existed: it keeps every all-pinning kernel's code byte for byte)
    if constexpr (PIN == PIN_ALL) asm volatile("" : "+v"(k.a), "+v"(k.a2), "+v"(k.two_M));
    else {
        if constexpr ((PIN & PIN_A) != 0) asm volatile("" : "+v"(k.a));
        if constexpr ((PIN & PIN_A2) != 0) asm volatile("" : "+v"(k.a2));
        if constexpr ((PIN & PIN_2M) != 0) asm volatile("" : "+v"(k.two_M));
    }
}

// Per-ray constants: the conserved p_phi = L (p_t = -1 throughout, metrics.py:187), what follows
// from it, and the ray's step-size table (axis-refine rays use tighter caps, metrics.py:591-611).
template <typename T> struct RayConsts {
    T L;
    T c_P;   // a^2 - a L   ->  P = r^2 + c_P        (P = (r^2 + a^2) E - a L, E = 1)
    T c_W;   // -2 a L      ->  W = L^2/s2 + c_W + a^2 s2
    T hb;        // base step: h_max, or min(h_max, 0.5) on axis-refine rays (metrics.py:591-593)
    bool refine; // axis-refine ray: tighter radius-band caps and retry floor
};

template <typename T>
__device__ __forceinline__ RayConsts<T> make_ray_consts(const KerrConsts<T> &k, T L, bool refine)
{
    RayConsts<T> rc;
    rc.L = L;
    rc.c_P = M<T>::fma(-k.a, L, k.a2);
    rc.c_W = T(-2) * k.a * L;
    rc.hb = refine ? M<T>::min(k.h_max, T(0.5)) : k.h_max;
    rc.refine = refine;
    return rc;
}

// Hamilton's equations for H = 1/2 g^{mu nu} p_mu p_nu in Boyer-Lindquist coordinates, reduced
// 5-D state (r, theta, phi, p_r, p_theta); the function the reference spends >95 % of its time in
// (metrics.py:221-303).  With E = -p_t = 1:
//     2 Sigma H = F = Delta p_r^2 + p_theta^2 + W(theta) - P(r)^2 / Delta,
//     W = L^2/sin^2 - 2 a L + a^2 sin^2,   P = r^2 + a^2 - a L,
// so dx/dlambda = dH/dp and dp/dlambda = -dH/dx = -(F_x - 2H Sigma_x) / (2 Sigma).  The 2H term is
// zero on a null geodesic but is kept: the reference differentiates the full H, and integration
// error drives H slightly off zero.  The three reciprocals 1/Sigma, 1/Delta, 1/sin^2 come from ONE
// hardware reciprocal of their product.  At or inside r_cut the reference returns zeros
// (metrics.py:228-231): every output carries the factor 1/Sigma, so masking that one factor (and
// evaluating at max(r, r_cut) so nothing overflows) does it.
//
// CHECKED = false leaves the r <= r_cut handling out: for callers that know, or verify afterwards, that
// the radius is outside (kerr_rk4_step_fast below).  Arithmetic otherwise identical.
//
// The three velocities are products -- dr = Delta (p_r / Sigma), dtheta = p_theta / Sigma, dphi = (1 / Sigma) u -- and the
// last stage of an RK4 step adds them to a running sum: the compiler (-ffp-contract=fast) fuses that product and sum,
// for the stage whose result has no other use.  kerr_rhs_parts hands out the factors so that the step can write that
// fma itself (kerr_rk4_step_impl): the rounding then no longer depends on what a compiler decides to fuse, and the
// packed form of the step (kerr_rk4_step_fast_pk) can be made to round identically.
template <typename T> struct KerrRhsParts {
    T Delta, iSpr; // dr = Delta * iSpr
    T iS;          // dtheta = p_theta * iS
    T u;           // dphi = iS * u
    T dpr, dpth;
};

template <typename T, bool CHECKED = true>
__device__ __forceinline__ KerrRhsParts<T> kerr_rhs_parts(const KerrConsts<T> &k, const RayConsts<T> &rc, T r_in, T s, T c, T pr, T pth)
{
    bool inside = CHECKED && r_in <= k.r_cut;
    const bool any_inside = CHECKED && wave_any(inside); // almost never: only a stage of the last steps before capture
    T r = r_in;
    if (__builtin_expect(any_inside, 0)) r = inside ? k.r_cut : r_in;
    T s2 = M<T>::sin2_floor(s);
    // (explicit fma, not r * r + a2 / L * is2 - a below: under -ffp-contract=fast the compiler decides per template
    // instantiation whether to fuse such an expression, and the checked and the branch-free variant of this function
    // must round identically -- found in round 2 when a variant that let unflagged lanes keep the checked step's
    // result differed from the other schedule in 41 of 4.2 M pixels by one ulp)
    T ra = M<T>::fma(r, r, k.a2);
    T Sigma = M<T>::fma(-k.a2, s2, ra);          // r^2 + a^2 cos^2 as r^2 + a^2 - a^2 sin^2 (the 1e-15 floor is far below an ulp)
    T Delta = M<T>::fma(-k.two_M, r, ra);
    // float64: r (r - 2M) + a^2 instead.  Delta above carries the rounding of ra, u (r^2 + a^2), which just outside the horizon
    // of a fast hole is (r^2 + a^2 + 2 M r) / Delta = 30 ... 1000 ulps of Delta itself, and every quotient P / Delta inherits
    // it; r - 2M is exact for M <= r <= 4M, so this form rounds Delta once.  One step from r = 1.3 ... 4 r_plus at
    // a = 0.998 went from 12.9 to under 8 units of tests/step_blocks.py.  The float32 forms keep the two-fma chain (one
    // instruction fewer in the issue-bound kernel, and their step stays inside the same bound: 2.9).
    if constexpr (sizeof(T) == 8) Delta = M<T>::fma(r, r - k.two_M, k.a2);
    T SD = Sigma * Delta;
    T t = M<T>::rcp_pos(SD * s2); // > 0: r >= r_cut > r_plus so Delta > 0, Sigma > 0, s2 >= 1e-15
    T iS = (Delta * s2) * t;
    T iD = (Sigma * s2) * t;
    T is2 = SD * t;
    if (__builtin_expect(any_inside, 0)) iS = inside ? T(0) : iS;
    T P = M<T>::fma(r, r, rc.c_P);
    T q = P * iD;
    T Lis2 = rc.L * is2;
    T pr2 = pr * pr;
    KerrRhsParts<T> o;
    o.Delta = Delta;
    o.iSpr = iS * pr;
    o.iS = iS;
    o.u = M<T>::fma(k.a, q, M<T>::fma(rc.L, is2, -k.a));
    // (dropping the 2H terms -- zero on a null geodesic -- would save instructions, but the reference's RK4
    // solution drifts off-shell at h = 1 and they matter: measured median |d final_alpha| 5.6e-6 without them
    // against 4.4e-7 with them, and p99 1e-1 against 2e-5)
    T W = M<T>::fma(rc.L, Lis2, M<T>::fma(k.a2, s2, rc.c_W));
    T F = M<T>::fma(Delta, pr2, M<T>::fma(pth, pth, M<T>::fma(-P, q, W)));
    T H2 = F * iS;
    // dp_r = -(F_r - 2H Sigma_r) / (2 Sigma) with F_r = (2r - 2M)(q^2 + p_r^2) - 4 r q, Sigma_r = 2r; the factor
    // 1/2 goes into the bracket:  -(1/Sigma) [ (r - M)(q^2 + p_r^2) - r (2q + 2H) ]
    T rt = r * M<T>::fma(T(2), q, H2);
    o.dpr = -iS * M<T>::fma(r - k.M, M<T>::fma(q, q, pr2), -rt);
    // dp_theta likewise: F_theta = 2 s c (a^2 - L^2/s^4), Sigma_theta = -2 a^2 s c:  -(1/Sigma) s c [a^2 (1 + 2H) - (L/s^2)^2]
    o.dpth = -iS * ((s * c) * M<T>::fma(H2, k.a2, M<T>::fma(-Lis2, Lis2, k.a2)));
    return o;
}

template <typename T, bool CHECKED = true>
__device__ __forceinline__ void kerr_rhs_sc(const KerrConsts<T> &k, const RayConsts<T> &rc, T r_in, T s, T c, T pr, T pth,
                                            T &dr, T &dth, T &dph, T &dpr, T &dpth)
{
    const KerrRhsParts<T> o = kerr_rhs_parts<T, CHECKED>(k, rc, r_in, s, c, pr, pth);
    dr = o.Delta * o.iSpr;
    dth = pth * o.iS;
    dph = o.iS * o.u;
    dpr = o.dpr;
    dpth = o.dpth;
}

template <typename T>
__device__ __forceinline__ void kerr_rhs(const KerrConsts<T> &k, const RayConsts<T> &rc, T r, T th, T pr, T pth,
                                         T &dr, T &dth, T &dph, T &dpr, T &dpth)
{
    T s, c;
    M<T>::sincos(th, s, c);
    kerr_rhs_sc(k, rc, r, s, c, pr, pth, dr, dth, dph, dpr, dpth);
}

// x^(-1/5) for the float64 step controllers (dense tracks: err^(-1/5), where solve_ivp's own libm differs from ours in
// the last bits too; DP45 with the reference's controller: err_norm^(-0.2)).  A float32 seed from the hardware log2 / exp2 (relative error ~1e-6) and two Newton steps on
// y^-5 = x,  y <- y + y (1 - x y^5) / 5  (quadratic: 1e-6 -> 3e-12 -> 1e-22, then the rounding of the evaluation,
// ~1 ulp): 18 instructions where exp2(-0.2 log2(x)) in float64 library code takes ~110.  Outside [1e-6, 1e4] the
// controller clamps the factor anyway (0.9 y > 10, or < 0.2), so any value on the right side of the clamp does; a NaN
// comes out as a NaN, as before.
__device__ __forceinline__ double pow_m02(double x)
{
    const float xf = (float)x;
    double y = (double)__builtin_amdgcn_exp2f(-0.2f * __builtin_amdgcn_logf(xf));
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double y2 = y * y, y5 = (y2 * y2) * y;
        y = __builtin_fma(y, 0.2 * __builtin_fma(-x, y5, 1.0), y);
    }
    y = x < 1e-6 ? 100.0 : y;
    y = x > 1e4 ? 0.1 : y;
    return y;
}

// sin and cos of th0 + d from (s0, c0) = sincos(th0): the stage states of a Runge-Kutta step differ from
// the step's base state by h * (a small angular velocity), so the 25-instruction argument reduction +
// polynomials shrink to an 11-instruction rotation.  The wave falls back to the full evaluation in the
// rare step where some lane's |d| exceeds 0.25 rad (wave-uniform branch).
template <typename T, bool CHECKED = true>
__device__ __forceinline__ void sincos_shift(T th0, T s0, T c0, T d, T &s, T &c)
{
    T sd, cd;
    M<T>::sincos_small(d, sd, cd);
    s = M<T>::fma(s0, cd, c0 * sd);
    c = M<T>::fma(c0, cd, -(s0 * sd));
    bool big = CHECKED && M<T>::abs(d) > T(0.25);
    if (__builtin_expect(CHECKED && wave_any(big), 0)) {
        // which formula a lane uses depends on ITS angle only, never on its neighbours: results stay
        // bit-identical however rays are grouped into waves (direct vs queue schedule, partitions)
        T sf, cf;
        M<T>::sincos(th0 + d, sf, cf);
        s = big ? sf : s;
        c = big ? cf : c;
    }
}

template <typename T> struct State5 {
    T r, th, ph, pr, pth;
};

// Classic RK4 step, metrics.py:306-323 (phi does not enter the right-hand side, so the stage states
// carry only r, theta, p_r, p_theta).
//
// CHECKED = true: every stage handles r <= r_cut and a stage angle offset beyond 0.25 rad on the spot (one
// wave-uniform branch each: seven per step).  CHECKED = false: no such branches; the step reports the
// smallest stage radius and the largest stage offset instead, so that the caller can tell afterwards
// whether either case occurred (then the unchecked result is wrong for that lane and must be replaced by
// the checked one) -- one test per step instead of seven, for the same results.
//
// Q1 = true: the caller knows that y.th reduces to the quadrant k = 1 (M<T>::sincos_q1); same bits, fewer instructions.
//
// UNIT = true: the caller knows that h == 1 in every lane (the `h` passed is not read).  h / 2 and h / 6 are then
// literals of the instructions instead of per-lane registers -- T(0.5) * T(1) is 0.5 and T(1) * T(1.0 / 6.0) is
// T(1.0 / 6.0), both exactly, so they are the multipliers of the general form at h = 1 -- and stage 4 needs no multiply at all: fma(1, k, y) is
// k + y rounded once, and d4 = 1 * k_th is k_th.  Same bits, one instruction fewer, and fourteen three-register fmas
// become the literal form.  The one trap is stage 4's radius: k_r is the ROUNDED product Delta * iSpr there (it also
// feeds the running sum), and under -ffp-contract=fast a plain k_r + y.r is compiled as fma(Delta, iSpr, y.r); the
// product goes through `unfused` first.  (k_pr and k_pth end in a product as well -- -iS * (...) -- same treatment.)
template <typename T, bool CHECKED, bool Q1 = false, bool UNIT = false>
__device__ __forceinline__ State5<T> kerr_rk4_step_impl(const KerrConsts<T> &k, const RayConsts<T> &rc,
                                                        const State5<T> &y, T h_in, T &min_r, T &max_d)
{
    static_assert(!UNIT || sizeof(T) == 4, "the unit-step form is float32 only");
    const T h = UNIT ? T(1) : h_in;
    T k_r, k_th, k_ph, k_pr, k_pth;
    T a_r, a_th, a_ph, a_pr, a_pth; // running k1 + 2 k2 + 2 k3 + k4
    T s0, c0, s, c;
    // the only full sincos of the step; stages rotate it (sincos_shift)
    if constexpr (Q1) M<T>::sincos_q1(y.th, s0, c0);
    else M<T>::sincos(y.th, s0, c0);
    kerr_rhs_sc<T, CHECKED>(k, rc, y.r, s0, c0, y.pr, y.pth, k_r, k_th, k_ph, k_pr, k_pth);
    a_r = k_r; a_th = k_th; a_ph = k_ph; a_pr = k_pr; a_pth = k_pth;
    T hh = T(0.5) * h;
    T t_r = M<T>::fma(hh, k_r, y.r), t_pr = M<T>::fma(hh, k_pr, y.pr), t_pth = M<T>::fma(hh, k_pth, y.pth);
    T d2 = hh * k_th;
    T r2 = t_r;
    sincos_shift<T, CHECKED>(y.th, s0, c0, d2, s, c);
    kerr_rhs_sc<T, CHECKED>(k, rc, t_r, s, c, t_pr, t_pth, k_r, k_th, k_ph, k_pr, k_pth);
    a_r = M<T>::fma(T(2), k_r, a_r); a_th = M<T>::fma(T(2), k_th, a_th); a_ph = M<T>::fma(T(2), k_ph, a_ph);
    a_pr = M<T>::fma(T(2), k_pr, a_pr); a_pth = M<T>::fma(T(2), k_pth, a_pth);
    t_r = M<T>::fma(hh, k_r, y.r); t_pr = M<T>::fma(hh, k_pr, y.pr); t_pth = M<T>::fma(hh, k_pth, y.pth);
    T d3 = hh * k_th;
    T r3 = t_r;
    sincos_shift<T, CHECKED>(y.th, s0, c0, d3, s, c);
    kerr_rhs_sc<T, CHECKED>(k, rc, t_r, s, c, t_pr, t_pth, k_r, k_th, k_ph, k_pr, k_pth);
    if constexpr (UNIT) { k_r = unfused(k_r); k_pr = unfused(k_pr); k_pth = unfused(k_pth); } // (before their first use: no copy)
    a_r = M<T>::fma(T(2), k_r, a_r); a_th = M<T>::fma(T(2), k_th, a_th); a_ph = M<T>::fma(T(2), k_ph, a_ph);
    a_pr = M<T>::fma(T(2), k_pr, a_pr); a_pth = M<T>::fma(T(2), k_pth, a_pth);
    T d4;
    if constexpr (UNIT) {
        t_r = k_r + y.r; t_pr = k_pr + y.pr; t_pth = k_pth + y.pth;
        d4 = k_th;
    } else {
        t_r = M<T>::fma(h, k_r, y.r); t_pr = M<T>::fma(h, k_pr, y.pr); t_pth = M<T>::fma(h, k_pth, y.pth);
        d4 = h * k_th;
    }
    sincos_shift<T, CHECKED>(y.th, s0, c0, d4, s, c);
    const KerrRhsParts<T> k4 = kerr_rhs_parts<T, CHECKED>(k, rc, t_r, s, c, t_pr, t_pth);
    if (!CHECKED) {
        // (a NaN stage value is ignored by min / max; it makes the step's result non-finite in either variant)
        min_r = M<T>::min(M<T>::min(r2, r3), t_r);
        max_d = M<T>::max(M<T>::max(M<T>::abs(d2), M<T>::abs(d3)), M<T>::abs(d4));
    }
    T h6 = h * T(1.0 / 6.0);
    State5<T> o;
    // (k1 + 2 k2 + 2 k3) + k4 with the velocity products of the last stage fused into the sum, see kerr_rhs_parts
    o.r = M<T>::fma(h6, M<T>::fma(k4.Delta, k4.iSpr, a_r), y.r);
    o.th = M<T>::fma(h6, M<T>::fma(t_pth, k4.iS, a_th), y.th);
    o.ph = M<T>::fma(h6, M<T>::fma(k4.iS, k4.u, a_ph), y.ph);
    o.pr = M<T>::fma(h6, a_pr + k4.dpr, y.pr);
    o.pth = M<T>::fma(h6, a_pth + k4.dpth, y.pth);
    return o;
}

template <typename T>
__device__ __forceinline__ State5<T> kerr_rk4_step(const KerrConsts<T> &k, const RayConsts<T> &rc,
                                                   const State5<T> &y, T h)
{
    T unused_r, unused_d;
    return kerr_rk4_step_impl<T, true>(k, rc, y, h, unused_r, unused_d);
}

// The branch-free variant; valid for a lane iff min_r > k.r_cut and max_d <= 0.25 (kerr_rk4_step_ok).
template <typename T, bool Q1 = false, bool UNIT = false>
__device__ __forceinline__ State5<T> kerr_rk4_step_fast(const KerrConsts<T> &k, const RayConsts<T> &rc,
                                                        const State5<T> &y, T h, T &min_r, T &max_d)
{
    return kerr_rk4_step_impl<T, false, Q1, UNIT>(k, rc, y, h, min_r, max_d);
}

// ---------------------------------------------------------------------------------------
// The same step for a wavefront that is ALONE on its SIMD (the last waves of a launch, hosting the few very long
// rays; k_kerr_direct's ghost-lane phase).  Such a wave issues one instruction per ~4.8 cycles whatever the
// instruction is (tools/issue_probe.py), and a packed v_pk_fma_f32 / v_pk_mul_f32 -- two float32 operations on a
// 64-bit register pair, each half of each source chosen by op_sel -- costs it 5.3: wherever two operations of the
// step take their operands from the same pairs they share one issue slot.  (With two or more waves per SIMD a
// packed instruction costs two issue slots and this form gains nothing: the bulk keeps the scalar step.)
// Every operation below is one of the scalar step's, with the same operands: a product x * y is written
// fma(x, y, -0) where its slot-mate is an fma -- identical bits, including the sign of a zero product -- so the
// result is bit-identical to kerr_rk4_step_fast (tests/test_gpu_ghost_lanes.py runs whole frames through either).
// Pairs: [ps, pc] polynomials of the stage rotation, [s, c], [s^2, s c], [r^2 + a^2, P], [Sigma, Delta] s^2 -> [1/Delta, 1/Sigma]
// after the one reciprocal, [L/s^2, .], [p_r/Sigma, dtheta], [dphi, 2H], [dp_r, dp_theta], and the RK4 bookkeeping of
// the (r, theta) and (p_r, p_theta) components.
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct PkStage {
    float dr, dth, dph; // LAST: unset
    f32x2 dp;           // [dp_r, dp_theta]
    float Delta, iSpr, iS, u; // LAST only: the factors of dr, dtheta, dphi (KerrRhsParts)
};

__device__ __forceinline__ f32x2 pk_bc(float x) { return (f32x2){x, x}; }
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// right-hand side at (r, [sin, cos], [p_r, p_theta]); kerr_rhs_sc<float, false>, LAST: kerr_rhs_parts<float, false>
template <bool LAST = false>
__device__ __forceinline__ PkStage kerr_rhs_pk(const KerrConsts<float> &k, const RayConsts<float> &rc, float r, f32x2 sc, f32x2 p)
{
#pragma clang fp contract(off)
    PkStage o;
    const f32x2 s2sc = pk_fma(pk_bc(sc.x), sc, (f32x2){1e-15f, -0.0f});          // [s^2 + 1e-15, s c]
    const float s2 = s2sc.x;
    const f32x2 raP = pk_fma(pk_bc(r), pk_bc(r), (f32x2){k.a2, rc.c_P});        // [r^2 + a^2, P]
    const float ra = raP.x, P = raP.y;
    const float Sigma = __builtin_fmaf(-k.a2, s2, ra);
    const float Delta = __builtin_fmaf(-k.two_M, r, ra);
    const f32x2 SDs2 = (f32x2){Sigma, Delta} * pk_bc(s2);                       // [Sigma s^2, Delta s^2]
    const float SD = Sigma * Delta;
    const float t = M<float>::rcp_pos(SD * s2);
    const f32x2 inv = SDs2 * pk_bc(t);                                          // [1/Delta, 1/Sigma]
    const float iD = inv.x, iS = inv.y;
    const float is2 = SD * t;
    const f32x2 Lu = pk_fma(pk_bc(rc.L), pk_bc(is2), (f32x2){-0.0f, -k.a});     // [L / s^2, L / s^2 - a]
    const float Lis2 = Lu.x;
    const float q = P * iD;
    const float pr2 = p.x * p.x;
    const float u2 = __builtin_fmaf(k.a, q, Lu.y);
    const float W = __builtin_fmaf(rc.L, Lis2, __builtin_fmaf(k.a2, s2, rc.c_W));
    const float F = __builtin_fmaf(Delta, pr2, __builtin_fmaf(p.y, p.y, __builtin_fmaf(-P, q, W)));
    float H2;
    if (LAST) {
        o.Delta = Delta; o.iSpr = iS * p.x; o.iS = iS; o.u = u2;
        H2 = F * iS;
    } else {
        const f32x2 ip = pk_bc(iS) * p;                                         // [p_r / Sigma, p_theta / Sigma]
        o.dr = Delta * ip.x;
        o.dth = ip.y;
        const f32x2 dphH = pk_bc(iS) * (f32x2){u2, F};                          // [dphi, 2H]
        o.dph = dphH.x;
        H2 = dphH.y;
    }
    const float rt = r * __builtin_fmaf(2.0f, q, H2);
    const float b = __builtin_fmaf(r - k.M, __builtin_fmaf(q, q, pr2), -rt);
    const float m2 = __builtin_fmaf(H2, k.a2, __builtin_fmaf(-Lis2, Lis2, k.a2));
    const float scm = s2sc.y * m2;
    o.dp = pk_bc(-iS) * (f32x2){b, scm};                                        // [dp_r, dp_theta]
    return o;
}

// [sin, cos] of th0 + d from cs0 = [cos, sin](th0); sincos_shift<float, false>
__device__ __forceinline__ f32x2 sincos_shift_pk(f32x2 cs0, float d)
{
#pragma clang fp contract(off)
    const float z = d * d;
    f32x2 pp = pk_fma(pk_bc(z), (f32x2){8.3333333333e-3f, -1.3888888889e-3f}, (f32x2){-1.6666666667e-1f, 4.1666666667e-2f});
    pp = pk_fma(pp, pk_bc(z), (f32x2){-0.0f, -0.5f});                            // [ps z, pc]
    const float sd = __builtin_fmaf(pp.x, d, d);
    const float cd = __builtin_fmaf(pp.y, z, 1.0f);
    const f32x2 x = pk_bc(sd) * cs0;                                            // [c0 sd, s0 sd]
    return pk_fma(__builtin_shufflevector(cs0, cs0, 1, 0), pk_bc(cd), (f32x2){x.x, -x.y}); // [s0 cd + c0 sd, c0 cd - s0 sd]
}

// cs0 = [cos, sin](y.th) comes in and [cos, sin] of the new polar angle goes out: the argument reduction of the NEXT
// step's base angle depends on nothing but o.th, which is ready well before the last stage's momenta are, so written
// here the scheduler can run it beside the tail of the last right-hand side instead of at the head of the next step,
// where everything waits for it (a lone wave is bound by the depth of its dependence chains).
__device__ __forceinline__ State5<float> kerr_rk4_step_fast_pk(const KerrConsts<float> &k, const RayConsts<float> &rc,
                                                               const State5<float> &y, f32x2 cs0, float h, float &min_r,
                                                               float &max_d, f32x2 &cs_out)
{
#pragma clang fp contract(off)
    const float s0 = cs0.y, c0 = cs0.x;
    const f32x2 yp = {y.pr, y.pth}, yrt = {y.r, y.th};
    PkStage g = kerr_rhs_pk(k, rc, y.r, (f32x2){s0, c0}, yp);
    f32x2 a_rt = {g.dr, g.dth}, a_p = g.dp; // running k1 + 2 k2 + 2 k3 + k4
    float a_ph = g.dph;
    const float hh = 0.5f * h;
    float t_r = __builtin_fmaf(hh, g.dr, y.r);
    f32x2 t_p = pk_fma(pk_bc(hh), g.dp, yp);
    const float d2 = hh * g.dth;
    const float r2 = t_r;
    g = kerr_rhs_pk(k, rc, t_r, sincos_shift_pk(cs0, d2), t_p);
    a_rt = pk_fma(pk_bc(2.0f), (f32x2){g.dr, g.dth}, a_rt);
    a_ph = __builtin_fmaf(2.0f, g.dph, a_ph);
    a_p = pk_fma(pk_bc(2.0f), g.dp, a_p);
    t_r = __builtin_fmaf(hh, g.dr, y.r);
    t_p = pk_fma(pk_bc(hh), g.dp, yp);
    const float d3 = hh * g.dth;
    const float r3 = t_r;
    g = kerr_rhs_pk(k, rc, t_r, sincos_shift_pk(cs0, d3), t_p);
    a_rt = pk_fma(pk_bc(2.0f), (f32x2){g.dr, g.dth}, a_rt);
    a_ph = __builtin_fmaf(2.0f, g.dph, a_ph);
    a_p = pk_fma(pk_bc(2.0f), g.dp, a_p);
    t_r = __builtin_fmaf(h, g.dr, y.r);
    t_p = pk_fma(pk_bc(h), g.dp, yp);
    const float d4 = h * g.dth;
    g = kerr_rhs_pk<true>(k, rc, t_r, sincos_shift_pk(cs0, d4), t_p);
    min_r = __builtin_fminf(__builtin_fminf(r2, r3), t_r);
    max_d = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(d2), __builtin_fabsf(d3)), __builtin_fabsf(d4));
    const float h6 = h * float(1.0 / 6.0);
    // the last stage's velocities enter the sums as fused products, as in kerr_rk4_step_impl
    const f32x2 sum_rt = pk_fma((f32x2){g.Delta, t_p.y}, (f32x2){g.iSpr, g.iS}, a_rt);
    const f32x2 o_rt = pk_fma(pk_bc(h6), sum_rt, yrt);
    const f32x2 o_p = pk_fma(pk_bc(h6), a_p + g.dp, yp);
    State5<float> o;
    o.r = o_rt.x; o.th = o_rt.y;
    {
        float sn, cn;
        M<float>::sincos(o.th, sn, cn);
        asm volatile("" : "+v"(sn), "+v"(cn)); // (pins the evaluation to this step: the compiler would sink it to its use, the head of the next one)
        cs_out = (f32x2){cn, sn};
    }
    o.ph = __builtin_fmaf(h6, __builtin_fmaf(g.iS, g.u, a_ph), y.ph);
    o.pr = o_p.x; o.pth = o_p.y;
    return o;
}

// What a streak carries from one step to the next besides the state: nothing, or (packed step) [cos, sin] of the polar angle
template <typename T, bool LONE> struct StepCarry {
    __device__ __forceinline__ void init(T) {}
};
template <> struct StepCarry<float, true> {
    f32x2 cs;
    __device__ __forceinline__ void init(float th)
    {
        float s, c;
        M<float>::sincos(th, s, c);
        cs = (f32x2){c, s};
    }
};

// LONE = true: the packed form where there is one (float32); the scalar step otherwise (Q1: its fixed-quadrant form,
// UNIT: its unit-step form)
template <typename T, bool LONE, bool Q1 = false, bool UNIT = false>
__device__ __forceinline__ State5<T> kerr_rk4_step_fast_for(const KerrConsts<T> &k, const RayConsts<T> &rc, const State5<T> &y,
                                                            const StepCarry<T, LONE> &cin, T h, T &min_r, T &max_d,
                                                            StepCarry<T, LONE> &cout)
{
    if constexpr (LONE && sizeof(T) == 4) return kerr_rk4_step_fast_pk(k, rc, y, cin.cs, h, min_r, max_d, cout.cs);
    else return kerr_rk4_step_fast<T, Q1, UNIT>(k, rc, y, h, min_r, max_d);
}

// Step-size rule of the reference's fixed-step RK4 tracer (metrics.py:597-611): h_base, capped in
// three radius bands around the capture radius (tighter caps on axis-refine rays) and by the
// remaining affine range.  Rays spend most of their steps far outside the outermost band
// (r >= 4 r_capture), and a wavefront is an 8x8 pixel tile, so whether ANY lane is inside is decided
// per wave and the band cascade is skipped otherwise.
template <typename T>
__device__ __forceinline__ T kerr_rk4_h(const KerrConsts<T> &k, const RayConsts<T> &rc, T r, T remaining)
{
    T h = rc.hb;
    if (wave_any(r < k.rc4)) {
        T c4 = rc.refine ? T(0.20) : T(0.25), c2 = rc.refine ? T(0.08) : T(0.10), c12 = rc.refine ? T(0.03) : T(0.05);
        h = (r < k.rc4) ? M<T>::min(h, c4) : h;
        h = (r < k.rc2) ? M<T>::min(h, c2) : h;
        h = (r < k.rc12) ? M<T>::min(h, c12) : h;
    }
    return M<T>::min(h, remaining);
}

// Event codes carried from the integrate kernel to the epilogue.
enum : int { EV_MAXRANGE = 2, EV_ESCAPED = 1, EV_CAPTURED = -1, EV_INVALID = 0, EV_PAD = 3, EV_RUNNING = 4 };

// Everything one ray carries between steps (registers).
template <typename T> struct RayState {
    State5<T> y;
    T lam;       // affine parameter so far
    T h_retry;   // > 0: retry the step with this (halved) h, metrics.py:615-626
    uint32_t steps;
};

template <typename T> __device__ __forceinline__ void ray_start(const KerrConsts<T> &k, RayState<T> &s, T p_r, T p_th)
{
    s.y.r = k.r_obs; s.y.th = k.theta_obs; s.y.ph = T(0); s.y.pr = p_r; s.y.pth = p_th;
    s.lam = T(0); s.h_retry = T(0); s.steps = 0;
}

// A streak of ordinary far-field steps.  While EVERY active lane of the wave is outside 4 r_capture with
// nothing to retry, the tracer's loop body (metrics.py:596-655) reduces to: h = min(h_base, remaining), one
// RK4 step, accept.  This loop does exactly that with ONE wave-uniform branch per step -- the predicate
// `good` says that the step was ordinary and that the lane is still in the far field afterwards -- where
// the general iteration below (kerr_rk4_advance) spends four.  Bulk waves take ~60 % of their steps here;
// for a wave hosting one of the few very long rays, alone on its SIMD at the end of the launch, a taken
// branch costs ~80 cycles, so this is what sets the length of the launch's tail.
// A lane for which `good` fails keeps its state (the general iteration redoes that step); lanes for which
// it holds keep the step -- lanes are independent, they need not stay in lockstep.  Same arithmetic as the
// general iteration (kerr_rk4_step_fast, same h), so which of the two paths took a step does not matter.
// Returns the number of loop iterations (wave-uniform).  LONE: the wave is alone on its SIMD (packed step, above).
//
// The loop exists twice.  The camera of a frame sits on or near the equator by default and a ray's polar angle stays
// within its orbital plane's inclination of pi/2, so most far-field steps start with every lane's angle inside
// (pi/4, 3 pi/4), where the step's one full sincos needs neither its quadrant logic nor the multiply and rint that
// find the quadrant (M<float>::sincos_q1: 14 instructions for 28, same bits).  Which loop runs is decided ONCE per
// call, on the state the streak starts from: if every active lane's angle is inside (k.eq_lo, k.eq_hi), the
// fixed-quadrant loop (EQ) runs, and `angle still inside the band` joins its continue condition -- tested on the NEW
// angle, which is the next step's base angle.  Nothing inside a step branches on it.  A lane whose step was ordinary
// but left the band keeps the step like any other (the selects on leaving look at `good` alone), and the call goes on
// in the general loop with what is left of max_steps: the wave takes the same attempts in the same order as with the
// band empty (k.eq_lo >= k.eq_hi: the switch, lt_set_eq_streak), each lane through the same arithmetic with the same
// h, so no output and no counter but `eq_done` can tell the two loops apart.  Float32, scalar step only: float64 and
// the packed lone-wave step run the general loop.
// `eq_done` += the attempts made in the fixed-quadrant loop (wave-uniform).

// The loop itself.  EQ: the fixed-quadrant form.  `done` counts attempts.  True if the loop left before max_steps
// attempts although every lane's last attempt was ordinary (EQ: some lane left the band; never without EQ).
//
// The per-step test is lane masks, not a per-lane bool: each compare of `good` goes into a ballot of its own, the masks
// are ANDed and compared with the active lanes' on the scalar unit, and only the code after the loop turns the mask back
// into a lane predicate for the keep/discard selects (lane_pred: no instruction).
// Finiteness is tested on the components that no range test of the same mask covers.  The old test was
//     F5 = finite(|r| + |th| + |ph| + |p_r| + |p_th|)   (summed left to right).
// A lane whose mask bit is set has rc4 <= r < r_escape, so r is finite, and -- a few hundred against 3.4e38 -- cannot
// move an overflow of the sum: it changes a partial sum only below 2^31, and through three more roundings, each of
// which can widen a one-ulp difference by 2^24 at most, that stays below 2^103, half an ulp of the largest float
// (float64: the same with its exponents).  So the general loop sums |th| + |ph| + |p_r| + |p_th|.  In the EQ loop the
// continue condition also holds the new angle inside the band, |th| < 2.4, and the same argument drops it from the
// sum: (mask & band) is (good & band) of the old test for every input.  `good` ALONE, which the selects and the
// return value use, is not: an angle outside the band may be huge or not a number.  On leaving the EQ loop -- once per
// call -- the old F5 itself is therefore ANDed into the lane's predicate (F5 implies the shorter sum finite: rounding
// is monotonic and every term is >= 0).  tests/test_streak_predicate_host.py holds both forms to the old predicate on
// a grid of edge values.
//
// UNIT (with EQ only): the form for a call in which every active lane steps by exactly 1 and none can come within a
// step of the range end -- kerr_rk4_streak decides both once per call and says why they hold for all of it.  The step
// takes its unit form (kerr_rk4_step_impl), lam advances by the literal, and `lam <= lam_limit` leaves the test: it
// is true on every attempt of such a call.  Nothing else differs, so neither an output nor a counter can tell.
template <typename T, bool LONE, bool EQ, bool UNIT = false>
__device__ __forceinline__ bool kerr_rk4_streak_loop(const KerrConsts<T> &k, const RayConsts<T> &rc, RayState<T> &s,
                                                     uint32_t max_steps, uint32_t &done)
{
    // One attempt: from state `from` at affine parameter lam into `to`; the mask of the lanes for which it was an
    // ordinary far-field step (EQ: up to F5, see above).
    // The streak only takes FULL base steps: h = h_base needs remaining >= h_base, i.e. lam <= lambda_max - h_base
    // (the tracer's h = min(h_base, remaining) is then h_base exactly).  A ray within one base step of the range end
    // fails the test and takes its last, shorter step in the general iteration.  With h invariant the step's h / 2 and
    // h / 6, the subtraction and the min leave the loop.
    // in_band: with EQ, the other half of the continue condition -- the new angle is inside the band.
    static_assert(!UNIT || (EQ && !LONE && sizeof(T) == 4), "the unit-step form belongs to the float32 fixed-quadrant loop");
    const T lam_limit = k.lambda_max - rc.hb;
    const uint64_t all = lane_mask(true);
    auto attempt = [&](const State5<T> &from, const StepCarry<T, LONE> &cfrom, T lam, State5<T> &to, StepCarry<T, LONE> &cto, T &h) -> uint64_t {
        h = UNIT ? T(1) : rc.hb;
        T min_r, max_d;
        to = kerr_rk4_step_fast_for<T, LONE, EQ, UNIT>(k, rc, from, cfrom, h, min_r, max_d, cto);
        T mag = (M<T>::abs(to.ph) + M<T>::abs(to.pr)) + M<T>::abs(to.pth);
        if constexpr (!EQ) mag = ((M<T>::abs(to.th) + M<T>::abs(to.ph)) + M<T>::abs(to.pr)) + M<T>::abs(to.pth);
        ++done;
        // (mag >= 0 or NaN: an ordered compare with the largest finite number is the finiteness test)
        return (UNIT ? all : lane_mask(lam <= lam_limit)) & lane_mask(mag <= M<T>::LARGEST) & lane_mask(to.r >= k.rc4) &
               lane_mask(to.r < k.r_escape) & lane_mask(min_r > k.r_cut) & lane_mask(!(max_d > T(0.25)));
    };
    auto in_band = [&](T th) -> uint64_t { return EQ ? lane_mask(th > k.eq_lo) & lane_mask(th < k.eq_hi) : all; };
    // The continue test as one scalar word, zero iff the loop goes on: every lane's bit is set and attempts are left
    // (done < max_steps < 2^31: the sign of the difference).
    auto stop_bits = [&](uint64_t ok) -> uint64_t { return (ok ^ all) | (uint64_t)(((done - max_steps) >> 31) ^ 1u); };
    // The state ping-pongs between two register sets (A = s.y, B) so that accepting an attempt costs no copies:
    // the loop body is two attempts, A -> B and B -> A, each followed by the one wave-uniform test.  On leaving,
    // a lane keeps the attempted state if its own predicate held, its previous state otherwise.  The loop has ONE
    // exit, and `second` says after which half it was taken: the selects are stated once, on (good == second), and
    // lie outside the loop.
    // One exit in the machine code too, which is what keeps the ping-pong free of copies.  Written with a `break` after
    // either attempt -- and equally when the compiler finds out that a failed first test decides the second -- the loop
    // has two exits; the backend then gives it one again by routing the first through a block where the second half's
    // results are formally defined (as undefined), and the register allocator, seeing set A live across that
    // definition, puts the results of B -> A into a third set and copies them to A on the way back: five v_mov per two
    // steps in every form of the loop.  So a failed first test only skips the second attempt, the exit is the one test
    // below it, and the word that carries the first test's outcome there passes through an empty asm, so that nothing
    // can tell the optimiser what it holds.  The hints keep both attempts on the fall-through path.
    // `steps` is settled on leaving: every lane in the loop took every attempt but the last (the loop goes on only
    // while all of them are good), and the lanes in the loop are the same from entry to exit.
    State5<T> b;
    StepCarry<T, LONE> ca, cb;
    ca.init(s.y.th);
    T h;
    const uint32_t before = done;
    uint64_t mask, second; // second: all ones if the loop leaves after its second attempt (B -> A), else zero
    for (;;) {
        mask = attempt(s.y, ca, s.lam, b, cb, h);
        second = 0ull;
        uint64_t stop = stop_bits(mask & in_band(b.th));
        asm volatile("" : "+s"(stop));
        if (__builtin_expect(stop == 0, 1)) {
            s.lam += h;
            mask = attempt(b, cb, s.lam, s.y, ca, h);
            second = ~0ull;
            stop = stop_bits(mask & in_band(s.y.th));
            asm volatile("" : "+s"(stop));
        }
        if (__builtin_expect(stop != 0, 0)) break;
        s.lam += h;
    }
    if constexpr (EQ) { // the lane's own `good`: the mask and F5 of the attempted state
        const bool sec = lane_pred(second);
        State5<T> to;
        to.r = sec ? s.y.r : b.r; to.th = sec ? s.y.th : b.th; to.ph = sec ? s.y.ph : b.ph;
        to.pr = sec ? s.y.pr : b.pr; to.pth = sec ? s.y.pth : b.pth;
        mask &= lane_mask(M<T>::finite(M<T>::abs(to.r) + M<T>::abs(to.th) + M<T>::abs(to.ph) + M<T>::abs(to.pr) + M<T>::abs(to.pth)));
    }
    const bool good = lane_pred(mask);
    const bool keep_a = lane_pred(~(mask ^ second)); // the lane's state is in A: good after B -> A, or not good after A -> B
    s.y.r = keep_a ? s.y.r : b.r; s.y.th = keep_a ? s.y.th : b.th; s.y.ph = keep_a ? s.y.ph : b.ph;
    s.y.pr = keep_a ? s.y.pr : b.pr; s.y.pth = keep_a ? s.y.pth : b.pth;
    s.lam = good ? s.lam + h : s.lam;
    s.steps += (done - before - 1u) + (good ? 1u : 0u);
    return EQ && (mask == all) & (done < max_steps);
}

template <typename T, bool LONE = false>
__device__ __forceinline__ uint32_t kerr_rk4_streak(const KerrConsts<T> &k, const RayConsts<T> &rc, RayState<T> &s,
                                                    uint32_t max_steps, uint32_t &eq_done)
{
    if (wave_any(!((s.y.r >= k.rc4) & (s.h_retry == T(0))))) return 0;
    uint32_t done = 0, eq = 0;
    bool more = true;
    if constexpr (!LONE && sizeof(T) == 4) {
        if ((lane_mask(s.y.th > k.eq_lo) & lane_mask(s.y.th < k.eq_hi)) == lane_mask(true)) {
            // The unit-step form of that loop, chosen here once per call like the band: every active lane's base step
            // is exactly 1 (every ray outside the axis-refine columns at the default h_max), and every lane starts the
            // call at least max_steps + 1 below the loop's range limit lambda_max - 1 (k.unit_lam; -inf: the switch
            // lt_set_unit_streak is off, or lambda_max > 2^13).  Then `lam <= lam_limit` holds on every attempt of the
            // call and the loop need not test it: attempt i <= max_steps - 1 sees lam after i additions of 1, each
            // rounded by at most half an ulp of a number below 2^13, 2^-12, so lam_i <= lam_0 + i (1 + 2^-12); the sum
            // tested below is rounded by 2^-12 at most as well, and lam_0 + max_steps + 1 <= lam_limit + 2^-12 gives
            // lam_i <= lam_limit - 2 + max_steps 2^-12 <= lam_limit - 1 for every max_steps <= 2^12
            // (tests/test_unit_streak_host.py replays the recurrence in float32 on both sides of the threshold).
            // (The margin is added to lam, a literal of that instruction; subtracted from the limit, which is wave-uniform,
            // it would be a register that lives through the whole kernel.)
            const T lam_far = s.lam + T(max_steps + 1u);
            if ((max_steps <= 4096u) & ((lane_mask(rc.hb == T(1)) & lane_mask(lam_far <= k.unit_lam)) == lane_mask(true)))
                more = kerr_rk4_streak_loop<T, LONE, true, true>(k, rc, s, max_steps, done);
            else
                more = kerr_rk4_streak_loop<T, LONE, true>(k, rc, s, max_steps, done);
            eq = done;
        }
    }
    if (more) kerr_rk4_streak_loop<T, LONE, false>(k, rc, s, max_steps, done);
#ifdef LT_EQ_COUNT_ALL // diagnostic build: count EVERY attempt of the scalar float32 streak (the eligible fraction's denominator)
    if constexpr (!LONE && sizeof(T) == 4) eq = done;
#endif
    eq_done += eq;
    return done;
}

// One iteration of the reference's fixed-step RK4 tracer (metrics.py:596-655): choose h, take an RK4
// step, halve-and-retry on a non-finite result, stop on the capture / escape crossing with the
// reference's linear interpolation.  Returns EV_RUNNING or the terminating event.  Both schedules of
// the integrate kernel call exactly this function, so they produce bit-identical results.
//
// Structure: the arithmetic is straight-line; whether every active lane took an ordinary step (no
// retry, no crossing, range not exhausted) is decided ONCE per wave with a ballot, so the hot path
// is one scalar branch instead of a nest of exec-mask regions; the per-lane logic of the rare cases
// sits behind it.
template <typename T>
__device__ __forceinline__ int kerr_rk4_advance(const KerrConsts<T> &k, const RayConsts<T> &rc, RayState<T> &s)
{
    T remaining = k.lambda_max - s.lam;
    T h = kerr_rk4_h(k, rc, s.y.r, remaining);
    if (__builtin_expect(wave_any(s.h_retry > T(0)), 0)) h = (s.h_retry > T(0)) ? s.h_retry : h;
    bool live = remaining > T(0); // then h > 0 too: every candidate for h is positive
    // (a lane whose range is exhausted still computes the step -- at most once per ray -- and drops it)
    T min_r, max_d;
    State5<T> n = kerr_rk4_step_fast(k, rc, s.y, h, min_r, max_d);
    // the branch-free step is wrong for a lane one of whose stages sat at r <= r_cut or turned by more than
    // 0.25 rad (both rare): such a lane takes the checked step below
    // (& and |, not && and ||: short-circuit evaluation would turn these predicates into branches)
    bool redo = (min_r <= k.r_cut) | (max_d > T(0.25));
    // all five components finite <=> the sum of their magnitudes is (NaN and inf both propagate)
    T mag = M<T>::abs(n.r) + M<T>::abs(n.th) + M<T>::abs(n.ph) + M<T>::abs(n.pr) + M<T>::abs(n.pth);
    bool ok = M<T>::finite(mag) & (n.r > T(0));
    // strictly between the capture and the escape radius: neither crossing test of the reference fires
    bool between = (n.r > k.r_capture) & (n.r < k.r_escape);
    bool plain = live & ok & between & !redo;
    if (__builtin_expect(!wave_any(!plain), 1)) {
        s.y = n;
        s.lam += h;
        s.h_retry = T(0);
        ++s.steps;
        return EV_RUNNING;
    }
    if (wave_any(redo)) {
        // per lane: only a flagged lane takes the checked result, so nobody's numbers depend on a neighbour
        State5<T> e = kerr_rk4_step(k, rc, s.y, h);
        n.r = redo ? e.r : n.r; n.th = redo ? e.th : n.th; n.ph = redo ? e.ph : n.ph;
        n.pr = redo ? e.pr : n.pr; n.pth = redo ? e.pth : n.pth;
        mag = M<T>::abs(n.r) + M<T>::abs(n.th) + M<T>::abs(n.ph) + M<T>::abs(n.pr) + M<T>::abs(n.pth);
        ok = M<T>::finite(mag) && n.r > T(0);
    }
    if (!live) return EV_MAXRANGE;
    ++s.steps;
    if (!ok) {
        T h_floor = M<T>::min(rc.refine ? T(0.01) : T(0.02), rc.hb); // metrics.py:594
        if (h <= h_floor) return EV_INVALID;
        s.h_retry = T(0.5) * h;
        return EV_RUNNING;
    }
    s.h_retry = T(0);
    bool cap_first = n.r <= k.r_capture && s.y.r > k.r_capture; // the reference tests capture first
    bool esc = !cap_first && n.r >= k.r_escape && s.y.r < k.r_escape;
    if (cap_first || esc) {
        T target = cap_first ? k.r_capture : k.r_escape;
        T denom = n.r - s.y.r;
        T frac = (denom == T(0)) ? T(1) : (target - s.y.r) / denom;
        frac = M<T>::min(M<T>::max(frac, T(0)), T(1));
        s.y.r = M<T>::fma(frac, n.r - s.y.r, s.y.r);
        s.y.th = M<T>::fma(frac, n.th - s.y.th, s.y.th);
        s.y.ph = M<T>::fma(frac, n.ph - s.y.ph, s.y.ph);
        s.y.pr = M<T>::fma(frac, n.pr - s.y.pr, s.y.pr);
        s.y.pth = M<T>::fma(frac, n.pth - s.y.pth, s.y.pth);
        return cap_first ? EV_CAPTURED : EV_ESCAPED;
    }
    s.y = n;
    s.lam += h;
    return EV_RUNNING;
}

// ---------------------------------------------------------------------------------------
// Schwarzschild orbit equation u'' = -u + 3 M u^2, u = 1/r (metrics.py:44-117)
// ---------------------------------------------------------------------------------------
template <typename T> struct SchwConsts {
    T M, three_M;
    T u0;         // 1 / r_obs
    T u_capture;  // 1 / (1.01 R_S)
    T u_escape;   // 1 / (2 r_obs)
    T h_max, phi_max;
    uint32_t n_full; // full h_max steps of the reference's loop, counted by the host as the reference accumulates phi
    T h_last;        // the shorter step that ends the range (0 if none)
};

// Returns the event code; u, w are the final values, phi_last the part of the last, shorter or interrupted, step used
// (phi_f = schw_full_steps * h_max + phi_last is rebuilt in float64 by the epilogue).
template <typename T>
__device__ __forceinline__ int schw_trace(const SchwConsts<T> &k, T &u, T &w, uint32_t &steps, T &phi_last)
{
    int ev = EV_MAXRANGE;
    steps = 0;
    phi_last = T(0);
    uint32_t n_total = k.n_full + (k.h_last > T(0) ? 1u : 0u);
    for (uint32_t i = 0; i < n_total; ++i) {
        T h = (i < k.n_full) ? k.h_max : k.h_last;
        T hh = T(0.5) * h;
        T k1u = w, k1w = M<T>::fma(k.three_M * u, u, -u);
        T tu = M<T>::fma(hh, k1u, u), tw = M<T>::fma(hh, k1w, w);
        T k2u = tw, k2w = M<T>::fma(k.three_M * tu, tu, -tu);
        tu = M<T>::fma(hh, k2u, u); tw = M<T>::fma(hh, k2w, w);
        T k3u = tw, k3w = M<T>::fma(k.three_M * tu, tu, -tu);
        tu = M<T>::fma(h, k3u, u); tw = M<T>::fma(h, k3w, w);
        T k4u = tw, k4w = M<T>::fma(k.three_M * tu, tu, -tu);
        T h6 = h * T(1.0 / 6.0);
        T un = M<T>::fma(h6, k1u + T(2) * (k2u + k3u) + k4u, u);
        T wn = M<T>::fma(h6, k1w + T(2) * (k2w + k3w) + k4w, w);
        bool cap = u < k.u_capture && un >= k.u_capture;
        bool esc = !cap && u > k.u_escape && un <= k.u_escape;
        if (cap || esc) {
            T target = cap ? k.u_capture : k.u_escape;
            T denom = un - u;
            T frac = (denom == T(0)) ? T(1) : (target - u) / denom;
            frac = M<T>::min(M<T>::max(frac, T(0)), T(1));
            phi_last = frac * h;
            w = M<T>::fma(frac, wn - w, w);
            u = target;
            ev = cap ? EV_CAPTURED : EV_ESCAPED;
            break;
        }
        u = un; w = wn;
        ++steps;
    }
    if (ev == EV_MAXRANGE && k.h_last > T(0)) phi_last = k.h_last; // the range ended with the shorter step
    return ev;
}

// Of the `steps` completed steps, the ones of length h_max (the last may be the shorter one).
template <typename T> __device__ __forceinline__ uint32_t schw_full_steps(const SchwConsts<T> &k, uint32_t steps)
{
    return steps < k.n_full ? steps : k.n_full;
}

} // namespace lt
