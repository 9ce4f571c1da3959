// lt_api_probes.inc -- included by lt_api.hip under LT_PROBES.
//
// Diagnostic microbenchmarks (tools/issue_probe.py, lone_step.py ...): compiled only into the probe build
// (`python __graft_entry__.py --probes` -> lib/libltrace_probes.so), never into the product library.
#include "lt_probe_pieces.hpp"

// A probe's measurement on the default stream: launch(false) as warm-up, then launch(true) between two events;
// elapsed milliseconds of the second.  The events are destroyed on every path.
template <typename Launch> static int time_launch(Launch launch, float *ms)
{
    hipEvent_t e0 = nullptr, e1 = nullptr;
    struct Destroy {
        hipEvent_t &a, &b;
        ~Destroy() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } destroy{e0, e1};
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    launch(false);
    HIP_TRY(hipEventRecord(e0, 0));
    launch(true);
    HIP_TRY(hipEventRecord(e1, 0));
    HIP_TRY(hipEventSynchronize(e1));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventElapsedTime(ms, e0, e1));
    return LT_OK;
}

// What the step and piece probes share: the Kerr constants (M 1, a 0.9), a 256-byte output, one workgroup of 256 per
// (CU, resident wave per SIMD).  After launch(timed, k, grid, out) ran twice: the shader clock from the kernel's own
// stamps (they come from the oldest wave, which wins issue arbitration: used for the clock only) and the SIMD cycles of
// the timed launch's wall time.
template <typename T, typename Launch>
static int time_kerr_probe(int waves_per_simd, Launch launch, double *cycles, double *clock_mhz)
{
    int rc;
    lt_metric m{LT_METRIC_KERR, 0, 1.0, 0.9};
    MetricConsts mc;
    if ((rc = make_metric(&m, 50.0, M_PI / 2, 0.0, &mc))) return rc;
    int cus;
    if ((rc = cu_count(&cus))) return rc;
    DevBuf out;
    if ((rc = out.alloc(256))) return rc;
    const unsigned grid = (unsigned)(cus * waves_per_simd);
    const KerrConsts<T> k = make_kerr<T>(mc, 5000.0, 1.0);
    float ms = 0;
    if ((rc = time_launch([&](bool timed) { launch(timed, k, grid, (T *)out.p); }, &ms))) return rc;
    unsigned long long h[2] = {0, 0};
    HIP_TRY(hipMemcpy(h, out.p, sizeof(h), hipMemcpyDeviceToHost));
    *clock_mhz = h[1] ? (double)h[0] / (double)h[1] * 100.0 : 0.0;
    *cycles = (double)ms * 1e-3 * *clock_mhz * 1e6;
    return LT_OK;
}

extern "C" int lt_valu_peak_probe(int mode, int iters, double *tflops)
{
    int rc = require_device();
    if (rc) return rc;
    DevBuf sink;
    if ((rc = sink.alloc(64))) return rc;
    hipDeviceProp_t prop;
    int dev;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    unsigned grid = (unsigned)prop.multiProcessorCount * 8; // 8 blocks of 256 = 32 waves per CU
    float ms = 0;
    if ((rc = time_launch([&](bool timed) { k_valu_probe<<<grid, 256>>>(mode, timed ? iters : 16, (float *)sink.p); }, &ms))) return rc;
    double fma_per_lane = (double)iters * 64.0 * (mode == 1 ? 2.0 : 1.0);
    double flops = fma_per_lane * 2.0 * 256.0 * grid;
    if (tflops) *tflops = flops / (ms * 1e-3) / 1e12;
    return LT_OK;
}

// VALU issue-cost probe: instruction class `index` (see lt_probe.hpp), `waves_per_simd` resident waves
// per SIMD (1..8) on every CU.  Reports the kernel time and the number of wave-instructions each SIMD
// issued, i.e. ns per wave-instruction per SIMD (multiply by the shader clock for cycles).
extern "C" int lt_valu_issue_probe(int index, int waves_per_simd, int iters, int constant_data, char *name_out,
                                   int name_len, double *ns_per_instr, double *clock_mhz)
{
    int rc = require_device();
    if (rc) return rc;
    if (index < 0 || index >= g_n_probes) return fail(LT_ERR_INVALID_ARG, "probe index %d out of range [0,%d)", index, g_n_probes);
    if (waves_per_simd < 1 || waves_per_simd > 8) return fail(LT_ERR_INVALID_ARG, "waves_per_simd must be 1..8");
    const ProbeEntry &pe = g_probes[index];
    if (name_out && name_len > 0) snprintf(name_out, (size_t)name_len, "%s", pe.name);
    int cus;
    if ((rc = cu_count(&cus))) return rc;
    DevBuf sink;
    if ((rc = sink.alloc(64))) return rc;
    unsigned grid = (unsigned)(cus * waves_per_simd);
    float sc = constant_data ? 0.0f : 0.999f;
    float ms = 0;
    if ((rc = time_launch([&](bool timed) { pe.kernel<<<grid, 256>>>(timed ? iters : 8, sc, (float *)sink.p); }, &ms))) return rc;
    double instr_per_simd = (double)iters * 64.0 * pe.instr_per_body * waves_per_simd; // 8 bodies x 8 chains
    if (ns_per_instr) *ns_per_instr = ms * 1e6 / instr_per_simd;
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpy(h, sink.p, sizeof(h), hipMemcpyDeviceToHost));
    if (clock_mhz) *clock_mhz = h[3] ? (double)h[2] / (double)h[3] * 100.0 : 0.0; // s_memtime / s_memrealtime(100 MHz)
    return LT_OK;
}

extern "C" int lt_valu_issue_probe_count(void) { return g_n_probes; }

// RK4-step issue probe: `iters` steps of the Kerr RK4 step per lane at `waves_per_simd` resident waves
// per SIMD.  Returns shader cycles per step per wave-slot-on-a-SIMD (i.e. elapsed cycles x
// waves_per_simd / iters ... divided back out: cycles one SIMD spends per wave-step) and the clock.
extern "C" int lt_rk4_step_probe(int precision, int waves_per_simd, int iters, double *cycles_per_wave_step,
                                 double *clock_mhz)
{
    int rc = require_device();
    if (rc) return rc;
    if (waves_per_simd < 1 || waves_per_simd > 8) return fail(LT_ERR_INVALID_ARG, "waves_per_simd must be 1..8");
    double cycles = 0, mhz = 0;
    rc = with_precision(precision, [&](auto t) {
        using T = decltype(t);
        return time_kerr_probe<T>(waves_per_simd, [&](bool timed, const KerrConsts<T> &k, unsigned grid, T *out) {
            k_probe_rk4_step<T><<<grid, 256>>>(k, timed ? iters : 16, (T)0.01, out);
        }, &cycles, &mhz);
    });
    if (rc) return rc;
    if (clock_mhz) *clock_mhz = mhz;
    if (cycles_per_wave_step) *cycles_per_wave_step = cycles / ((double)iters * waves_per_simd);
    return LT_OK;
}

// Piece probe (diagnostic): PIECE 0 sincos, 1 right-hand side without sincos, 2 the same without the
// reciprocal, 3 the two polynomials alone; 4 evaluations per loop iteration.  Returns SIMD cycles per
// evaluation per wave.
using PieceKernel = void (*)(KerrConsts<float>, int, float *);
template <int... N> static constexpr std::array<PieceKernel, sizeof...(N)> piece_kernels(std::integer_sequence<int, N...>)
{
    return {&k_probe_piece<N>...};
}

extern "C" int lt_piece_probe(int piece, int waves_per_simd, int iters, double *cycles_per_eval, double *clock_mhz)
{
    int rc = require_device();
    if (rc) return rc;
    static constexpr auto kernels = piece_kernels(std::make_integer_sequence<int, 8>{});
    const PieceKernel kernel = kernels[piece >= 0 && piece < 7 ? piece : 7];
    double cycles = 0, mhz = 0;
    rc = time_kerr_probe<float>(waves_per_simd, [&](bool timed, const KerrConsts<float> &k, unsigned grid, float *out) {
        kernel<<<grid, 256>>>(k, timed ? iters : 16, out);
    }, &cycles, &mhz);
    if (rc) return rc;
    if (clock_mhz) *clock_mhz = mhz;
    if (cycles_per_eval) *cycles_per_eval = cycles / ((double)iters * 4.0 * waves_per_simd);
    return LT_OK;
}
