// tools/scratch/eq_sincos_check.hip -- the fixed-quadrant sincos against the general one, on the host, exhaustively.
//
// Every float32 in [M<float>::EQ_BAND_LO, M<float>::EQ_BAND_HI] (13 170 115 values) goes through the header's own
// M<float>::sincos and M<float>::sincos_q1; both results must agree in every bit and every value must reduce to the
// quadrant k = 1.  No GPU needed: the two functions are __host__ __device__ and this calls their host side.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o /tmp/eq_sincos_check tools/scratch/eq_sincos_check.hip
//   /tmp/eq_sincos_check          (prints the counts; exit status 0 iff nothing differs)
// -ffp-contract=off: the device code's only products that feed an addition are written as fma already.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../light-path-tracer_amd/csrc/lt_device.hpp"

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

int main()
{
    const uint32_t lo = bits(lt::M<float>::EQ_BAND_LO), hi = bits(lt::M<float>::EQ_BAND_HI);
    uint64_t n = 0, differ = 0, outside = 0;
    for (uint32_t u = lo; u <= hi; ++u) {
        float x, s0, c0, s1, c1;
        memcpy(&x, &u, 4);
        lt::M<float>::sincos(x, s0, c0);
        lt::M<float>::sincos_q1(x, s1, c1);
        ++n;
        if (bits(s0) != bits(s1) || bits(c0) != bits(c1)) {
            if (!differ) printf("first difference at x = %.9g (0x%08x): sin %08x / %08x, cos %08x / %08x\n", x, u, bits(s0), bits(s1), bits(c0), bits(c1));
            ++differ;
        }
        if (rintf(x * 0.636619772367581343f) != 1.0f) ++outside;
    }
    printf("band [%.9g, %.9g]: %llu float32 values, %llu differ, %llu do not reduce to k = 1\n", lt::M<float>::EQ_BAND_LO,
           lt::M<float>::EQ_BAND_HI, (unsigned long long)n, (unsigned long long)differ, (unsigned long long)outside);
    return differ || outside ? 1 : 0;
}
