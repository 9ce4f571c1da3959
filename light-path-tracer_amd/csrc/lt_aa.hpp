// lt_aa.hpp -- the resolve epilogue of the supersampled frame (include/ltrace.h, "supersampled frames"): K3 of
// lt_render_aa_dev.  K1 and K2 are the mode's own kernels, launched on a band of the FINE frame (the camera with
// width W S, height H S); this kernel reads the band's ray records, shades each of a pixel's S x S sub-samples with the
// device functions the mode's own epilogue uses -- load_result, shade, disk_shade, the images sum -- and writes their
// mean, so that the result is the box filter of the fine frame the existing entry point renders, bit for bit.
//
// One work-item per SUB-SAMPLE, so the body is the mode's own epilogue body without a loop around it (a serial j, i
// loop per output pixel was built first: the compiler hoisted every float64 literal of load_result / shade out of it and
// the kernel held 179-218 VGPRs, the register problem k_epilogue_frame's old grid-stride loop had).  A workgroup takes
// P = AA_BLOCK / S^2 neighbouring output pixels of one output row; work-item t shades sub-sample t % S^2 of pixel
// t / S^2 and leaves its float32 colour and its class in LDS; after a barrier the first P work-items add their pixel's
// S^2 colours in the order of the definition -- j (fine row) outer, i (fine column) inner, float64 from 0.0 -- and
// write P neighbouring output pixels.  Every work-item holds one ray, so the counters go through flush_stats.
#pragma once
#include "lt_disk_images.hpp"

namespace lt {

constexpr int AA_PLAIN = 0, AA_DISK = 1, AA_DISK_IMAGES = 2; // LT_AA_*
constexpr int AA_MAX_SAMPLES = 8;                            // LT_AA_MAX_SAMPLES
constexpr int AA_BLOCK = 256;

// Row-segment addressing of the resolve (AaListOut of lt_aa_adaptive.hpp is the other): slot x of row blockIdx.y of the
// launch is output pixel (x, y) of the band, sub-sample (i, j) of it is the band's record of fine pixel (x S + i, y S + j),
// and the result goes to y W + x of the band's outputs -- (rows, W) of OUTPUT pixels from the band's first row on; the
// colour goes to FrameOut's rgb / rgba.
struct AaOut {
    int samples;    // S
    int W;          // output width: the fine frame's is W S
    uint8_t *cover; // (rows, W, 4): the pixel's sub-rays that escaped, were captured, were invalid, hit the disk; or NULL
    __device__ __forceinline__ bool live(int x) const { return x < W; }
    __device__ __forceinline__ void pixel(int n, int &x, int &y) const { x = n; y = (int)blockIdx.y; }
    __device__ __forceinline__ int64_t record(const CamConsts &c, int, int, int ix, int lrow) const { return pixel_to_q(c, ix, lrow); }
    __device__ __forceinline__ int64_t out(int x) const { return (int64_t)blockIdx.y * W + x; }
};

// One sub-sample: the colour the mode's epilogue writes for fine pixel (ix, lrow) of the band, whose ray record is q
// (Addr::record of aa_resolve below), the ray for
// the counters (acc), whether it counts as on the disk (the ray ended there / has a hit) and its hits.
//   AA_PLAIN        k_epilogue_frame (tb_symmetry = 0)
//   AA_DISK         k_epilogue_disk
//   AA_DISK_IMAGES  k_epilogue_disk_images
// Statement for statement what those kernels do for the colour; the per-ray outputs they also write have no place here.
template <typename T, int MODE, bool HAS_BG>
__device__ __forceinline__ void aa_sample(const CamConsts &c, const MetricConsts &m, const DiskShade &ds,
                                          const typename Vec4<T>::type *__restrict__ fin0,
                                          const typename Vec4<T>::type *__restrict__ fin1, const FrameOut &o,
                                          const DiskImagesOut &di, int64_t q, int ix, int lrow, bool colour, float *rgb,
                                          int &nch, StatAcc &acc, bool &on_disk, uint32_t &nh)
{
    RayResult res;
    nch = (HAS_BG && o.bg) ? o.bg_c : 3;
    if constexpr (MODE == AA_DISK) {
        const typename Vec4<T>::type v0 = fin0[q], v1 = fin1[q];
        if ((int)v1.z == EV_DISK) {
            on_disk = true;
            res.status = STATUS_DISK;
            res.fa = __builtin_nan("");
            res.n_half = half_orbits((double)v0.z);
            res.steps = (uint32_t)v1.w;
            const float r32 = (float)v0.x;
            const float g32 = (float)disk_redshift(ds.M, ds.a, (double)v0.x, (double)v1.y);
            disk_shade(ds, r32, g32, nch, rgb);
        } else {
            load_result<T>(m, fin0, fin1, q, res);
        }
        const float fa32 = (res.status == 1) ? (float)res.fa : __builtin_nanf("");
        const long long wl = res.n_half < 0 ? 0 : (res.n_half > 65535 ? 65535 : res.n_half);
        if (colour && !on_disk) shade<HAS_BG>(c, o, ix, local_to_global_row(c, lrow), fa32, (int)wl, rgb, nch);
    } else {
        load_result<T>(m, fin0, fin1, q, res);
        const float fa32 = (res.status == 1) ? (float)res.fa : __builtin_nanf("");
        const long long wl = res.n_half < 0 ? 0 : (res.n_half > 65535 ? 65535 : res.n_half);
        if constexpr (MODE == AA_PLAIN) {
            if (colour) shade<HAS_BG>(c, o, ix, local_to_global_row(c, lrow), fa32, (int)wl, rgb, nch);
        } else {
            nh = di.hits[q];
            const int ns = (int)(nh < (uint32_t)di.max_images ? nh : (uint32_t)di.max_images);
            const double xi = (double)fin1[q].y;
            const typename Vec2<T>::type *img = (const typename Vec2<T>::type *)di.img;
            if (HAS_BG && o.bg && colour) shade<HAS_BG>(c, o, ix, local_to_global_row(c, lrow), fa32, (int)wl, rgb, nch);
            double sum[3] = {(double)rgb[0], (double)rgb[1], (double)rgb[2]};
            for (int j = 0; j < di.max_images; ++j) {
                if (j < ns) {
                    const typename Vec2<T>::type v = img[(int64_t)j * di.n_q + q];
                    const float r32 = (float)v.x;
                    const float g32 = (float)disk_redshift(ds.M, ds.a, (double)v.x, xi);
                    double e[3];
                    disk_emission(ds, r32, g32, e);
                    if (nch == 1) sum[0] += (e[0] + e[1] + e[2]) / 3.0;
                    else { sum[0] += e[0]; sum[1] += e[1]; sum[2] += e[2]; }
                }
            }
            if (ns > 0) for (int ch = 0; ch < 3; ++ch) rgb[ch] = (float)fmin(fmax(sum[ch], 0.0), 1.0);
            on_disk = nh > 0;
        }
    }
    acc.add(res);
}

// The resolve, both phases, of a workgroup of AA_BLOCK: slot n = blockIdx.x P + pl of the launch (P = AA_BLOCK / S^2 slots
// per workgroup) is an output pixel by Addr's rule -- AaOut above or AaListOut of lt_aa_adaptive.hpp, resolved at compile
// time: live(n), pixel(n) -> (x, y), record(c, n, k, ix, lrow) -> the sub-sample's ray record, out(n) -> where the result goes.
template <typename T, int MODE, bool HAS_BG, typename Addr>
__device__ __forceinline__ void aa_resolve(const CamConsts &c, const MetricConsts &m, const DiskShade &ds,
                                           const typename Vec4<T>::type *__restrict__ fin0,
                                           const typename Vec4<T>::type *__restrict__ fin1, const FrameOut &o,
                                           const DiskImagesOut &di, const Addr &aa)
{
    __shared__ float sh_rgb[AA_BLOCK][3];
    __shared__ uint8_t sh_class[AA_BLOCK]; // bits 0-1: escaped / captured / invalid / none of them; bit 2: on the disk
    const int S = aa.samples, S2 = S * S, P = AA_BLOCK / S2;
    const int t = (int)threadIdx.x, pl = t / S2, k = t - pl * S2; // slot of the group, sub-sample (row-major)
    const int n = (int)blockIdx.x * P + pl;
    const bool colour = o.rgb || o.rgba;
    StatAcc acc;
    bool on_disk = false;
    uint32_t nh = 0;
    int nch = (HAS_BG && o.bg) ? o.bg_c : 3;
    if (pl < P && aa.live(n)) {
        int x, y;
        aa.pixel(n, x, y);
        const int j = k / S, i = k - j * S;
        float rgb[3] = {0.0f, 0.0f, 0.0f};
        aa_sample<T, MODE, HAS_BG>(c, m, ds, fin0, fin1, o, di, aa.record(c, n, k, x * S + i, y * S + j), x * S + i, y * S + j, colour, rgb,
                                   nch, acc, on_disk, nh);
        sh_rgb[t][0] = rgb[0]; sh_rgb[t][1] = rgb[1]; sh_rgb[t][2] = rgb[2];
        sh_class[t] = (uint8_t)((acc.esc ? 0 : acc.cap ? 1 : acc.inv ? 2 : 3) | (on_disk ? 4 : 0));
    }
    __syncthreads();
    const int no = (int)blockIdx.x * P + t; // the slot this work-item resolves
    if (t < P && aa.live(no)) {
        const int64_t p = aa.out(no);
        double sum[3] = {0.0, 0.0, 0.0};
        uint32_t esc = 0, cap = 0, inv = 0, disk = 0;
        for (int s = t * S2; s < (t + 1) * S2; ++s) {
            sum[0] += (double)sh_rgb[s][0]; sum[1] += (double)sh_rgb[s][1]; sum[2] += (double)sh_rgb[s][2];
            const uint32_t cl = sh_class[s];
            esc += (cl & 3) == 0; cap += (cl & 3) == 1; inv += (cl & 3) == 2;
            disk += cl >> 2;
        }
        if (colour) {
            const double s2 = (double)S2;
            const float rgb[3] = {(float)(sum[0] / s2), (float)(sum[1] / s2), (float)(sum[2] / s2)};
            if (o.rgb) for (int ch = 0; ch < nch; ++ch) o.rgb[p * nch + ch] = rgb[ch];
            if (o.rgba) store_rgba(o, p, rgb, nch);
        }
        if (aa.cover) {
            uchar4 cv;
            cv.x = (uint8_t)esc; cv.y = (uint8_t)cap; cv.z = (uint8_t)inv; cv.w = (uint8_t)disk;
            reinterpret_cast<uchar4 *>(aa.cover)[p] = cv;
        }
    }
    // words 6, 7: the rays on the disk / with a hit, and all hits (-> LT_STAT_DISK, LT_STAT_DISK_HITS)
    flush_stats<8>(o.stats, acc, m, on_disk, nh);
}

// c: the camera block of the band of the FINE frame (c.W = aa.W S columns, c.rows_local = gridDim.y S rows); o: its
// background (fine size) and the partial counter sets, with rgb / rgba the band's OUTPUT rows; grid = (segments of
// P = AA_BLOCK / S^2 output pixels, output rows of the band).
template <typename T, int MODE, bool HAS_BG>
__global__ void __launch_bounds__(AA_BLOCK) k_epilogue_aa(CamConsts c, MetricConsts m, DiskShade ds,
                                                          const typename Vec4<T>::type *__restrict__ fin0,
                                                          const typename Vec4<T>::type *__restrict__ fin1, FrameOut o,
                                                          DiskImagesOut di, AaOut aa)
{
    aa_resolve<T, MODE, HAS_BG>(c, m, ds, fin0, fin1, o, di, aa);
}

} // namespace lt
