// lt_api_stages.inc -- included at the end of lt_api.hip.
//
// Stage-wise entry points: the reference's image pipeline is three separate functions
// (build_alpha_lookup -> precompute_final_alpha_lookup[_2d] -> render_lensed_image), and code written
// against it calls them one by one.  lt_render fuses them; these two give the first and the last
// stage on their own so that the reference's call sequence has a GPU twin for every step
// (the middle stage is lt_trace_batch_*).

namespace lt {

// image_lens.py:133-152 (alpha, float32) and :193-216 (theta float64, axis-refine columns)
__global__ void __launch_bounds__(256) k_pixel_angles(CamConsts c, float *__restrict__ alpha, double *__restrict__ theta)
{
    int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)c.W * c.H) return;
    int iy = (int)(p / c.W), ix = (int)(p - (int64_t)iy * c.W);
    double al, th;
    pixel_angles(c, ix, iy, al, th);
    if (alpha) alpha[p] = (float)al;
    if (theta) theta[p] = th;
}

// image_lens.py:296-397 from caller-supplied lookups
__global__ void __launch_bounds__(256) k_shade_lookup(CamConsts c, FrameOut o, const float *__restrict__ fa,
                                                      const uint16_t *__restrict__ winding)
{
    int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (int64_t)c.W * c.H) return;
    int iy = (int)(p / c.W), ix = (int)(p - (int64_t)iy * c.W);
    float rgb[3];
    int nch;
    shade(c, o, ix, iy, fa[p], winding ? (int)winding[p] : 0, rgb, nch);
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

} // namespace lt

static int make_camera_only(const lt_camera *cam, double axis_refine_frac, CamConsts *c)
{
    if (!cam || cam->width <= 0 || cam->height <= 0) return fail(LT_ERR_INVALID_ARG, "bad camera");
    const bool front = camera_pinhole(cam, axis_refine_frac, c); // (zero-fills *c first)
    c->refine_on = front;
    c->rows_local = c->trace_rows = c->H;
    c->row_block = c->H; c->n_parts = 1; c->part = 0;
    c->tiles_x = (c->W + 7) / 8; c->tiles_y = (c->H + 7) / 8;
    return LT_OK;
}

// Replaces build_alpha_lookup (image_lens.py:133-152) and the theta / axis-refine part of
// precompute_final_alpha_lookup_2d (image_lens.py:193-216).  HOST pointers, any may be NULL:
// out_alpha (H, W) float32, out_theta (H, W) float64, out_axis_cols (W) bytes.
extern "C" int lt_pixel_angles(const lt_camera *cam, double axis_refine_frac, float *out_alpha, double *out_theta,
                               uint8_t *out_axis_cols)
{
    int rc = require_device();
    if (rc) return rc;
    CamConsts c;
    if ((rc = make_camera_only(cam, axis_refine_frac, &c))) return rc;
    size_t n = (size_t)c.W * c.H;
    DevBuf da, dt;
    if (out_alpha && (rc = da.alloc(n * 4))) return rc;
    if (out_theta && (rc = dt.alloc(n * 8))) return rc;
    if (out_alpha || out_theta) {
        k_pixel_angles<<<(unsigned)((n + 255) / 256), 256>>>(c, (float *)da.p, (double *)dt.p);
        HIP_TRY(hipGetLastError());
        if (out_alpha) HIP_TRY(hipMemcpy(out_alpha, da.p, n * 4, hipMemcpyDeviceToHost));
        if (out_theta) HIP_TRY(hipMemcpy(out_theta, dt.p, n * 8, hipMemcpyDeviceToHost));
    }
    if (out_axis_cols)
        for (int ix = 0; ix < c.W; ++ix)
            out_axis_cols[ix] = c.refine_on && fabs(((double)ix - c.half_W) / c.fx - c.bh_x_cam) <= c.refine_thresh;
    return LT_OK;
}

// Replaces render_lensed_image (image_lens.py:296-397) for caller-supplied lookups, plus the RGBA8
// conversion of imsave.  HOST pointers: bg (H, W, bg_channels) float32, fa (H, W) float32, winding
// (H, W) uint16 or NULL; out_rgb (H, W, bg_channels) float32 and / or out_rgba (H, W, 4) uint8.
extern "C" int lt_shade(const lt_camera *cam, int32_t loop_around, const float *bg, int32_t bg_channels, const float *fa,
                        const uint16_t *winding, float *out_rgb, uint8_t *out_rgba)
{
    int rc = require_device();
    if (rc) return rc;
    if (!bg || !fa) return fail(LT_ERR_INVALID_ARG, "lt_shade needs a background and a final_alpha lookup");
    if (bg_channels != 1 && bg_channels != 3) return fail(LT_ERR_INVALID_ARG, "bg_channels must be 1 or 3");
    CamConsts c;
    if ((rc = make_camera_only(cam, 0.07, &c))) return rc;
    c.loop_around = loop_around;
    size_t n = (size_t)c.W * c.H;
    DevBuf dbg, dfa, dw, drgb, drgba;
    if ((rc = dbg.alloc(n * bg_channels * 4)) || (rc = dfa.alloc(n * 4))) return rc;
    HIP_TRY(hipMemcpy(dbg.p, bg, n * bg_channels * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dfa.p, fa, n * 4, hipMemcpyHostToDevice));
    if (winding) {
        if ((rc = dw.alloc(n * 2))) return rc;
        HIP_TRY(hipMemcpy(dw.p, winding, n * 2, hipMemcpyHostToDevice));
    }
    if (out_rgb && (rc = drgb.alloc(n * bg_channels * 4))) return rc;
    if (out_rgba && (rc = drgba.alloc(n * 4))) return rc;
    FrameOut fo{(const float *)dbg.p, bg_channels, nullptr, nullptr, nullptr, nullptr, (float *)drgb.p, (uint8_t *)drgba.p, nullptr};
    k_shade_lookup<<<(unsigned)((n + 255) / 256), 256>>>(c, fo, (const float *)dfa.p, winding ? (const uint16_t *)dw.p : nullptr);
    HIP_TRY(hipGetLastError());
    if (out_rgb) HIP_TRY(hipMemcpy(out_rgb, drgb.p, n * bg_channels * 4, hipMemcpyDeviceToHost));
    if (out_rgba) HIP_TRY(hipMemcpy(out_rgba, drgba.p, n * 4, hipMemcpyDeviceToHost));
    return LT_OK;
}
