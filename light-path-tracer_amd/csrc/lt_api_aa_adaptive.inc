// lt_api_aa_adaptive.inc -- included at the end of lt_api.hip, after lt_api_aa.inc.
//
// Host side of the adaptively supersampled frame (include/ltrace.h, "adaptive supersampling"): the plan, the base pass
// (lt_render_aa's bands, unchanged, at samples_lo), the flag kernel over the whole frame, ONE wait for the stream to read
// the number of refined pixels -- launch sizes need it --, then the refined pass in chunks of the list: the list prologue,
// the mode's integrate kernel on the chunk's records exactly as the batch twins launch it, and the list epilogue, which
// overwrites the listed pixels.  List, count and scratch belong to the (device, stream) slot and only grow.

extern "C" void lt_default_aa_adaptive(lt_aa_adaptive *a)
{
    memset(a, 0, sizeof(*a));
    a->samples_lo = 1;
    a->samples_hi = 4;
    a->mode = LT_AA_PLAIN;
    a->max_images = 3;
    a->band_rows = 0;    // automatic
    a->chunk_pixels = 0; // automatic
    a->contrast = 0.0625f;
}

struct AaAdaptivePlan {
    AaPlan base;              // the base pass: lt_render_aa with `lo`
    lt_aa lo{};
    int64_t chunk_pixels = 0; // refined pixels per chunk
    lt_camera fine_hi{};      // the camera of the S_hi fine frame
};

// Refusals in the order the header gives them: the adaptive fields, then lt_render_aa's for the base pass, the S_hi fine
// frame, the frame's size, partitions.
static int aa_adaptive_plan(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *ad,
                            const lt_disk *disk, AaAdaptivePlan *p)
{
    int rc;
    if (!cam || !metric || !opts || !ad) return fail(LT_ERR_INVALID_ARG, "null camera / metric / opts / adaptive");
    if (ad->samples_lo < 1 || ad->samples_lo > 4) return fail(LT_ERR_INVALID_ARG, "samples_lo %d not in [1, 4]", (int)ad->samples_lo);
    if (ad->samples_hi <= ad->samples_lo || ad->samples_hi > LT_AA_MAX_SAMPLES)
        return fail(LT_ERR_INVALID_ARG, "samples_hi %d not in (samples_lo = %d, %d]", (int)ad->samples_hi, (int)ad->samples_lo, LT_AA_MAX_SAMPLES);
    if (std::isnan(ad->contrast)) return fail(LT_ERR_INVALID_ARG, "contrast is NaN");
    if (ad->chunk_pixels < 0) return fail(LT_ERR_INVALID_ARG, "chunk_pixels %d is negative", (int)ad->chunk_pixels);
    p->lo = lt_aa{ad->samples_lo, ad->mode, ad->max_images, ad->band_rows};
    if ((rc = aa_plan(cam, metric, opts, &p->lo, disk, &p->base))) return rc;
    const int S = ad->samples_hi;
    if ((rc = aa_fine_camera(cam, S, &p->fine_hi))) return rc;
    if ((int64_t)cam->width * cam->height > INT32_MAX) // (the list holds 32-bit pixel indices)
        return fail(LT_ERR_INVALID_ARG, "a frame of %d x %d pixels: more than 2^31 - 1", cam->width, cam->height);
    if (p->base.o.n_parts != 1 || p->base.o.block_owner)
        return fail(LT_ERR_UNSUPPORTED, "adaptive supersampling renders the whole frame: the 3 x 3 test reads rows a partition does not "
                                        "own (n_parts %d%s)", p->base.o.n_parts, p->base.o.block_owner ? ", block_owner table" : "");
    // a chunk's records: per ray what a band's rays need (aa_plan), S_hi^2 rays per pixel, whole wavefronts, < 2^31 of them
    const size_t per_ray = aa_ray_bytes(p->base.o.precision, ad->mode, ad->max_images);
    const int64_t n_pix = (int64_t)cam->width * cam->height, S2 = (int64_t)S * S;
    int64_t chunk = ad->chunk_pixels ? (int64_t)ad->chunk_pixels : (int64_t)((((size_t)LT_AA_BAND_BYTES / per_ray) & ~(size_t)63) / (size_t)S2);
    chunk = std::min(chunk, ((int64_t)INT32_MAX - 63) / S2);
    chunk = std::max<int64_t>(1, std::min(chunk, n_pix));
    p->chunk_pixels = chunk;
    return LT_OK;
}

extern "C" int lt_aa_adaptive_plan(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *ad,
                                   const lt_disk *disk, int64_t *base_band_bytes, int64_t *chunk_pixels)
{
    AaAdaptivePlan p;
    int rc = aa_adaptive_plan(cam, metric, opts, ad, disk, &p);
    if (rc) return rc;
    if (base_band_bytes) *base_band_bytes = (int64_t)p.base.band_bytes;
    if (chunk_pixels) *chunk_pixels = p.chunk_pixels;
    return LT_OK;
}

// The S_hi fine camera as ONE partition of the whole frame: local rows are global rows, no tiles (the list kernels take
// their pixels from the list).  What k_prologue_camera and the epilogues read of a band's block is set as make_camera sets it.
static void make_list_camera(const lt_camera &fine, int kind, const lt_opts &o, CamConsts *c)
{
    const bool front = camera_pinhole(&fine, o.axis_refine_frac, c);
    c->row_block = o.row_block; c->n_parts = 1; c->part = 0;
    c->rows_local = c->trace_rows = fine.height;
    c->loop_around = o.loop_around;
    c->refine_on = front && kind == LT_METRIC_KERR;
}

// One chunk of the list: n entries from d_list on.  own: the host call's timing quad, or NULL (opts->timing: a pooled one).
static int aa_refine_chunk(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, double lambda_max, const lt_aa_adaptive *ad,
                           const DiskParams *disk, const uint32_t *d_list, int n, int W, const float *d_bg_hi, int32_t bg_channels,
                           float *d_rgb, uint8_t *d_rgba, uint8_t *d_cover, uint64_t *d_stats, const EventQuad *own)
{
    int rc;
    hipStream_t s = (hipStream_t)o.stream;
    const int S = ad->samples_hi, S2 = S * S;
    const int64_t n_q = ((int64_t)n * S2 + 63) / 64 * 64;
    const size_t elem = elem_size(o.precision);
    Workspace w;
    // (the records overwrite whatever a frame left in the workspace: get_workspace clears the slot's record key, and
    // nothing here sets one, so the next frame on the stream runs its own prologue)
    if ((rc = get_workspace(s, (size_t)n_q, elem, &w))) return rc;
    DiskRecordsBuf recs;
    if ((rc = get_disk_records(s, n_q, elem, disk, &recs))) return rc;
    Timer tm;
    if ((rc = tm.begin(o.timing != 0, own))) return rc;
    const FrameOut fo{d_bg_hi, bg_channels, nullptr, nullptr, nullptr, nullptr, d_rgb, d_rgba, d_stats ? (uint64_t *)w.partials : nullptr};
    if ((rc = tm.mark(0, s))) return rc;
    with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_prologue_aa_list<T><<<(unsigned)((n_q + 255) / 256), 256, 0, s>>>(c, mc, d_list, n, S, W, w.ic<T>(), n_q);
    });
    HIP_TRY(hipGetLastError());
    if ((rc = tm.mark(1, s))) return rc;
    if ((rc = launch_integrate_any(mc, o, lambda_max, w, n_q, s, d_stats, disk, recs))) return rc;
    if ((rc = tm.mark(2, s))) return rc;
    const int per_group = AA_BLOCK / S2; // list entries of a workgroup
    if ((rc = launch_aa_resolve(c, mc, o, ad->mode, w, fo, d_stats, s, disk, recs, AaListOut{S, W, d_cover, d_list, n},
                                dim3((unsigned)((n + per_group - 1) / per_group)))))
        return rc;
    if ((rc = tm.mark(3, s))) return rc;
    tm.finish();
    return LT_OK;
}

static int aa_check_backgrounds(const float *bg_lo, const float *bg_hi, int32_t bg_channels)
{
    if ((bg_lo == nullptr) != (bg_hi == nullptr)) return fail(LT_ERR_INVALID_ARG, "the two backgrounds are both NULL or both given");
    return aa_check_bg_channels(bg_lo, bg_channels);
}

// A planned call on device pointers.  quads: the host call's -- the launches are timed with private quads of the slot
// (aa_events, grown to one per band, one for the flag kernel and one per chunk, as lt_render_aa grows them to its bands)
// and *quads is how many were recorded, for the caller to add up after its last wait --, or NULL (opts->timing: pooled
// quads, as many).
static int aa_adaptive_run(const lt_camera *cam, const lt_metric *metric, const lt_aa_adaptive *ad, const AaAdaptivePlan &p,
                           const float *d_bg_lo, const float *d_bg_hi, int32_t bg_channels, float *d_rgb, uint8_t *d_rgba,
                           uint8_t *d_cover, uint8_t *d_level, uint64_t *d_stats, int *quads)
{
    int rc = aa_check_backgrounds(d_bg_lo, d_bg_hi, bg_channels);
    if (rc) return rc;
    const lt_opts &o = p.base.o;
    hipStream_t s = (hipStream_t)o.stream;
    const int W = cam->width, H = cam->height, nch = d_bg_lo ? bg_channels : 3;
    const size_t n_pix = (size_t)W * H;
    StreamSlot *sl;
    if ((rc = get_slot(s, &sl))) return rc;
    // what the flag kernel reads and the caller did not ask for; the list with its count in front
    const bool colour_test = ad->contrast >= 0.0f;
    Carver cv;
    const size_t off_cover = d_cover ? 0 : cv.take(n_pix * 4), off_rgb = (d_rgb || !colour_test) ? 0 : cv.take(n_pix * nch * sizeof(float));
    if ((rc = grow(sl->aa_scratch, cv.off, s)) || (rc = grow(sl->aa_list, 256 + n_pix * sizeof(uint32_t), s))) return rc;
    uint8_t *base_cover = d_cover ? d_cover : (uint8_t *)sl->aa_scratch.p + off_cover;
    float *base_rgb = d_rgb ? d_rgb : (colour_test ? (float *)((char *)sl->aa_scratch.p + off_rgb) : nullptr);
    unsigned int *d_count = (unsigned int *)sl->aa_list.p;
    uint32_t *d_list = (uint32_t *)((char *)sl->aa_list.p + 256);
    const int n_bands = p.base.n_bands;
    if (quads) {
        if ((rc = aa_slot_events(sl, n_bands + 1))) return rc;
        *quads = n_bands + 1;
    }

    // 1. the base pass
    if ((rc = aa_render_bands(cam, metric, &p.lo, p.base, d_bg_lo, bg_channels, base_rgb, d_rgba, base_cover, d_stats,
                              quads ? sl->aa_events.data() : nullptr)))
        return rc;
    // 2. the three tests on every pixel; the flag kernel's time counts as prologue (marks 1, 2, 3 coincide)
    {
        Timer tm;
        if ((rc = tm.begin(o.timing != 0, quads ? &sl->aa_events[(size_t)n_bands] : nullptr))) return rc;
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned int), s));
        if ((rc = tm.mark(0, s))) return rc;
        for (int y0 = 0; y0 < H; y0 += 65535) { // (grid.y carries the row: at most 65535 per launch)
            const dim3 grid((unsigned)((W + AA_FLAG_BLOCK - 1) / AA_FLAG_BLOCK), (unsigned)std::min(H - y0, 65535));
            k_aa_flag<<<grid, AA_FLAG_BLOCK, 0, s>>>((const uchar4 *)base_cover, base_rgb, nch, W, H, y0, ad->samples_lo, ad->samples_hi,
                                                     ad->mode, ad->contrast, d_level, d_list, d_count);
        }
        HIP_TRY(hipGetLastError());
        for (int i = 1; i < 4; ++i) if ((rc = tm.mark(i, s))) return rc;
        tm.finish();
        if (d_stats) k_aa_count_to_stats<<<1, 1, 0, s>>>(d_count, (unsigned long long *)d_stats, LT_STAT_AA_REFINED);
        HIP_TRY(hipGetLastError());
    }
    // 3. the one wait of the call: the refined pass's launch sizes follow from the count
    unsigned int n_refined = 0;
    HIP_TRY(hipMemcpyAsync(&n_refined, d_count, sizeof(n_refined), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_refined == 0) return LT_OK; // nothing further is launched
    if ((size_t)n_refined > n_pix) return fail(LT_ERR_HIP, "the flag kernel counted %u pixels of %zu", n_refined, n_pix);

    // 4. the refined pass, chunk after chunk
    MetricConsts mc;
    if ((rc = make_metric(metric, cam->r_obs, cam->theta_obs, o.h_max, &mc))) return rc;
    count_evals(o.integrator, &mc);
    CamConsts c;
    make_list_camera(p.fine_hi, metric->kind, o, &c);
    const double lambda_max = fmax(5000.0, 6.0 * cam->r_obs); // metrics.py:1132
    const int64_t n_chunks = ((int64_t)n_refined + p.chunk_pixels - 1) / p.chunk_pixels;
    if (quads && (rc = aa_slot_events(sl, n_bands + 1 + (int)n_chunks))) return rc;
    for (int64_t k0 = 0; k0 < (int64_t)n_refined; k0 += p.chunk_pixels) {
        const int n = (int)std::min<int64_t>(p.chunk_pixels, (int64_t)n_refined - k0);
        const EventQuad *own = quads ? &sl->aa_events[(size_t)(*quads)++] : nullptr;
        if ((rc = aa_refine_chunk(c, mc, o, lambda_max, ad, p.base.has_disk ? &p.base.dp : nullptr, d_list + k0, n, W, d_bg_hi, bg_channels,
                                  d_rgb, d_rgba, d_cover, d_stats, own)))
            return rc;
    }
    return LT_OK;
}

extern "C" int lt_render_aa_adaptive_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *ad,
                                         const lt_disk *disk, const float *d_bg_lo, const float *d_bg_hi, int32_t bg_channels,
                                         float *d_rgb, uint8_t *d_rgba, uint8_t *d_cover, uint8_t *d_level, uint64_t *d_stats)
{
    int rc = require_device();
    if (rc) return rc;
    AaAdaptivePlan p;
    if ((rc = aa_adaptive_plan(cam, metric, opts, ad, disk, &p))) return rc;
    return aa_adaptive_run(cam, metric, ad, p, d_bg_lo, d_bg_hi, bg_channels, d_rgb, d_rgba, d_cover, d_level, d_stats, nullptr);
}

extern "C" int lt_render_aa_adaptive(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa_adaptive *ad,
                                     const lt_disk *disk, const float *bg_lo, const float *bg_hi, int32_t bg_channels, float *out_rgb,
                                     uint8_t *out_rgba, uint8_t *out_cover, uint8_t *out_level, lt_stats *stats)
{
    int rc = require_device();
    if (rc) return rc;
    AaAdaptivePlan p;
    if ((rc = aa_adaptive_plan(cam, metric, opts, ad, disk, &p))) return rc;
    if ((rc = aa_check_backgrounds(bg_lo, bg_hi, bg_channels))) return rc;
    const size_t n = (size_t)cam->width * cam->height, s_lo = (size_t)ad->samples_lo, s_hi = (size_t)ad->samples_hi;
    lt_stats st;
    memset(&st, 0, sizeof(st));
    Staging sg; // the two backgrounds in, the resolved outputs alone out
    const int i_stats = sg.out(st.counters, LT_STAT_WORDS, 8);
    const int i_lo = sg.in(bg_lo, n * s_lo * s_lo, bg_channels * sizeof(float)), i_hi = sg.in(bg_hi, n * s_hi * s_hi, bg_channels * sizeof(float));
    const int i_rgb = sg.out(out_rgb, n, (bg_lo ? bg_channels : 3) * 4), i_rgba = sg.out(out_rgba, n, 4), i_cover = sg.out(out_cover, n, 4);
    const int i_level = sg.out(out_level, n, 1);
    if ((rc = sg.commit((hipStream_t)p.base.o.stream))) return rc;
    HIP_TRY(hipMemsetAsync(sg.dev<char>(i_stats), 0, LT_STAT_WORDS * 8, sg.s));
    p.base.o.timing = 0;
    int quads = 0;
    if ((rc = aa_adaptive_run(cam, metric, ad, p, sg.dev<const float>(i_lo), sg.dev<const float>(i_hi), bg_channels, sg.dev<float>(i_rgb),
                              sg.dev<uint8_t>(i_rgba), sg.dev<uint8_t>(i_cover), sg.dev<uint8_t>(i_level), sg.dev<uint64_t>(i_stats), &quads)))
        return rc;
    for (int i : {i_rgba, i_cover, i_level, i_rgb, i_stats}) if ((rc = sg.fetch(i))) return rc;
    HIP_TRY(hipStreamSynchronize(sg.s));
    if ((rc = aa_add_times(sg.sl, quads, &st))) return rc; // kernel times are summed over bands, the flag kernel and chunks
    if (stats) *stats = st;
    return LT_OK;
}
