// lt_api_aa.inc -- included at the end of lt_api.hip, after the disks.
//
// Host side of the supersampled frame (include/ltrace.h, "supersampled frames"): the plan (checks, the rows of this
// partition, the bands), the launch of the resolve epilogue of lt_aa.hpp, and the entry points.  A band is a frame of
// its own to render_dev_impl: the FINE camera (W S x H S) with row blocks of row_block S rows, restricted to the band's
// blocks.  Camera, workspace, record reuse, prologue and integrate launches are therefore lt_render's, unchanged; only
// the epilogue differs.  A call of one band hands the caller's partition on as it is (no table unless the caller gave
// one); a call of several bands uploads the partition's block list once and gives every band its piece of it.

extern "C" void lt_default_aa(lt_aa *a)
{
    memset(a, 0, sizeof(*a));
    a->samples = 2;
    a->mode = LT_AA_PLAIN;
    a->max_images = 3;
    a->band_rows = 0; // automatic
}

// What a call will do, from host arithmetic alone.
struct AaPlan {
    lt_opts o;                  // checked; row_block, n_parts, part, block_owner are the OUTPUT frame's
    bool has_disk = false;
    DiskParams dp{};
    std::vector<int32_t> owned; // this partition's row blocks, ascending
    int64_t rows = 0;           // ... and output rows
    int band_blocks = 1;        // row blocks per band
    int n_bands = 0;
    size_t band_bytes = 0;      // ray records of the largest band
    lt_camera fine{};           // the camera of the fine frame
};

// Output rows of row block b of a frame of `height` rows.
static int64_t block_rows(int64_t b, int row_block, int height)
{
    const int64_t r0 = b * row_block, r1 = r0 + row_block;
    return (r1 < height ? r1 : height) - r0;
}

// The ray records of one ray: three 4-vectors, plus the thin disk's slots and count.
static size_t aa_ray_bytes(int precision, int mode, int max_images)
{
    const size_t elem = elem_size(precision);
    return 3 * 4 * elem + (mode == LT_AA_DISK_IMAGES ? (size_t)max_images * 2 * elem + sizeof(uint32_t) : 0);
}

// The fine frame's camera: `cam` with W S x H S pixels, refused when a side does not fit 31 bits.
static int aa_fine_camera(const lt_camera *cam, int S, lt_camera *fine)
{
    if ((int64_t)cam->width * S > INT32_MAX || (int64_t)cam->height * S > INT32_MAX)
        return fail(LT_ERR_INVALID_ARG, "fine frame of %d x %d pixels times %d", cam->width, cam->height, S);
    *fine = *cam;
    fine->width = cam->width * S;
    fine->height = cam->height * S;
    return LT_OK;
}

static int aa_check_bg_channels(const float *bg, int32_t bg_channels)
{
    if (bg && bg_channels != 1 && bg_channels != 3) return fail(LT_ERR_INVALID_ARG, "bg_channels must be 1 or 3");
    return LT_OK;
}

// Refusals in the order the header gives them: samples and mode, then the mode's own, then lt_render_dev's.
static int aa_plan(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa, const lt_disk *disk,
                   AaPlan *p)
{
    int rc;
    if (!cam || !metric || !opts || !aa) return fail(LT_ERR_INVALID_ARG, "null camera / metric / opts / aa");
    if (aa->samples < 1 || aa->samples > LT_AA_MAX_SAMPLES)
        return fail(LT_ERR_INVALID_ARG, "samples %d not in [1, %d]", (int)aa->samples, LT_AA_MAX_SAMPLES);
    if (aa->mode != LT_AA_PLAIN && aa->mode != LT_AA_DISK && aa->mode != LT_AA_DISK_IMAGES)
        return fail(LT_ERR_INVALID_ARG, "unknown supersampling mode %d", (int)aa->mode);
    p->has_disk = aa->mode != LT_AA_PLAIN;
    if (p->has_disk && (rc = resolve_disk(metric, cam->r_obs, opts->schedule, disk, aa->mode == LT_AA_DISK_IMAGES ? &aa->max_images : nullptr, &p->dp)))
        return rc;
    if (cam->width <= 0 || cam->height <= 0) return fail(LT_ERR_INVALID_ARG, "empty frame %dx%d", cam->width, cam->height);
    const int S = aa->samples;
    if ((rc = aa_fine_camera(cam, S, &p->fine))) return rc;
    p->o = *opts;
    if ((rc = check_opts(metric, &p->o))) return rc;
    lt_opts &o = p->o;
    o.tb_symmetry = 0; // (the definition's plain mode; the disks ignore it)
    if ((int64_t)o.row_block * S > INT32_MAX) return fail(LT_ERR_INVALID_ARG, "row_block %d times %d samples", o.row_block, S);
    if ((rc = partition_blocks(cam->height, o, &p->owned, &p->rows))) return rc;
    if (aa->band_rows < 0 || aa->band_rows % o.row_block)
        return fail(LT_ERR_INVALID_ARG, "band_rows %d is not a multiple of row_block %d", (int)aa->band_rows, o.row_block);
    // ray records of one band: every ray of the padded fine tiles
    const size_t per_ray = aa_ray_bytes(o.precision, aa->mode, aa->max_images);
    const size_t fine_cols = ((size_t)cam->width * S + 7) / 8 * 8;
    auto bytes_of = [&](int64_t blocks) { return (((size_t)blocks * o.row_block * S + 7) / 8 * 8) * fine_cols * per_ray; };
    int64_t blocks = aa->band_rows ? aa->band_rows / o.row_block : (int64_t)p->owned.size();
    if (!aa->band_rows) { // automatic: the most row blocks whose fine rows, padded to whole tiles, fit the budget
        const size_t fit = ((size_t)LT_AA_BAND_BYTES / (fine_cols * per_ray)) & ~(size_t)7;
        blocks = std::min<int64_t>(blocks, (int64_t)(fit / ((size_t)o.row_block * S)));
    }
    // (a band is one launch grid of the epilogues: at most 65535 fine rows)
    const int64_t grid_blocks = 65535 / ((int64_t)o.row_block * S);
    if (grid_blocks >= 1 && blocks > grid_blocks) blocks = grid_blocks;
    if (blocks < 1) blocks = 1;
    if (blocks > (int64_t)p->owned.size() && !p->owned.empty()) blocks = (int64_t)p->owned.size();
    p->band_blocks = (int)blocks;
    p->n_bands = (int)(((int64_t)p->owned.size() + blocks - 1) / blocks);
    p->band_bytes = p->owned.empty() ? 0 : WS_CTRL_BYTES + bytes_of(blocks);
    return LT_OK;
}

extern "C" int64_t lt_aa_band_bytes(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                                    const lt_disk *disk, int32_t *band_rows, int32_t *n_bands)
{
    AaPlan p;
    int rc = aa_plan(cam, metric, opts, aa, disk, &p);
    if (rc) return rc;
    if (band_rows) *band_rows = p.band_blocks * p.o.row_block;
    if (n_bands) *n_bands = p.n_bands;
    return (int64_t)p.band_bytes;
}

// The resolve launch of both supersampling paths: k_epilogue_aa over `grid` for the row-segment addressing (AaOut),
// k_epilogue_aa_list for the list addressing (AaListOut), on the records of `w` / `recs`, and the fold of the counters.
template <typename Addr>
static int launch_aa_resolve(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, int aa_mode, const Workspace &w,
                             const FrameOut &fo, uint64_t *d_stats, hipStream_t s, const DiskParams *disk, const DiskRecordsBuf &recs,
                             const Addr &ao, dim3 grid)
{
    DiskShade ds{};
    DiskImagesOut di{};
    if (disk) ds = DiskShade{mc.M, mc.a, disk->r_in, disk->q, disk->exposure};
    if (disk && disk->max_images) di = DiskImagesOut{recs.p, recs.hits, (int64_t)w.n_q, disk->max_images, nullptr, nullptr};
    const bool has_bg = fo.bg != nullptr && (fo.rgb || fo.rgba);
    auto launch = [&](auto t, auto mode, auto bg) {
        using T = decltype(t);
        constexpr int MODE = decltype(mode)::value;
        constexpr bool BG = decltype(bg)::value;
        if constexpr (std::is_same<Addr, AaOut>::value) k_epilogue_aa<T, MODE, BG><<<grid, AA_BLOCK, 0, s>>>(c, mc, ds, w.fin0<T>(), w.fin1<T>(), fo, di, ao);
        else k_epilogue_aa_list<T, MODE, BG><<<grid, AA_BLOCK, 0, s>>>(c, mc, ds, w.fin0<T>(), w.fin1<T>(), fo, di, ao);
    };
    with_precision(o.precision, [&](auto t) {
        auto with_bg = [&](auto mode) {
            if (has_bg) launch(t, mode, std::true_type{});
            else launch(t, mode, std::false_type{});
        };
        if (aa_mode == LT_AA_PLAIN) with_bg(std::integral_constant<int, AA_PLAIN>{});
        else if (aa_mode == LT_AA_DISK) with_bg(std::integral_constant<int, AA_DISK>{});
        else with_bg(std::integral_constant<int, AA_DISK_IMAGES>{});
    });
    if (d_stats) k_stats_reduce<<<1, STAT_SLOTS, 0, s>>>(w.partials, (unsigned long long *)d_stats, LT_STAT_DISK, LT_STAT_DISK_HITS);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

static int launch_epilogue_aa(const CamConsts &c, const MetricConsts &mc, const lt_opts &o, const Workspace &w, const FrameOut &fo,
                              uint64_t *d_stats, hipStream_t s, const DiskParams *disk, const DiskRecordsBuf &recs, const AaBand &aa)
{
    // the kernel indexes the fine band by (x S + i, y S + j): the band render_dev_impl built must be exactly that
    if (c.W != aa.W * aa.samples || (int64_t)c.rows_local != aa.rows * aa.samples || c.trace_rows != c.rows_local || c.use_tb ||
        (int64_t)c.tiles_x * c.tiles_y * 64 != (int64_t)w.n_q)
        return fail(LT_ERR_INVALID_ARG, "supersampling: band of %d x %d fine pixels for %d x %lld output pixels times %d", c.W,
                    c.rows_local, aa.W, (long long)aa.rows, aa.samples);
    const int per_group = AA_BLOCK / (aa.samples * aa.samples); // output pixels of a workgroup
    return launch_aa_resolve(c, mc, o, aa.mode, w, fo, d_stats, s, disk, recs, AaOut{aa.samples, aa.W, aa.d_cover},
                             dim3((unsigned)((aa.W + per_group - 1) / per_group), (unsigned)aa.rows));
}

// The bands of a planned call, one after the other on the call's stream.  own: one private timing quad per band
// (lt_render_aa), or NULL (opts->timing: a pooled quad per band, all of them summed by lt_timing_collect).
static int aa_render_bands(const lt_camera *cam, const lt_metric *metric, const lt_aa *aa, const AaPlan &p, const float *d_bg,
                           int32_t bg_channels, float *d_rgb, uint8_t *d_rgba, uint8_t *d_cover, uint64_t *d_stats,
                           const EventQuad *own)
{
    int rc = aa_check_bg_channels(d_bg, bg_channels);
    if (rc) return rc;
    const int S = aa->samples, W = cam->width;
    const int nch = d_bg ? bg_channels : 3;
    lt_opts o = p.o;
    o.row_block = p.o.row_block * S;
    int64_t row0 = 0; // output rows of the bands before this one
    for (int b = 0; b < p.n_bands; ++b) {
        const size_t i0 = (size_t)b * p.band_blocks, i1 = std::min(p.owned.size(), i0 + (size_t)p.band_blocks);
        int64_t rows = 0;
        for (size_t i = i0; i < i1; ++i) rows += block_rows(p.owned[i], p.o.row_block, cam->height);
        const AaBand band{S, aa->mode, W, rows, d_cover ? d_cover + row0 * W * 4 : nullptr, p.n_bands > 1 ? &p.owned : nullptr, i0, i1 - i0};
        rc = render_dev_impl(&p.fine, metric, &o, d_bg, bg_channels, nullptr, nullptr, nullptr, nullptr,
                             d_rgb ? d_rgb + row0 * W * nch : nullptr, d_rgba ? d_rgba + row0 * W * 4 : nullptr, d_stats,
                             own ? own + b : nullptr, p.has_disk ? &p.dp : nullptr, &band);
        if (rc) return rc;
        row0 += rows;
    }
    return LT_OK;
}

extern "C" int lt_render_aa_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                                const lt_disk *disk, const float *d_bg, int32_t bg_channels, float *d_rgb, uint8_t *d_rgba,
                                uint8_t *d_cover, uint64_t *d_stats)
{
    int rc = require_device();
    if (rc) return rc;
    AaPlan p;
    if ((rc = aa_plan(cam, metric, opts, aa, disk, &p))) return rc;
    return aa_render_bands(cam, metric, aa, p, d_bg, bg_channels, d_rgb, d_rgba, d_cover, d_stats, nullptr);
}

// One private timing quad per launch group of a host-pointer call (a band; the adaptive call's flag kernel and chunks), kept by the slot (grown to the most bands a call had).
static int aa_slot_events(StreamSlot *sl, int n_bands)
{
    while ((int)sl->aa_events.size() < n_bands) {
        EventQuad q{};
        for (int i = 0; i < 4; ++i)
            if (hipEventCreate(&q.e[i]) != hipSuccess) {
                for (int j = 0; j < i; ++j) (void)hipEventDestroy(q.e[j]);
                return fail(LT_ERR_HIP, "hipEventCreate failed");
            }
        sl->aa_events.push_back(q);
    }
    return LT_OK;
}

// The kernel times of the slot's first n quads, added to st: after the wait that follows their launches.
static int aa_add_times(const StreamSlot *sl, int n, lt_stats *st)
{
    for (int b = 0; b < n; ++b) {
        float ms[3] = {0, 0, 0};
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], sl->aa_events[(size_t)b].e[i], sl->aa_events[(size_t)b].e[i + 1]));
        st->prologue_ms += ms[0]; st->integrate_ms += ms[1]; st->epilogue_ms += ms[2];
    }
    return LT_OK;
}

extern "C" int lt_render_aa(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_aa *aa,
                            const lt_disk *disk, const float *bg, int32_t bg_channels, float *out_rgb, uint8_t *out_rgba,
                            uint8_t *out_cover, lt_stats *stats)
{
    int rc = require_device();
    if (rc) return rc;
    AaPlan p;
    if ((rc = aa_plan(cam, metric, opts, aa, disk, &p))) return rc;
    if ((rc = aa_check_bg_channels(bg, bg_channels))) return rc;
    const size_t S = (size_t)aa->samples, n = (size_t)p.rows * cam->width;
    lt_stats st;
    memset(&st, 0, sizeof(st));
    Staging sg; // the background at fine size in, the resolved outputs alone out
    const int i_stats = sg.out(st.counters, LT_STAT_WORDS, 8);
    const int i_bg = sg.in(bg, (size_t)cam->height * S * cam->width * S, bg_channels * sizeof(float));
    const int i_rgb = sg.out(out_rgb, n, (bg ? bg_channels : 3) * 4), i_rgba = sg.out(out_rgba, n, 4), i_cover = sg.out(out_cover, n, 4);
    if ((rc = sg.commit((hipStream_t)p.o.stream))) return rc;
    HIP_TRY(hipMemsetAsync(sg.dev<char>(i_stats), 0, LT_STAT_WORDS * 8, sg.s));
    if ((rc = aa_slot_events(sg.sl, p.n_bands))) return rc;
    p.o.timing = 0;
    if ((rc = aa_render_bands(cam, metric, aa, p, sg.dev<const float>(i_bg), bg_channels, sg.dev<float>(i_rgb), sg.dev<uint8_t>(i_rgba),
                              sg.dev<uint8_t>(i_cover), sg.dev<uint64_t>(i_stats), sg.sl->aa_events.data())))
        return rc;
    for (int i : {i_rgba, i_cover, i_rgb, i_stats}) if ((rc = sg.fetch(i))) return rc;
    HIP_TRY(hipStreamSynchronize(sg.s));
    if ((rc = aa_add_times(sg.sl, p.n_bands, &st))) return rc; // kernel times are summed over the bands
    if (stats) *stats = st;
    return LT_OK;
}
