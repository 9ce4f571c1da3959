// lt_api_transfer.inc -- included at the end of lt_api.hip, after lt_api_thermal.inc.
//
// Host side of the reverberation response (include/ltrace.h, "reverberation"): the refusals in the header's order -- the
// disk spectrum's resolve first, then the g grid's, then the struct's fields, the tables, the key cap and the output --,
// the constants the host computes once, and the launches of lt_transfer.hpp and k_sum_blocks on the default stream.
// The kernel's header is included here, so that lt_api.hip names this file alone.
#include "lt_transfer.hpp"

static_assert(TR_MAX_TAU == LT_TRANSFER_MAX_TAU && TR_MAX_KEYS == LT_TRANSFER_MAX_KEYS, "lt_transfer.hpp restates the header's constants");
static_assert((size_t)LT_SPECTRUM_BLOCKS * LT_TRANSFER_MAX_KEYS * sizeof(double) == (size_t)LT_SPECTRUM_WORKSPACE_BYTES,
              "the partials of the most keys are exactly the spectra's workspace, in one batch");

extern "C" void lt_default_transfer(lt_transfer *t)
{
    memset(t, 0, sizeof(*t));
    t->tau_min = 0.0;
    t->tau_max = 256.0;
    t->n_tau = 64;
    t->n_r = 2;
    t->r_min = 6.0;
    t->r_max = 20.0;
}

// Refusals in the header's order and the constants of its steps 2 and 4 that are computed once.
static int resolve_transfer(const void *hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric, const lt_disk *disk,
                            const lt_spectrum *spec, const lt_transfer *tr, const double *delay, const double *emis, const void *out,
                            SpectrumGrid *sg, TransferShade *ts, int *n_keys)
{
    DiskShade ds;
    int rc = resolve_disk_spectrum(hits, R, W, max_images, metric, disk, &ds);
    if (rc || (rc = resolve_spectrum(spec, max_images, sg))) return rc;
    if (!tr) return fail(LT_ERR_INVALID_ARG, "null transfer");
    if (!std::isfinite(tr->tau_min) || !std::isfinite(tr->tau_max) || !(tr->tau_max > tr->tau_min))
        return fail(LT_ERR_INVALID_ARG, "transfer needs tau_min < tau_max, both finite");
    if (tr->n_tau < 1 || tr->n_tau > LT_TRANSFER_MAX_TAU)
        return fail(LT_ERR_INVALID_ARG, "transfer n_tau %d not in [1, %d]", (int)tr->n_tau, LT_TRANSFER_MAX_TAU);
    if (tr->n_r < 2 || tr->n_r > LT_THERMAL_MAX_NODES)
        return fail(LT_ERR_INVALID_ARG, "transfer n_r %d not in [2, %d]", (int)tr->n_r, LT_THERMAL_MAX_NODES);
    if (!(tr->r_min > 0.0) || !(tr->r_max > tr->r_min) || !std::isfinite(tr->r_max))
        return fail(LT_ERR_INVALID_ARG, "transfer needs 0 < r_min < r_max, both finite");
    if (!std::isfinite(tr->t_ref)) return fail(LT_ERR_INVALID_ARG, "transfer t_ref must be finite");
    if (!delay || !emis) return fail(LT_ERR_INVALID_ARG, "null delay / emis");
    const int64_t keys = (int64_t)sg->planes * (tr->n_tau + 2) * (sg->n_bins + 2);
    if (keys > LT_TRANSFER_MAX_KEYS)
        return fail(LT_ERR_INVALID_ARG, "transfer: planes (n_tau + 2) (n_bins + 2) = %lld keys exceed %d", (long long)keys, LT_TRANSFER_MAX_KEYS);
    if (!out) return fail(LT_ERR_INVALID_ARG, "null out");
    *ts = TransferShade{tr->tau_min, tr->tau_max, (double)tr->n_tau / (tr->tau_max - tr->tau_min),
                        tr->r_min,   tr->r_max,   (double)(tr->n_r - 1) / (tr->r_max - tr->r_min),
                        tr->t_ref,   ds.exposure, tr->n_tau, tr->n_r};
    *n_keys = (int)keys;
    return LT_OK;
}

extern "C" int lt_disk_transfer_dev(const float *d_hits, const uint8_t *d_n_hits, int32_t R, int32_t W, int32_t max_images,
                                    const lt_metric *metric, const lt_disk *disk, const lt_spectrum *spec, const lt_transfer *transfer,
                                    const double *d_delay, const double *d_emis, double *d_out)
{
    SpectrumGrid sg;
    TransferShade ts;
    int n_keys;
    int rc = resolve_transfer(d_hits, R, W, max_images, metric, disk, spec, transfer, d_delay, d_emis, d_out, &sg, &ts, &n_keys);
    if (rc) return rc;
    const dim3 grid(SP_BLOCKS, (unsigned)((n_keys + TR_TILE - 1) / TR_TILE));
    return launch_two_stage(1, n_keys, d_out, [&](double *partial) {
        k_disk_transfer_partial<<<grid, 256, transfer_lds_bytes(max_images)>>>(d_hits, d_n_hits, (int64_t)R * W, max_images, ts, sg, d_delay,
                                                                               d_emis, n_keys, partial);
    });
}

extern "C" int lt_disk_transfer(const float *hits, const uint8_t *n_hits, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                                const lt_disk *disk, const lt_spectrum *spec, const lt_transfer *transfer, const double *delay,
                                const double *emis, double *out)
{
    SpectrumGrid sg;
    TransferShade ts;
    int n_keys;
    int rc = resolve_transfer(hits, R, W, max_images, metric, disk, spec, transfer, delay, emis, out, &sg, &ts, &n_keys);
    if (rc) return rc;
    return staged_hits_call(hits, n_hits, R, W, max_images, {{delay, (size_t)transfer->n_r, 8}, {emis, (size_t)transfer->n_r, 8}},
                            {out, (size_t)n_keys, 8}, [&](void *const *in, void *const *out_) {
        return lt_disk_transfer_dev((const float *)in[0], (const uint8_t *)in[1], R, W, max_images, metric, disk, spec, transfer,
                                    (const double *)in[2], (const double *)in[3], (double *)out_[0]);
    });
}
