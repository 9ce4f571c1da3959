// lt_api_polarization.inc -- included at the end of lt_api.hip, after lt_api_hotspot.inc.
//
// Host side of the linear polarization (include/ltrace.h, "linear polarization"): the polarized trace is the timed trace
// with DiskParams::pol set (same checks, same frame plumbing, the kernels of lt_polarization.hpp); the Stokes frame and
// light curve read the caller's records and run on the default stream, as the hot spot's do.

extern "C" void lt_default_bfield(lt_bfield *b)
{
    memset(b, 0, sizeof(*b));
    b->b_z = 1.0;
    b->pol_frac = 0.7;
}

// Refusals of a field and of an observer, and the rule's constants.
static int resolve_bfield(const lt_metric *metric, double r_obs, double theta_obs, const lt_bfield *b, PolConsts *pc)
{
    if (!metric || !b) return fail(LT_ERR_INVALID_ARG, "null metric / field");
    if (metric->kind != LT_METRIC_KERR) return fail(LT_ERR_UNSUPPORTED, "polarization needs LT_METRIC_KERR");
    if (!(metric->M > 0.0) || !(fabs(metric->a) <= metric->M)) return fail(LT_ERR_INVALID_ARG, "bad metric (M %g, a %g)", metric->M, metric->a);
    const double n2 = b->b_r * b->b_r + b->b_phi * b->b_phi + b->b_z * b->b_z;
    if (!std::isfinite(n2) || !(n2 > 0.0)) return fail(LT_ERR_INVALID_ARG, "the field (b_r, b_phi, b_z) must be finite and not zero");
    if (!(b->pol_frac >= 0.0) || !(b->pol_frac <= 1.0)) return fail(LT_ERR_INVALID_ARG, "pol_frac %g not in [0, 1]", b->pol_frac);
    if (!(r_obs > 0.0) || !std::isfinite(r_obs) || !std::isfinite(theta_obs)) return fail(LT_ERR_INVALID_ARG, "bad observer (r %g, theta %g)", r_obs, theta_obs);
    const double a = metric->a, s = sin(theta_obs), c = cos(theta_obs);
    const double g_tt = -(1.0 - 2.0 * metric->M * r_obs / (r_obs * r_obs + a * a * c * c));
    if (!(g_tt < 0.0) || !(s != 0.0) || !(r_obs * r_obs - 2.0 * metric->M * r_obs + a * a > 0.0))
        return fail(LT_ERR_INVALID_ARG, "no static observer off the axis at r %g, theta %g (g_tt %g)", r_obs, theta_obs, g_tt);
    const double n = sqrt(n2);
    *pc = PolConsts{metric->M, a, r_obs, s, c, {b->b_r / n, b->b_phi / n, b->b_z / n}};
    return LT_OK;
}

static void launch_epilogue_disk_pol(const CamConsts &c, const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w,
                                     const FrameOut &fo, const DiskImagesOut &di, const DiskRecordsBuf &recs, hipStream_t s,
                                     const DiskParams &dp)
{
    launch_epilogue_rows(c, o, fo, [&](auto t, auto, dim3 ge) {
        using T = decltype(t);
        k_epilogue_disk_pol<T><<<ge, EPILOGUE_BLOCK, 0, s>>>(c, mc, ds, dp.pc, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), fo, di, (const T *)recs.tim,
                                                             (const typename Vec2<T>::type *)recs.mom, (float *)dp.d_pol);
    });
}

static void launch_epilogue_arrays_disk_pol(const MetricConsts &mc, const DiskShade &ds, const lt_opts &o, const Workspace &w, int64_t n,
                                            double *d_fa, int64_t *d_w, int8_t *d_st, uint32_t *d_ev, double *d_hits, int32_t *d_n_hits,
                                            hipStream_t s, const DiskParams &dp, const DiskRecordsBuf &recs)
{
    with_precision(o.precision, [&](auto t) {
        using T = decltype(t);
        k_epilogue_arrays_disk_pol<T><<<(unsigned)((n + 255) / 256), 256, 0, s>>>(mc, ds, dp.pc, w.ic<T>(), w.fin0<T>(), w.fin1<T>(), n, d_fa, d_w,
                                                                                 d_st, d_ev, recs.img<T>(), recs.hits, (int64_t)w.n_q,
                                                                                 dp.max_images, (const T *)recs.tim,
                                                                                 (const typename Vec2<T>::type *)recs.mom, d_hits, d_n_hits,
                                                                                 (double *)dp.d_pol);
    });
}

// What the polarized frame entry points do before the frame plumbing takes over.
static int pol_frame_setup(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk, const lt_bfield *field,
                           int32_t *max_images, DiskParams *dp)
{
    int rc = disk_frame_setup(cam, metric, opts, disk, max_images, dp);
    if (rc || (rc = resolve_bfield(metric, cam->r_obs, cam->theta_obs, field, &dp->pc))) return rc;
    dp->timed = dp->pol = true;
    return LT_OK;
}

extern "C" int lt_trace_disk_pol_dev(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                     const lt_bfield *field, int32_t max_images, float *d_fa, uint16_t *d_w, int8_t *d_status,
                                     uint32_t *d_steps, float *d_hits, uint8_t *d_n_hits, float *d_pol, uint64_t *d_stats)
{
    DiskParams dp;
    int rc = pol_frame_setup(cam, metric, opts, disk, field, &max_images, &dp);
    if (rc) return rc;
    dp.d_images = d_hits;
    dp.d_n_hits = d_n_hits;
    dp.d_pol = d_pol;
    return render_dev_impl(cam, metric, opts, nullptr, 3, d_fa, d_w, d_status, d_steps, nullptr, nullptr, d_stats, nullptr, &dp);
}

extern "C" int lt_trace_disk_pol(const lt_camera *cam, const lt_metric *metric, const lt_opts *opts, const lt_disk *disk,
                                 const lt_bfield *field, int32_t max_images, float *out_fa, uint16_t *out_w, int8_t *out_status,
                                 uint32_t *out_steps, float *out_hits, uint8_t *out_n_hits, float *out_pol, lt_stats *stats)
{
    DiskParams dp;
    int rc = pol_frame_setup(cam, metric, opts, disk, field, &max_images, &dp);
    if (rc) return rc;
    return render_host_impl(cam, metric, opts, nullptr, 3, out_fa, out_w, out_status, out_steps, nullptr, nullptr, stats, &dp, nullptr,
                            out_hits, out_n_hits, out_pol);
}

extern "C" int lt_trace_batch_kerr_disk_pol(double M, double a, double r_obs, const double *alphas, const double *thetas,
                                            double theta_obs, double lambda_max, const uint8_t *axis_refines, int integrator,
                                            int precision, const lt_disk *disk, const lt_bfield *field, int32_t max_images, int64_t n,
                                            double *out_fa, int64_t *out_w, int8_t *out_status, double *out_hits, int32_t *out_n_hits,
                                            double *out_pol, uint32_t *out_rhs_evals)
{
    lt_metric m{LT_METRIC_KERR, 0, M, a};
    DiskParams dp;
    lt_opts o;
    MetricConsts mc;
    int rc = disk_batch_setup(&m, r_obs, theta_obs, integrator, precision, disk, &max_images, &dp, &o, &mc);
    if (rc || (rc = resolve_bfield(&m, r_obs, theta_obs, field, &dp.pc))) return rc;
    dp.timed = dp.pol = true;
    return trace_batch(mc, o, lambda_max, alphas, thetas, axis_refines, n, out_fa, out_w, out_status, out_rhs_evals, &dp, nullptr,
                       out_hits, out_n_hits, out_pol);
}

extern "C" int lt_polarization_probe(const lt_metric *metric, double r_obs, double theta_obs, const lt_bfield *field, const double *p_phi,
                                     const double *hit, const double *cam, int64_t n, double *out)
{
    int rc = require_device();
    if (rc) return rc;
    PolConsts pc;
    if ((rc = resolve_bfield(metric, r_obs, theta_obs, field, &pc))) return rc;
    if (n <= 0) return LT_OK;
    if (!p_phi || !hit || !cam || !out) return fail(LT_ERR_INVALID_ARG, "null array");
    Staging st;
    const int i_l = st.in(p_phi, n, 8), i_h = st.in(hit, n, 24), i_c = st.in(cam, n, 16);
    const int i_o = st.out(out, n, 32);
    if ((rc = st.commit(nullptr))) return rc;
    k_polarization_probe<<<(unsigned)((n + 63) / 64), 64>>>(pc, st.dev<const double>(i_l), st.dev<const double>(i_h), st.dev<const double>(i_c), n,
                                                            st.dev<double>(i_o));
    HIP_TRY(hipGetLastError());
    if ((rc = st.fetch(i_o))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return LT_OK;
}

extern "C" int lt_disk_timed_advance_probe(const lt_metric *metric, double r_obs, double lambda_max, double h_max, double r_in, double r_out,
                                           int integrator, int precision, int pol, const double *states, const double *p_phi,
                                           const uint8_t *refine, const double *aux, const uint32_t *steps, const uint8_t *act,
                                           const double *k1, const double *sc0, const double *lane, const int32_t *lane_int, int64_t n,
                                           int32_t max_images, int32_t iters, double *out_state, double *out_aux, double *out_k1,
                                           double *out_sc, int32_t *out_int, double *out_lane, int32_t *out_lane_int, double *out_img,
                                           double *out_tim, double *out_mom, double *out_trace)
{
    MetricConsts mc;
    DiskParams dp;
    int rc = disk_probe_setup(metric, r_obs, r_in, r_out, &mc, &dp);
    if (rc) return rc;
    if (precision != 32 && precision != 64) return fail(LT_ERR_INVALID_ARG, "precision must be 32 or 64");
    const bool is_dp45 = integrator == LT_INTEGRATOR_DP45 || integrator == LT_INTEGRATOR_DP45_EXACT;
    if (!(integrator == LT_INTEGRATOR_RK4 || (is_dp45 && precision == 64)))
        return fail(LT_ERR_UNSUPPORTED, "the timed advance probe runs RK4 (float32, float64), DP45 and DP45-exact (float64)");
    if (!(h_max > 0.0)) return fail(LT_ERR_INVALID_ARG, "h_max must be positive");
    if (max_images < 1 || max_images > DISK_MAX_IMAGES) return fail(LT_ERR_INVALID_ARG, "max_images %d not in [1, %d]", max_images, DISK_MAX_IMAGES);
    if (iters < 1 || iters > (1 << 20)) return fail(LT_ERR_INVALID_ARG, "iters %d not in [1, 2^20]", iters);
    if (n <= 0) return LT_OK;
    if (out_trace && (double)n * iters * 7 > (double)(1 << 28)) return fail(LT_ERR_INVALID_ARG, "trace of %lld x %d rows too large", (long long)n, iters);
    if (!states || !p_phi || !refine || !aux || !steps || !act || !lane || !lane_int || !out_state || !out_aux || !out_k1 || !out_sc ||
        !out_int || !out_lane || !out_lane_int || !out_img || !out_tim || !out_mom)
        return fail(LT_ERR_INVALID_ARG, "null pointer");
    const size_t el = elem_size(precision), slots = (size_t)max_images * (size_t)n, tr = out_trace ? (size_t)n * iters * 56 : 0;
    DevBuf ds, dl, dr, da, dst, dac, dk, dsc, dla, dli, wi, wt, wm, os, oa, ok, osc, oi, ol, oli, og, ot, om, otr;
    if ((rc = probe_upload(ds, states, n * 40)) || (rc = probe_upload(dl, p_phi, n * 8)) || (rc = probe_upload(dr, refine, n)) ||
        (rc = probe_upload(da, aux, n * 16)) || (rc = probe_upload(dst, steps, n * 4)) || (rc = probe_upload(dac, act, n)) ||
        (rc = probe_upload(dk, k1, n * 40)) || (rc = probe_upload(dsc, sc0, n * 16)) || (rc = probe_upload(dla, lane, n * 40)) ||
        (rc = probe_upload(dli, lane_int, n * 8)) || (rc = wi.alloc(slots * 2 * el)) || (rc = wt.alloc(slots * el)) ||
        (rc = wm.alloc(slots * 2 * el)) || (rc = os.alloc(n * 40)) || (rc = oa.alloc(n * 16)) || (rc = ok.alloc(n * 40)) ||
        (rc = osc.alloc(n * 16)) || (rc = oi.alloc(n * 12)) || (rc = ol.alloc(n * 40)) || (rc = oli.alloc(n * 8)) ||
        (rc = og.alloc(slots * 16)) || (rc = ot.alloc(slots * 8)) || (rc = om.alloc(slots * 16)) || (tr && (rc = otr.alloc(tr))))
        return rc;
    if (tr) HIP_TRY(hipMemset(otr.p, 0xff, tr)); // NaN in the rows of iterations a lane did not run
    TimedProbeIo io{};
    io.states = (const double *)ds.p; io.p_phi = (const double *)dl.p; io.aux = (const double *)da.p; io.k1 = (const double *)dk.p;
    io.sc0 = (const double *)dsc.p; io.lane = (const double *)dla.p; io.refine = (const uint8_t *)dr.p; io.act = (const uint8_t *)dac.p;
    io.steps = (const uint32_t *)dst.p; io.lane_int = (const int32_t *)dli.p; io.n = n; io.max_images = max_images; io.iters = iters;
    io.w_img = wi.p; io.w_tim = wt.p; io.w_mom = wm.p;
    io.out_state = (double *)os.p; io.out_aux = (double *)oa.p; io.out_k1 = (double *)ok.p; io.out_sc = (double *)osc.p;
    io.out_lane = (double *)ol.p; io.out_img = (double *)og.p; io.out_tim = (double *)ot.p; io.out_mom = (double *)om.p;
    io.trace = tr ? (double *)otr.p : nullptr; io.out_int = (int32_t *)oi.p; io.out_lane_int = (int32_t *)oli.p;
    auto launch = [&](auto t, auto integ) {
        using T = decltype(t);
        using Integ = decltype(integ);
        const unsigned g = (unsigned)((n + 63) / 64);
        if (pol) k_disk_timed_advance_probe<T, Integ, true><<<g, 64>>>(make_kerr<T>(mc, lambda_max, h_max), make_disk_consts<T>(mc, dp), io);
        else k_disk_timed_advance_probe<T, Integ, false><<<g, 64>>>(make_kerr<T>(mc, lambda_max, h_max), make_disk_consts<T>(mc, dp), io);
    };
    if (integrator == LT_INTEGRATOR_DP45_EXACT) launch(double{}, Dp45<double, true>{});
    else if (integrator == LT_INTEGRATOR_DP45) launch(double{}, Dp45<double, false>{});
    else if (precision == 32) launch(float{}, Rk4<float>{});
    else launch(double{}, Rk4<double>{});
    HIP_TRY(hipGetLastError());
    if ((rc = probe_download(out_state, os, n * 40)) || (rc = probe_download(out_aux, oa, n * 16)) || (rc = probe_download(out_k1, ok, n * 40)) ||
        (rc = probe_download(out_sc, osc, n * 16)) || (rc = probe_download(out_int, oi, n * 12)) || (rc = probe_download(out_lane, ol, n * 40)) ||
        (rc = probe_download(out_lane_int, oli, n * 8)) || (rc = probe_download(out_img, og, slots * 16)) ||
        (rc = probe_download(out_tim, ot, slots * 8)) || (rc = probe_download(out_mom, om, slots * 16)) ||
        (tr && (rc = probe_download(out_trace, otr, tr)))) return rc;
    return LT_OK;
}

// The hot spot's refusals (resolve_hotspot) plus the field's and the polarization records'.
static int resolve_stokes(const void *hits, const void *pol, int32_t R, int32_t W, int32_t max_images, const lt_metric *metric,
                          const lt_disk *disk, const lt_hotspot *spot, const lt_bfield *field, DiskShade *ds, HotspotShade *hs)
{
    int rc = resolve_hotspot(hits, R, W, max_images, metric, disk, spot, ds, hs);
    if (rc) return rc;
    PolConsts pc;
    if ((rc = resolve_bfield(metric, 4.0 * metric->M, M_PI / 2, field, &pc))) return rc; // (the observer plays no part here)
    if (!pol) return fail(LT_ERR_INVALID_ARG, "null pol");
    return LT_OK;
}

extern "C" int lt_shade_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                   int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                   const lt_bfield *field, double t_obs, float *d_iqu)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_stokes(d_hits, d_pol, R, W, max_images, metric, disk, spot, field, &ds, &hs);
    if (rc || (rc = check_t_obs(t_obs))) return rc;
    if (!d_iqu) return fail(LT_ERR_INVALID_ARG, "null out");
    const int64_t n_px = (int64_t)R * W;
    k_shade_stokes<<<(unsigned)((n_px + 255) / 256), 256>>>(d_hits, d_n_hits, d_pol, n_px, max_images, ds, hs, field->pol_frac, t_obs, d_iqu);
    HIP_TRY(hipGetLastError());
    return LT_OK;
}

extern "C" int lt_shade_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W, int32_t max_images,
                               const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot, const lt_bfield *field, double t_obs,
                               float *out_iqu)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_stokes(hits, pol, R, W, max_images, metric, disk, spot, field, &ds, &hs);
    if (rc) return rc;
    const size_t n = (size_t)R * W, rec = (size_t)max_images * 16;
    return staged_call({{hits, n, rec}, {n_hits, n, 1}, {pol, n, rec}}, {{out_iqu, n, 12}}, [&](void *const *in, void *const *out) {
        return lt_shade_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric, disk, spot,
                                   field, t_obs, (float *)out[0]);
    });
}

extern "C" int lt_hotspot_lightcurve_stokes_dev(const float *d_hits, const uint8_t *d_n_hits, const float *d_pol, int32_t R, int32_t W,
                                                int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                                const lt_bfield *field, double t_start, double dt, int32_t n_times, double *d_out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_stokes(d_hits, d_pol, R, W, max_images, metric, disk, spot, field, &ds, &hs);
    if (rc) return rc;
    return launch_lightcurve(t_start, dt, n_times, d_out, [&](dim3 grid, double *partial) {
        k_lightcurve_stokes_partial<<<grid, 256>>>(d_hits, d_n_hits, d_pol, (int64_t)R * W, max_images, hs, field->pol_frac, t_start, dt,
                                                   partial);
    });
}

extern "C" int lt_hotspot_lightcurve_stokes(const float *hits, const uint8_t *n_hits, const float *pol, int32_t R, int32_t W,
                                            int32_t max_images, const lt_metric *metric, const lt_disk *disk, const lt_hotspot *spot,
                                            const lt_bfield *field, double t_start, double dt, int32_t n_times, double *out)
{
    DiskShade ds;
    HotspotShade hs;
    int rc = resolve_stokes(hits, pol, R, W, max_images, metric, disk, spot, field, &ds, &hs);
    if (rc || (rc = check_n_times(n_times))) return rc;
    const size_t n = (size_t)R * W, rec = (size_t)max_images * 16;
    return staged_call({{hits, n, rec}, {n_hits, n, 1}, {pol, n, rec}}, {{out, (size_t)n_times, 24}}, [&](void *const *in, void *const *out_) {
        return lt_hotspot_lightcurve_stokes_dev((const float *)in[0], (const uint8_t *)in[1], (const float *)in[2], R, W, max_images, metric,
                                                disk, spot, field, t_start, dt, n_times, (double *)out_[0]);
    });
}
