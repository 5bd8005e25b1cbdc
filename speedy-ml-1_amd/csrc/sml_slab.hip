// sml_slab.hip -- the slab ocean of an E-member forecast on one rank: the slab reservoirs'
// step for every member through one stream of their weights (sml_res_step_members) and
// sendrecievegrid's sst half (mpires.f90:288-478, 575-767) with a member dimension, one
// launch per stage (sml_slab.hpp).  The single-member loop's slab ocean
// (parallelmain.f90:216-249; cpl_sea.f90:38-46) is this context at E = 1 over one rank's
// share of the regions: sml_hybrid_set_slab / sml_hybrid_start_slab and the slab stages of
// sml_hybrid_predict / sml_hybrid_advance drive sml::slab_* below; the host of an
// ensemble strings the C calls together in that loop's order
// (speedy_ml_amd.ensemble.EnsembleLoop).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "sml_devmem.hpp"
#include "sml_internal.hpp"
#include "sml_slab.hpp"
#include "sml_slab_layout.hpp"
#include "sml_slab_series.hpp"

using namespace sml;

struct sml_slab {
    DevMem mem;  // first: every device buffer below is its
    sml_reservoirs *atmo = nullptr, *res = nullptr;
    int E = 1, numregions = 0, nlocal = 0, nout = 0, xw = 0;
    int64_t fb_packed = 0;  // the atmo context's packed feedback size, for the C ABI's stride checks
    int nslab = 0, nsst = 4, ratio = 28, tot_fb = 0, n_sst_el = 0;
    int timestep = 6, timestep_slab = 168;
    double sst_bias = 0.0;  // current_sst_bias, for each member's sml_dyn_set_hybrid_sst
    const double *base = nullptr, *mask = nullptr;  // base_sst_grid, sea_mask (96, 48)
    // per member, packed: the slab feedback [tot_fb], the slab outvecs [nslab][nsst], the
    // ring [ratio - 1][tot_fb], wholegrid_sst [96 * 48]; the slabs' sst mean / std [nslab][2]
    double *d_fb = nullptr, *d_ov = nullptr, *d_ring = nullptr, *d_sst = nullptr, *d_ms = nullptr;
    int32_t *d_ring_src = nullptr, *d_row = nullptr, *d_sst_src = nullptr, *d_sfb = nullptr, *d_sgrid = nullptr;
    uint16_t *d_sreg = nullptr;
    std::vector<char> started;  // per member
    bool dirty = false;
    int64_t fb_stride() const { return std::max(tot_fb, 1); }
    int64_t ov_stride() const { return std::max(nslab * nsst, 1); }
    int64_t ring_stride() const { return std::max<int64_t>((int64_t)(ratio - 1) * tot_fb, 1); }
};

namespace {

template <typename T>
int upload(sml_slab *s, T **d, const std::vector<T> &v) {
    if (s->mem.device(d, std::max<size_t>(v.size(), 1), false)) return fail(SML_ERR_NOMEM, "slab tables");
    if (!v.empty()) SML_HIP(hipMemcpy(*d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return SML_OK;
}

int create_impl(sml_slab *s, const double *d_base_sst, const double *d_sea_mask, int timestep, int timestep_slab) {
    int numregions = 0, snum = 0, sncs = 0, snout = 0, sE = 0;
    if (int rc = sml_res_info(s->atmo, &numregions, &s->nlocal, nullptr, &s->nout, nullptr)) return rc;
    if (int rc = sml_res_info(s->res, &snum, &s->nslab, &sncs, &snout, nullptr)) return rc;
    if (int rc = sml_res_members(s->atmo, &s->E)) return rc;
    if (int rc = sml_res_members(s->res, &sE)) return rc;
    SML_REQUIRE(sE == s->E, "the slab context holds %d members, the atmo context %d (sml_res_set_members)", sE, s->E);
    const int nlocal = s->nlocal, nslab = s->nslab;
    std::vector<int> ids(nlocal), sids(nslab), ninp(nlocal), sninp(nslab);
    std::vector<int64_t> off(nlocal + 1), soff(nslab + 1);
    if (int rc = sml_res_info(s->atmo, nullptr, nullptr, nullptr, nullptr, ids.data())) return rc;
    if (int rc = sml_res_info(s->res, nullptr, nullptr, nullptr, nullptr, sids.data())) return rc;
    if (int rc = sml_res_feedback_offsets(s->atmo, off.data())) return rc;
    if (int rc = sml_res_feedback_offsets(s->res, soff.data())) return rc;
    for (int i = 0; i < nlocal; ++i)
        if (int rc = sml_res_ninp(s->atmo, i, &ninp[i])) return rc;
    for (int j = 0; j < nslab; ++j)
        if (int rc = sml_res_ninp(s->res, j, &sninp[j])) return rc;
    // the index tables and their consistency checks: host arithmetic (sml_slab_layout.cpp)
    SlabTables tb;
    if (int rc = build_slab_tables({numregions, nlocal, s->nout, ids.data(), ninp.data(), off.data(), snum, nslab, sncs,
                                    snout, sids.data(), sninp.data(), soff.data()},
                                   &tb))
        return rc;
    s->numregions = numregions;
    s->fb_packed = off[nlocal];
    s->nsst = snout;
    s->ratio = timestep_slab / timestep;
    s->timestep = timestep;
    s->timestep_slab = timestep_slab;
    s->base = d_base_sst;
    s->mask = d_sea_mask;
    s->tot_fb = (int)tb.ring_src.size();
    s->n_sst_el = (int)tb.sfb.size();
    s->xw = tb.xw;
    if (int rc = upload(s, &s->d_ring_src, tb.ring_src)) return rc;
    if (int rc = upload(s, &s->d_row, tb.row)) return rc;
    if (int rc = upload(s, &s->d_sst_src, tb.src)) return rc;
    if (int rc = upload(s, &s->d_sfb, tb.sfb)) return rc;
    if (int rc = upload(s, &s->d_sgrid, tb.sgrid)) return rc;
    if (int rc = upload(s, &s->d_sreg, tb.sreg)) return rc;
    const size_t E = (size_t)s->E;
    s->mem.device(&s->d_fb, E * s->fb_stride());
    s->mem.device(&s->d_ov, E * s->ov_stride());
    s->mem.device(&s->d_ring, E * s->ring_stride());
    s->mem.device(&s->d_sst, E * kGrid2d);
    s->mem.device(&s->d_ms, std::max<size_t>((size_t)2 * nslab, 1));
    if (s->mem.status()) return fail(SML_ERR_NOMEM, "slab buffers");
    s->started.assign(s->E, 0);
    return SML_OK;
}

// the members' local outvecs [E][nlocal][xw], every region's [E][numregions][xw] and
// feedbacks [E][>= the packed feedback]: the C ABI's checks, against sizes stored at create
int check_ov_stride(const sml_slab *s, int64_t ov_stride) {
    SML_REQUIRE(ov_stride >= (int64_t)s->nlocal * s->xw, "ov_stride %lld smaller than nlocal * the exchange width %d",
                (long long)ov_stride, s->xw);
    return SML_OK;
}
int check_fb_stride(const sml_slab *s, int64_t fb_stride) {
    SML_REQUIRE(fb_stride >= s->fb_packed, "fb_stride %lld smaller than the packed feedback size %lld",
                (long long)fb_stride, (long long)s->fb_packed);
    return SML_OK;
}

}  // namespace

// ---- the context behind the C ABI (sml_internal.hpp): what the native loop drives at one
// member over its rank's share of the regions.  The stage functions check no argument and
// allocate nothing: the loop enqueues them every step on its serial path.
int sml::slab_create(sml_reservoirs *atmo, sml_reservoirs *slab, const double *d_base_sst, const double *d_sea_mask,
                     int timestep, int timestep_slab, double sst_bias, sml_slab **out) {
    *out = nullptr;
    if (int rc = check_slab_cadence(timestep, timestep_slab)) return rc;
    sml_slab *s = new (std::nothrow) sml_slab();
    if (!s) return fail(SML_ERR_NOMEM, "host allocation failed");
    s->atmo = atmo;
    s->res = slab;
    s->sst_bias = sst_bias;
    if (int rc = create_impl(s, d_base_sst, d_sea_mask, timestep, timestep_slab)) {
        delete s;
        return rc;
    }
    *out = s;
    return SML_OK;
}

// start_prediction_slab's hand-over for one member (mod_slab_ocean_reservoir.f90:769-800,
// parallelmain.f90:216-222): 272 K in every sst column of the member's exchange rows
// (mpires.f90:366-372), its slab outvecs over them, its ring cleared
// (initialize_prediction_slab, :747-748).  The slabs' sst mean / std are read again on
// every start: a host may load new slab weights between two starts, and the start
// synchronises anyway.
int sml::slab_start(sml_slab *s, int member, const double *d_slab_outvec, double *d_outvec, int64_t ov_stride,
                    void *stream) {
    hipStream_t m = (hipStream_t)stream;
    std::vector<double> ms(2 * (size_t)s->nslab);
    for (int j = 0; j < s->nslab; ++j) {
        double mean[36], stdv[36];
        if (int rc = sml_res_mean_std(s->res, j, mean, stdv)) return rc;
        ms[2 * j] = mean[35];  // sst_mean_std_idx = the atmo grid's, 36 (mod_slab_ocean_reservoir.f90:1548)
        ms[2 * j + 1] = stdv[35];
    }
    if (s->nslab)  // (a rank without sst regions has no slab mean / std)
        SML_HIP(hipMemcpyAsync(s->d_ms, ms.data(), ms.size() * 8, hipMemcpyHostToDevice, m));
    double *ov = d_outvec + (size_t)member * ov_stride;
    double *sov = s->d_ov + (size_t)member * s->ov_stride();
    if (s->tot_fb)
        SML_HIP(hipMemsetAsync(s->d_ring + (size_t)member * s->ring_stride(), 0,
                               (size_t)(s->ratio - 1) * s->tot_fb * 8, m));
    const int n = s->nslab * s->nsst;
    if (s->nlocal) launch_slab_fill(s->nsst, s->nlocal, s->nout, s->xw, ov, 0, 1, m);
    if (n) {
        SML_HIP(hipMemcpyAsync(sov, d_slab_outvec, (size_t)n * 8, hipMemcpyDeviceToDevice, m));
        launch_slab_rows(sov, 0, s->d_row, s->nslab, s->nsst, s->nlocal, s->nout, s->xw, ov, 0, 1, m);
    }
    SML_HIP(hipGetLastError());
    SML_HIP(hipStreamSynchronize(m));
    s->dirty = true;
    s->started[member] = 1;
    return SML_OK;
}

// predict_slab_ml of every member's slab reservoirs on a slab step (parallelmain.f90:236-249:
// mod(t_next * timestep, timestep_slab) == 0, the default ml_only_ocean set by
// initialize_slab_ocean_model), nothing on the others: the feedback is the mean of the
// ring as the previous step's sendrecievegrid left it (mpires.f90:757), and the new sst
// goes into the local exchange rows
int sml::slab_predict(sml_slab *s, int64_t t_next, double *d_outvec, int64_t ov_stride, void *stream, int *predicted) {
    if (predicted) *predicted = 0;
    for (int e = 0; e < s->E; ++e)
        if (!s->started[e]) return fail(SML_ERR_STATE, "sml_slab_start of member %d first", e);
    if ((t_next * s->timestep) % s->timestep_slab != 0) return SML_OK;
    // a slab step on every rank: the other ranks' rows carry new sst, so wholegrid_sst
    // and the window's sst are rebuilt too, even when this rank predicts none
    s->dirty = true;
    if (predicted) *predicted = 1;
    if (s->nslab == 0) return SML_OK;
    hipStream_t m = (hipStream_t)stream;
    launch_slab_avg(s->d_ring, s->ring_stride(), s->ratio - 1, s->tot_fb, s->d_fb, s->fb_stride(), s->E, m);
    SML_HIP(hipGetLastError());
    if (int rc = sml_res_step_members(s->res, s->d_fb, s->fb_stride(), nullptr, 0, s->d_ov, s->ov_stride(), m))
        return rc;
    launch_slab_rows(s->d_ov, s->ov_stride(), s->d_row, s->nslab, s->nsst, s->nlocal, s->nout, s->xw, d_outvec,
                     ov_stride, s->E, m);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// sendrecievegrid's sst half (mpires.f90:288-319, 458-472, 575-581, 733-736) after a
// change of any region's slab sst: the E wholegrid_sst grids from every region's exchange
// rows (global region order) and the sst entries of the E local atmo feedbacks
int sml::slab_sst(sml_slab *s, const double *d_outvec_all, int64_t all_stride, double *d_feedback, int64_t fb_stride,
                  void *stream, int *wrote) {
    if (wrote) *wrote = 0;
    if (!s->dirty) return SML_OK;
    hipStream_t m = (hipStream_t)stream;
    launch_sst_grid(d_outvec_all, all_stride, s->d_sst_src, s->base, s->mask, s->d_sst, kGrid2d, s->E, m);
    SML_HIP(hipGetLastError());
    if (s->n_sst_el) {
        launch_sst_feedback(s->d_sst, kGrid2d, s->d_sfb, s->d_sgrid, s->d_sreg, s->d_ms, s->n_sst_el, d_feedback,
                            fb_stride, s->E, m);
        SML_HIP(hipGetLastError());
    }
    s->dirty = false;
    if (wrote) *wrote = 1;
    return SML_OK;
}

// averaged_atmo_input_vec(:, mod(t-1, R-1)+1) of every member from the E feedbacks (mpires.f90:755)
int sml::slab_ring(sml_slab *s, int64_t t, const double *d_feedback, int64_t fb_stride, void *stream) {
    if (!s->tot_fb) return SML_OK;
    double *col = s->d_ring + (size_t)((t - 1) % (s->ratio - 1)) * s->tot_fb;
    launch_slab_ring(d_feedback, fb_stride, s->d_ring_src, s->tot_fb, col, s->ring_stride(), s->E, (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

void sml::slab_strides(const sml_slab *s, int64_t *ov_stride, int64_t *all_stride, int64_t *fb_stride) {
    *ov_stride = (int64_t)s->nlocal * s->xw;
    *all_stride = (int64_t)s->numregions * s->xw;
    *fb_stride = s->fb_packed;
}

// ---- the C ABI: argument checks over the above
extern "C" int sml_slab_create(sml_reservoirs *atmo, sml_reservoirs *slab, const double *d_base_sst,
                               const double *d_sea_mask, int timestep, int timestep_slab, double sst_bias,
                               sml_slab **out) {
    SML_REQUIRE(out, "null argument");
    *out = nullptr;
    SML_REQUIRE(atmo && slab && d_base_sst && d_sea_mask, "null argument");
    if (int rc = check_slab_cadence(timestep, timestep_slab)) return rc;
    // (the members' exchange rows are read as every region's: one buffer for both)
    SML_REQUIRE(res_in_global_order(atmo), "the atmo context must hold every region, in global order (one rank)");
    sml_slab *s = nullptr;
    if (int rc = slab_create(atmo, slab, d_base_sst, d_sea_mask, timestep, timestep_slab, sst_bias, &s)) return rc;
    if (int rc = sml_res_set_outvec_ld(atmo, s->xw)) {
        delete s;
        return rc;
    }
    *out = s;
    return SML_OK;
}

extern "C" int sml_slab_destroy(sml_slab *s) {
    if (!s) return SML_OK;
    (void)hipDeviceSynchronize();
    delete s;
    return SML_OK;
}

extern "C" int sml_slab_info(const sml_slab *s, int *members, int *exchange_width, int *nslab, int *ring_columns,
                             int *ring_len, double *sst_bias) {
    SML_REQUIRE(s, "null context");
    if (members) *members = s->E;
    if (exchange_width) *exchange_width = s->xw;
    if (nslab) *nslab = s->nslab;
    if (ring_columns) *ring_columns = s->ratio - 1;
    if (ring_len) *ring_len = s->tot_fb;
    if (sst_bias) *sst_bias = s->sst_bias;
    return SML_OK;
}

extern "C" int sml_slab_start(sml_slab *s, int member, const double *d_slab_outvec, double *d_outvec,
                              int64_t ov_stride, void *stream) {
    SML_REQUIRE(s && d_outvec, "null argument");
    SML_REQUIRE(member >= 0 && member < s->E, "member %d out of range [0, %d)", member, s->E);
    SML_REQUIRE(s->nslab == 0 || d_slab_outvec, "null slab outvec");
    if (int rc = check_ov_stride(s, ov_stride)) return rc;
    return slab_start(s, member, d_slab_outvec, d_outvec, ov_stride, stream);
}

extern "C" int sml_slab_predict(sml_slab *s, int64_t t_next, double *d_outvec, int64_t ov_stride, void *stream,
                                int *predicted) {
    SML_REQUIRE(s && d_outvec && t_next >= 1, "bad argument");
    if (predicted) *predicted = 0;
    if (int rc = check_ov_stride(s, ov_stride)) return rc;
    return slab_predict(s, t_next, d_outvec, ov_stride, stream, predicted);
}

extern "C" int sml_slab_sst(sml_slab *s, const double *d_outvec, int64_t ov_stride, double *d_feedback,
                            int64_t fb_stride, void *stream, int *wrote) {
    SML_REQUIRE(s && d_outvec && d_feedback, "null argument");
    if (wrote) *wrote = 0;
    if (int rc = check_ov_stride(s, ov_stride)) return rc;
    if (int rc = check_fb_stride(s, fb_stride)) return rc;
    return slab_sst(s, d_outvec, ov_stride, d_feedback, fb_stride, stream, wrote);
}

extern "C" int sml_slab_ring(sml_slab *s, int64_t t, const double *d_feedback, int64_t fb_stride, void *stream) {
    SML_REQUIRE(s && d_feedback && t >= 1, "bad argument");
    if (int rc = check_fb_stride(s, fb_stride)) return rc;
    return slab_ring(s, t, d_feedback, fb_stride, stream);
}

// ---- the slab reservoirs' training inputs (sml_slab_series.hpp): every argument is
// checked before anything is enqueued -- the scalars first, which need no context
extern "C" int sml_slab_train_series(sml_reservoirs *atmo, const sml_reservoirs *slab, const double *d_g4,
                                     int64_t g4_stride, const double *d_g2, const double *d_pr, const double *d_sst,
                                     const double *d_tisr, int64_t g2_stride, int T, int window, int divisor, int t0,
                                     int ncols, double *d_out, int64_t out_stride, void *stream) {
    SML_REQUIRE(T >= 1, "T = %d: a series holds one step at least", T);
    SML_REQUIRE(window >= 1 && window <= 1024, "window = %d outside [1, 1024]", window);
    SML_REQUIRE(divisor >= 1, "divisor = %d: at least 1", divisor);
    SML_REQUIRE(t0 >= 0 && ncols >= 0 && (int64_t)t0 + ncols <= T, "columns t0 = %d, ncols = %d leave the series' %d steps",
                t0, ncols, T);
    SML_REQUIRE(g4_stride >= kGrid4d, "g4_stride %lld smaller than the 4-d grid's %d doubles", (long long)g4_stride,
                kGrid4d);
    SML_REQUIRE(g2_stride >= kGrid2d, "g2_stride %lld smaller than a 2-d grid's %d doubles", (long long)g2_stride,
                kGrid2d);
    SML_REQUIRE(g4_stride % 2 == 0, "g4_stride %lld is odd: every step's 4-d grid must be 16-byte aligned",
                (long long)g4_stride);
    SML_REQUIRE(atmo && slab, "null reservoir context");
    SML_REQUIRE(d_g4 && d_g2 && d_pr && d_sst && d_out, "null argument (d_g4, d_g2, d_pr, d_sst and d_out are needed)");
    SML_REQUIRE((uintptr_t)d_g4 % 16 == 0, "d_g4 %p is not 16-byte aligned", (const void *)d_g4);
    // both contexts as the getters report them, for the layout unit's checks
    int numregions = 0, nlocal = 0, nout = 0, snum = 0, nslab = 0, sncs = 0, snout = 0;
    if (int rc = sml_res_info(atmo, &numregions, &nlocal, nullptr, &nout, nullptr)) return rc;
    if (int rc = sml_res_info(slab, &snum, &nslab, &sncs, &snout, nullptr)) return rc;
    std::vector<int> ids(nlocal), sids(nslab), ninp(nlocal), sninp(nslab);
    std::vector<int64_t> off(nlocal + 1), soff(nslab + 1);
    if (int rc = sml_res_info(atmo, nullptr, nullptr, nullptr, nullptr, ids.data())) return rc;
    if (int rc = sml_res_info(slab, nullptr, nullptr, nullptr, nullptr, sids.data())) return rc;
    if (int rc = sml_res_feedback_offsets(atmo, off.data())) return rc;
    if (int rc = sml_res_feedback_offsets(slab, soff.data())) return rc;
    for (int i = 0; i < nlocal; ++i)
        if (int rc = sml_res_ninp(atmo, i, &ninp[i])) return rc;
    for (int j = 0; j < nslab; ++j)
        if (int rc = sml_res_ninp(slab, j, &sninp[j])) return rc;
    SlabSeriesDev tb{};
    if (int rc = res_slab_series(atmo, {numregions, nlocal, nout, ids.data(), ninp.data(), off.data(), snum, nslab, sncs,
                                        snout, sids.data(), sninp.data(), soff.data()},
                                 &tb))
        return rc;
    SML_REQUIRE(out_stride >= soff[nslab], "out_stride %lld smaller than the slab's packed feedback size %lld",
                (long long)out_stride, (long long)soff[nslab]);
    if (ncols == 0 || tb.tot == 0) return SML_OK;
    const SlabSeriesIn in{d_g4, d_g2, d_pr, d_sst, d_tisr, g4_stride, g2_stride};
    launch_slab_series(tb.src, tb.l, tb.row, tb.meanstd, in, tb.tot, window, divisor, t0, t0 + ncols, d_out, out_stride,
                       (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_slab_buffers(const sml_slab *s, const double **d_sst_grid, int64_t *sst_stride,
                                const double **d_ring, int64_t *ring_stride, const double **d_slab_feedback,
                                int64_t *fb_stride, const double **d_slab_outvec, int64_t *ov_stride) {
    SML_REQUIRE(s, "null context");
    if (d_sst_grid) *d_sst_grid = s->d_sst;
    if (sst_stride) *sst_stride = kGrid2d;
    if (d_ring) *d_ring = s->d_ring;
    if (ring_stride) *ring_stride = s->ring_stride();
    if (d_slab_feedback) *d_slab_feedback = s->d_fb;
    if (fb_stride) *fb_stride = s->fb_stride();
    if (d_slab_outvec) *d_slab_outvec = s->d_ov;
    if (ov_stride) *ov_stride = s->ov_stride();
    return SML_OK;
}
