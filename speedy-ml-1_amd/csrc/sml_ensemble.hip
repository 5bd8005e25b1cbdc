// sml_ensemble.hip -- the products of an E-member forecast on one rank: the per-point mean
// and spread of the members' assembled grids and, per step, a row of area-weighted scores
// against a verifying analysis (rmse of the mean, spread, fair CRPS, bias, rank histogram)
// for each of the 34 fields, in two device tables the context owns.  The kernels are in
// sml_ens_products.hpp, the field table, the weights and the argument checks in the
// host-only sml_ens_layout.cpp.  Every launch is stream-ordered with no host
// synchronisation; the calls on one context are to be ordered among themselves (they share
// the row partials), as a loop's main stream orders them (speedy_ml_amd.ensemble).
#include <hip/hip_runtime.h>

#include <new>

#include "sml_devmem.hpp"
#include "sml_ens_layout.hpp"
#include "sml_ens_products.hpp"
#include "sml_internal.hpp"

using namespace sml;

struct sml_ens {
    DevMem mem;  // first: every device buffer below is its
    int E = 1, T = 1;
    double *d_w = nullptr;         // [48] the weight of one point of row j
    double *d_scores = nullptr;    // [T][34][4]
    int32_t *d_ranks = nullptr;    // [T][34][33]
    double *d_part = nullptr;      // [34][48][4] the row partials of the step in flight
    int32_t *d_rpart = nullptr;    // [34][48][33]
    int64_t nscores() const { return ens_score_offset(T, 0); }
    int64_t nranks() const { return ens_rank_offset(T, 0); }
};

extern "C" int sml_ens_weights(double *w48) { return ens_weights(w48); }

extern "C" int sml_ens_create(int members, int capacity_steps, sml_ens **out) {
    SML_REQUIRE(out, "null argument");
    *out = nullptr;
    if (int rc = check_ens_create(members, capacity_steps)) return rc;
    double w[kYGrid];
    if (int rc = ens_weights(w)) return rc;
    sml_ens *e = new (std::nothrow) sml_ens();
    if (!e) return fail(SML_ERR_NOMEM, "host allocation failed");
    e->E = members;
    e->T = capacity_steps;
    e->mem.device(&e->d_w, kYGrid, false);
    e->mem.device(&e->d_scores, (size_t)e->nscores(), false);
    e->mem.device(&e->d_ranks, (size_t)e->nranks(), false);
    e->mem.device(&e->d_part, (size_t)kEnsFields * kYGrid * kEnsScores);
    e->mem.device(&e->d_rpart, (size_t)kEnsFields * kYGrid * kEnsRankBins);
    int rc = e->mem.status() ? fail(SML_ERR_NOMEM, "ensemble product tables") : SML_OK;
    if (!rc && hipMemcpy(e->d_w, w, sizeof w, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(SML_ERR_HIP, "the area weights' upload failed");
    if (!rc) {
        launch_ens_reset(e->d_scores, e->nscores(), e->d_ranks, e->nranks(), nullptr);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess)
            rc = fail(SML_ERR_HIP, "the tables' first reset failed");
    }
    if (rc) {
        delete e;
        return rc;
    }
    *out = e;
    return SML_OK;
}

extern "C" int sml_ens_destroy(sml_ens *e) {
    if (!e) return SML_OK;
    (void)hipDeviceSynchronize();
    delete e;
    return SML_OK;
}

extern "C" int sml_ens_info(const sml_ens *e, int *members, int *capacity_steps, int *fields, int *scores_per_field,
                            int *rank_bins) {
    SML_REQUIRE(e, "null context");
    if (members) *members = e->E;
    if (capacity_steps) *capacity_steps = e->T;
    if (fields) *fields = kEnsFields;
    if (scores_per_field) *scores_per_field = kEnsScores;
    if (rank_bins) *rank_bins = kEnsRankBins;
    return SML_OK;
}

extern "C" int sml_ens_reset(sml_ens *e, void *stream) {
    SML_REQUIRE(e, "null context");
    launch_ens_reset(e->d_scores, e->nscores(), e->d_ranks, e->nranks(), (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_ens_moments(sml_ens *e, const double *d_g4, int64_t g4_stride, const double *d_g2,
                               const double *d_pr, int64_t g2_stride, double *d_mean4, double *d_mean2,
                               double *d_meanpr, double *d_spread4, double *d_spread2, double *d_spreadpr,
                               void *stream) {
    SML_REQUIRE(e, "null context");
    if (int rc = check_ens_members(d_g4, g4_stride, d_g2, g2_stride)) return rc;
    if (int rc = check_ens_quads(d_mean4, "d_mean4")) return rc;
    if (int rc = check_ens_quads(d_spread4, "d_spread4")) return rc;
    launch_ens_moments(d_g4, g4_stride, d_g2, d_pr, g2_stride, d_mean4, d_mean2, d_meanpr, d_spread4, d_spread2,
                       d_spreadpr, e->E, (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_ens_scores(sml_ens *e, const double *d_g4, int64_t g4_stride, const double *d_g2,
                              const double *d_pr, int64_t g2_stride, const double *d_truth4, const double *d_truth2,
                              const double *d_truthpr, int t, void *stream) {
    SML_REQUIRE(e, "null context");
    if (int rc = check_ens_members(d_g4, g4_stride, d_g2, g2_stride)) return rc;
    if (int rc = check_ens_truth(d_truth4, d_truth2, d_truthpr)) return rc;
    if (int rc = check_ens_quads(d_truth4, "d_truth4")) return rc;
    if (int rc = check_ens_row(t, e->T)) return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_ens_rows(d_g4, g4_stride, d_g2, d_pr, g2_stride, d_truth4, d_truth2, d_truthpr, e->d_w, e->E, e->d_part,
                    e->d_rpart, st);
    SML_HIP(hipGetLastError());
    launch_ens_fields(e->d_part, e->d_rpart, d_truth4 != nullptr, d_pr != nullptr, d_pr && d_truthpr,
                      e->d_scores + ens_score_offset(t, 0), e->d_ranks + ens_rank_offset(t, 0), st);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_ens_read(sml_ens *e, int t0, int count, double *scores, int32_t *ranks) {
    SML_REQUIRE(e, "null context");
    if (int rc = check_ens_read(t0, count, e->T)) return rc;
    SML_HIP(hipDeviceSynchronize());
    if (scores && count)
        SML_HIP(hipMemcpy(scores, e->d_scores + ens_score_offset(t0, 0), (size_t)ens_score_offset(count, 0) * 8,
                          hipMemcpyDeviceToHost));
    if (ranks && count)
        SML_HIP(hipMemcpy(ranks, e->d_ranks + ens_rank_offset(t0, 0), (size_t)ens_rank_offset(count, 0) * 4,
                          hipMemcpyDeviceToHost));
    return SML_OK;
}
