// sml_hybrid.hip -- the hybrid prediction loop of one rank, native: reservoir predict
// for the rank's regions, the outvec exchange (RCCL all-gather over xGMI), the
// global grid assembly, SPEEDY's run_model on the GPU, and the re-tiling of the
// next step's inputs.
//
// Reference: the time loop of src/parallelmain.f90:204-270 -- `predict` per region
// (:225-234), `sendrecievegrid` (src/mpires.f90:218-780: outvecs gathered at the root
// :338-430, assembled :300-478, `run_model` :549 -> :1516-1628, tiles scattered
// :558-751, `run_speedy` broadcast :721), and the loop exit on run_speedy
// (:268-270).
//
// Schedule ("Overlap"): predict needs the feedback tiles for
// the state update and for W_out(:, ncs+1:) x~, and SPEEDY's local vector only for
// W_out(:, 1:ncs) local_model -- the split the reference computes under
// outvec_component_contribs (mod_reservoir.f90:1456-1459).  With overlap on, the
// update + v_ml readout (main stream) run while SPEEDY integrates the previous
// step's window (side stream), on disjoint CUs; results are bit-identical to the
// one-stream schedule.
//
//   main : begin(fb_t) .. wait(lm_t) finish_grid -> [all-gather] -> assemble -> tile fb_t+1
//   side :   [run_model of step t-1 -> forecast grids]            wait(grid_t) run_model ..
//
// The loop's parts live beside it: the communicator (sml_comm), the cross-stream hops
// (sml_hops.hpp), the exchange plan, the calendar and the step's schedule
// (sml_hybrid_layout, host arithmetic), the slab ocean (sml_slab.hip, at one member).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "sml_comm.hpp"
#include "sml_devmem.hpp"
#include "sml_hybrid_layout.hpp"
#include "sml_internal.hpp"
#include "sml_timeline.hpp"

SML_TL_DEFINE(hybrid)

#include "sml_hops.hpp"

using namespace sml;

struct sml_hybrid {
    DevMem mem;  // first: every device and pinned buffer below is its; freed last, after the streams
    sml_reservoirs *res = nullptr;
    sml_dynamics *dyn = nullptr;
    sml_comm *comm = nullptr;
    int numregions = 0, nlocal = 0, ncs = 0, nout = 0;
    int nleap = 24;
    double delt = 900.0, alph = 0.5, rob = 0.05, wil = 0.53;
    bool overlap = true;
    hipStream_t main = nullptr, side = nullptr;
    bool own_streams = false;
    // the two cross-stream dependencies of the overlapped schedule (sml_hops.hpp)
    Hops hops;
    // where the step's serial chain runs (sml_hybrid_set_chain): the two-stream schedule
    // above (the finish, exchange and assembly on the main stream, two hops around every
    // window), or on SPEEDY's stream right after the window:
    //   side : window_t-1 .. wait(begun_t) finish -> [all-gather] -> assemble -> signal(grid_t) -> window_t
    //   main :   wait(grid_t-1) tile fb_t -> begin_t -> signal(begun_t)        wait(grid_t) tile ..
    // so no hop sits between two pieces of the critical path (the re-tiling and the
    // begin, which need the assembled grid, are the main stream's).  The requested modes,
    // and the schedule they give (reschedule): the step only reads `sched`
    int chain_mode = SML_CHAIN_AUTO, hop_mode = SML_HOP_AUTO;
    LoopSchedule sched;
    // caller-owned device buffers
    double *fb = nullptr, *lm = nullptr, *ov = nullptr, *g4 = nullptr, *g2 = nullptr, *pr = nullptr, *f4 = nullptr,
           *f2 = nullptr;
    const double *tisr = nullptr;
    // exchange staging (world > 1): send [maxc][nout], recv [world][maxc][nout],
    // and the region-order permutation when the shares are uneven
    int maxc = 0;
    bool contiguous = true;
    double *d_send = nullptr, *d_recv = nullptr, *d_glob = nullptr;
    int32_t *d_perm = nullptr;
    bool started = false, predicted = false, advanced = false;
    // sml_hybrid_step on one rank: the finish also assembled the grids (the exchange is
    // the identity), so the advance that follows skips sml_exchange_assemble
    bool assembled = false;
    // pipelined (sml_hybrid_set_pipelined): each advance issues the next step's begin
    // (update + v_ml readout) on the main stream as soon as its feedback is tiled;
    // begun_next: that begin is in flight, so the next predict only finishes
    bool pipelined = false, begun_next = false;
    // sml_hybrid_set_force_exchange: a world-1 loop with a transport takes the world > 1
    // exchange path (send slab -> ncclAllGather -> advance from the receive slab)
    bool force_exchange = false;
    int64_t allgathers = 0;  // ncclAllGather calls issued by sml_hybrid_step (sml_hybrid_exchanges)
    // the hourly tisr table [cal.nhours][48][96] on the device and the loop's calendar
    const double *tisr_table = nullptr;
    LoopCalendar cal;
    // the exchange row: the outvec (nout), + the slab ocean's sst of the region's
    // resolved points when the slab is on (as sendrecievegrid sends them, mpires.f90:358-383)
    int xw = 0;
    int res_cus = 0;     // the CUs of the main stream's mask (0: no mask)
    int speedy_cus = 0;  // the CUs of the side (SPEEDY) stream's mask (0: no mask)
    // slab ocean (parallelmain.f90:216-249; mpires.f90:288-478, 575-767; cpl_sea.f90:38-46):
    // sml_slab.hip's context at one member, its wholegrid_sst and bias for run_model's
    // sst_hybrid, and the packed strides of the loop's rows and feedback
    sml_slab *slab = nullptr;
    bool slab_started = false;
    const double *slab_sst_grid = nullptr;
    double slab_bias = 0.0;
    int64_t ov_stride = 0, all_stride = 0, fb_stride = 0;

    hipStream_t chain_stream() const { return sched.chain_on_side ? side : main; }
};

namespace {

// global region order from the all-gather's [rank][maxc] slabs: glob row r = slab row
// perm[r] (sml_exchange_plan)
__global__ void k_gather_rows(const double *__restrict__ recv, const int32_t *__restrict__ perm,
                              double *__restrict__ glob, int nout, int total) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int r = e / nout, o = e % nout;
    glob[e] = recv[(size_t)perm[r] * nout + o];
}

// the exchange staging for rows of h->xw doubles (world > 1): the loop's own
// all-gather's send / receive slabs (when the communicator has a transport) and the
// region-order copy of uneven shares
int alloc_exchange(sml_hybrid *h) {
    for (double **p : {&h->d_send, &h->d_recv, &h->d_glob}) h->mem.release(p);
    const size_t row = (size_t)h->xw;
    const int world = h->comm->world;
    if (h->comm->has_transport() && h->maxc > 0) {
        h->mem.device(&h->d_send, (size_t)h->maxc * row);  // (zero: its padding rows are sent as they are)
        h->mem.device(&h->d_recv, (size_t)world * h->maxc * row, false);
    }
    if (!h->contiguous) h->mem.device(&h->d_glob, (size_t)h->numregions * row, false);
    if (h->mem.status()) return fail(SML_ERR_NOMEM, "exchange buffers");
    return SML_OK;
}

// dispatch serialised by the runtime or a profiler: the HIP runtime's
// AMD_SERIALIZE_KERNEL, rocprofv3's counter collection (ROCPROF_COUNTER_COLLECTION,
// set by `rocprofv3 --pmc` / `-i`)
bool env_on(const char *name) {
    const char *e = getenv(name);
    return e && *e && std::strcmp(e, "0") != 0 && std::strcmp(e, "false") != 0 && std::strcmp(e, "False") != 0;
}

bool dispatch_serialised() { return env_on("AMD_SERIALIZE_KERNEL") || env_on("ROCPROF_COUNTER_COLLECTION"); }

int drain(sml_hybrid *h) {
    if (h->main) SML_HIP(hipStreamSynchronize(h->main));
    if (h->side && h->side != h->main) SML_HIP(hipStreamSynchronize(h->side));
    return SML_OK;
}

// the schedule of the modes in effect (loop_schedule).  Both streams are drained by now,
// so no wait of one kind is left pending on a signal of the other.
void reschedule(sml_hybrid *h) {
    h->sched = loop_schedule({h->overlap, h->side != h->main, h->chain_mode, h->hop_mode, h->res_cus > 0,
                              env_on("SML_HYBRID_EVENTS"), dispatch_serialised()});
    h->hops.flavour = h->sched.use_events ? Hops::kEvents : h->sched.use_kernels ? Hops::kKernel : Hops::kWaitValue;
}

}  // namespace

// hop mode: SML_HOP_AUTO, SML_HOP_WAIT_VALUE, SML_HOP_EVENTS, SML_HOP_KERNEL
// (loop_schedule).  Drains both streams first.
extern "C" int sml_hybrid_set_hop_mode(sml_hybrid *h, int mode) {
    SML_REQUIRE(h && (mode == SML_HOP_AUTO || mode == SML_HOP_WAIT_VALUE || mode == SML_HOP_EVENTS ||
                      mode == SML_HOP_KERNEL),
                "bad hop mode %d", mode);
    if (int rc = drain(h)) return rc;
    h->hop_mode = mode;
    reschedule(h);
    return SML_OK;
}

// the give-up time of every in-kernel wait of the loop (the kernel hops, and run_model's
// exit waiting for its safety check), microseconds; default 4 s (hops) / 1 s (check)
extern "C" int sml_hybrid_set_hop_timeout(sml_hybrid *h, int64_t microseconds) {
    SML_REQUIRE(h && microseconds >= 0, "bad argument");
    if (int rc = drain(h)) return rc;
    h->hops.timeout = (long long)microseconds * 100;  // wall_clock64 runs at 100 MHz
    return sml::dyn_set_check_timeout(h->dyn, std::min<long long>(h->hops.timeout, 100000000ll));
}

// pipelined loop (see sml_hybrid::pipelined); switching it off keeps a begin already
// in flight for the next predict
extern "C" int sml_hybrid_set_pipelined(sml_hybrid *h, int on) {
    SML_REQUIRE(h, "null context");
    h->pipelined = on != 0;
    return SML_OK;
}

// the step's serial chain (finish -> exchange -> assembly -> tiling): SML_CHAIN_AUTO,
// SML_CHAIN_TWO_STREAMS, SML_CHAIN_SPEEDY (loop_schedule).  Drains both streams first.
extern "C" int sml_hybrid_set_chain(sml_hybrid *h, int mode) {
    SML_REQUIRE(h && (mode == SML_CHAIN_AUTO || mode == SML_CHAIN_TWO_STREAMS || mode == SML_CHAIN_SPEEDY),
                "bad chain mode %d", mode);
    SML_REQUIRE(!h->predicted, "sml_hybrid_set_chain between predict and advance");
    if (int rc = drain(h)) return rc;
    h->chain_mode = mode;
    reschedule(h);
    return SML_OK;
}

extern "C" int sml_hybrid_chain(const sml_hybrid *h, int *requested, int *effective) {
    SML_REQUIRE(h, "null context");
    if (requested) *requested = h->chain_mode;
    if (effective) *effective = h->sched.chain_effective;
    return SML_OK;
}

// the stream the local outvecs are ready on after sml_hybrid_predict, and on which a
// host-driven exchange should run before sml_hybrid_advance
extern "C" int sml_hybrid_exchange_stream(const sml_hybrid *h, void **stream) {
    SML_REQUIRE(h && stream, "null argument");
    *stream = h->chain_stream();
    return SML_OK;
}

extern "C" int sml_hybrid_set_force_exchange(sml_hybrid *h, int on) {
    SML_REQUIRE(h, "null context");
    if (on && !h->force_exchange) {
        SML_REQUIRE(h->comm && h->comm->has_transport(), "forcing the exchange needs a communicator with a transport");
        SML_REQUIRE(!h->predicted, "sml_hybrid_set_force_exchange between predict and advance");
        if (h->comm->world == 1) {  // the one-rank plan: maxc = every region, contiguous
            h->maxc = h->nlocal;
            h->contiguous = true;
            if (int rc = alloc_exchange(h)) return rc;
        }
    }
    h->force_exchange = on != 0;
    return SML_OK;
}

// the requested mode and the one in effect (SML_HOP_WAIT_VALUE, SML_HOP_EVENTS or SML_HOP_KERNEL)
extern "C" int sml_hybrid_hop_mode(const sml_hybrid *h, int *requested, int *effective) {
    SML_REQUIRE(h, "null context");
    if (requested) *requested = h->hop_mode;
    if (effective) *effective = h->sched.hop_effective;
    return SML_OK;
}

extern "C" int sml_hybrid_destroy(sml_hybrid *h) {
    if (!h) return SML_OK;
    if (h->main) (void)hipStreamSynchronize(h->main);
    if (h->side) (void)hipStreamSynchronize(h->side);
    (void)sml_slab_destroy(h->slab);  // before the loop's own memory goes
    if (h->own_streams) {
        if (h->side && h->side != h->main) (void)hipStreamDestroy(h->side);
        if (h->main) (void)hipStreamDestroy(h->main);
    }
    h->hops.destroy_events();
    delete h;
    return SML_OK;
}

extern "C" int sml_hybrid_create(sml_reservoirs *res, sml_dynamics *dyn, sml_comm *comm, int nleap, double delt,
                                 double alph, double rob, double wil, int overlap, int speedy_cus, sml_hybrid **out) {
    SML_REQUIRE(out && res && dyn && nleap >= 0 && delt > 0.0, "bad argument");
    *out = nullptr;
    sml_hybrid *h = new (std::nothrow) sml_hybrid();
    if (!h) return fail(SML_ERR_NOMEM, "host allocation failed");
    auto bail = [&](int rc) {
        sml_hybrid_destroy(h);
        return rc;
    };
    h->res = res;
    h->dyn = dyn;
    h->comm = comm;
    h->nleap = nleap;
    h->delt = delt;
    h->alph = alph;
    h->rob = rob;
    h->wil = wil;
    h->overlap = overlap != 0;
    if (int rc = sml_res_info(res, &h->numregions, &h->nlocal, &h->ncs, &h->nout, nullptr)) return bail(rc);
    const int world = comm ? comm->world : 1, rank = comm ? comm->rank : 0;
    // the communicator's decomposition must be the one the reservoir context holds
    std::vector<int> mine(h->numregions), ids(h->nlocal);
    const int cnt = processor_regions(h->numregions, world, rank, mine.data());
    if (int rc = sml_res_info(res, nullptr, nullptr, nullptr, nullptr, ids.data())) return bail(rc);
    // (without a communicator any subset is accepted for predict / advance around a
    // host exchange; sml_hybrid_step then needs every region local)
    if (comm && (cnt != h->nlocal || !std::equal(ids.begin(), ids.end(), mine.begin())))
        return bail(fail(SML_ERR_ARG, "the reservoir context does not hold rank %d of %d's processor_decomposition",
                         rank, world));
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return bail(fail(SML_ERR_HIP, "no device"));
    // streams: non-default (the legacy NULL stream would serialise the two chains);
    // with overlap and 0 < speedy_cus < CUs, SPEEDY's chain gets CUs [0, speedy_cus)
    // and the reservoir a disjoint range after it (sml_stream_create_cu_range)
    h->own_streams = true;
    if (h->overlap && speedy_cus > 0 && speedy_cus < ncu) {
        void *s = nullptr, *m = nullptr;
        if (int rc = sml_stream_create_cu_range(0, speedy_cus, &s)) return bail(rc);
        h->side = (hipStream_t)s;
        // the reservoir on CUs [speedy_cus, speedy_cus + res_cus): one CU per 6 of the
        // rank's regions (a multiple of 8: the same count on every XCD), at least 64, at
        // most all the CUs SPEEDY does not use.  At 6 regions per CU the begin (update +
        // v_ml readout) takes about the window's time beside it; more CUs only add HBM
        // pressure on the window, fewer make the begin the critical path.  Same box
        // (DESIGN.md §4): N = 1 (1152 regions) 192 CUs 1137 vs 160 1095; the 2-rank share
        // 96 CUs 1254 vs 192 1230; 4-rank 64 1282 vs 192 1264; 8-rank 64 1298 vs 192
        // 1290 steps/s.  SML_RES_CUS overrides the count.
        int res_cus = std::min(ncu - speedy_cus, std::max(64, ((h->nlocal + 5) / 6 + 7) / 8 * 8));
        if (const char *er = getenv("SML_RES_CUS")) res_cus = std::min(std::max(atoi(er), 1), ncu - speedy_cus);
        if (int rc = sml_stream_create_cu_range(speedy_cus, res_cus, &m)) return bail(rc);
        h->main = (hipStream_t)m;
        // run_model's safety check (re-grid + min/max beside the window) on the CUs
        // left over, else on the reservoir's: never on SPEEDY's, where its blocks
        // slowed the window's first kernels (k_st_gridspec 21 vs 17.6 us, rocprof r02u)
        const int spare = ncu - speedy_cus - res_cus;
        if (int rc = spare > 0 ? sml_dyn_set_check_cus(dyn, speedy_cus + res_cus, spare)
                               : sml_dyn_set_check_cus(dyn, speedy_cus, res_cus))
            return bail(rc);
        if (int rc = sml_res_set_read_waves(res, 0)) return bail(rc);  // pacing pays only on shared CUs
        if (int rc = sml_res_set_update_cus(res, res_cus)) return bail(rc);  // one balanced-update block per CU
        h->res_cus = res_cus;
        h->speedy_cus = speedy_cus;
    } else {
        if (hipStreamCreateWithFlags(&h->main, hipStreamNonBlocking) != hipSuccess)
            return bail(fail(SML_ERR_HIP, "stream"));
        if (h->overlap) {
            int lo = 0, hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
            if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, hi) != hipSuccess)
                return bail(fail(SML_ERR_HIP, "stream"));
        } else {
            h->side = h->main;
        }
    }
    if (int rc = h->hops.create(h->mem)) return bail(rc);
    h->xw = h->nout;
    if (world > 1) {
        std::vector<int32_t> perm(h->numregions);
        int contig = 1;
        if (int rc = sml_exchange_plan(h->numregions, world, &h->maxc, &contig, perm.data())) return bail(rc);
        h->contiguous = contig != 0;
        if (!h->contiguous &&
            (h->mem.device(&h->d_perm, (size_t)h->numregions, false) != SML_OK ||
             hipMemcpy(h->d_perm, perm.data(), perm.size() * 4, hipMemcpyHostToDevice) != hipSuccess))
            return bail(fail(SML_ERR_NOMEM, "exchange buffers"));
        if (int rc = alloc_exchange(h)) return bail(rc);
    }
    if (int rc = drain(h)) return bail(rc);
    reschedule(h);  // SML_HOP_AUTO, SML_CHAIN_AUTO
    *out = h;
    return SML_OK;
}

extern "C" int sml_hybrid_set_buffers(sml_hybrid *h, double *d_feedback, double *d_local_model, double *d_outvec,
                                      double *d_grid4d, double *d_grid2d, double *d_precip, double *d_fc4d,
                                      double *d_fc2d, const double *d_tisr) {
    SML_REQUIRE(h && d_feedback && d_outvec && d_grid4d && d_grid2d && d_precip && d_fc4d && d_fc2d,
                "null buffer");
    SML_REQUIRE(h->ncs == 0 || d_local_model, "a hybrid context needs d_local_model");
    h->fb = d_feedback;
    h->lm = d_local_model;
    h->ov = d_outvec;
    h->g4 = d_grid4d;
    h->g2 = d_grid2d;
    h->pr = d_precip;
    h->f4 = d_fc4d;
    h->f2 = d_fc2d;
    h->tisr = d_tisr;
    return SML_OK;
}

extern "C" int sml_hybrid_set_tisr(sml_hybrid *h, const double *d_tisr) {
    SML_REQUIRE(h, "null context");
    h->tisr = d_tisr;
    return SML_OK;
}

// the loop's calendar (run_model / get_tisr_by_date's get_current_time_delta_hour,
// mpires.f90:1545, :1661): start year, the hours before the first prediction step
// (traininglength + prediction marker + synclength) and the hours per step; turns on
// the window's date-driven forcing.  Resets the step count and the February latch.
extern "C" int sml_hybrid_set_calendar(sml_hybrid *h, int startyear, int64_t hours_base, int step_hours) {
    SML_REQUIRE(h && step_hours > 0 && hours_base >= 0, "bad argument");
    h->cal.set_calendar(startyear, hours_base, step_hours);
    return SML_OK;
}

// the calendar date of the next window (the advance after the last one issued)
extern "C" int sml_hybrid_window_date(sml_hybrid *h, int *date) {
    SML_REQUIRE(h && date, "null argument");
    SML_REQUIRE(h->cal.cal_on, "no calendar (sml_hybrid_set_calendar)");
    return h->cal.window_date(date);
}

extern "C" int sml_hybrid_set_tisr_table(sml_hybrid *h, const double *d_table, int nhours, int startyear,
                                         int64_t hours_base, int step_hours) {
    SML_REQUIRE(h && (d_table == nullptr || (nhours >= 8760 && step_hours > 0 && hours_base >= 0)), "bad argument");
    h->tisr_table = d_table;
    h->cal.set_tisr_table(nhours, startyear, hours_base, step_hours);
    return SML_OK;
}

// the SAVEd February of the reference's month table (mod_calendar.f90:40,61-63) as
// the host's own calendar calls left it: every get_current_time_delta_hour of the
// process shares it (training windows mod_reservoir.f90:355/632/638, the prediction
// start mpires.f90:108/489, run_model :1545), so a host that met a leap year before
// the loop's first tisr lookup passes 1 here.  sml_hybrid_set_tisr_table resets it
// to 0 (a process whose calendar has not met a leap year).
extern "C" int sml_hybrid_set_feb29(sml_hybrid *h, int feb29) {
    SML_REQUIRE(h, "null context");
    h->cal.feb29 = feb29 != 0;
    return SML_OK;
}

extern "C" int sml_hybrid_get_feb29(const sml_hybrid *h, int *feb29) {
    SML_REQUIRE(h && feb29, "null argument");
    *feb29 = h->cal.feb29;
    return SML_OK;
}

extern "C" int sml_hybrid_streams(const sml_hybrid *h, void **main, void **side) {
    SML_REQUIRE(h, "null context");
    if (main) *main = h->main;
    if (side) *side = h->side;
    return SML_OK;
}

extern "C" int sml_hybrid_cus(const sml_hybrid *h, int *speedy_cus, int *res_cus) {
    SML_REQUIRE(h, "null context");
    if (speedy_cus) *speedy_cus = h->speedy_cus;
    if (res_cus) *res_cus = h->res_cus;
    return SML_OK;
}

// start_prediction's hand-over (src/mod_reservoir.f90:938-959, parallelmain.f90:207-216):
// the first step's feedback tiles from an analysis grid and the local model from a
// SPEEDY forecast of it, both copied into the loop's buffers (on the main stream,
// ordered after the caller's legacy-stream work)
extern "C" int sml_hybrid_start(sml_hybrid *h, const double *d_g4, const double *d_g2, const double *d_pr,
                                const double *d_f4, const double *d_f2) {
    SML_REQUIRE(h && h->fb, "sml_hybrid_set_buffers first");
    SML_REQUIRE(d_g4 && d_g2 && d_pr && d_f4 && d_f2, "null argument");
    SML_HIP(hipDeviceSynchronize());
    // a restart after a pipelined run: the begin the last advance issued was built from
    // the old feedback -- discard it (the state rolls back to the one it read), so the
    // first predict begins from the feedback tiled here
    if (h->begun_next) {
        if (int rc = sml_res_step_cancel(h->res)) return rc;
        h->begun_next = false;
    }
    const size_t n4 = (size_t)kGrid4d * 8, n2 = (size_t)kGrid2d * 8;
    if (d_g4 != h->g4) SML_HIP(hipMemcpyAsync(h->g4, d_g4, n4, hipMemcpyDeviceToDevice, h->main));
    if (d_g2 != h->g2) SML_HIP(hipMemcpyAsync(h->g2, d_g2, n2, hipMemcpyDeviceToDevice, h->main));
    if (d_pr != h->pr) SML_HIP(hipMemcpyAsync(h->pr, d_pr, n2, hipMemcpyDeviceToDevice, h->main));
    if (d_f4 != h->f4) SML_HIP(hipMemcpyAsync(h->f4, d_f4, n4, hipMemcpyDeviceToDevice, h->main));
    if (d_f2 != h->f2) SML_HIP(hipMemcpyAsync(h->f2, d_f2, n2, hipMemcpyDeviceToDevice, h->main));
    if (int rc = sml_res_tile_inputs(h->res, h->g4, h->g2, h->pr, h->f4, h->f2, h->tisr, h->fb, h->lm, h->main))
        return rc;
    if (int rc = h->hops.signal(kHopLm, h->main)) return rc;
    SML_HIP(hipStreamSynchronize(h->main));  // (the chain on SPEEDY's stream reads these on the other stream)
    h->started = true;
    h->predicted = h->advanced = false;
    return SML_OK;
}

// ------------------------------------------------------------------ slab ocean
// the slab ocean in the loop (parallelmain.f90:216-249, sendrecievegrid's sst half).
// Before sml_hybrid_set_buffers: the exchange rows widen to nout + resx*resy.
extern "C" int sml_hybrid_set_slab(sml_hybrid *h, sml_reservoirs *slab, const double *d_base_sst,
                                   const double *d_sea_mask, int timestep, int timestep_slab, double sst_bias) {
    SML_REQUIRE(h && slab && d_base_sst && d_sea_mask, "null argument");
    SML_REQUIRE(!h->slab, "the slab ocean is set already");
    SML_REQUIRE(!h->ov, "sml_hybrid_set_slab must precede sml_hybrid_set_buffers (the exchange rows widen)");
    sml_slab *s = nullptr;
    if (int rc = slab_create(h->res, slab, d_base_sst, d_sea_mask, timestep, timestep_slab, sst_bias, &s)) return rc;
    auto bail = [&](int rc) {
        (void)sml_slab_destroy(s);
        return rc;
    };
    int xw = 0;
    if (int rc = sml_slab_info(s, nullptr, &xw, nullptr, nullptr, nullptr, &h->slab_bias)) return bail(rc);
    if (int rc = sml_slab_buffers(s, &h->slab_sst_grid, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))
        return bail(rc);
    h->xw = xw;
    if (int rc = sml_res_set_outvec_ld(h->res, xw)) return bail(rc);
    if (h->res_cus > 0)  // the slab step runs on the main stream too
        if (int rc = sml_res_set_update_cus(slab, h->res_cus)) return bail(rc);
    if (h->comm && (h->comm->world > 1 || h->force_exchange))
        if (int rc = alloc_exchange(h)) return bail(rc);
    slab_strides(s, &h->ov_stride, &h->all_stride, &h->fb_stride);
    h->slab = s;
    return SML_OK;
}

// start_prediction_slab's hand-over (sml::slab_start): the slab reservoirs' sst
// [nslab][resx*resy] until their first prediction (the host synchronizes their states,
// sml_res_start_prediction).  After sml_hybrid_start, before the first step; the first
// step's exchange builds the SST.
extern "C" int sml_hybrid_start_slab(sml_hybrid *h, const double *d_slab_outvec) {
    SML_REQUIRE(h && h->slab, "sml_hybrid_set_slab first");
    SML_REQUIRE(h->ov && h->started, "sml_hybrid_start first");
    int nslab = 0;
    if (int rc = sml_slab_info(h->slab, nullptr, nullptr, &nslab, nullptr, nullptr, nullptr)) return rc;
    SML_REQUIRE(nslab == 0 || d_slab_outvec, "null slab outvec");
    if (int rc = slab_start(h->slab, 0, d_slab_outvec, h->ov, h->ov_stride, h->main)) return rc;
    h->slab_started = true;
    return SML_OK;
}

// the exchange row length: nout, or nout + the slab sst of the region's points
extern "C" int sml_hybrid_exchange_width(const sml_hybrid *h, int *width) {
    SML_REQUIRE(h && width, "null argument");
    *width = h->xw;
    return SML_OK;
}

// the slab state for hosts and tests: wholegrid_sst(96, 48) of the last exchange, the
// ring [timestep_slab/timestep - 1][tot] of averaged inputs (tot = *ring_len), the
// last slab feedback and slab outvecs [nslab][resx*resy]
extern "C" int sml_hybrid_slab_buffers(const sml_hybrid *h, const double **d_sst_grid, const double **d_ring,
                                       int *ring_len, const double **d_slab_feedback, const double **d_slab_outvec) {
    SML_REQUIRE(h && h->slab, "no slab ocean in this loop");
    if (int rc = sml_slab_info(h->slab, nullptr, nullptr, nullptr, nullptr, ring_len, nullptr)) return rc;
    return sml_slab_buffers(h->slab, d_sst_grid, nullptr, d_ring, nullptr, d_slab_feedback, nullptr, d_slab_outvec,
                            nullptr);
}

// predict for every local region (parallelmain.f90:225-234): the local outvecs in
// d_outvec on the main stream; with `assemble` (sml_hybrid_step on one rank) the
// finish also scatters them into the global grids
namespace {
int predict_impl(sml_hybrid *h, bool assemble) {
    SML_REQUIRE(h, "null context");
    if (!h->started) return fail(SML_ERR_STATE, "sml_hybrid_start first");
    if (h->slab && !h->slab_started) return fail(SML_ERR_STATE, "sml_hybrid_start_slab first");
    if (h->predicted) return fail(SML_ERR_STATE, "sml_hybrid_predict twice without sml_hybrid_advance");
    const LoopSchedule &sc = h->sched;
    h->assembled = false;
    if (h->overlap) {
        // (pipelined: the previous advance issued it already, unless the host discarded
        // it since -- sml_res_set_state / sml_res_step_cancel)
        int begun = 0;
        if (h->begun_next)
            if (int rc = sml_res_step_begun(h->res, &begun)) return rc;
        if (!begun)
            if (int rc = sml_res_step_begin(h->res, h->fb, h->main)) return rc;
        h->begun_next = false;
        if (h->slab)
            if (int rc = slab_predict(h->slab, h->cal.t + 1, h->ov, h->ov_stride, h->main, nullptr)) return rc;
        // chain: the finish follows the window on SPEEDY's stream, once the begin is done
        hipStream_t xs = h->chain_stream();
        if (sc.chain)
            if (int rc = h->hops.signal(kHopBegun, h->main)) return rc;
        if (sc.finish_in_kernel && h->nlocal > 0) {  // waited for inside the finish (no wait kernel)
            if (!sc.chain) {
                // SPEEDY's forecast of the previous window, waited for inside the finish: its
                // weights load while the window runs (k_res_finish_grid's wflag; the main
                // stream's later work still follows the finish, so it follows the window too).
                // The finish's blocks spin on the reservoir's CUs, and the window's exit (the
                // forecast's producer) waits for its safety check, which runs on those CUs:
                // the finish launches only once that check is done (a CP wait on the main
                // stream, satisfied while the window still runs), or a host that enqueues
                // steps without polling run_speedy could starve the check behind the finish
                void *ev = nullptr;
                if (int rc = sml::dyn_check_event(h->dyn, &ev)) return rc;
                if (ev) SML_HIP(hipStreamWaitEvent(h->main, (hipEvent_t)ev, 0));
            }
            if (int rc = sml::res_finish_wait(h->res, h->hops.word(sc.finish_hop), h->hops.seq(sc.finish_hop),
                                              h->hops.late_word(), h->hops.timeout))
                return rc;
        } else if (int rc = h->hops.wait(sc.finish_hop, xs)) {  // (two streams: SPEEDY's forecast of the previous window)
            return rc;
        }
        // the local-model tiling fused into the v_p finish: one launch fewer on the
        // critical path; on one rank the assembly too (one more)
        if (assemble) {
            if (int rc = sml_res_step_finish_assemble(h->res, h->f4, h->f2, h->lm, h->ov, h->g4, h->g2, h->pr, xs))
                return rc;
            h->assembled = true;
        } else if (int rc = sml_res_step_finish_grid(h->res, h->f4, h->f2, h->lm, h->ov, xs)) {
            return rc;
        }
    } else {  // one pass over W_out: the same sums as begin + finish
        if (int rc = sml_res_step(h->res, h->fb, h->lm, h->ov, h->main)) return rc;
        if (h->slab)
            if (int rc = slab_predict(h->slab, h->cal.t + 1, h->ov, h->ov_stride, h->main, nullptr)) return rc;
    }
    h->predicted = true;
    return SML_OK;
}
}  // namespace

extern "C" int sml_hybrid_predict(sml_hybrid *h) { return predict_impl(h, false); }

// sendrecievegrid's assembly + run_model + re-tiling (mpires.f90:300-751) from the
// outvecs of every region in global region order ([numregions][nout], device)
extern "C" int sml_hybrid_advance(sml_hybrid *h, const double *d_outvec_all) {
    SML_REQUIRE(h && d_outvec_all, "null argument");
    if (!h->predicted) return fail(SML_ERR_STATE, "sml_hybrid_advance without sml_hybrid_predict");
    const LoopSchedule &sc = h->sched;
    hipStream_t m = h->main, s = h->side;
    // the assembly's stream: the main stream (two hops around the window), or SPEEDY's,
    // right behind the window (sml_hybrid_set_chain); the re-tiling is the main stream's
    hipStream_t c = h->chain_stream();
    // (sml_hybrid_step on one rank: its predict assembled these very outvecs already)
    const bool done = h->assembled && d_outvec_all == h->ov;
    h->assembled = false;
    if (!done)
        if (int rc = sml_exchange_assemble(h->res, d_outvec_all, h->g4, h->g2, h->pr, c)) return rc;
    // after a change of any region's slab sst: wholegrid_sst from the exchange rows, the
    // atmo feedback's sst entries, and run_model's sst_hybrid into the window (cpl_sea.f90:38-46)
    int sst_new = 0;  // a new hybrid SST reaches sst_am this step
    if (h->slab) {
        if (int rc = slab_sst(h->slab, d_outvec_all, h->all_stride, h->fb, h->fb_stride, c, &sst_new)) return rc;
        if (sst_new)
            if (int rc = sml_dyn_set_hybrid_sst(h->dyn, h->slab_sst_grid, h->slab_bias, c)) return rc;
    }
    if (h->cal.cal_on) {
        // run_model's date for this step (mpires.f90:1545, timestep = t + 1; before the
        // tisr lookup below, as the reference's calls meet the February latch) and the
        // window's forcing at that date (agcm_init, ini_agcm_init.f90:57-89), after the
        // previous window (the finish waited for its forecast) and any new hybrid SST
        int date[4];
        if (int rc = h->cal.next_date(date)) return rc;
        // on SPEEDY's stream, behind the previous window and beside the finish / assembly,
        // unless this step's new SST (written on c) must reach qcorh first
        if (int rc = sml_dyn_fordate(h->dyn, date[0], date[1], date[2], sst_new ? c : s)) return rc;
    }
    if (sc.entry_sig) {  // run_model is enqueued before the main stream's wait for its signal
        int adds = 0;
        if (int rc = sml::dyn_run_model_entry_signal(h->dyn, h->hops.word(kHopGrid), &adds)) return rc;
        h->hops.add_seq(kHopGrid, (uint64_t)adds);
        if (int rc = sml_dyn_run_model(h->dyn, h->g4, h->g2, h->nleap, h->delt, h->alph, h->rob, h->wil, h->f4, h->f2,
                                       s))
            return rc;
    } else if (h->overlap) {  // the assembled grid: to SPEEDY's stream (two-stream) / to the main stream (chain)
        if (int rc = h->hops.signal(kHopGrid, c)) return rc;
    }
    if (sc.chain)
        if (int rc = h->hops.wait(kHopGrid, m)) return rc;
    ++h->cal.t;
    if (int rc = sml_res_tile_feedback(h->res, h->g4, h->g2, h->pr, h->tisr_table ? nullptr : h->tisr, h->fb, m))
        return rc;
    if (h->tisr_table) {  // get_tisr_by_date(..., timestep - 1, ...) for the next feedback (mpires.f90:726-728)
        int idx = 0;
        if (int rc = h->cal.tisr_index(&idx)) return rc;
        if (int rc = sml_res_tile_tisr_field(h->res, h->tisr_table + (size_t)(idx - 1) * kGrid2d, h->fb, m))
            return rc;
    }
    if (h->slab)  // averaged_atmo_input_vec(:, mod(t-1, R-1)+1), mpires.f90:755
        if (int rc = slab_ring(h->slab, h->cal.t, h->fb, h->fb_stride, m)) return rc;
    if (sc.entry_wait) {  // the entry's specx waits for the assembled grid in-kernel
        if (int rc = sml::dyn_run_model_wait(h->dyn, h->hops.word(kHopGrid), h->hops.seq(kHopGrid),
                                             h->hops.late_word(), h->hops.timeout))
            return rc;
    } else if (sc.hops) {
        if (int rc = h->hops.wait(kHopGrid, s)) return rc;
    }
    // kernel hops: the forecast's signal is a store that run_model issues right behind
    // its exit (inside the window graph when the exit is captured there); the loop's
    // sequence number moves only once run_model is enqueued, so a run_model that fails
    // leaves no store pending and no finish waiting for one.  (The exit's own blocks
    // signalling instead, an agent-scope release each, measured no faster: DESIGN.md §4c)
    const uint64_t lm_next = h->hops.seq(kHopLm) + 1;
    if (sc.exit_store)
        if (int rc = sml::dyn_run_model_exit_store(h->dyn, h->hops.word(kHopLm), lm_next)) return rc;
    if (!sc.entry_sig)
        if (int rc = sml_dyn_run_model(h->dyn, h->g4, h->g2, h->nleap, h->delt, h->alph, h->rob, h->wil, h->f4, h->f2,
                                       s)) {
            if (sc.exit_store) (void)sml::dyn_run_model_exit_store(h->dyn, nullptr, 0);
            return rc;
        }
    if (sc.exit_store) h->hops.set_seq(kHopLm, lm_next);
    if (sc.hops && !sc.exit_store) {
        if (int rc = h->hops.signal(kHopLm, s)) return rc;
    } else if (!h->overlap && h->ncs) {
        if (int rc = sml_res_tile_local_model(h->res, h->f4, h->f2, h->lm, s)) return rc;
    }
    // pipelined: the next step's begin from the feedback just tiled, on the main stream,
    // beside this window (it would be the next predict's first launch anyway)
    if (h->pipelined && h->overlap) {
        if (int rc = sml_res_step_begin(h->res, h->fb, m)) return rc;
        h->begun_next = true;
    }
    h->predicted = false;
    h->advanced = true;
    return SML_OK;
}

// advance from the all-gather's output d_recv[world][maxc][nout] (sml_exchange_plan):
// the slabs are global region order with even shares, else k_gather_rows permutes
// them into it first (on the chain's stream)
extern "C" int sml_hybrid_advance_slabs(sml_hybrid *h, const double *d_recv) {
    SML_REQUIRE(h && d_recv, "null argument");
    const int world = h->comm ? h->comm->world : 1;
    if (world == 1 || h->contiguous) return sml_hybrid_advance(h, d_recv);  // slabs in region order
    if (!h->predicted) return fail(SML_ERR_STATE, "sml_hybrid_advance_slabs without sml_hybrid_predict");
    const int total = h->numregions * h->xw;
    hipLaunchKernelGGL(k_gather_rows, dim3((total + 255) / 256), dim3(256), 0, h->chain_stream(), d_recv, h->d_perm,
                       h->d_glob, h->xw, total);
    SML_HIP(hipGetLastError());
    return sml_hybrid_advance(h, h->d_glob);
}

// one hybrid step with the loop's own exchange: identity on one rank, else the
// all-gather of every rank's outvec slab (RCCL over xGMI) on the chain's stream
extern "C" int sml_hybrid_step(sml_hybrid *h) {
    SML_REQUIRE(h, "null context");
    if (int rc = h->hops.late_check("sml_hybrid_step")) return rc;  // a host word: no sync
    const int world = h->comm ? h->comm->world : 1;
    if (world == 1 && h->nlocal != h->numregions)
        return fail(SML_ERR_STATE, "one rank holds %d of %d regions: exchange through sml_hybrid_advance",
                    h->nlocal, h->numregions);
    if (world > 1 && !h->comm->has_transport())
        return fail(SML_ERR_STATE, "rank %d of %d has no transport: exchange through sml_hybrid_advance_slabs",
                    h->comm->rank, world);
    // one rank: the exchange is the identity, so the finish assembles the grids itself;
    // forced, it goes through the transport as at world > 1
    const bool identity = world == 1 && !h->force_exchange;
    const bool fuse = identity && h->overlap && sml::res_in_global_order(h->res);
    if (int rc = predict_impl(h, fuse)) return rc;
    if (identity) return sml_hybrid_advance(h, h->ov);
    // (world > 1, or world 1 forced through the transport)
    // even shares (1152 / N for N = 1, 2, 4, 8): the outvecs go out of ov as they are;
    // uneven ones are padded to the largest share through d_send (one copy more on the
    // critical path; d_send's padding rows stay zero)
    hipStream_t xs = h->chain_stream();
    const double *send = h->ov;
    if (h->nlocal != h->maxc) {
        SML_HIP(hipMemcpyAsync(h->d_send, h->ov, (size_t)h->nlocal * h->xw * 8, hipMemcpyDeviceToDevice, xs));
        send = h->d_send;
    }
    if (int rc = sml_comm_allgather(h->comm, send, h->d_recv, (int64_t)h->maxc * h->xw, xs)) return rc;
    ++h->allgathers;
    return sml_hybrid_advance_slabs(h, h->d_recv);
}

extern "C" int sml_hybrid_exchanges(const sml_hybrid *h, int64_t *allgathers) {
    SML_REQUIRE(h && allgathers, "null argument");
    *allgathers = h->allgathers;
    return SML_OK;
}

// run_speedy after the last advance (mpires.f90:721, :1623): 0 ends the prediction
// (parallelmain.f90:268-270).  Waits for that step's safety check only.
extern "C" int sml_hybrid_run_speedy(sml_hybrid *h, int *run) {
    SML_REQUIRE(h && run, "null argument");
    if (!h->advanced) {
        *run = 1;
        return SML_OK;
    }
    if (int rc = sml_dyn_last_safe(h->dyn, run, nullptr)) return rc;
    // once that step's check is done, every wait of the step has run (the check follows
    // the entry specx -- behind k_io_entry, or behind the window's first row kernel's go
    // when the entry is inside the window graph -- which follows the finish), or the
    // check's own hand-off gave up (reported below): a wait that gave up fails the step
    // here, so a host polling per step (parallelmain.f90:268-270) stops instead of
    // going on from NaN forecasts; run_speedy is then 0
    if (int rc = h->hops.late_check("sml_hybrid_run_speedy")) {
        *run = 0;
        return rc;
    }
    if (int rc = sml::dyn_check_late(h->dyn)) {
        *run = 0;
        return rc;
    }
    return SML_OK;
}

// wait for every issued step; the local model of the last window is tiled as the
// one-stream loop leaves it (the overlapped loop tiles it inside the next finish)
extern "C" int sml_hybrid_sync(sml_hybrid *h) {
    SML_REQUIRE(h, "null context");
    if (h->overlap && h->advanced && h->ncs) {
        if (h->sched.hops)
            if (int rc = h->hops.wait(kHopLm, h->main)) return rc;
        if (int rc = sml_res_tile_local_model(h->res, h->f4, h->f2, h->lm, h->chain_stream())) return rc;
    }
    SML_HIP(hipStreamSynchronize(h->main));
    SML_HIP(hipStreamSynchronize(h->side));
    if (int rc = h->hops.late_check("sml_hybrid_sync")) return rc;
    return sml::dyn_check_late(h->dyn);
}
