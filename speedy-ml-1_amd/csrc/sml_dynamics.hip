// sml_dynamics.hip -- one SPEEDY dynamics time step on gfx950.
//
// Reference: step (src/dyn_step.f90:1-128) =
//   grtend  (src/dyn_grtend.f90:1-279): 50 inverse transforms of the j2 state,
//           grid-point dynamics, physics hook (phypar, :225), 73 forward transforms
//   sptend  (src/dyn_sptend.f90:1-67) + geop (src/dyn_geop.f90:1-33)
//   implic  (src/dyn_implic.f90:1-68)         (alph != 0)
//   hordif, stratospheric drag, tracer diffusion (dyn_step.f90:60-112, :130-151)
//   timint with trunct, Robert-Williams filter  (dyn_step.f90:114-127, :153-190)
//
// MI355X design: the reference's ~164 one-field transforms per step become 7
// batched MFMA transform launches (gridy on 50 fields, gridx kcos=1/2, specx
// scaled/unscaled, specy on 73 fields); the grid-point dynamics is one kernel
// with a thread per grid column (vertical recurrences in registers); everything
// after the forward transforms (vds/lap assembly, sptend, geop, implic, hordif,
// drag, timint) runs in two kernels with a thread per spectral coefficient (m, n)
// that owns all levels, variables and both time levels of that coefficient, so no
// stage needs a grid-wide synchronisation.
//
// Physics (phypar, dyn_grtend.f90:223-226) runs on the GPU when the context has
// boundary fields (sml_dyn_set_physics): grtend always evaluates it on time level 1
// (dyn_step.f90:45), so the step adds 41 inverse transforms of level 1 (ucos,
// vcos, t, q, geop(1), ps; phy_phypar.f90:54-66) to the same batched launches and
// one column-physics kernel (sml_physics.hpp) whose tendencies enter where phypar
// adds them (after the dynamical tendencies, before the spectral conversion).
// Without boundary fields the tendencies come from an optional input buffer (a
// host that keeps phypar on the CPU) or are zero.
//
// This file is the unit's host side -- the context, the launches and the C ABI -- and
// the one translation unit that compiles its kernels, which live in headers by stage
// (sml_dyn_*.hpp, included below).  The context's host state is three objects: DevMem
// (every allocation), IoCheck (iogrid(30)'s safety check beside the window) and the
// round-robin caches of sml_dyn_cache.hpp (impint table slots, captured graphs).
#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "sml_dynamics_tables.hpp"
#include "sml_spectral_internal.hpp"
#include "sml_timeline.hpp"

SML_TL_DEFINE(dynamics)

// every kernel of the unit, by stage, in the order of a step: one translation unit,
// one set of compile flags (the Makefile's FLAGS_sml_dynamics)
// clang-format off
#include "sml_dyn_layout.hpp"
#include "sml_dyn_unfused.hpp"
#include "sml_dyn_fused.hpp"
#include "sml_dyn_io.hpp"
#include "sml_dyn_forcing.hpp"
// clang-format on
#include "sml_devmem.hpp"
#include "sml_dyn_cache.hpp"

using namespace sml;

namespace {

struct GraphRelease {
    void operator()(hipGraphExec_t &g) const {
        if (g) (void)hipGraphExecDestroy(g);
        g = nullptr;
    }
};

// the stream the context captures its graphs on, created at the first capture
struct CaptureStream {
    hipStream_t s = nullptr;
    CaptureStream() = default;
    CaptureStream(const CaptureStream &) = delete;
    CaptureStream &operator=(const CaptureStream &) = delete;
    ~CaptureStream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

// iogrid(30)'s safety check (ppo_iogrid.f90:556-571): the re-grid of the entry state
// and its min / max of u, v, t, q, on a stream of its own beside the window, and the
// hand-offs of its result to run_model's exit and to the host.  The only code that
// reads or writes these fields.
struct IoCheck {
    // wiring, set once by sml_dyn_create
    sml_spectral *sp = nullptr;
    DevMem *mem = nullptr;       // the context's owner, for the lazy allocations below
    double *d_minmax = nullptr;  // the context's min/max of u, v, t, q: where a check without a caller's buffer writes
    // the check's inputs [kNIo][kSF], Fourier [kNIo][kVF] and grid [kNIo][kGF] buffers
    double *d_chk = nullptr;
    // The check's own stream with the events around it.  ev_fork: recorded on the caller's
    // stream once the check's inputs are written there, waited for by chk_stream.
    // ev_chk: recorded behind every check on chk_stream (the check's last operation).
    hipStream_t chk_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_chk = nullptr;
    // ev_chk is recorded and nobody has waited for it (nor taken the counter hand-off in
    // its place): the check may still read d_chk and write its min/max, so the next user
    // of either waits first (wait_pending)
    bool chk_pending = false;
    // run_model's exit learns the check's result from a device counter instead of an
    // event wait on its stream: the check's k_io_minmax adds 4 per counted check and the
    // exit polls for the target.  chk_count is the number of counted checks launched:
    // the counter reaches next_target() = 4 * (chk_count + 1) with the check about to be
    // launched, and last_target() = 4 * chk_count with the last one launched
    unsigned *d_chk_cnt = nullptr;
    unsigned chk_count = 0;
    // the last launch added to the counter (on chk_stream, writing d_minmax): only then
    // may an exit take the hand-off, and only then does d_chk_late speak of this check
    bool chk_counted = false;
    // An exit (or k_check_go) that timed out stores the counter target of the check it
    // gave up on into this pinned, host-visible word, read without a copy by last() and
    // late_reported(), which resets it.  chk_timeout: their give-up time in ticks
    unsigned *d_chk_late = nullptr;
    long long chk_timeout = 100000000ll;
    // host copy of the last check's min/max (pinned; written behind the check on its
    // stream): mm_issued says that copy was enqueued and ev_mm marks its end, for a host
    // loop that reads run_speedy without a device sync.  mm_last: the device min/max of
    // the last check, wherever it ran (read synchronously when !mm_issued)
    double *h_mm = nullptr;
    hipEvent_t ev_mm = nullptr;
    bool mm_issued = false;
    const double *mm_last = nullptr;
    // The entry inside the window graph: the check waits on its own stream (k_check_go)
    // for *d_go >= the window's number, which the window's first row kernel stores as it
    // starts (k_io_entry's outputs are released by then) -- no event fork after
    // k_io_entry.  go_count: the number of the last such window (they count from 1)
    uint64_t *d_go = nullptr;
    uint64_t go_count = 0;

    IoCheck() = default;
    IoCheck(const IoCheck &) = delete;
    IoCheck &operator=(const IoCheck &) = delete;
    ~IoCheck();

    int allocate();
    int ensure_stream();
    unsigned next_target() const { return 4u * (chk_count + 1); }
    unsigned last_target() const { return 4u * chk_count; }
    int next_go(uint64_t *go);
    int launch(hipStream_t st, double *d_mm, uint64_t go = 0);
    int wait_pending(hipStream_t st);
    bool take_handoff();
    void exit_waits_for_counter(IoExit *ex, unsigned target, const uint64_t *xa) const;
    int last(double *mm, int *safe);
    bool late_reported();
    int sync();
    int reset_stream(int first_cu, int num_cus);
    void set_timeout(long long ticks) { chk_timeout = ticks; }
    uint64_t *go_word() const { return d_go; }
    double *inputs() const { return d_chk; }  // where k_io_prep / k_io_entry leave the check's spectral inputs
    hipStream_t stream() const { return chk_stream; }
    // the event behind the last check issued on the check stream (null if none)
    hipEvent_t event() const { return chk_stream ? ev_chk : nullptr; }
};

}  // namespace

struct sml_dynamics {
    DevMem mem;  // first: destroyed last, after the graphs, streams and events below
    sml_spectral *sp = nullptr;
    DynTables tab;
    DynTables *d_tab = nullptr;   // current impint slot (one of d_tabs)
    double *d_tabm = nullptr;     // per slot: TabM of every m (the fused spectral stage's per-m tables)
    DynTables *d_tabs = nullptr;  // kTabSlots device copies keyed by (dt, alph): stepone's
                                  // three impint calls per window become pointer switches
    static constexpr int kTabSlots = 4;
    RoundRobinCache<ImpintKey, NoValue, kTabSlots> slots;
    double *d_state = nullptr;
    double *d_phis = nullptr, *d_tcorh = nullptr, *d_qcorh = nullptr, *d_phi = nullptr;
    double *d_specin = nullptr, *d_varm = nullptr, *d_grid = nullptr, *d_gfwd = nullptr, *d_sfwd = nullptr;
    double *d_vfm = nullptr;  // fused step: m-major forward Fourier coefficients [m][73][lat][2]
    double *d_pfl = nullptr;  // specy's MFMA B operands in lane order [m][k-step][lane][S, D] (k_pack_pfwd)
    double *d_sm = nullptr;   // fused step: m-major state [2][m][var 5][lev 2][kx][n p], ping-pong:
                              // k_st_spec reads one buffer and writes the other (StepCtl::sm, sm_buf)
    long long *d_dbg = nullptr;  // diagnostic phase stamps (SML_DYN_STAMPS=1)
    double *d_tend = nullptr;
    double *d_phys = nullptr;  // physics tendencies: staging for a host's, or the GPU phypar's output
    double *d_minmax = nullptr;  // iogrid(30) safety check: min/max of u, v, t, q
    double *d_io = nullptr;      // staging for the host iogrid calls (grid4d + logp)
    // iogrid(30)'s safety check (re-grid + min/max) runs on its own stream beside the window
    IoCheck chk;
    // one-shot hooks of the next run_model, taken (and so cleared) as it starts; the next
    // from_grid takes the entry's two
    struct RunModelHooks {
        HopWait entry_wait;             // the entry waits in-kernel for its input grids (sml::dyn_run_model_wait)
        uint64_t *entry_sig = nullptr;  // the entry signals its input grid in-kernel (sml::dyn_run_model_entry_signal)
        // the exit is followed by a store of exit_store_value to *exit_store
        // (sml::dyn_run_model_exit_store: the hybrid loop's forecast hop)
        uint64_t *exit_store = nullptr;
        uint64_t exit_store_value = 0;
    } hooks;
    bool impint_done = false;
    // GPU physics (phypar): tables, boundary fields [kNBc][ngp], radiation state
    PhysTables ptab;
    PhysTables *d_ptab = nullptr;
    double *d_pbc = nullptr, *d_rad = nullptr, *d_pio = nullptr;
    bool phys_on = false;
    // ini_sea's hybrid block (cpl_sea.f90:38-46): the coupler's sst_am as set_physics
    // gave it, sea-ice fraction / temperature, and the hybrid SST grid last applied
    // (sml_dyn_set_hybrid_sst; re-applied when set_physics brings a new sst_am)
    double *d_sst_cpl = nullptr, *d_sice = nullptr, *d_tice = nullptr;
    const double *hyb_sst = nullptr;
    double hyb_bias = 0.0;
    // agcm_init's per-window forcing (sml_dyn_fordate): inbcon's surface fields
    // [3][ngp] = fmask_l, fmask_s, alb0; the coupler's monthly climatologies
    // [5][12][ngp] = stl12, snowd12, soilw12, sst12, sice12 (optional); the two grid
    // fields of tcorh / qcorh and their Fourier coefficients
    double *d_surf = nullptr, *d_clim = nullptr, *d_ford = nullptr;
    bool surf_on = false, clim_on = false;
    // fordate's inputs change with the date or a setter: the generation of the
    // setters' inputs and the date of the last fordate (recomputed only on a change)
    long long ford_gen = 1, ford_done = 0;
    int ford_date[2] = {0, 0};
    int ford_count = 0;  // fordate recomputations issued (sml_dyn_fordate_count)
    // step kernels: the fused form (default: 2-3 launches per chained step, FMA
    // contraction) or the 8/9-launch form whose transforms are FFTPACK's separate
    // multiplies and adds (sml_dyn_set_fused; the two agree to rounding)
    bool fused = true;
    bool nograph = false;  // SML_DYN_NOGRAPH=1: the window's launches issued directly, not replayed
    // mod_lflags lradsw (module default .true.) and stloop's istep (at_gcm.f90:81)
    bool lradsw = true;
    int istep = 1;
    // leapfrog replay: one step(2, 2, ...) captured as a hipGraph per lradsw value
    // (declared behind chk and ahead of the graphs: the graphs go first, then this
    // stream, then the check's stream and events, then the memory)
    CaptureStream cap;
    RoundRobinCache<LeapfrogKey, hipGraphExec_t, 1, GraphRelease> replay[2];
    // whole-window replay (sml_dyn_window): stepone + nleap leapfrog steps, one graph; with
    // run_model's exit captured behind the window, and with it the entry (iogrid(30)'s
    // specx + k_io_entry) in front of it, their fixed arguments are part of the key (the
    // per-launch values come from d_xa, written before each launch).
    // [prepared entry (sml_dyn_run_model)][entry lradsw] x kReplayWays graphs each, so a
    // caller alternating its forecast / input buffers (ping-pong) replays one graph per
    // buffer set instead of re-capturing the window every call; round-robin eviction
    static constexpr int kReplayWays = 4;
    RoundRobinCache<WindowKey, hipGraphExec_t, kReplayWays, GraphRelease> wreplay[4];
    // a graph-captured run_model's per-launch values: [0] the check count the exit waits
    // for, [1] the hop value its store writes, [2] the hop value the entry specx waits for,
    // [3] the window's number, which its first row kernel hands the safety check
    // (k_set_xa right before the graph; k_io_entry when only the exit is captured)
    uint64_t *d_xa = nullptr;
    // the entry goes inside the window graph (IoCheck's go hand-off) for a run_model with
    // no capture of the caller's and not under serialised dispatch
    bool serialized = false;  // AMD_SERIALIZE_KERNEL / rocprofv3's counter collection at create
};

// ------------------------------------------------------------------ API
extern "C" int sml_dyn_destroy(sml_dynamics *d) {
    if (!d) return SML_OK;
    // the check stream's work completes first; then the context's members go in the
    // reverse of their order there: graphs, streams and events, memory
    (void)d->chk.sync();
    sml_spectral *sp = d->sp;
    delete d;
    if (sp) sml_spectral_destroy(sp);
    return SML_OK;
}

namespace {

// the context's buffers that live as long as it does, each with its size
int allocate_buffers(sml_dynamics *d) {
    DevMem &m = d->mem;
    if (const char *e = std::getenv("SML_DYN_STAMPS"))
        if (*e && *e != '0') m.device(&d->d_dbg, (size_t)kStampKernels * kStampBlocks * kStamps);
    m.device(&d->d_tabs, sml_dynamics::kTabSlots);
    m.device(&d->d_tabm, (size_t)sml_dynamics::kTabSlots * kMX * kTabMDoubles + kTabMPad);
    m.device(&d->d_state, kStateSize);
    m.device(&d->d_phis, kSF);
    m.device(&d->d_tcorh, 2 * kSF);
    d->d_qcorh = d->d_tcorh ? d->d_tcorh + kSF : nullptr;  // one allocation: fordate's spec writes both fields
    m.device(&d->d_phi, kKX * kSF);
    m.device(&d->d_specin, (size_t)kNInvMax * kSF);
    m.device(&d->d_varm, (size_t)(kNInvMax > kNFwd ? kNInvMax : kNFwd) * kVF);
    m.device(&d->d_grid, (size_t)kNInvMax * kGF);
    m.device(&d->d_gfwd, (size_t)kNFwd * kGF);
    m.device(&d->d_sfwd, (size_t)kNFwd * kSF);
    m.device(&d->d_tend, kTendSize);
    m.device(&d->d_vfm, (size_t)kMX * kVFm);
    m.device(&d->d_sm, (size_t)2 * kMX * kSM);
    m.device(&d->d_pfl, (size_t)kMX * (kIY / 4) * 64 * 2);
    m.device(&d->d_phys, (size_t)4 * kKX * kGF);
    m.device(&d->d_minmax, 8);
    m.device(&d->d_io, (size_t)4 * kKX * kGF + kGF);
    m.device(&d->d_ptab, 1);
    m.device(&d->d_pbc, (size_t)kNBc * kNGP);
    m.device(&d->d_rad, kRadSize);
    m.device(&d->d_pio, (size_t)(5 * kKX + 1 + 4 * kKX) * kNGP);
    m.device(&d->d_sst_cpl, kNGP);
    m.device(&d->d_sice, kNGP);
    m.device(&d->d_tice, kNGP);
    m.device(&d->d_surf, (size_t)3 * kNGP);
    m.device(&d->d_ford, (size_t)2 * (kGF + kVF));
    d->chk.sp = d->sp;
    d->chk.mem = &d->mem;
    d->chk.d_minmax = d->d_minmax;
    return d->chk.allocate();
}

int upload_tabm(sml_dynamics *d, int i);

}  // namespace

extern "C" int sml_dyn_create(double radius, sml_dynamics **out) {
    SML_REQUIRE(out, "out is null");
    *out = nullptr;
    sml_dynamics *d = new (std::nothrow) sml_dynamics();
    if (!d) return fail(SML_ERR_NOMEM, "host allocation failed");
    int rc = sml_spectral_create(radius, &d->sp);
    if (rc) {
        delete d;
        return rc;
    }
    build_dyn_indyns(spectral_host_tables(d->sp), &d->tab);
    build_phys_tables(d->tab, &d->ptab);
    if (const char *e = std::getenv("SML_DYN_NOGRAPH")) d->nograph = *e && *e != '0';
    // dispatch serialised by the runtime or a profiler's counter passes: the check must
    // not wait for a kernel enqueued after it (IoCheck::launch's go hand-off)
    for (const char *v : {"AMD_SERIALIZE_KERNEL", "ROCPROF_COUNTER_COLLECTION"})
        if (const char *e = std::getenv(v)) d->serialized = d->serialized || (*e && std::strcmp(e, "0") != 0);
    if ((rc = allocate_buffers(d))) {
        sml_dyn_destroy(d);
        return rc;
    }
    d->d_tab = d->d_tabs;
    hipError_t e = hipMemcpy(d->d_tab, &d->tab, sizeof(DynTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d->d_ptab, &d->ptab, sizeof(PhysTables), hipMemcpyHostToDevice);
    if (e == hipSuccess) {  // specy's packed B operands from the spectral context's forward Legendre table
        const int n = kMX * (kIY / 4) * 64;
        hipLaunchKernelGGL(k_pack_pfwd, dim3((n + 255) / 256), dim3(256), 0, 0, spectral_dev(d->sp).pfwd, d->d_pfl);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        sml_dyn_destroy(d);
        return fail(SML_ERR_HIP, "sml_dyn_create: %s", hipGetErrorString(e));
    }
    // slot 0's per-m copy too: run_model's entry (k_io_entry) reads the current slot's
    // TabM, before any impint when it is the first call
    if (int rc = upload_tabm(d, 0)) {
        sml_dyn_destroy(d);
        return rc;
    }
    *out = d;
    return SML_OK;
}

namespace {

// the per-m TabM copies of d->tab into slot i of d_tabm
int upload_tabm(sml_dynamics *d, int i) {
    std::vector<double> tm((size_t)kMX * kTabMDoubles);
    for (int m = 0; m < kMX; ++m)
        for (int q = 0; q < kTabMDoubles; ++q) tm[(size_t)m * kTabMDoubles + q] = tabm_value(&d->tab, m, q);
    SML_HIP(hipMemcpy(d->d_tabm + (size_t)i * kMX * kTabMDoubles, tm.data(), tm.size() * 8, hipMemcpyHostToDevice));
    return SML_OK;
}

// impint(dt, alph): the tables' slot becomes the current one (*slot, if asked for).  A
// miss never evicts one of the `pinned` slots (a window holds three at once)
int impint_slot(sml_dynamics *d, double dt, double alph, unsigned pinned, int *slot) {
    bool hit = false;
    const int i = d->slots.acquire(ImpintKey{dt, alph}, pinned, &hit);
    if (i < 0) return fail(SML_ERR_STATE, "sml_dyn_impint: every table slot is pinned");
    if (!hit) {  // (a hit: no host work, no copy)
        build_dyn_impint(dt, alph, &d->tab);
        // the copy is ordered before later launches on the legacy stream; kernels still
        // reading an evicted slot were launched earlier and complete first
        auto upload = [&]() {
            SML_HIP(hipDeviceSynchronize());
            SML_HIP(hipMemcpy(d->d_tabs + i, &d->tab, sizeof(DynTables), hipMemcpyHostToDevice));
            return upload_tabm(d, i);
        };
        if (int rc = upload()) {
            d->slots.drop(i);  // whatever the slot holds now, it is not this key's tables
            return rc;
        }
    }
    d->d_tab = d->d_tabs + i;
    d->impint_done = true;
    if (slot) *slot = i;
    return SML_OK;
}

}  // namespace

extern "C" int sml_dyn_impint(sml_dynamics *d, double dt, double alph) {
    SML_REQUIRE(d, "null context");
    return impint_slot(d, dt, alph, 0, nullptr);
}

extern "C" int sml_dyn_set_forcing(sml_dynamics *d, const double *phis, const double *tcorh, const double *qcorh) {
    SML_REQUIRE(d, "null context");
    if (phis) SML_HIP(hipMemcpy(d->d_phis, phis, kSF * 8, hipMemcpyHostToDevice));
    if (tcorh) SML_HIP(hipMemcpy(d->d_tcorh, tcorh, kSF * 8, hipMemcpyHostToDevice));
    if (qcorh) SML_HIP(hipMemcpy(d->d_qcorh, qcorh, kSF * 8, hipMemcpyHostToDevice));
    ++d->ford_gen;  // a later sml_dyn_fordate recomputes what the host has just replaced
    return SML_OK;
}

extern "C" int sml_dyn_get_forcing(sml_dynamics *d, double *phis, double *tcorh, double *qcorh) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    if (phis) SML_HIP(hipMemcpy(phis, d->d_phis, kSF * 8, hipMemcpyDeviceToHost));
    if (tcorh) SML_HIP(hipMemcpy(tcorh, d->d_tcorh, kSF * 8, hipMemcpyDeviceToHost));
    if (qcorh) SML_HIP(hipMemcpy(qcorh, d->d_qcorh, kSF * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_set_state(sml_dynamics *d, const double *vor, const double *div, const double *t,
                                 const double *ps, const double *tr) {
    SML_REQUIRE(d && vor && div && t && ps && tr, "null argument");
    const size_t f3 = 2 * kKX * kSF * 8;
    SML_HIP(hipMemcpy(d->d_state + kOffVor, vor, f3, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_state + kOffDiv, div, f3, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_state + kOffT, t, f3, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_state + kOffTr, tr, f3, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_state + kOffPs, ps, 2 * kSF * 8, hipMemcpyHostToDevice));
    return SML_OK;
}

extern "C" int sml_dyn_get_state(sml_dynamics *d, double *vor, double *div, double *t, double *ps, double *tr) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    const size_t f3 = 2 * kKX * kSF * 8;
    if (vor) SML_HIP(hipMemcpy(vor, d->d_state + kOffVor, f3, hipMemcpyDeviceToHost));
    if (div) SML_HIP(hipMemcpy(div, d->d_state + kOffDiv, f3, hipMemcpyDeviceToHost));
    if (t) SML_HIP(hipMemcpy(t, d->d_state + kOffT, f3, hipMemcpyDeviceToHost));
    if (tr) SML_HIP(hipMemcpy(tr, d->d_state + kOffTr, f3, hipMemcpyDeviceToHost));
    if (ps) SML_HIP(hipMemcpy(ps, d->d_state + kOffPs, 2 * kSF * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_get_phi(sml_dynamics *d, double *phi) {
    SML_REQUIRE(d && phi, "null argument");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(phi, d->d_phi, kKX * kSF * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_get_tendencies(sml_dynamics *d, double *tend) {
    SML_REQUIRE(d && tend, "null argument");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(tend, d->d_tend, kTendSize * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_state_device(sml_dynamics *d, double **d_state, double **d_phys) {
    SML_REQUIRE(d, "null context");
    if (d_state) *d_state = d->d_state;
    if (d_phys) *d_phys = d->d_phys;
    return SML_OK;
}

namespace {

// what one step's launches depend on besides step()'s own arguments
struct StepCtl {
    const DynTables *tab;  // the impint slot of the step's (dt, alph)
    bool lradsw;           // shortwave radiation on this step (GPU physics)
    // the fused step only.  chained: the previous step's k_st_spec left the m-major state
    // in buffer sm and this step's gridy output (its next_j2 was this j2), else the step
    // starts from the reference-layout state; next_j2 > 0: this step's k_st_spec does that
    // for step (.., next_j2) in buffer 1 - sm, else it writes the reference-layout state
    bool chained = false;
    int next_j2 = 0;
    int sm = 0;
    // the last step (next_j2 == 0) of a run_model window: the Fourier buffer its k_st_spec
    // fills with iogrid(31)'s gridy (spectral layout), else null
    double *io_exit = nullptr;
    // the row kernel (GPU physics) hands *go_src to *go_dst at its start, or null
    const uint64_t *go_src = nullptr;
    uint64_t *go_dst = nullptr;
};

// the unfused launches of one step(j1, j2, dt, alph, rob, wil) on stream st: 7
// without GPU physics, 8 with it
int launch_step_unfused(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                        const double *d_phys, const StepCtl &c, hipStream_t st) {
    const DynTables *T = c.tab;
    const bool phys = d->phys_on;
    const int n1 = phys ? kNInv1P : kNInv1, nin = phys ? kNInvP : kNInv;
    // 1. grtend: inverse transforms of the j2 state (+ phypar's level-1 inputs)
    hipLaunchKernelGGL(k_dyn_prep, dim3((kMN + 127) / 128, kKX + 1), dim3(128), 0, st, d->d_state, d->d_specin, T,
                       d->d_phis, j2, n1, phys ? 1 : 0);
    SML_HIP(hipGetLastError());
    if (int rc = spectral_gridy(d->sp, d->d_specin, d->d_varm, nin, st)) return rc;
    if (int rc = spectral_gridx_split(d->sp, d->d_varm, d->d_grid, nin, n1, st)) return rc;
    // 2. physics (phypar on level 1), then grid-point dynamics + physics tendencies
    if (phys) {
        const double *G = d->d_grid;
        hipLaunchKernelGGL(k_phys, dim3(kNGP / 64), dim3(64), 0, st, G + (size_t)(n1 + 2 * kKX + 2) * kGF,
                           G + (size_t)(n1 + 3 * kKX + 2) * kGF, G + (size_t)kPT1 * kGF, G + (size_t)kPQ1 * kGF,
                           G + (size_t)kPPhi1 * kGF, G + (size_t)kPPs1 * kGF, d->d_pbc, d->d_rad, d->d_ptab,
                           c.lradsw ? 1 : 0, d->d_phys);
        SML_HIP(hipGetLastError());
        d_phys = d->d_phys;
    }
    hipLaunchKernelGGL(k_dyn_gridpoint, dim3((kGF + 255) / 256), dim3(256), 0, st, d->d_grid, d_phys, d->d_gfwd, T,
                       n1);
    SML_HIP(hipGetLastError());
    // 3. forward transforms: vdspec inputs x 1/cos (kcos = 2), the rest plain
    if (int rc = spectral_specx_split(d->sp, d->d_gfwd, d->d_varm, kNFwd, kNFwdScaled, st)) return rc;
    if (int rc = spectral_specy(d->sp, d->d_varm, d->d_sfwd, kNFwd, st)) return rc;
    hipLaunchKernelGGL(k_dyn_combine, dim3((kMN + 127) / 128, kKX), dim3(128), 0, st, d->d_sfwd, d->d_tend, T);
    SML_HIP(hipGetLastError());
    // 4. sptend / implic / diffusion / time integration
    const int j4 = (alph == 0.0) ? j2 : 1;
    hipLaunchKernelGGL(k_dyn_tail, dim3(kSF / kTailC), dim3(kTailC * kKX), 0, st, d->d_state, d->d_tend, d->d_phi,
                       d->d_phis, d->d_tcorh, d->d_qcorh, T, j1, j4, dt, alph, rob, wil);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// buffer b of the m-major state (two, so k_st_spec's second block of an m never
// reads a slice its lead block already advanced)
double *sm_buf(sml_dynamics *d, int b) { return d->d_sm + (size_t)b * kMX * kSM; }

// the per-m TabM copies of impint slot T
const double *tabm_of(const sml_dynamics *d, const DynTables *T) {
    return d->d_tabm + (size_t)(T - d->d_tabs) * kMX * kTabMDoubles;
}

// the fused step: [k_state_to_m k_st_inv] (k_st_rows | k_st_gridspec_p) k_st_spec
int launch_step_fused(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                      const double *d_phys, const StepCtl &c, hipStream_t st) {
    const DynTables *T = c.tab;
    const bool phys = d->phys_on;
    const int n1 = phys ? kNInv1P : kNInv1, nin = phys ? kNInvP : kNInv;
    const SpectralDev sd = spectral_dev(d->sp);
    const int next_j2 = dt > 0.0 ? c.next_j2 : 0;  // tendencies only: the state does not advance
    const int conv_blocks = (kMX * kSM + 255) / 256;
    if (!c.chained) {
        hipLaunchKernelGGL(k_state_to_m, dim3(conv_blocks), dim3(256), 0, st, d->d_state, sm_buf(d, c.sm));
        SML_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_st_inv, dim3(kMX), dim3(kSpecThreads), 0, st, sm_buf(d, c.sm), d->d_phis, T, sd.pinv,
                           d->d_varm, j2, n1, nin);
        SML_HIP(hipGetLastError());
    }
    if (phys) {
        hipLaunchKernelGGL(k_st_gridspec_p, dim3(kIL), dim3(kGpThreads), 0, st, d->d_varm, d->d_vfm, sd.wa, sd.cosgr, T,
                           d->d_pbc, d->d_rad, d->d_ptab, c.lradsw ? 1 : 0, c.go_src, c.go_dst, d->d_dbg);
        SML_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_st_rows, dim3(kIL), dim3(kRowThreads), 0, st, d->d_varm, d->d_vfm, sd.wa, sd.cosgr, T,
                           d_phys, d->d_dbg);
        SML_HIP(hipGetLastError());
    }
    const int j4 = (alph == 0.0) ? j2 : 1;
    hipLaunchKernelGGL(k_st_spec, dim3(kSpecStride * kSpecSplit), dim3(kSpecBlk), 0, st, d->d_vfm, d->d_pfl, sd.wt,
                       sm_buf(d, c.sm), sm_buf(d, 1 - c.sm), d->d_tend,
                       d->d_phi, d->d_phis, d->d_tcorh, d->d_qcorh, T, j1, j4, dt, alph, rob, wil, sd.pinv, d->d_varm,
                       next_j2, n1, nin, tabm_of(d, T), d->d_state, next_j2 > 0 ? nullptr : c.io_exit, d->d_dbg);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

int launch_step(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil, const double *d_phys,
                const StepCtl &c, hipStream_t st) {
    return d->fused ? launch_step_fused(d, j1, j2, dt, alph, rob, wil, d_phys, c, st)
                    : launch_step_unfused(d, j1, j2, dt, alph, rob, wil, d_phys, c, st);
}

// what body(stream) enqueues, captured and instantiated as *out (null on an error);
// what: the caller's name for the messages
template <class Body>
int capture_graph(sml_dynamics *d, const char *what, Body body, hipGraphExec_t *out) {
    *out = nullptr;
    hipStream_t &cs = d->cap.s;
    if (!cs) SML_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    hipGraph_t g = nullptr;
    SML_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    const int rc = body(cs);
    hipError_t e = hipStreamEndCapture(cs, &g);  // whatever rc: the stream leaves capture mode
    if (rc || e != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        return rc ? rc : fail(SML_ERR_HIP, "%s capture: %s", what, hipGetErrorString(e));
    }
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(SML_ERR_HIP, "%s instantiate: %s", what, hipGetErrorString(e));
    }
    return SML_OK;
}

}  // namespace

extern "C" int sml_dyn_step(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                            const double *d_phys, void *stream) {
    SML_REQUIRE(d, "null context");
    SML_REQUIRE((j1 == 1 || j1 == 2) && (j2 == 1 || j2 == 2), "j1/j2 must be 1 or 2");
    SML_REQUIRE(!(d->phys_on && d_phys), "physics runs on the GPU (sml_dyn_set_physics): d_phys must be NULL");
    if (!d->impint_done) return fail(SML_ERR_STATE, "sml_dyn_impint must be called before sml_dyn_step");
    return launch_step(d, j1, j2, dt, alph, rob, wil, d_phys, StepCtl{d->d_tab, d->lradsw}, (hipStream_t)stream);
}

namespace {

// the step(2, 2, dt, ...) graph for one lradsw value, (re)captured when its inputs change
int leapfrog_graph(sml_dynamics *d, bool lradsw, const LeapfrogKey &key, const double *d_phys, hipGraphExec_t *out) {
    auto &cache = d->replay[lradsw ? 1 : 0];
    bool hit = false;
    const int w = cache.acquire(key, 0, &hit);
    if (!hit) {
        const StepCtl c{d->d_tab, lradsw};
        if (int rc = capture_graph(
                d, "sml_dyn_leapfrog",
                [&](hipStream_t st) { return launch_step(d, 2, 2, key.dt, key.alph, key.rob, key.wil, d_phys, c, st); },
                &cache.value(w))) {
            cache.drop(w);
            return rc;
        }
    }
    *out = cache.value(w);
    return SML_OK;
}

}  // namespace

extern "C" int sml_dyn_leapfrog(sml_dynamics *d, int nsteps, double dt, double alph, double rob, double wil,
                                const double *d_phys, void *stream) {
    SML_REQUIRE(d && nsteps >= 0, "bad argument");
    SML_REQUIRE(!(d->phys_on && d_phys), "physics runs on the GPU (sml_dyn_set_physics): d_phys must be NULL");
    if (!d->impint_done) return fail(SML_ERR_STATE, "sml_dyn_impint must be called before sml_dyn_leapfrog");
    // stloop (dyn_stloop.f90:37-56): lradsw = (mod(istep, nstrad) == 1) before each step
    for (int i = 0; i < nsteps; ++i) {
        const bool lradsw = (d->istep % kNstrad == 1);
        hipGraphExec_t exec = nullptr;  // without GPU physics lradsw is irrelevant: one graph
        const LeapfrogKey key{dt, alph, rob, wil, d_phys, d->d_tab, d->phys_on};
        if (int rc = leapfrog_graph(d, d->phys_on && lradsw, key, d_phys, &exec)) return rc;
        SML_HIP(hipGraphLaunch(exec, (hipStream_t)stream));
        d->lradsw = lradsw;
        ++d->istep;
    }
    return SML_OK;
}

namespace {
// ------------------------------------------------------------------ IoCheck
IoCheck::~IoCheck() {
    if (chk_stream) {
        (void)hipStreamSynchronize(chk_stream);
        (void)hipStreamDestroy(chk_stream);
    }
    for (hipEvent_t ev : {ev_fork, ev_chk, ev_mm})
        if (ev) (void)hipEventDestroy(ev);
}

// the buffers the check needs from the start
int IoCheck::allocate() {
    mem->device(&d_chk, (size_t)kNIo * (kSF + kVF + kGF));
    mem->device(&d_chk_cnt, 2);
    mem->pinned(&d_chk_late, 1, hipHostMallocCoherent);
    return mem->status();
}

int IoCheck::ensure_stream() {
    if (!chk_stream) SML_HIP(hipStreamCreateWithFlags(&chk_stream, hipStreamNonBlocking));
    if (!ev_fork) SML_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    if (!ev_chk) SML_HIP(hipEventCreateWithFlags(&ev_chk, hipEventDisableTiming));
    return SML_OK;
}

// the number of the next window whose entry is inside its graph (launch's go)
int IoCheck::next_go(uint64_t *go) {
    if (!d_go) {
        if (int rc = mem->device(&d_go, 1)) return rc;
        go_count = 0;
    }
    *go = ++go_count;
    return SML_OK;
}

// The check from its spectral inputs in d_chk (k_io_prep / k_io_entry, already on st):
// the re-grid and its min / max run on chk_stream beside the window.  A caller's d_mm is
// ready in st's order; the internal one (nullptr) only for the next user of d_chk (which
// waits for it).  go > 0 (the entry inside the window graph): instead of an event fork
// from st, the check's stream waits in-kernel for the window's first row kernel to store go
int IoCheck::launch(hipStream_t st, double *d_mm, uint64_t go) {
    double *cs = d_chk, *cv = cs + (size_t)kNIo * kSF, *cg = cv + (size_t)kNIo * kVF;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SML_HIP(hipStreamIsCapturing(st, &cap));
    hipStream_t cst = st;
    if (cap == hipStreamCaptureStatusNone) {
        if (int rc = ensure_stream()) return rc;
        cst = chk_stream;
        if (go) {
            hipLaunchKernelGGL(k_check_go, dim3(1), dim3(64), 0, cst, d_go, go, d_chk_late, next_target(),
                               chk_timeout);
            SML_HIP(hipGetLastError());
        } else {
            SML_HIP(hipEventRecord(ev_fork, st));
            SML_HIP(hipStreamWaitEvent(chk_stream, ev_fork, 0));
        }
    } else if (go) {
        return fail(SML_ERR_STATE, "IoCheck::launch: a go hand-off while the stream is captured");
    }
    if (int rc = spectral_gridy(sp, cs, cv, kNIo, cst)) return rc;
    if (int rc = spectral_gridx_range(sp, cv, cg, kNIo, 0, kNIoWind, cst)) return rc;
    double *mm = d_mm ? d_mm : d_minmax;
    // on the check stream, for run_model's exit: the counter hand-off (4 adds per check)
    const bool counted = cst != st && !d_mm;
    hipLaunchKernelGGL(k_io_minmax, dim3(4), dim3(1024), 0, cst, cg, mm, counted ? d_chk_cnt : nullptr,
                       go ? d_chk_late : nullptr, next_target());
    SML_HIP(hipGetLastError());
    if (counted) ++chk_count;
    chk_counted = counted;
    mm_last = mm;
    mm_issued = false;
    if (cst != st) {  // a host copy for last(), behind the check on its stream
        if (!h_mm) {
            if (int rc = mem->pinned(&h_mm, 8, hipHostMallocDefault)) return rc;
            SML_HIP(hipEventCreateWithFlags(&ev_mm, hipEventDisableTiming));
        }
        SML_HIP(hipMemcpyAsync(h_mm, mm, 8 * sizeof(double), hipMemcpyDeviceToHost, cst));
        SML_HIP(hipEventRecord(ev_mm, cst));
        mm_issued = true;
        SML_HIP(hipEventRecord(ev_chk, cst));
        chk_pending = true;
        if (d_mm) {
            SML_HIP(hipStreamWaitEvent(st, ev_chk, 0));
            chk_pending = false;
        }
    }
    return SML_OK;
}

// the previous check still reads d_chk / writes its min/max: st waits for it
int IoCheck::wait_pending(hipStream_t st) {
    if (chk_pending) {
        SML_HIP(hipStreamWaitEvent(st, ev_chk, 0));
        chk_pending = false;
    }
    return SML_OK;
}

// The last check is pending and counted: run_model's exit may wait in-kernel for its
// counter target instead of st waiting for ev_chk.  The check is complete once that exit
// has run, so nothing is pending then.  False: no such check, nothing changes
bool IoCheck::take_handoff() {
    if (!(chk_pending && chk_counted)) return false;
    chk_pending = false;
    return true;
}

// such an exit's arguments: the count to reach is `target`, or xa[0] (and target 0) for an
// exit replayed inside a graph (its arguments are fixed)
void IoCheck::exit_waits_for_counter(IoExit *ex, unsigned target, const uint64_t *xa) const {
    ex->cnt = d_chk_cnt;
    ex->late = d_chk_late;
    ex->timeout = chk_timeout;
    ex->target = target;
    ex->xa = xa;
}

// the last check's min/max on the host and run_speedy's verdict on it: waits only for
// that check
int IoCheck::last(double *mm, int *safe) {
    if (mm_issued) {
        // a host loop polls this once per step (parallelmain.f90:268-270): spin on the
        // event rather than hipEventSynchronize, whose wait policy may yield the thread
        // on a loaded host and wake it late, stalling the next step's enqueue
        hipError_t q;
        while ((q = hipEventQuery(ev_mm)) == hipErrorNotReady) {
        }
        SML_HIP(q);
        std::memcpy(mm, h_mm, 8 * sizeof(double));
    } else if (mm_last) {  // issued on the caller's stream (capture): synchronous copy
        SML_HIP(hipDeviceSynchronize());
        SML_HIP(hipMemcpy(mm, mm_last, 8 * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        return fail(SML_ERR_STATE, "sml_dyn_last_safe before any sml_dyn_from_grid");
    }
    *safe = sml_dyn_is_safe(mm);
    // an exit that gave up on this check took the window as unsafe (it did so before the
    // check completed, so the word is final here).  The word holds the counter target of
    // the check the exit gave up on: a late exit of an earlier window, not yet reported
    // through late_reported(), does not make this one unsafe
    if (d_chk_late && chk_counted && __atomic_load_n(d_chk_late, __ATOMIC_ACQUIRE) == last_target()) *safe = 0;
    return SML_OK;
}

// an exit gave up on its check since the last call: reported once, then reset.  The word
// is host memory: no copy, no sync -- callers read it once the exit has run
bool IoCheck::late_reported() {
    if (!d_chk_late || !__atomic_load_n(d_chk_late, __ATOMIC_ACQUIRE)) return false;
    __atomic_store_n(d_chk_late, 0u, __ATOMIC_RELEASE);
    return true;
}

int IoCheck::sync() {
    if (chk_stream) SML_HIP(hipStreamSynchronize(chk_stream));
    return SML_OK;
}

// the check on compute units [first_cu, first_cu + num_cus), or anywhere (num_cus = 0)
int IoCheck::reset_stream(int first_cu, int num_cus) {
    if (chk_stream) {  // the old stream's check completes first
        SML_HIP(hipStreamSynchronize(chk_stream));
        SML_HIP(hipStreamDestroy(chk_stream));
        chk_stream = nullptr;
        chk_pending = false;
    }
    if (num_cus > 0) {
        void *s = nullptr;
        if (int rc = sml_stream_create_cu_range(first_cu, num_cus, &s)) return rc;
        chk_stream = (hipStream_t)s;
    }
    return ensure_stream();
}

// run_model's entry: iogrid(30)'s specx (waiting for its grid when w.flag) and the per-m
// k_io_entry (specy, the combine into level 1 with impint slot T's tables, the check's
// inputs, the m-major state in buffer 0, step(1, 1)'s gridy); xa: an exit captured in the
// window graph takes its per-launch values from there (k_io_entry stores xa0 / xa1), else null
int launch_entry(sml_dynamics *d, const DynTables *T, const double *d_grid4d, const double *d_logp, HopWait w,
                 hipStream_t st, uint64_t *xa, uint64_t xa0, uint64_t xa1) {
    if (int rc = spectral_specx_io(d->sp, d_grid4d, d_logp, d->d_vfm, kNIoWind, st, w)) return rc;
    const SpectralDev sd = spectral_dev(d->sp);
    const bool phys = d->phys_on;
    hipLaunchKernelGGL(k_io_entry, dim3(kMX), dim3(kSpecThreads), 0, st, d->d_vfm, d->d_pfl, sd.wt, d->d_state,
                       sm_buf(d, 0), d->chk.inputs(), d->d_phis, tabm_of(d, T), sd.pinv, d->d_varm,
                       phys ? kNInv1P : kNInv1, phys ? kNInvP : kNInv, xa, xa0, xa1);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// One SPEEDY window after iogrid(30): stepone (ini_stepone.f90:19-34: step(1, 1,
// delt/2), step(1, 2, delt) with the lradsw the previous window left) and nleap x
// step(2, 2, 2 delt) with stloop's radiation clock restarted at istep = 1
// (dyn_stloop.f90:37-56, at_gcm.f90:81), captured once as ONE hipGraph per
// (entry lradsw, delt, alph, rob, wil, physics on, impint slots) and replayed with
// a single launch, so the host thread never waits on the window's ~200 kernels.

// run_model's exit as enqueue_window issues it behind the window: iogrid(31)'s gridx
// (IoExit) and an optional one-lane store (the hybrid loop's forecast hop)
// and, with `entry`, run_model's entry in front of the window: iogrid(30)'s specx (its
// hop wait's value from d_xa) and k_io_entry, the first row kernel handing *go_src to the
// safety check's *go
struct EntrySpec {
    const double *g4, *logp;
    HopWait w;
    uint64_t *go;
    const uint64_t *go_src;
};
struct ExitSpec {
    const double *varm;
    double *fc4, *fc2;
    IoExit ex;
    uint64_t *store;
    const EntrySpec *entry;
};
struct WindowPlan {
    int nleap;
    double dts[3];  // delt / 2, delt, 2 delt
    double alph, rob, wil;
    DynTables *tab[3];  // their impint slots (4 cached slots hold all three tables at once)
    bool lradsw;        // stepone's: what the previous window left
    // prepared: the m-major state and step(1, 1)'s gridy output are already in place
    // (k_io_entry, fused path of sml_dyn_run_model), so the window starts at the row
    // kernel of the first step and its last kernel does iogrid(31)'s gridy
    bool prepared;
    const ExitSpec *exit;  // or null
};

// the window's launches on st: [entry] step(1, 1) step(1, 2) nleap x step(2, 2) [exit [store]]
int enqueue_window(sml_dynamics *d, hipStream_t st, const WindowPlan &p) {
    StepCtl c{p.tab[0], p.lradsw, p.prepared};
    c.io_exit = p.prepared ? d->d_varm : nullptr;
    if (p.exit && p.exit->entry) {
        // (with the tables the entry read when it was launched before the graph: the
        // last impint's, 2 delt, as the previous window left them)
        const EntrySpec *en = p.exit->entry;
        if (int rc = launch_entry(d, p.tab[2], en->g4, en->logp, en->w, st, nullptr, 0, 0)) return rc;
        c.go_src = en->go_src;  // the first row kernel lets the safety check go
        c.go_dst = en->go;
    }
    // consecutive steps chained: each step's last kernel prepares the next one's inverse
    // transforms (j2 = 1 for step(1, 1), then 2) in the other m-major buffer
    auto step = [&](int j1, int j2, int i, bool last) {
        c.tab = p.tab[i];
        c.next_j2 = last ? 0 : 2;
        const int rc = launch_step(d, j1, j2, p.dts[i], p.alph, p.rob, p.wil, nullptr, c, st);
        c.chained = true;
        if (!last) c.sm = 1 - c.sm;
        c.go_src = nullptr;
        c.go_dst = nullptr;
        return rc;
    };
    if (int rc = step(1, 1, 0, false)) return rc;
    if (int rc = step(1, 2, 1, p.nleap == 0)) return rc;
    for (int i = 0; i < p.nleap; ++i) {
        c.lradsw = (1 + i) % kNstrad == 1;
        if (int rc = step(2, 2, 2, i + 1 == p.nleap)) return rc;
    }
    if (const ExitSpec *x = p.exit) {  // iogrid(31)'s gridx and the hop's store behind the window
        if (int rc = spectral_gridx_run_model_exit(d->sp, x->varm, x->fc4, x->fc2, kNIoWind, x->ex, st)) return rc;
        if (x->store) {
            hipLaunchKernelGGL(k_flag_store, dim3(1), dim3(64), 0, st, x->store, x->ex.xa);
            SML_HIP(hipGetLastError());
        }
    }
    return SML_OK;
}

// what identifies p's captured launches
WindowKey window_key(const sml_dynamics *d, const WindowPlan &p) {
    WindowKey k;
    k.nleap = p.nleap;
    k.delt = p.dts[1];
    k.alph = p.alph;
    k.rob = p.rob;
    k.wil = p.wil;
    k.phys_on = d->phys_on;
    k.fused = d->fused;
    k.prepared = p.prepared;
    k.tab = {p.tab[0], p.tab[1], p.tab[2]};
    if (const ExitSpec *x = p.exit) {
        k.has_exit = true;
        k.exit = {x->varm, x->fc4, x->fc2, x->ex.mm, x->ex.in4, x->ex.inlp, x->ex.cnt, x->ex.timeout, x->store};
        if (const EntrySpec *en = x->entry) {
            k.has_entry = true;
            k.entry = {en->w.flag, en->w.late, en->w.sig, en->w.timeout, en->w.vptr, en->go};
        }
    }
    return k;
}

// the graph of p's launches: replayed, or captured into a way of its class
int window_graph(sml_dynamics *d, const WindowPlan &p, hipGraphExec_t *out) {
    auto &cache = d->wreplay[(p.lradsw ? 1 : 0) + (p.prepared ? 2 : 0)];
    bool hit = false;
    const int w = cache.acquire(window_key(d, p), 0, &hit);
    if (!hit) {
        if (int rc = capture_graph(
                d, "sml_dyn_window", [&](hipStream_t st) { return enqueue_window(d, st, p); }, &cache.value(w))) {
            cache.drop(w);
            return rc;
        }
    }
    *out = cache.value(w);
    return SML_OK;
}

int window_impl(sml_dynamics *d, int nleap, double delt, double alph, double rob, double wil, hipStream_t st,
                bool prepared, const ExitSpec *exit = nullptr) {
    WindowPlan p{nleap, {0.5 * delt, delt, 2.0 * delt}, alph, rob, wil, {}, d->lradsw, prepared, exit};
    unsigned taken = 0;  // the slots this window holds: a later miss must not evict them
    for (int i = 0; i < 3; ++i) {
        int slot = 0;
        if (int rc = impint_slot(d, p.dts[i], alph, taken, &slot)) return rc;
        p.tab[i] = d->d_tab;
        taken |= d->slots.pin(slot);
    }
    if (d->nograph) {  // the same launches, issued one by one on the stream (A/B: SML_DYN_NOGRAPH=1)
        if (int rc = enqueue_window(d, st, p)) return rc;
    } else {
        hipGraphExec_t exec = nullptr;
        if (int rc = window_graph(d, p, &exec)) return rc;
        SML_HIP(hipGraphLaunch(exec, st));
    }
    d->d_tab = p.tab[2];
    d->istep = 1 + nleap;
    if (nleap > 0) d->lradsw = (nleap % kNstrad == 1);
    return SML_OK;
}
}  // namespace

extern "C" int sml_dyn_window(sml_dynamics *d, int nleap, double delt, double alph, double rob, double wil,
                              void *stream) {
    SML_REQUIRE(d && nleap >= 0 && delt > 0.0, "bad argument");
    return window_impl(d, nleap, delt, alph, rob, wil, (hipStream_t)stream, false);
}

extern "C" int sml_dyn_set_clock(sml_dynamics *d, int istep, int lradsw) {
    SML_REQUIRE(d, "null context");
    d->istep = istep;
    d->lradsw = lradsw != 0;
    return SML_OK;
}

extern "C" int sml_dyn_get_clock(const sml_dynamics *d, int *istep, int *lradsw) {
    SML_REQUIRE(d, "null context");
    if (istep) *istep = d->istep;
    if (lradsw) *lradsw = d->lradsw ? 1 : 0;
    return SML_OK;
}

// run_model's SST hand-over (mpires.f90:1576-1584: internal_state_vector%sst_hybrid)
// as agcm_init's ini_sea applies it to the window's sst_am (cpl_sea.f90:38-46):
// d_sst_grid(96, 48) device; NULL restores the coupler's sst_am.  On `stream`, so a
// loop orders it before its next window.
extern "C" int sml_dyn_set_hybrid_sst(sml_dynamics *d, const double *d_sst_grid, double sst_bias, void *stream) {
    SML_REQUIRE(d, "null context");
    SML_REQUIRE(d->phys_on, "sml_dyn_set_physics must provide the boundary fields first");
    d->hyb_sst = d_sst_grid;
    d->hyb_bias = sst_bias;
    ++d->ford_gen;
    hipLaunchKernelGGL(k_hybrid_sst, dim3((kNGP + 255) / 256), dim3(256), 0, (hipStream_t)stream, d->d_sst_cpl,
                       d_sst_grid, d->d_sice, d->d_tice, sst_bias, d->d_pbc + (size_t)kBcSst * kNGP);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_dyn_set_physics(sml_dynamics *d, const double *bc) {
    SML_REQUIRE(d, "null context");
    if (!bc) {
        d->phys_on = false;
        return SML_OK;
    }
    SML_HIP(hipDeviceSynchronize());  // steps in flight may still read the old fields
    SML_HIP(hipMemcpy(d->d_pbc, bc, (size_t)kNBc * kNGP * 8, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_sst_cpl, bc + (size_t)kBcSst * kNGP, kNGP * 8, hipMemcpyHostToDevice));
    d->phys_on = true;
    ++d->ford_gen;
    if (d->hyb_sst) {  // a hybrid SST is in force: ini_sea applies it to every new sst_am
        if (int rc = sml_dyn_set_hybrid_sst(d, d->hyb_sst, d->hyb_bias, nullptr)) return rc;
        SML_HIP(hipDeviceSynchronize());
    }
    return SML_OK;
}

// sea-ice fraction and temperature of the coupler (sice_am, tice_am; cpl_sea.f90:
// 190-194), host [ngp] each; NULL = no ice (zero fraction)
extern "C" int sml_dyn_set_sea_ice(sml_dynamics *d, const double *sice, const double *tice) {
    SML_REQUIRE(d && (sice == nullptr) == (tice == nullptr), "sice and tice go together");
    SML_HIP(hipDeviceSynchronize());
    if (sice) {
        SML_HIP(hipMemcpy(d->d_sice, sice, kNGP * 8, hipMemcpyHostToDevice));
        SML_HIP(hipMemcpy(d->d_tice, tice, kNGP * 8, hipMemcpyHostToDevice));
    } else {
        SML_HIP(hipMemset(d->d_sice, 0, kNGP * 8));
        SML_HIP(hipMemset(d->d_tice, 0, kNGP * 8));
    }
    ++d->ford_gen;
    if (d->hyb_sst) return sml_dyn_set_hybrid_sst(d, d->hyb_sst, d->hyb_bias, nullptr);
    return SML_OK;
}

extern "C" int sml_dyn_get_sea_ice(sml_dynamics *d, double *sice, double *tice) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    if (sice) SML_HIP(hipMemcpy(sice, d->d_sice, kNGP * 8, hipMemcpyDeviceToHost));
    if (tice) SML_HIP(hipMemcpy(tice, d->d_tice, kNGP * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

// the boundary fields as phypar reads them, host [kNBc][ngp] (sml_dyn_set_physics order)
extern "C" int sml_dyn_get_physics(sml_dynamics *d, double *bc) {
    SML_REQUIRE(d && bc, "null argument");
    SML_REQUIRE(d->phys_on, "no boundary fields (sml_dyn_set_physics)");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(bc, d->d_pbc, (size_t)kNBc * kNGP * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

// inbcon's time-independent surface fields fordate reads (ini_inbcon.f90:38-70,
// 140-156): host [3][ngp] = fmask_l (mod_cli_land), fmask_s (mod_cli_sea), alb0
// (mod_surfcon); NULL switches sml_dyn_fordate off
extern "C" int sml_dyn_set_surface(sml_dynamics *d, const double *surf) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    d->surf_on = surf != nullptr;
    if (surf) SML_HIP(hipMemcpy(d->d_surf, surf, (size_t)3 * kNGP * 8, hipMemcpyHostToDevice));
    ++d->ford_gen;
    return SML_OK;
}

// the coupler's monthly climatologies (inbcon, ini_inbcon.f90:71-230): host
// [5][12][ngp] = stl12, snowd12, soilw12 (mod_cli_land), sst12, sice12 (mod_cli_sea),
// month 1 first; NULL: sml_dyn_fordate keeps the coupler fields the host set
// (sml_dyn_set_physics' stl_am / sst_am / soilw_am / snowc, sml_dyn_set_sea_ice)
extern "C" int sml_dyn_set_climatology(sml_dynamics *d, const double *clim) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    if (clim) {
        if (!d->d_clim)
            if (int rc = d->mem.device(&d->d_clim, (size_t)5 * 12 * kNGP, false)) return rc;  // filled right below
        SML_HIP(hipMemcpy(d->d_clim, clim, (size_t)5 * 12 * kNGP * 8, hipMemcpyHostToDevice));
    }
    d->clim_on = clim != nullptr;
    ++d->ford_gen;
    return SML_OK;
}

// agcm_init's forcing for a window at (iyear, imonth, iday) on `stream`: coupler,
// hybrid SST, fordate (see k_fordate).  A no-op when neither the date nor any input
// changed since the last call (the window's forcing stays as computed); force != 0
// recomputes anyway.  Ordered on `stream`: the next window on that stream reads it.
extern "C" int sml_dyn_fordate_ex(sml_dynamics *d, int iyear, int imonth, int iday, int force, void *stream) {
    // the days of newdate's 365-day table (ini_fordate / mod_date), plus February 29,
    // which the reference calendar emits once its SAVEd February latch is set
    // (mod_calendar.f90:40, 61-63); a later day would extrapolate tmonth past the month
    static const int kMonthDays[12] = {31, 29, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    SML_REQUIRE(d && imonth >= 1 && imonth <= 12 && iday >= 1 && iday <= kMonthDays[imonth - 1],
                "bad date %d-%d-%d", iyear, imonth, iday);
    SML_REQUIRE(d->phys_on, "sml_dyn_set_physics must provide the boundary fields first");
    SML_REQUIRE(d->surf_on, "sml_dyn_set_surface must provide fmask_l, fmask_s and alb0 first");
    (void)iyear;  // only the co2 trend reads the year (lco2 = .false.)
    if (!force && d->ford_done == d->ford_gen && d->ford_date[0] == imonth && d->ford_date[1] == iday)
        return SML_OK;
    hipStream_t st = (hipStream_t)stream;
    ForDate fd;
    phys_fordate_weights(imonth, iday, &fd);
    FordateArgs a;
    phys_sol_oz_lat(d->ptab, fd.tyear, &a.sol[0][0]);
    for (int k = 0; k < 5; ++k) {
        a.m5[k] = fd.m5[k];
        a.w5[k] = fd.w5[k];
    }
    a.mi[0] = fd.mi[0];
    a.mi[1] = fd.mi[1];
    a.wmon = fd.wmon;
    a.clim = d->clim_on ? 1 : 0;
    a.hyb = d->hyb_sst ? 1 : 0;
    a.bias = d->hyb_bias;
    double *grid = d->d_ford, *varm = d->d_ford + 2 * kGF;
    hipLaunchKernelGGL(k_fordate, dim3((kNGP + 255) / 256), dim3(256), 0, st, a, d->d_surf, d->d_clim, d->hyb_sst,
                       d->d_pbc, d->d_sst_cpl, d->d_sice, d->d_tice, grid);
    SML_HIP(hipGetLastError());
    // spec (specx + specy) of corh -> tcorh, qcorh (contiguous)
    if (int rc = spectral_specx(d->sp, grid, varm, 2, 0, st)) return rc;
    if (int rc = spectral_specy(d->sp, varm, d->d_tcorh, 2, st)) return rc;
    d->ford_done = d->ford_gen;
    d->ford_date[0] = imonth;
    d->ford_date[1] = iday;
    ++d->ford_count;
    return SML_OK;
}

extern "C" int sml_dyn_fordate(sml_dynamics *d, int iyear, int imonth, int iday, void *stream) {
    return sml_dyn_fordate_ex(d, iyear, imonth, iday, 0, stream);
}

extern "C" int sml_dyn_fordate_count(const sml_dynamics *d, int *count) {
    SML_REQUIRE(d && count, "null argument");
    *count = d->ford_count;
    return SML_OK;
}

extern "C" int sml_dyn_set_rad_state(sml_dynamics *d, const double *rad) {
    SML_REQUIRE(d, "null context");
    SML_HIP(hipDeviceSynchronize());
    if (rad)
        SML_HIP(hipMemcpy(d->d_rad, rad, kRadSize * 8, hipMemcpyHostToDevice));
    else
        SML_HIP(hipMemset(d->d_rad, 0, kRadSize * 8));
    return SML_OK;
}

extern "C" int sml_dyn_get_rad_state(sml_dynamics *d, double *rad) {
    SML_REQUIRE(d && rad, "null argument");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(rad, d->d_rad, kRadSize * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_phypar(sml_dynamics *d, const double *d_ug1, const double *d_vg1, const double *d_tg1,
                              const double *d_qg1, const double *d_phig1, const double *d_pslg1, int lradsw,
                              double *d_tend, void *stream) {
    SML_REQUIRE(d && d_ug1 && d_vg1 && d_tg1 && d_qg1 && d_phig1 && d_pslg1 && d_tend, "null argument");
    SML_REQUIRE(d->phys_on, "sml_dyn_set_physics must provide the boundary fields first");
    hipLaunchKernelGGL(k_phys, dim3(kNGP / 64), dim3(64), 0, (hipStream_t)stream, d_ug1, d_vg1, d_tg1, d_qg1,
                       d_phig1, d_pslg1, d->d_pbc, d->d_rad, d->d_ptab, lradsw ? 1 : 0, d_tend);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_dyn_phypar_host(sml_dynamics *d, const double *ug1, const double *vg1, const double *tg1,
                                   const double *qg1, const double *phig1, const double *pslg1, int lradsw,
                                   double *tend) {
    SML_REQUIRE(d && ug1 && vg1 && tg1 && qg1 && phig1 && pslg1 && tend, "null argument");
    const size_t f3 = (size_t)kKX * kNGP;
    double *b = d->d_pio;
    const double *src[5] = {ug1, vg1, tg1, qg1, phig1};
    for (int i = 0; i < 5; ++i) SML_HIP(hipMemcpy(b + i * f3, src[i], f3 * 8, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(b + 5 * f3, pslg1, kNGP * 8, hipMemcpyHostToDevice));
    double *out = b + 5 * f3 + kNGP;
    if (int rc = sml_dyn_phypar(d, b, b + f3, b + 2 * f3, b + 3 * f3, b + 4 * f3, b + 5 * f3, lradsw, out, nullptr))
        return rc;
    SML_HIP(hipMemcpy(tend, out, 4 * f3 * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_sol_oz(const sml_dynamics *d, double tyear, double *fields5) {
    SML_REQUIRE(d && fields5, "null argument");
    phys_sol_oz(d->ptab, tyear, fields5);
    return SML_OK;
}

extern "C" int sml_phys_sflset(const double *phi0, double *forog) {
    SML_REQUIRE(phi0 && forog, "null argument");
    phys_sflset(phi0, forog);
    return SML_OK;
}

namespace {
// iogrid(30) with the entry specx's hop wait / signal w
int from_grid(sml_dynamics *d, const double *d_grid4d, const double *d_logp, double *d_minmax, hipStream_t st,
              HopWait w) {
    const DynTables *T = d->d_tab;
    // entry (:503-518): real(4) copies, q clip, then vdspec kcos = 2 (x cosgr) on the
    // winds and none on the rest: one specx launch reading variables3d / logp
    if (int rc = spectral_specx_io(d->sp, d_grid4d, d_logp, d->d_varm, kNIoWind, st, w)) return rc;
    if (int rc = spectral_specy(d->sp, d->d_varm, d->d_sfwd, kNIo, st)) return rc;
    hipLaunchKernelGGL(k_io_combine, dim3((kMN + 127) / 128, kKX), dim3(128), 0, st, d->d_sfwd, d->d_state, T);
    SML_HIP(hipGetLastError());
    // the safety check (:556-571) reads the new state: its k_io_prep stays on st (the
    // window overwrites the state), the rest of it beside the window
    hipLaunchKernelGGL(k_io_prep, dim3((kMN + 127) / 128, kKX), dim3(128), 0, st, d->d_state, d->chk.inputs(), T);
    SML_HIP(hipGetLastError());
    return d->chk.launch(st, d_minmax);
}
}  // namespace

extern "C" int sml_dyn_from_grid(sml_dynamics *d, const double *d_grid4d, const double *d_logp, double *d_minmax,
                                 void *stream) {
    SML_REQUIRE(d && d_grid4d && d_logp, "null argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = d->chk.wait_pending(st)) return rc;
    HopWait w = std::exchange(d->hooks.entry_wait, HopWait{});  // one launch
    w.sig = std::exchange(d->hooks.entry_sig, nullptr);
    return from_grid(d, d_grid4d, d_logp, d_minmax, st, w);
}

extern "C" int sml_dyn_to_grid(sml_dynamics *d, double *d_grid4d, double *d_logp, void *stream) {
    SML_REQUIRE(d && d_grid4d && d_logp, "null argument");
    hipStream_t st = (hipStream_t)stream;
    // exit (:590-595): the state re-gridded (k_io_prep, gridy, gridx) with the gridx
    // writing variables3d / logp directly
    hipLaunchKernelGGL(k_io_prep, dim3((kMN + 127) / 128, kKX), dim3(128), 0, st, d->d_state, d->d_specin, d->d_tab);
    SML_HIP(hipGetLastError());
    if (int rc = spectral_gridy(d->sp, d->d_specin, d->d_varm, kNIo, st)) return rc;
    return spectral_gridx_io(d->sp, d->d_varm, d_grid4d, d_logp, kNIoWind, st);
}

extern "C" int sml_dyn_is_safe(const double *minmax) {
    if (!minmax) return 0;
    return io_state_safe(minmax) ? 1 : 0;  // u, v, t, q thresholds (ppo_iogrid.f90:563-577)
}

namespace {
// run_model's exit arguments: the q floor, the check's min/max (run_model's checks all
// write d_minmax) and the window's input grids.  counted: the exit kernel itself waits for
// the check's counter, so no event wait (a barrier packet with a cross-queue dependency)
// on the window's stream; the count to reach is `target`, or xa[0] (and target 0) for an
// exit replayed inside a graph (its arguments are fixed).  The check is complete once such
// an exit has run, so the next user of d_chk needs no wait either
IoExit run_model_exit(const sml_dynamics *d, const double *d_grid4d, const double *d_logp, bool counted,
                      unsigned target, const uint64_t *xa) {
    IoExit ex{0.000001, d->d_minmax, d_grid4d, d_logp};
    if (counted) d->chk.exit_waits_for_counter(&ex, target, xa);
    return ex;
}
}  // namespace

// run_model (src/mpires.f90:1516-1628) on the device: agcm_main's window entry
// iogrid(30) with its safety check, the window (integrated whatever the check says:
// the outcome is selected at the exit), iogrid(31), then run_model's q floor; when
// the entry state was unsafe agcm_main skipped the integration (at_gcm.f90:37) and
// the forecast is the input grid (q floored).  The check runs beside the window on
// the context's check stream; the exit waits for it.
extern "C" int sml_dyn_run_model(sml_dynamics *d, const double *d_grid4d, const double *d_logp, int nleap,
                                 double delt, double alph, double rob, double wil, double *d_fc4d, double *d_fc2d,
                                 void *stream) {
    SML_REQUIRE(d && d_grid4d && d_logp && d_fc4d && d_fc2d, "null argument");
    SML_REQUIRE(d_fc4d != d_grid4d && d_fc2d != d_logp, "the forecast must not overwrite the window's input");
    SML_REQUIRE(nleap >= 0 && delt > 0.0, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    if (int rc = d->chk.wait_pending(st)) return rc;
    const sml_dynamics::RunModelHooks h = std::exchange(d->hooks, {});  // one launch
    HopWait w = h.entry_wait;
    w.sig = h.entry_sig;
    // The fused form: iogrid(30)'s specx, then ONE per-m launch for specy, the combine
    // into level 1, the check's inputs, the m-major state and step(1, 1)'s gridy
    // (k_io_entry); the window then starts at the first row kernel.
    // The exit inside the window graph: needs the check's counter hand-off (no event
    // wait between the window and the exit; the check counts unless captured) and the
    // graph path.  Its per-launch values go through d_xa.
    // And the entry inside it too (r06): specx + k_io_entry as the graph's first nodes,
    // the safety check forked by the first row kernel's go store instead of an event
    // after k_io_entry -- one launch boundary fewer on the chain, and the graph's launch
    // hidden behind the entry's wait.  Not under serialised dispatch (the check, enqueued
    // after the graph, would run after the exit that waits for it)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    SML_HIP(hipStreamIsCapturing(st, &cap));
    const bool exit_in_graph = d->fused && !d->nograph && cap == hipStreamCaptureStatusNone;
    const bool entry_in_graph = exit_in_graph && d->phys_on && !d->serialized;
    if (exit_in_graph && !d->d_xa)  // (k_set_xa / k_io_entry write its words before each launch)
        if (int rc = d->mem.device(&d->d_xa, 4, false)) return rc;
    const unsigned target = d->chk.next_target();  // the check counter once this window's check is done
    auto exit_spec = [&](const EntrySpec *en) {  // the exit (and entry) in the window graph
        return ExitSpec{d->d_varm,    d_fc4d, d_fc2d, run_model_exit(d, d_grid4d, d_logp, true, 0, d->d_xa),
                        h.exit_store, en};
    };

    auto no_handoff = [] {  // an exit in the graph has nothing else to wait with
        return fail(SML_ERR_STATE, "sml_dyn_run_model: the safety check did not take the counter hand-off");
    };

    if (entry_in_graph) {
        uint64_t go = 0;
        if (int rc = d->chk.next_go(&go)) return rc;
        hipLaunchKernelGGL(k_set_xa, dim3(1), dim3(64), 0, st, d->d_xa, (uint64_t)target, h.exit_store_value,
                           w.value, go);
        SML_HIP(hipGetLastError());
        EntrySpec en{d_grid4d, d_logp, w, d->chk.go_word(), d->d_xa + 3};
        if (w.flag) en.w.vptr = d->d_xa + 2;
        const ExitSpec es = exit_spec(&en);
        if (int rc = window_impl(d, nleap, delt, alph, rob, wil, st, true, &es)) return rc;
        // enqueued after the graph, so whatever queue it shares, its producer is ahead
        if (int rc = d->chk.launch(st, nullptr, go)) return rc;
        return d->chk.take_handoff() ? (int)SML_OK : no_handoff();
    }

    if (d->fused) {  // the entry with the current impint slot's tables, as the previous window left them
        if (int rc = launch_entry(d, d->d_tab, d_grid4d, d_logp, w, st, exit_in_graph ? d->d_xa : nullptr, target,
                                  h.exit_store_value))
            return rc;
        if (int rc = d->chk.launch(st, nullptr)) return rc;
    } else if (int rc = from_grid(d, d_grid4d, d_logp, nullptr, st, w)) {
        return rc;
    }
    if (exit_in_graph) {
        if (!d->chk.take_handoff()) return no_handoff();
        const ExitSpec es = exit_spec(nullptr);
        return window_impl(d, nleap, delt, alph, rob, wil, st, true, &es);
    }

    if (int rc = window_impl(d, nleap, delt, alph, rob, wil, st, d->fused)) return rc;
    // the exit waits for the counter itself, else its stream for the check's min/max
    const bool counted = d->chk.take_handoff();
    if (int rc = d->chk.wait_pending(st)) return rc;
    if (!d->fused) {  // the fused window's last kernel did iogrid(31)'s prep + gridy already
        hipLaunchKernelGGL(k_io_prep, dim3((kMN + 127) / 128, kKX), dim3(128), 0, st, d->d_state, d->d_specin,
                           d->d_tab);
        SML_HIP(hipGetLastError());
        if (int rc = spectral_gridy(d->sp, d->d_specin, d->d_varm, kNIo, st)) return rc;
    }
    if (int rc = spectral_gridx_run_model_exit(d->sp, d->d_varm, d_fc4d, d_fc2d, kNIoWind,
                                               run_model_exit(d, d_grid4d, d_logp, counted, target, nullptr), st))
        return rc;
    if (h.exit_store) {
        hipLaunchKernelGGL(k_flag_store_value, dim3(1), dim3(64), 0, st, h.exit_store, h.exit_store_value);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

extern "C" int sml_dyn_set_check_cus(sml_dynamics *d, int first_cu, int num_cus) {
    SML_REQUIRE(d && first_cu >= 0 && num_cus >= 0, "bad argument");
    return d->chk.reset_stream(first_cu, num_cus);
}

// run_speedy of the last sml_dyn_from_grid / sml_dyn_run_model (is_safe_to_run_speedy,
// broadcast as run_speedy, src/mpires.f90:721, 1623): waits only for that check
extern "C" int sml_dyn_last_safe(sml_dynamics *d, int *safe, double *minmax) {
    SML_REQUIRE(d && safe, "null argument");
    double mm[8];
    if (int rc = d->chk.last(mm, safe)) return rc;
    if (minmax) std::memcpy(minmax, mm, sizeof mm);
    return SML_OK;
}

// the next run_model's entry specx waits in-kernel until *flag >= value; on a timeout
// (ticks) it marks *late and transforms NaN (the window's check then fails)
int sml::dyn_run_model_wait(sml_dynamics *d, const uint64_t *flag, uint64_t value, unsigned *late,
                            long long timeout) {
    SML_REQUIRE(d && flag && late, "null argument");
    d->hooks.entry_wait = HopWait{flag, value, late};
    d->hooks.entry_wait.timeout = timeout;
    return SML_OK;
}

int sml::dyn_set_check_timeout(sml_dynamics *d, long long timeout) {
    SML_REQUIRE(d && timeout >= 0, "bad argument");
    d->chk.set_timeout(timeout);
    return SML_OK;
}

extern "C" int sml_dyn_set_check_timeout(sml_dynamics *d, int64_t microseconds) {
    SML_REQUIRE(d && microseconds >= 0, "bad argument");
    if (int rc = d->chk.sync()) return rc;
    return sml::dyn_set_check_timeout(d, (long long)std::min<int64_t>(microseconds, INT64_MAX / 100) * 100);
}

extern "C" int sml_dyn_set_fused(sml_dynamics *d, int fused) {
    SML_REQUIRE(d, "null context");
    d->fused = fused != 0;
    return SML_OK;
}

extern "C" int sml_dyn_check_stream(const sml_dynamics *d, void **stream) {
    SML_REQUIRE(d && stream, "null argument");
    *stream = d->chk.stream();
    return SML_OK;
}

// the event behind the last safety check issued on the check stream (null if none)
int sml::dyn_check_event(sml_dynamics *d, void **ev) {
    SML_REQUIRE(d && ev, "null argument");
    *ev = (void *)d->chk.event();
    return SML_OK;
}

// the next run_model's entry kernel (iogrid(30)'s specx) adds *adds to *counter as it
// starts: its input grid is complete and released by then
int sml::dyn_run_model_entry_signal(sml_dynamics *d, uint64_t *counter, int *adds) {
    SML_REQUIRE(d && counter && adds, "null argument");
    d->hooks.entry_sig = counter;
    *adds = spectral_specx_io_blocks();
    return SML_OK;
}

// the next run_model's exit is followed (on its stream, inside the window graph when the
// exit is captured there) by a one-lane store of value to *flag; flag = NULL withdraws it
int sml::dyn_run_model_exit_store(sml_dynamics *d, uint64_t *flag, uint64_t value) {
    SML_REQUIRE(d, "null argument");
    d->hooks.exit_store = flag;
    d->hooks.exit_store_value = value;
    return SML_OK;
}

// a run_model exit that gave up waiting for its safety check (it then took the window
// as unsafe): reported once, then reset.  The word is host memory: no copy, no sync --
// callers read it once the exit has run (sml_hybrid_run_speedy, after the check's event)
int sml::dyn_check_late(sml_dynamics *d) {
    if (d && d->chk.late_reported())
        return fail(SML_ERR_STATE, "run_model's exit did not receive its safety check in time (window taken as unsafe)");
    return SML_OK;
}

extern "C" int sml_dyn_from_grid_host(sml_dynamics *d, const double *grid4d, const double *logp, double *minmax,
                                      int *safe) {
    SML_REQUIRE(d && grid4d && logp, "null argument");
    const size_t n4 = (size_t)4 * kKX * kGF;
    SML_HIP(hipMemcpy(d->d_io, grid4d, n4 * 8, hipMemcpyHostToDevice));
    SML_HIP(hipMemcpy(d->d_io + n4, logp, kGF * 8, hipMemcpyHostToDevice));
    if (int rc = sml_dyn_from_grid(d, d->d_io, d->d_io + n4, d->d_minmax, nullptr)) return rc;
    double mm[8];
    SML_HIP(hipMemcpy(mm, d->d_minmax, sizeof mm, hipMemcpyDeviceToHost));
    if (minmax) std::memcpy(minmax, mm, sizeof mm);
    if (safe) *safe = sml_dyn_is_safe(mm);
    return SML_OK;
}

extern "C" int sml_dyn_to_grid_host(sml_dynamics *d, double *grid4d, double *logp) {
    SML_REQUIRE(d && grid4d && logp, "null argument");
    const size_t n4 = (size_t)4 * kKX * kGF;
    if (int rc = sml_dyn_to_grid(d, d->d_io, d->d_io + n4, nullptr)) return rc;
    SML_HIP(hipMemcpy(grid4d, d->d_io, n4 * 8, hipMemcpyDeviceToHost));
    SML_HIP(hipMemcpy(logp, d->d_io + n4, kGF * 8, hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_dyn_step_host(sml_dynamics *d, int j1, int j2, double dt, double alph, double rob, double wil,
                                 const double *phys) {
    SML_REQUIRE(d, "null context");
    const double *dp = nullptr;
    if (phys) {
        SML_REQUIRE(!d->phys_on, "physics runs on the GPU (sml_dyn_set_physics): phys must be NULL");
        SML_HIP(hipMemcpy(d->d_phys, phys, (size_t)4 * kKX * kGF * 8, hipMemcpyHostToDevice));
        dp = d->d_phys;
    }
    if (int rc = sml_dyn_step(d, j1, j2, dt, alph, rob, wil, dp, nullptr)) return rc;
    SML_HIP(hipDeviceSynchronize());
    return SML_OK;
}

// diagnostic: the phase stamps of the last fused launches ([4][96][8] wall_clock64
// ticks, 100 MHz); not part of the ABI header
#ifdef SML_PSTAMPS
// the physics sub-phase stamps of the last row kernel (profiling build only)
extern "C" int sml_dbg_pst(long long *out) {
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pst), sizeof(long long) * kIL * 32, 0, hipMemcpyDeviceToHost));
    return SML_OK;
}
#endif

extern "C" int sml_dbg_dyn_stamps(sml_dynamics *d, long long *out) {
    SML_REQUIRE(d && out && d->d_dbg, "stamps not enabled (SML_DYN_STAMPS=1 at creation)");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(out, d->d_dbg, kStampKernels * kStampBlocks * kStamps * sizeof(long long), hipMemcpyDeviceToHost));
    return SML_OK;
}
