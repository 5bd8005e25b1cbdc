// sml_reservoir.hip -- batched reservoir forward (predict) for every region of a
// rank, plus the device-side exchange/tiling that replaces sendrecievegrid's
// gather / scatter loops.
//
// Reference: predict (src/mod_reservoir.f90:1416-1487), per region on the host:
//     y = A x                (MKL_SPARSE_D_MV, COO, :1442)
//     temp = W_in feedback   (dense n x ninp matmul, :1443)
//     x = (1-a) x + a tanh(y + temp)
//     x~ = x with every 2nd node squared (:1448-1449)
//     outvec = W_out [local_model; x~]  (:1454), then unstandardize (:1469)
//
// MI355X design (DESIGN.md "Reservoir"):
//   * all regions of the rank run in two launches (update + readout), no host loop;
//   * A is CSR (rows in the file's entry order, so every row sums in the same order
//     as the reference's COO traversal) with 16-bit column indices;
//   * W_in is CSR too: the trained matrix has one entry per row (train_reservoir,
//     :260-278), so the 26.5 MB dense matmul per region becomes n gathers;
//   * W_out is stored transposed ([nout][ld], rows padded to 16 B) in the file
//     precision (fp32 by default: NF90_REAL, mod_io.f90:1282, exact widening);
//     the readout streams it from HBM once per step with fp64 accumulation and
//     wave-level reductions -- this kernel carries ~90 % of the step's bytes;
//   * unstandardize is fused into the readout's epilogue.
//
// This file is the unit's host side -- the context, the launchers and the C ABI -- and
// the one translation unit that compiles its kernels, which live in headers by stage
// (sml_res_*.hpp, included below; the SML_UPD_NT / SML_READ_NT defaults sit beside the
// loads they switch).  The context's memory has one owner (DevMem); which kernel form
// each stage takes, and with what LDS, is worked out on the host by step_shape
// (sml_reservoir_layout.hpp) whenever one of its inputs changes.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "sml_counter_rng.hpp"
#include "sml_devmem.hpp"
#include "sml_internal.hpp"
#include "sml_reservoir_layout.hpp"
#include "sml_slab_layout.hpp"
#include "sml_timeline.hpp"

SML_TL_DEFINE(reservoir)

// every kernel of the unit, by stage: one translation unit, one set of compile flags
// clang-format off
#include "sml_res_rows.hpp"
#include "sml_res_update.hpp"
#include "sml_res_drive.hpp"
#include "sml_res_radius.hpp"
#include "sml_res_tiling.hpp"
#include "sml_res_series.hpp"
#include "sml_res_noise.hpp"
#include "sml_res_readout.hpp"
#include "sml_res_members.hpp"
// clang-format on

using namespace sml;

namespace {

// the three events of each timed step (start, update done, readout done)
struct StepEvents {
    std::vector<hipEvent_t> ev;
    int cap = 0, used = 0;
    bool on = false;
    StepEvents() = default;
    StepEvents(const StepEvents &) = delete;
    StepEvents &operator=(const StepEvents &) = delete;
    ~StepEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

// (PoolPlan: rd, ld, the ELL caps, the pools' sizes tot_*, maxn / maxninp -- plan_pools)
struct sml_reservoirs : PoolPlan {
    DevMem mem;  // first: every device buffer below is its; all freed together with the context
    int numregions = 0, nlocal = 0, ncs = 0, nout = 0, nout_pad = 0, wdtype = SML_F32;
    // row stride of the outvec arrays (sml_res_set_outvec_ld): nout, or wider when the
    // hybrid loop carries the slab ocean's sst beside each outvec in its exchange rows
    int ov_ld = 0;
    double leakage = 1.0;
    std::vector<int> region_ids, n, k, ninp;
    std::vector<unsigned char> sst, loaded;
    std::vector<RegionGeom> geom;
    void *d_wlm = nullptr;
    std::vector<int64_t> w_nz_cap;  // reserved W_in CSR nnz per region (n at create: one entry per row as
                                    // trained; grow_win_pool re-lays the pool for a denser W_in)
    int device = 0;
    // device buffers
    RegionDev *d_rd = nullptr;
    int32_t *d_a_rp = nullptr, *d_w_rp = nullptr;
    uint16_t *d_a_col = nullptr, *d_w_col = nullptr;
    void *d_a_val = nullptr, *d_w_val = nullptr, *d_wout = nullptr;
    // ELL copies (row-major per region), used when rows are short enough
    uint16_t *d_a_ell_col = nullptr, *d_w_ell_col = nullptr;
    void *d_a_ell_val = nullptr, *d_w_ell_val = nullptr;
    uint64_t *d_a_om = nullptr;   // A's overflow bits, one word per 64 rows
    uint32_t *d_a_ob = nullptr;   // overflow entries before each word (region-local)
    uint16_t *d_a_oc = nullptr;   // overflow entries: column
    void *d_a_ov = nullptr;       //                   value
    void *d_zero = nullptr;       // 256 zero bytes: the target of the balanced update's unused loads
    double *d_x[2] = {nullptr, nullptr};
    double *d_meanstd = nullptr;
    // [members][nlocal][nout_pad] W_out(:, ncs+1:) x~ of the step in flight (member e's sums at
    // e * nlocal * nout_pad: sml_res_set_members lays it out with the states)
    double *d_part = nullptr;
    // cap on the waves of the v_ml readout (the half that runs beside SPEEDY's window;
    // 0: one wave per item).  Sharing CUs with SPEEDY, uncapped it takes ~6 TB/s and
    // SPEEDY's latency-bound kernels stall behind it; paced at 2048 waves (~4.7 TB/s)
    // the overlapped step is 1.75 ms instead of 1.98 (profiles/r01p).  On CUs of its
    // own the pacing does not matter: sml_res_set_read_waves(0).
    int read_waves = 2048;
    // the inputs of the step's shape beside the sizes (reshape below):
    // sml_res_step_begin's form (sml_res_set_begin_mode): 0 the update grid then the
    // v_ml readout grid, 1 one fused launch (k_res_begin, 2 blocks per CU), 2 fused with
    // the readout's loads unrolled twice (1 block per CU)
    int begin_mode = 0;
    // the fallback forms forced (sml_res_set_reference_paths); each is also taken where
    // the layout does not fit the default, which is the shape's decision:
    bool no_ell = false;            // CSR copies only
    bool per_region = false;        // k_res_update, a block per (region, part), not the balanced update
    bool finish_ungrouped = false;  // the v_p finish one thread per output (vp_sum), not in column groups
    bool stepwise_drive = false;    // the training drive as m launches of the update, each after a column
                                    // writer (k_drive_record), not k_res_drive
    // sml_res_spectral_radius (k_res_radius): x and y in d_rad_xy ([2 * row0[r]]: x then y
    // of region r; allocated at the first call that needs it) instead of LDS -- forced
    // (sml_res_set_reference_paths), or taken by a region whose 2 n doubles exceed max_lds.
    // d_rad_part [nlocal][3][16]: the waves' partial min / max; d_rad_out [nlocal] results
    bool radius_global = false;
    double *d_rad_xy = nullptr, *d_rad_part = nullptr;
    RadiusOut *d_rad_out = nullptr;
    StepShape shape;  // which form each stage takes, its LDS: what the launchers read and the ABI reports
    // ensemble members (sml_res_set_members): member e's state at e * tot_xaug doubles of
    // d_x[0] / d_x[1], so member 0 is the single-member context's state; mshape: the members
    // kernels' tiles (member_shape), kept with the step's shape
    int members = 1;
    MemberShape mshape;
    MemberFinish mfin;      // the members' grid finish: its tile (member_finish)
    int fin_tile_want = 0;  // 0: the build's tile; else a measurement's choice (sml_res_dbg_set_finish_tile)
    int32_t *d_tgt_idx = nullptr;  // [nlocal][nout] the targets' positions in each region's feedback
    // the next grid finish waits in-kernel for *fin_wflag >= fin_wval (sml::res_finish_wait)
    const uint64_t *fin_wflag = nullptr;
    uint64_t fin_wval = 0;
    unsigned *fin_wlate = nullptr;
    long long fin_wtimeout = 400000000ll;  // wall_clock64 ticks
    // the balanced update: row0 [nlocal+1] = the regions' rows concatenated; upd_cus: the
    // CUs the launches get (sml_res_set_update_cus; 0 = every CU of the device)
    int upd_cus = 0, ncu = 0;
    // its per-block first regions, one table per grid size G (a paced begin and an
    // uncapped step alternate two sizes): tables in one device buffer at offset
    // G (G - 1) / 2, built once per G; blk_off[G] = -1 until then
    std::vector<int32_t> blk_off;
    std::vector<std::vector<int32_t>> blk_host;  // the host tables (async copies' sources stay alive)
    int blk_cap = 0;  // largest G the buffer holds
    size_t max_lds = 0;  // the device's LDS per workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock)
    int32_t *d_row0 = nullptr, *d_blk_r0 = nullptr;
    std::vector<int32_t> row0_h;
    int8_t *d_outl = nullptr;
    int32_t *d_asm_dst = nullptr;   // [numregions*nout] -> concatenated grid index
    int32_t *d_fb_src = nullptr;    // [tot_fb]
    uint8_t *d_fb_l = nullptr;      // [tot_fb]
    uint16_t *d_fb_reg = nullptr;   // [tot_fb]
    // tisr entries of the feedback (get_tisr_by_date, mpires.f90:1644-1676): feedback
    // index, grid2d index of the overlap-tile point, local region
    int tot_tisr = 0;
    int32_t *d_tisr_fb = nullptr, *d_tisr_grid = nullptr;
    uint16_t *d_tisr_reg = nullptr;
    int32_t *d_lm_src = nullptr;    // [nlocal*ncs]
    uint8_t *d_lm_l = nullptr;
    // the series calls (sml_res_series_stats, sml_res_tile_series): their tables
    // (build_series_tables) and the statistics' workspace, allocated at the first such call
    int32_t *d_ser_src = nullptr, *d_ser_pt_off = nullptr, *d_ser_pt_grid = nullptr;
    uint8_t *d_ser_l = nullptr;
    unsigned char *d_ser_sst = nullptr;  // [nlocal] the regions' sst flags
    double *d_ser_work = nullptr;        // SeriesWork: (2 * kSerSplitMax + 1) * kSerPoints doubles
    // sml_slab_train_series' table over this (atmo) context's sst regions (build_slab_series_tables),
    // allocated at the first such call: source, slot and local row of every slab feedback entry
    int32_t *d_sls_src = nullptr;
    uint8_t *d_sls_l = nullptr;
    uint16_t *d_sls_row = nullptr;
    int sls_tot = -1;  // entries; -1: not built
    // the input noise (sml_res_set_input_noise; nothing of it exists before that call):
    // the entries' local regions (a generic context's own table; d_fb_reg elsewhere) and
    // the regions' keys of streams 4 and 5 [nlocal][2]
    bool noise_set = false;
    double noise_mag = 0.0, noise_eps = 0.0;
    uint16_t *d_nz_reg = nullptr;
    uint64_t *d_nz_key = nullptr;
    double *d_io = nullptr;         // staging for sml_res_step_host
    size_t d_io_n = 0;
    StepEvents timers;
    std::vector<double> meanstd_h;  // host copy [nlocal][72]
    // generic context (sml_res_create_generic: the slab-ocean reservoir): ninp given,
    // no exchange tables, every output unstandardized with the mean / std slot out_l[o]
    bool generic = false;
    std::vector<int8_t> out_l;

    // ---- the step state: d_x[cur] is the state; begun = sml_res_step_begin issued, its
    // finish pending.  These two functions are the only writers of cur and begun.
    // One advance of the state: launch(x_old, x_new) issues it; the buffers swap when it
    // was issued (a refused launch leaves the state where it was).  open: the step stays
    // begun until close().
    template <typename F>
    int advance(bool open, F &&launch) {
        if (int rc = launch(static_cast<const double *>(d_x[cur]), d_x[1 - cur])) return rc;
        cur = 1 - cur;
        begun = open;
        return SML_OK;
    }
    // a begun step ends: finished, or (roll_back) discarded with the old state current again
    void close(bool roll_back = false) {
        if (roll_back && begun) cur = 1 - cur;
        begun = false;
    }
    const double *x_now() const { return d_x[cur]; }
    double *x_now() { return d_x[cur]; }
    bool is_begun() const { return begun; }

private:
    int cur = 0;
    bool begun = false;
};

namespace {

// --------------------------------------------------------------- host helpers
size_t wbytes(const sml_reservoirs *c) { return c->wdtype == SML_F32 ? 4 : 8; }

// the one dispatch on the weights' storage dtype: f(float{}) or f(double{})
template <typename F>
auto with_wt(const sml_reservoirs *c, F &&f) {
    if (c->wdtype == SML_F32) return f(float{});
    return f(double{});
}

// a pool of count weights in the storage dtype (16 bytes at least)
int wpool(sml_reservoirs *c, void **p, int64_t count, bool zero) {
    unsigned char *b = nullptr;
    const int rc = c->mem.device(&b, (size_t)std::max<int64_t>(count * (int64_t)wbytes(c), 16), zero);
    *p = b;
    return rc;
}

// count elements (one at least), not filled: every word is uploaded or written before it is read
template <typename T>
int pool(sml_reservoirs *c, T **p, int64_t count, bool zero = false) {
    return c->mem.device(p, (size_t)std::max<int64_t>(count, 1), zero);
}

template <typename T>
int upload(T *dst, const std::vector<T> &src) {
    if (!src.empty()) SML_HIP(hipMemcpy(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return SML_OK;
}

int check_region(const sml_reservoirs *c, int i) {
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(i >= 0 && i < c->nlocal, "local region index %d out of range [0,%d)", i, c->nlocal);
    return SML_OK;
}

int check_loaded(const sml_reservoirs *c) {
    for (int i = 0; i < c->nlocal; ++i)
        if (!c->loaded[i]) return fail(SML_ERR_STATE, "local region %d has no weights loaded", i);
    return SML_OK;
}

// ------------------------------------------------------------------ shape
// the step's shape from the context's sizes and switches: called where one of them
// changes (create, a region's load, sml_res_set_reference_paths, sml_res_set_begin_mode)
void reshape(sml_reservoirs *c) {
    bool ell_ok = true;  // every local region's A and W_in in ELL form
    for (int i = 0; i < c->nlocal; ++i)
        if (c->rd[i].a_w <= 0 || c->rd[i].w_w <= 0) ell_ok = false;
    c->shape = step_shape({c->maxn, c->maxninp, c->nout_pad, c->ncs, c->nlocal, c->max_lds, ell_ok, c->begin_mode,
                           c->per_region, c->finish_ungrouped, c->stepwise_drive});
    c->mshape = member_shape({c->members, c->shape.lds_region, c->shape.region_lds, c->max_lds});
    c->mfin = member_finish(c->members, c->fin_tile_want);
}

// the calls that advance one state through the single-member kernels: refused while the
// context holds members, whose buffers they would move out from under the others
int check_single(const sml_reservoirs *c, const char *what) {
    if (c->members > 1)
        return fail(SML_ERR_STATE, "%s on a context of %d members: call sml_res_set_members(c, 1) first", what,
                    c->members);
    return SML_OK;
}

// the exchange / tiling tables (build_region_tables): each allocated, then uploaded
int build_tables(sml_reservoirs *c) {
    const TablesIn in{c->numregions, c->nlocal, c->ncs, c->nout, c->geom.data(), c->sst.data(), c->ninp.data(),
                      c->rd.data(), c->tot_fb, c->generic ? c->out_l.data() : nullptr};
    RegionTables t;
    if (int rc = build_region_tables(in, &t)) return rc;
    auto mk = [c](auto **d, const auto &v) {
        const int rc = pool(c, d, (int64_t)v.size());
        return rc ? rc : upload(*d, v);
    };
    if (c->generic) return mk(&c->d_outl, t.outl);
    c->tot_tisr = (int)t.tisr_fb.size();
    int rc;
    if ((rc = mk(&c->d_asm_dst, t.asm_dst)) || (rc = mk(&c->d_fb_src, t.fb_src)) || (rc = mk(&c->d_fb_l, t.fb_l)) ||
        (rc = mk(&c->d_fb_reg, t.fb_reg)) || (rc = mk(&c->d_lm_src, t.lm_src)) || (rc = mk(&c->d_lm_l, t.lm_l)) ||
        (rc = mk(&c->d_outl, t.outl)) || (rc = mk(&c->d_tisr_fb, t.tisr_fb)) ||
        (rc = mk(&c->d_tisr_grid, t.tisr_grid)) || (rc = mk(&c->d_tisr_reg, t.tisr_reg)) ||
        (rc = mk(&c->d_tgt_idx, t.tgt_idx)))
        return rc;
    return SML_OK;
}

// W_in's CSR pool holds n entries per region at create (the trained W_in has one
// entry per row, mod_reservoir.f90:260-278).  A denser W_in -- up to the dense
// win(n, ninp) of the reference's matmul (:1443) -- re-lays the pool: region i gets
// room for wnz entries, the other regions' entries move device to device, every
// region's offset is re-uploaded.  The ELL copy stays one slot per row: such a region
// is read from the CSR form.  A failure before the switch gives the new pools back and
// leaves the old ones in place.
int grow_win_pool(sml_reservoirs *c, int i, int64_t wnz) {
    const size_t wb = wbytes(c);
    std::vector<int64_t> off(c->nlocal);
    int64_t tot = 0;
    for (int j = 0; j < c->nlocal; ++j) {
        off[j] = tot;
        tot += (j == i) ? wnz : c->w_nz_cap[j];
    }
    uint16_t *col = nullptr;
    void *val = nullptr;
    pool(c, &col, tot);
    wpool(c, &val, tot, false);
    hipError_t e = hipSuccess;
    if (c->mem.status() == SML_OK) e = hipDeviceSynchronize();  // steps in flight read the old pool
    for (int j = 0; j < c->nlocal && c->mem.status() == SML_OK && e == hipSuccess; ++j) {
        if (j == i || !c->loaded[j] || c->w_nz_cap[j] == 0) continue;
        e = hipMemcpy(col + off[j], c->d_w_col + c->rd[j].w_nz, c->w_nz_cap[j] * 2, hipMemcpyDeviceToDevice);
        if (e == hipSuccess)
            e = hipMemcpy((char *)val + off[j] * wb, (char *)c->d_w_val + c->rd[j].w_nz * wb, c->w_nz_cap[j] * wb,
                          hipMemcpyDeviceToDevice);
    }
    if (c->mem.status() != SML_OK || e != hipSuccess) {
        c->mem.release(&col);
        c->mem.release(&val);
        return c->mem.status() ? c->mem.status() : fail(SML_ERR_HIP, "grow_win_pool: %s", hipGetErrorString(e));
    }
    c->mem.release(&c->d_w_col);
    c->mem.release(&c->d_w_val);
    c->d_w_col = col;
    c->d_w_val = val;
    c->w_nz_cap[i] = wnz;
    c->tot_w_nz = tot;
    for (int j = 0; j < c->nlocal; ++j) c->rd[j].w_nz = off[j];
    SML_HIP(hipMemcpy(c->d_rd, c->rd.data(), sizeof(RegionDev) * c->nlocal, hipMemcpyHostToDevice));
    return SML_OK;
}

// one upload of a region's load: src to byte offset `at` of a pool (nothing for an
// empty vector: a layout the region does not have; A's CSR entries are copied whatever
// their count, k = 0 included)
template <typename T>
int put(void *pool, size_t at, const std::vector<T> &src, bool always = false) {
    if (always || !src.empty())
        SML_HIP(hipMemcpy((char *)pool + at, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return SML_OK;
}

// pack the region on the host (pack_region: every check is made there, so a rejected
// load changes nothing on the device), then upload what it holds
template <typename SrcT, typename StoT>
int load_region_impl(sml_reservoirs *c, int i, const int *rows, const int *cols, const SrcT *vals, const SrcT *win,
                     const SrcT *wout, const double *mean, const double *std) {
    PackedRegion<StoT> p;
    const PackIn in{i, c->k[i], c->ncs, c->nout, c->nout_pad, c->a_ell_cap[i], c->w_ell_cap[i]};
    if (int rc = pack_region(in, c->rd[i], rows, cols, vals, win, wout, &p)) return rc;
    if (p.wnz > c->w_nz_cap[i])  // a W_in denser than trained (up to the dense n x ninp matmul, :1443)
        if (int rc = grow_win_pool(c, i, p.wnz)) return rc;
    RegionDev &rg = c->rd[i];
    const size_t wb = sizeof(StoT);
    int rc;
    if ((rc = put(c->d_a_rp, rg.a_rp * 4, p.rp)) || (rc = put(c->d_a_col, rg.a_nz * 2, p.acol, true)) ||
        (rc = put(c->d_a_val, rg.a_nz * wb, p.aval, true)) || (rc = put(c->d_w_rp, rg.w_rp * 4, p.wrp)) ||
        (rc = put(c->d_w_col, rg.w_nz * 2, p.wcol)) || (rc = put(c->d_w_val, rg.w_nz * wb, p.wval)) ||
        (rc = put(c->d_wout, rg.wout * wb, p.wt)) || (rc = put(c->d_wlm, rg.wlm * wb, p.wl)) ||
        (rc = put(c->d_a_ell_col, rg.a_ell * 2, p.a_ec)) || (rc = put(c->d_a_ell_val, rg.a_ell * wb, p.a_ev)) ||
        (rc = put(c->d_a_om, rg.a_om * 8, p.om)) || (rc = put(c->d_a_ob, rg.a_om * 4, p.ob)) ||
        (rc = put(c->d_a_oc, rg.a_oe * 2, p.oc)) || (rc = put(c->d_a_ov, rg.a_oe * wb, p.ovv)) ||
        (rc = put(c->d_w_ell_col, rg.w_ell * 2, p.w_ec)) || (rc = put(c->d_w_ell_val, rg.w_ell * wb, p.w_ev)))
        return rc;
    rg.a_w = p.a_w;
    rg.a_ov = p.a_ov;
    rg.w_w = p.w_w;
    rg.w_q = p.w_q;
    rg.w_magic = p.w_magic;
    reshape(c);  // (the region's ELL form is one of the shape's inputs)
    SML_HIP(hipMemcpy(c->d_rd + i, &rg, sizeof(RegionDev), hipMemcpyHostToDevice));
    double ms[2 * kMeanStd];
    std::memcpy(ms, mean, sizeof(double) * kMeanStd);
    std::memcpy(ms + kMeanStd, std, sizeof(double) * kMeanStd);
    std::memcpy(&c->meanstd_h[(size_t)i * 2 * kMeanStd], ms, sizeof ms);
    SML_HIP(hipMemcpy(c->d_meanstd + (size_t)i * 2 * kMeanStd, ms, sizeof ms, hipMemcpyHostToDevice));
    c->loaded[i] = 1;
    return SML_OK;
}

// create: validate, plan, allocate, upload.  The context is the unique_ptr's until the
// last step has passed, so every refusal below frees all of it.
int res_create_impl(int numregions, int nlocal, const int *region_ids, const unsigned char *sst_flags,
                    const int *n, const int *k, int chunk_speedy, int nout, int weight_dtype, double leakage,
                    const int *ninp_generic, const signed char *out_index, sml_reservoirs **out) {
    SML_REQUIRE(out != nullptr, "out is null");
    *out = nullptr;
    int fx, fy;
    SML_REQUIRE(decompose(numregions, &fx, &fy), "numregions %d does not decompose the 96x48 grid", numregions);
    SML_REQUIRE(nlocal >= 0 && nlocal <= numregions && nlocal < 65536, "bad nlocal %d", nlocal);
    SML_REQUIRE(nlocal == 0 || (region_ids && sst_flags && n && k), "null per-region arrays");
    SML_REQUIRE(chunk_speedy >= 0 && nout > 0, "bad chunk sizes (%d, %d)", chunk_speedy, nout);
    SML_REQUIRE(weight_dtype == SML_F32 || weight_dtype == SML_F64, "weight_dtype must be SML_F32 or SML_F64");
    std::unique_ptr<sml_reservoirs> owner(new (std::nothrow) sml_reservoirs());
    sml_reservoirs *c = owner.get();
    if (!c) return fail(SML_ERR_NOMEM, "host allocation failed");
    c->numregions = numregions;
    c->nlocal = nlocal;
    c->ncs = chunk_speedy;
    c->nout = nout;
    c->nout_pad = (nout + kRows - 1) / kRows * kRows;
    c->ov_ld = nout;
    c->wdtype = weight_dtype;
    c->leakage = leakage;
    c->generic = ninp_generic != nullptr;
    if (c->generic) c->out_l.assign(out_index, out_index + nout);
    (void)hipGetDevice(&c->device);
    (void)hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, c->device);
    {
        int lds = 0;
        (void)hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device);
        c->max_lds = (size_t)std::max(lds, 0);
    }
    c->region_ids.assign(region_ids, region_ids + nlocal);
    c->sst.assign(sst_flags, sst_flags + nlocal);
    c->n.assign(n, n + nlocal);
    c->k.assign(k, k + nlocal);
    c->loaded.assign(nlocal, 0);
    c->meanstd_h.assign((size_t)nlocal * 2 * kMeanStd, 0.0);
    c->geom.resize(nlocal);
    c->ninp.resize(nlocal);
    // --- validate
    for (int i = 0; i < nlocal; ++i) {
        SML_REQUIRE(region_geom(numregions, region_ids[i], &c->geom[i]), "region id %d out of range", region_ids[i]);
        SML_REQUIRE(n[i] > 0 && n[i] <= 65535 && k[i] >= 0, "region %d: n=%d (1..65535) k=%d", i, n[i], k[i]);
        const RegionGeom &g = c->geom[i];
        SML_REQUIRE(c->generic || (kVars * g.resx * g.resy * kZGrid + 2 * g.resx * g.resy == nout &&
                                   (!chunk_speedy || chunk_speedy == kVars * g.resx * g.resy * kZGrid + g.resx * g.resy)),
                    "nout %d / chunk_speedy %d do not match the %dx%d region tiles", nout, chunk_speedy, g.resx,
                    g.resy);
        c->ninp[i] = c->generic ? ninp_generic[i] : region_ninp(g, sst_flags[i] != 0);
        SML_REQUIRE(c->ninp[i] > 0 && c->ninp[i] <= 65535, "region %d: ninp %d (1..65535)", i, c->ninp[i]);
    }
    // --- plan: every region's offsets into the pools, the pools' sizes; the step's shape
    static_cast<PoolPlan &>(*c) = plan_pools({nlocal, n, k, c->ninp.data(), chunk_speedy, c->nout_pad, c->no_ell});
    c->w_nz_cap.assign(n, n + nlocal);
    c->row0_h.assign(nlocal + 1, 0);
    for (int i = 0; i < nlocal; ++i) c->row0_h[i + 1] = c->row0_h[i] + n[i];
    reshape(c);
    // --- allocate: filled with zeros where a kernel may read a word no load has written
    // (the zero bytes, the row pointers, W_out's padding, the states), plain otherwise
    wpool(c, &c->d_zero, 256 / (int64_t)wbytes(c), true);
    pool(c, &c->d_a_rp, c->tot_a_rp, true);
    pool(c, &c->d_w_rp, c->tot_w_rp, true);
    wpool(c, &c->d_wout, c->tot_wout, true);
    wpool(c, &c->d_wlm, std::max<int64_t>(c->tot_wlm, 1), true);
    pool(c, &c->d_x[0], c->tot_xaug, true);
    pool(c, &c->d_x[1], c->tot_xaug, true);
    pool(c, &c->d_a_ell_col, c->tot_a_ell);
    wpool(c, &c->d_a_ell_val, c->tot_a_ell, false);
    pool(c, &c->d_w_ell_col, c->tot_w_ell);
    wpool(c, &c->d_w_ell_val, c->tot_w_ell, false);
    pool(c, &c->d_a_om, c->tot_a_om);
    pool(c, &c->d_a_ob, c->tot_a_om);
    pool(c, &c->d_a_oc, c->tot_a_oe);
    wpool(c, &c->d_a_ov, c->tot_a_oe, false);
    pool(c, &c->d_rd, nlocal);
    pool(c, &c->d_a_col, c->tot_a_nz);
    wpool(c, &c->d_a_val, c->tot_a_nz, false);
    pool(c, &c->d_w_col, c->tot_w_nz);
    wpool(c, &c->d_w_val, c->tot_w_nz, false);
    pool(c, &c->d_meanstd, (int64_t)nlocal * 2 * kMeanStd);
    pool(c, &c->d_part, (int64_t)std::max(nlocal, 1) * c->nout_pad);
    pool(c, &c->d_row0, nlocal + 1);
    if (int rc = c->mem.status()) return rc;
    // --- upload (unit std / zero mean until loaded)
    for (int i = 0; i < nlocal; ++i)
        for (int l = 0; l < kMeanStd; ++l) c->meanstd_h[(size_t)i * 2 * kMeanStd + kMeanStd + l] = 1.0;
    int rc;
    if ((rc = upload(c->d_rd, c->rd)) || (rc = upload(c->d_meanstd, c->meanstd_h)) || (rc = build_tables(c)) ||
        (rc = upload(c->d_row0, c->row0_h)))
        return rc;
    *out = owner.release();
    return SML_OK;
}

Ell make_ell(const sml_reservoirs *c) {
    return Ell{c->d_a_ell_col, c->d_a_ell_val, c->d_w_ell_col, c->d_w_ell_val, c->d_a_om,
               c->d_a_ob,      c->d_a_oc,      c->d_a_ov,      c->d_zero};
}

// ------------------------------------------------------------------ launchers
// (each reads the form and the LDS of its stage from c->shape; what depends on the
// call's own arguments -- the balanced grid, np / ovf, the readout's pacing -- is here)

// x_new = (1 - leak) x + leak tanh(A x + W_in u) for every local region (+ x~, x_aug)
int launch_update_bal(sml_reservoirs *c, const double *xo, double *xn, const double *d_feedback, hipStream_t st) {
    const StepShape &s = c->shape;
    const int64_t total = c->row0_h[c->nlocal];
    int G = c->upd_cus > 0 ? c->upd_cus : std::max(c->ncu, 1);  // one block per CU the launch gets
    G = (int)std::max<int64_t>(1, std::min<int64_t>(G, total));
    if (G > c->blk_cap) {  // (the buffer grows only past the largest grid seen: rare, synchronous)
        const int cap = std::max(G, std::max(c->ncu, c->upd_cus));
        if (c->d_blk_r0) {
            SML_HIP(hipDeviceSynchronize());
            c->mem.release(&c->d_blk_r0);
            c->blk_cap = 0;
        }
        if (int rc = pool(c, &c->d_blk_r0, (int64_t)cap * (cap + 1) / 2)) return rc;
        c->blk_off.assign(cap + 1, -1);
        c->blk_cap = cap;
    }
    if (c->blk_off[G] < 0) {  // each block's first region, for this grid: once per G
        c->blk_off[G] = G * (G - 1) / 2;
        c->blk_host.push_back(block_first_regions(c->row0_h, G));  // ordered before the launch on st
        SML_HIP(hipMemcpyAsync(c->d_blk_r0 + c->blk_off[G], c->blk_host.back().data(), (size_t)G * 4,
                               hipMemcpyHostToDevice, st));
    }
    const int32_t *blk_r0 = c->d_blk_r0 + c->blk_off[G];
    const Ell ell = make_ell(c);
    // the pairs every pass loads (the widest region's; 2 at least) and whether any
    // region keeps an overflow list
    int np = 2;
    bool ovf = false;
    for (int i = 0; i < c->nlocal; ++i) {
        np = std::max(np, (c->rd[i].a_w + 1) / 2);
        ovf = ovf || c->rd[i].a_ov;
    }
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(G), dim3(kUpdThreads), s.lds_bal, st, c->d_rd, c->d_row0, blk_r0, c->nlocal,
                           total, ell, xo, xn, d_feedback, c->leakage, s.lds_x, s.lds_buf);
    };
    // two passes of A / W_in rows in flight (a third measured slower: 114-124 VGPRs)
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        if (np == 2) ovf ? go(k_res_update_bal<WT, 2, true, 2>) : go(k_res_update_bal<WT, 2, false, 2>);
        else if (np == 3) ovf ? go(k_res_update_bal<WT, 3, true, 2>) : go(k_res_update_bal<WT, 3, false, 2>);
        else ovf ? go(k_res_update_bal<WT, 4, true, 2>) : go(k_res_update_bal<WT, 4, false, 2>);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

int launch_update(sml_reservoirs *c, const double *xo, double *xn, const double *d_feedback, hipStream_t st) {
    const StepShape &s = c->shape;
    if (s.balanced) return launch_update_bal(c, xo, xn, d_feedback, st);
    const int nlog = s.parts * c->nlocal;
    const Ell ell = make_ell(c);
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern, size_t shared) {
            hipLaunchKernelGGL(kern, dim3(nlog), dim3(kUpdThreads), shared, st, c->d_rd, c->d_a_rp, c->d_a_col,
                               (const WT *)c->d_a_val, c->d_w_rp, c->d_w_col, (const WT *)c->d_w_val, ell, xo, xn,
                               d_feedback, c->leakage, s.parts, s.lds_x, nlog);
        };
        if (s.region_lds) go(k_res_update<WT, true, 4>, s.lds_region);
        else go(k_res_update<WT, false, 4>, 0);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the fused begin (shape.begin_fused): a block per region
int launch_begin(sml_reservoirs *c, const double *xo, double *xn, const double *d_feedback, hipStream_t st) {
    const StepShape &s = c->shape;
    const Ell ell = make_ell(c);
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(c->nlocal), dim3(kBeginThreads), s.lds_region, st, c->d_rd, c->d_a_rp,
                               c->d_a_col, (const WT *)c->d_a_val, c->d_w_rp, c->d_w_col, (const WT *)c->d_w_val, ell,
                               xo, xn, d_feedback, c->ncs, c->leakage, s.lds_x, (const WT *)c->d_wout, c->d_part,
                               c->nout_pad, s.groups);
        };
        if (c->begin_mode == 2) go(k_res_begin<WT, 2, 2>);
        else go(k_res_begin<WT, 1, 4>);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// xs: the state the readout's x~ comes from (the one the update just wrote; unused
// by the finish)
template <int kMode>
void launch_readout(sml_reservoirs *c, const double *xs, const double *d_local_model, double *d_outvec,
                    hipStream_t st, double *d_raw = nullptr) {
    if constexpr (kMode == kReadFinish) {
        const int total = c->nlocal * c->nout_pad;
        with_wt(c, [&](auto tag) {
            using WT = decltype(tag);
            hipLaunchKernelGGL(k_res_finish<WT>, dim3((total + 255) / 256), dim3(256), 0, st, c->d_rd,
                               (const WT *)c->d_wlm, d_local_model, c->d_meanstd, c->d_outl, c->d_part, d_outvec,
                               c->nout, c->ov_ld, c->nout_pad, c->ncs, c->nlocal, d_raw);
        });
    } else {
        const StepShape &s = c->shape;
        const int nitems = c->nlocal * s.groups;
        // the v_ml half runs beside SPEEDY's window: c->read_waves > 0 caps its waves
        // (each takes a run of items) so it leaves HBM headroom for the window
        int ipw = 1;
        if (kMode == kReadML && c->read_waves > 0 && c->read_waves < nitems)
            ipw = (nitems + c->read_waves - 1) / c->read_waves;
        const int nwaves = (nitems + ipw - 1) / ipw;
        const int nblocks = (nwaves + s.wpb - 1) / s.wpb;
        with_wt(c, [&](auto tag) {
            using WT = decltype(tag);
            auto go = [&](auto kern) {
                hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * s.wpb), 0, st, c->d_rd, (const WT *)c->d_wout,
                                   (const WT *)c->d_wlm, xs, d_local_model, c->d_meanstd, c->d_outl, c->d_part,
                                   d_outvec, c->nout, c->ov_ld, c->nout_pad, c->ncs, s.groups, nitems, ipw);
            };
            if (s.wide) go(k_res_readout<WT, kMode, kRowsWide>);
            else go(k_res_readout<WT, kMode, kRows>);
        });
    }
}

// the finish from SPEEDY's forecast grids (k_res_finish_grid), grouped where the shape
// allows, with or without the assembly.  part: the partial sums it adds (c->d_part, or one
// member's rows of it)
template <bool kAsm>
void launch_finish_grid(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d, double *d_local_model,
                        double *d_outvec, double *d_grid4d, double *d_grid2d, double *d_precip, hipStream_t st,
                        const double *part = nullptr) {
    if (!part) part = c->d_part;
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(c->nlocal), dim3(256), 0, st, c->d_rd, (const WT *)c->d_wlm, c->d_lm_src,
                               c->d_lm_l, d_fc4d, d_fc2d, d_local_model, c->d_meanstd, c->d_outl, part, d_outvec,
                               c->nout, c->ov_ld, c->nout_pad, c->ncs, c->d_asm_dst, d_grid4d, d_grid2d, d_precip,
                               c->fin_wflag, c->fin_wval, c->fin_wlate, c->fin_wtimeout);
        };
        if (c->shape.finish_grouped) go(k_res_finish_grid<WT, kAsm, true>);
        else go(k_res_finish_grid<WT, kAsm, false>);
    });
    c->fin_wflag = nullptr;  // one launch
    c->fin_wlate = nullptr;
}

// ---- ensemble members (sml_res_members.hpp): every member's update, then every member's
// readout, each in one launch over tiles of members (c->mshape)
int launch_update_mem(sml_reservoirs *c, const double *xo, double *xn, const double *d_feedback, int64_t fb_stride,
                      hipStream_t st) {
    const StepShape &s = c->shape;
    const MemberShape &ms = c->mshape;
    if (ms.update_tile < 1 || ms.update_tile > kMemberTile || ms.lds > c->max_lds)
        return fail(SML_ERR_STATE, "the members update has no tile for this context (tile %d, %zu bytes of LDS)",
                    ms.update_tile, ms.lds);
    const int ntiles = (c->members + ms.update_tile - 1) / ms.update_tile;
    const int nlog = s.parts * c->nlocal;
    const Ell ell = make_ell(c);
    const MemberArgs mem{c->members, ms.update_tile, c->tot_xaug, fb_stride, 0, 0};
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(nlog * ntiles), dim3(kUpdThreads), ms.lds, st, c->d_rd, c->d_a_rp,
                               c->d_a_col, (const WT *)c->d_a_val, c->d_w_rp, c->d_w_col, (const WT *)c->d_w_val, ell,
                               xo, xn, d_feedback, c->leakage, s.parts, s.lds_x, s.lds_buf, ntiles, mem);
        };
        // (a tile of 3 or 4 only in a build with kMemberTile 4)
        if (kMemberTile == 2 || ms.update_tile <= 2)
            ms.update_lds ? go(k_res_update_mem<WT, true, 2>) : go(k_res_update_mem<WT, false, 2>);
        else if constexpr (kMemberTile > 2)
            ms.update_lds ? go(k_res_update_mem<WT, true, 4>) : go(k_res_update_mem<WT, false, 4>);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the partial sums of one member of a begun step
int64_t part_stride(const sml_reservoirs *c) { return (int64_t)c->nlocal * c->nout_pad; }

// xs: the state buffer the update just wrote (member e's x_aug rows at e * tot_xaug).
// kReadML (the members' begin): v_ml alone into c->d_part; c->read_waves > 0 caps the
// launch's waves, as it paces k_res_readout<kReadML> (the kernel strides over its items)
template <int kMode>
int launch_readout_mem(sml_reservoirs *c, const double *xs, const double *d_local_model, int64_t lm_stride,
                       double *d_outvec, int64_t ov_stride, hipStream_t st) {
    const StepShape &s = c->shape;
    const MemberShape &ms = c->mshape;
    const int nitems = c->nlocal * s.groups;
    int nwaves = nitems * ms.readout_streams;
    if (kMode == kReadML && c->read_waves > 0) nwaves = std::min(nwaves, c->read_waves);
    const int nblocks = (nwaves + s.wpb - 1) / s.wpb;
    const MemberArgs mem{c->members, ms.readout_tile, c->tot_xaug, 0, lm_stride, ov_stride, part_stride(c)};
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64 * s.wpb), 0, st, c->d_rd, (const WT *)c->d_wout,
                               (const WT *)c->d_wlm, xs, d_local_model, c->d_meanstd, c->d_outl, c->d_part, d_outvec,
                               c->nout, c->ov_ld, c->nout_pad, c->ncs, s.groups, nitems, ms.readout_streams, mem);
        };
        if (kMemberTile == 2 || ms.readout_tile <= 2)
            s.wide ? go(k_res_readout_mem<WT, kMode, kRowsWide, 2>) : go(k_res_readout_mem<WT, kMode, kRows, 2>);
        else if constexpr (kMemberTile > 2)
            s.wide ? go(k_res_readout_mem<WT, kMode, kRowsWide, 4>) : go(k_res_readout_mem<WT, kMode, kRows, 4>);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the members' finish from local models (k_res_finish_mem)
int launch_finish_mem(sml_reservoirs *c, const double *d_local_model, int64_t lm_stride, double *d_outvec,
                      int64_t ov_stride, hipStream_t st) {
    const int64_t total = (int64_t)c->members * c->nlocal * c->nout_pad;
    const MemberArgs mem{c->members, 1, 0, 0, lm_stride, ov_stride, part_stride(c)};
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        hipLaunchKernelGGL(k_res_finish_mem<WT>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c->d_rd,
                           (const WT *)c->d_wlm, d_local_model, c->d_meanstd, c->d_outl, c->d_part, d_outvec, c->nout,
                           c->ov_ld, c->nout_pad, c->ncs, c->nlocal, mem);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the members' finish from their forecast grids (k_res_finish_grid_mem), a block per
// (region, tile of c->mfin.tile members); c->mfin.looped: k_res_finish_grid once per member
// on that member's pointers instead (the same bits)
template <bool kAsm>
int launch_finish_grid_mem(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d, double *d_local_model,
                           double *d_outvec, double *d_grid4d, double *d_grid2d, double *d_precip,
                           const FinMemArgs &a, hipStream_t st) {
    if (c->mfin.looped) {
        for (int64_t e = 0; e < c->members; ++e)
            launch_finish_grid<kAsm>(c, d_fc4d ? d_fc4d + e * a.fc4s : nullptr, d_fc2d ? d_fc2d + e * a.fc2s : nullptr,
                                     d_local_model ? d_local_model + e * a.lms : nullptr, d_outvec + e * a.ovs,
                                     kAsm ? d_grid4d + e * a.g4s : nullptr, kAsm ? d_grid2d + e * a.g2s : nullptr,
                                     kAsm ? d_precip + e * a.g2s : nullptr, st, c->d_part + e * a.ps);
        SML_HIP(hipGetLastError());
        return SML_OK;
    }
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(c->nlocal * a.tiles), dim3(256), 0, st, c->d_rd, (const WT *)c->d_wlm,
                               c->d_lm_src, c->d_lm_l, d_fc4d, d_fc2d, d_local_model, c->d_meanstd, c->d_outl,
                               c->d_part, d_outvec, c->nout, c->ov_ld, c->nout_pad, c->ncs, c->d_asm_dst, d_grid4d,
                               d_grid2d, d_precip, a);
        };
        const bool grp = c->shape.finish_grouped;
        if (a.tile <= 2) grp ? go(k_res_finish_grid_mem<WT, kAsm, true, 2>) : go(k_res_finish_grid_mem<WT, kAsm, false, 2>);
        else grp ? go(k_res_finish_grid_mem<WT, kAsm, true, kFinTileMax>)
                 : go(k_res_finish_grid_mem<WT, kAsm, false, kFinTileMax>);
    });
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the events of one timed step (sml_res_enable_timing), when the context has a free
// slot: stamp(0) before the step, stamp(1) after the update, stamp(2) after the readout
struct StepTimer {
    StepEvents &t;
    hipStream_t st;
    hipEvent_t *ev;
    StepTimer(sml_reservoirs *c, hipStream_t stream)
        : t(c->timers), st(stream), ev(t.on && t.used < t.cap ? &t.ev[3 * t.used] : nullptr) {}
    int stamp(int q) {
        if (!ev) return SML_OK;
        SML_HIP(hipEventRecord(ev[q], st));
        if (q == 2) ++t.used;
        return SML_OK;
    }
};

}  // namespace

// ------------------------------------------------------------------ API
extern "C" int sml_res_destroy(sml_reservoirs *c) {
    delete c;
    return SML_OK;
}

extern "C" int sml_res_create(int numregions, int nlocal, const int *region_ids, const unsigned char *sst_flags,
                              const int *n, const int *k, int chunk_speedy, int nout, int weight_dtype,
                              double leakage, sml_reservoirs **out) {
    return res_create_impl(numregions, nlocal, region_ids, sst_flags, n, k, chunk_speedy, nout, weight_dtype, leakage,
                           nullptr, nullptr, out);
}

extern "C" int sml_res_create_generic(int numregions, int nlocal, const int *region_ids, const int *ninp,
                                      const int *n, const int *k, int chunk_speedy, int nout,
                                      const signed char *out_index, int weight_dtype, double leakage,
                                      sml_reservoirs **out) {
    SML_REQUIRE(nlocal == 0 || (ninp && out_index), "null ninp / out_index");
    for (int o = 0; o < nout && out_index; ++o)
        SML_REQUIRE(out_index[o] >= -1 && out_index[o] < kMeanStd, "out_index[%d] = %d outside [-1, 36)", o,
                    out_index[o]);
    std::vector<unsigned char> sst(std::max(nlocal, 1), 0);
    return res_create_impl(numregions, nlocal, region_ids, sst.data(), n, k, chunk_speedy, nout, weight_dtype,
                           leakage, ninp, out_index, out);
}

// the row stride of every outvec array the context writes (sml_res_step*, the
// finish kernels) and of sml_exchange_assemble's input (>= nout)
extern "C" int sml_res_set_outvec_ld(sml_reservoirs *c, int ld) {
    SML_REQUIRE(c && ld >= c->nout, "bad outvec row stride %d", ld);
    SML_REQUIRE(!c->is_begun(), "sml_res_set_outvec_ld inside a begun step");
    c->ov_ld = ld;
    return SML_OK;
}

extern "C" int sml_res_info(const sml_reservoirs *c, int *numregions, int *nlocal, int *chunk_speedy, int *nout,
                            int *region_ids) {
    SML_REQUIRE(c, "null context");
    if (numregions) *numregions = c->numregions;
    if (nlocal) *nlocal = c->nlocal;
    if (chunk_speedy) *chunk_speedy = c->ncs;
    if (nout) *nout = c->nout;
    if (region_ids) std::memcpy(region_ids, c->region_ids.data(), sizeof(int) * c->nlocal);
    return SML_OK;
}

extern "C" int sml_res_ninp(const sml_reservoirs *c, int i, int *ninp) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(ninp, "ninp is null");
    *ninp = c->ninp[i];
    return SML_OK;
}

// the mean / std (36 each) local region i standardizes with (host copy of the loaded ones)
extern "C" int sml_res_mean_std(const sml_reservoirs *c, int i, double *mean, double *std) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(mean && std, "null argument");
    std::memcpy(mean, &c->meanstd_h[(size_t)i * 2 * kMeanStd], kMeanStd * 8);
    std::memcpy(std, &c->meanstd_h[(size_t)i * 2 * kMeanStd + kMeanStd], kMeanStd * 8);
    return SML_OK;
}

extern "C" int sml_res_feedback_offsets(const sml_reservoirs *c, int64_t *offsets) {
    SML_REQUIRE(c && offsets, "null argument");
    for (int i = 0; i < c->nlocal; ++i) offsets[i] = c->rd[i].fb;
    offsets[c->nlocal] = c->tot_fb;
    return SML_OK;
}

extern "C" int sml_res_load_region_f32(sml_reservoirs *c, int i, const int *rows, const int *cols, const float *vals,
                                       const float *win, const float *wout, const double *mean, const double *std) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(win && wout && mean && std && (c->k[i] == 0 || (rows && cols && vals)), "null weight array");
    return with_wt(c, [&](auto tag) {
        return load_region_impl<float, decltype(tag)>(c, i, rows, cols, vals, win, wout, mean, std);
    });
}

extern "C" int sml_res_load_region_f64(sml_reservoirs *c, int i, const int *rows, const int *cols,
                                       const double *vals, const double *win, const double *wout,
                                       const double *mean, const double *std) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(win && wout && mean && std && (c->k[i] == 0 || (rows && cols && vals)), "null weight array");
    return with_wt(c, [&](auto tag) {
        return load_region_impl<double, decltype(tag)>(c, i, rows, cols, vals, win, wout, mean, std);
    });
}

extern "C" int sml_res_set_state_member(sml_reservoirs *c, int member, int i, const double *x) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(member >= 0 && member < c->members, "member %d out of range [0,%d)", member, c->members);
    SML_REQUIRE(x, "x is null");
    // a begun step read the state being replaced: it is discarded (sml_res_step_cancel)
    if (int rc = sml_res_step_cancel(c)) return rc;
    SML_HIP(hipMemcpy(c->x_now() + (size_t)member * c->tot_xaug + c->rd[i].x, x, (size_t)c->n[i] * 8,
                      hipMemcpyHostToDevice));
    return SML_OK;
}

extern "C" int sml_res_get_state_member(sml_reservoirs *c, int member, int i, double *x) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(member >= 0 && member < c->members, "member %d out of range [0,%d)", member, c->members);
    SML_REQUIRE(x, "x is null");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(x, c->x_now() + (size_t)member * c->tot_xaug + c->rd[i].x, (size_t)c->n[i] * 8,
                      hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_res_set_state(sml_reservoirs *c, int i, const double *x) {
    return sml_res_set_state_member(c, 0, i, x);
}

extern "C" int sml_res_get_state(sml_reservoirs *c, int i, double *x) { return sml_res_get_state_member(c, 0, i, x); }

// The number of members (1 .. SML_RES_MAX_MEMBERS; 1 at create).  Both state buffers are
// laid out anew, filled with zeros: the members kept (member 0 always) are copied over,
// new members start from x = 0 with zero row padding, which the readout's 16-byte loads
// run over.  A set-up call: it waits for the device.
extern "C" int sml_res_set_members(sml_reservoirs *c, int members) {
    SML_REQUIRE(c, "null context");
    SML_REQUIRE(members >= 1 && members <= kMaxMembers, "members %d outside 1..%d", members, kMaxMembers);
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_set_members inside a begun step");
    if (members == c->members) return SML_OK;
    SML_HIP(hipDeviceSynchronize());  // steps in flight read the old buffers
    const int64_t keep = (int64_t)std::min(members, c->members) * c->tot_xaug;
    double *nx[2] = {nullptr, nullptr};
    pool(c, &nx[0], (int64_t)members * c->tot_xaug, true);
    pool(c, &nx[1], (int64_t)members * c->tot_xaug, true);
    double *npart = nullptr;  // scratch of the step in flight: nothing to keep
    pool(c, &npart, (int64_t)members * std::max(c->nlocal, 1) * c->nout_pad);
    hipError_t e = hipSuccess;
    for (int q = 0; q < 2 && c->mem.status() == SML_OK && e == hipSuccess && keep > 0; ++q)
        e = hipMemcpy(nx[q], c->d_x[q], (size_t)keep * 8, hipMemcpyDeviceToDevice);
    if (c->mem.status() != SML_OK || e != hipSuccess) {
        c->mem.release(&nx[0]);
        c->mem.release(&nx[1]);
        c->mem.release(&npart);
        return c->mem.status() ? c->mem.status()
                               : fail(SML_ERR_HIP, "sml_res_set_members: %s", hipGetErrorString(e));
    }
    for (int q = 0; q < 2; ++q) {
        c->mem.release(&c->d_x[q]);
        c->d_x[q] = nx[q];
    }
    c->mem.release(&c->d_part);
    c->d_part = npart;
    c->members = members;
    reshape(c);
    return SML_OK;
}

extern "C" int sml_res_members(const sml_reservoirs *c, int *members) {
    SML_REQUIRE(c && members, "null argument");
    *members = c->members;
    return SML_OK;
}

// the tiles the members kernels run with (member_shape): members per update block, whether
// their x and u are staged in LDS, members per W_out load of the readout
extern "C" int sml_res_member_tile(const sml_reservoirs *c, int *update_tile, int *update_lds, int *readout_tile) {
    SML_REQUIRE(c && update_tile && update_lds && readout_tile, "null argument");
    *update_tile = c->mshape.update_tile;
    *update_lds = c->mshape.update_lds ? 1 : 0;
    *readout_tile = c->mshape.readout_tile;
    return SML_OK;
}

// the CUs the context's launches get (a CU-masked stream: the hybrid loop's reservoir
// stream); the balanced update runs one block per CU.  0 = every CU of the device.
extern "C" int sml_res_set_update_cus(sml_reservoirs *c, int cus) {
    SML_REQUIRE(c && cus >= 0, "bad argument");
    c->upd_cus = cus;
    return SML_OK;
}

// 1 when sml_res_step / _begin run the balanced update (k_res_update_bal), 0 for the
// per-region k_res_update (a region in CSR form, n > 7168, ninp > 1024, SML_RES_PATH_PER_REGION)
extern "C" int sml_res_update_balanced(sml_reservoirs *c, int *balanced) {
    SML_REQUIRE(c && balanced, "null argument");
    *balanced = c->shape.balanced ? 1 : 0;
    return SML_OK;
}

extern "C" int sml_res_ell_layout(sml_reservoirs *c, int i, int *a_width, int *a_overflow, int *win_q,
                                  int *win_ell) {
    if (int rc = check_region(c, i)) return rc;
    SML_REQUIRE(a_width && a_overflow && win_q && win_ell, "null argument");
    const RegionDev &r = c->rd[i];
    *a_width = r.a_w;
    *a_overflow = r.a_ov;
    *win_q = r.w_q;
    *win_ell = r.w_w;
    return SML_OK;
}

// the fallback paths forced for every region (bitwise the defaults, which take them
// only where a region's structure does not fit): SML_RES_PATH_CSR -- A and W_in from
// their CSR copies, no ELL layout (before any region is loaded); SML_RES_PATH_PER_REGION
// -- k_res_update, a block per (region, part), instead of the balanced update;
// SML_RES_PATH_UNGROUPED_FINISH -- the v_p finish one thread per output;
// SML_RES_PATH_STEPWISE_DRIVE -- the training drive one update launch per column;
// SML_RES_PATH_RADIUS_GLOBAL -- the spectral radius's x and y in the context's scratch
extern "C" int sml_res_set_reference_paths(sml_reservoirs *c, int flags) {
    SML_REQUIRE(c && (flags & ~31) == 0, "bad argument");
    const bool csr = flags & SML_RES_PATH_CSR;
    if (csr != c->no_ell) {
        for (unsigned char l : c->loaded)
            SML_REQUIRE(!l, "sml_res_set_reference_paths(SML_RES_PATH_CSR) after a region was loaded");
        c->no_ell = csr;
        // (the ELL buffers stay sized for the default: a region is laid out in ELL only
        // while its cap is non-zero, at load)
        for (int i = 0; i < c->nlocal; ++i) {
            c->a_ell_cap[i] = ell_cap_a(c->n[i], c->k[i], csr);
            c->w_ell_cap[i] = ell_cap_w(csr);
        }
    }
    c->per_region = flags & SML_RES_PATH_PER_REGION;
    c->finish_ungrouped = flags & SML_RES_PATH_UNGROUPED_FINISH;
    c->stepwise_drive = flags & SML_RES_PATH_STEPWISE_DRIVE;
    c->radius_global = flags & SML_RES_PATH_RADIUS_GLOBAL;
    reshape(c);
    return SML_OK;
}

extern "C" int sml_res_set_read_waves(sml_reservoirs *c, int waves) {
    SML_REQUIRE(c && waves >= 0, "bad argument");
    c->read_waves = waves;
    return SML_OK;
}

extern "C" int sml_res_set_begin_mode(sml_reservoirs *c, int mode) {
    SML_REQUIRE(c && mode >= 0 && mode <= 2, "bad argument");
    c->begin_mode = mode;
    reshape(c);
    return SML_OK;
}

extern "C" int sml_res_begin_fused(const sml_reservoirs *c, int *fused) {
    SML_REQUIRE(c && fused, "null argument");
    *fused = c->shape.begin_fused ? 1 : 0;
    return SML_OK;
}

extern "C" int sml_res_enable_timing(sml_reservoirs *c, int capacity) {
    SML_REQUIRE(c, "null context");
    SML_REQUIRE(capacity >= 0, "capacity must be >= 0");
    StepEvents &t = c->timers;
    while (t.cap < capacity) {
        for (int q = 0; q < 3; ++q) {
            hipEvent_t e;
            SML_HIP(hipEventCreate(&e));
            t.ev.push_back(e);
        }
        ++t.cap;
    }
    t.on = capacity > 0;
    t.used = 0;
    return SML_OK;
}

extern "C" int sml_res_kernel_times(sml_reservoirs *c, float *update_ms, float *readout_ms, int max_steps,
                                    int *count) {
    SML_REQUIRE(c && count, "null argument");
    StepEvents &t = c->timers;
    const int n = std::min(t.used, max_steps);
    for (int s = 0; s < n; ++s) {
        SML_HIP(hipEventSynchronize(t.ev[3 * s + 2]));
        float a = 0, b = 0;
        SML_HIP(hipEventElapsedTime(&a, t.ev[3 * s], t.ev[3 * s + 1]));
        SML_HIP(hipEventElapsedTime(&b, t.ev[3 * s + 1], t.ev[3 * s + 2]));
        if (update_ms) update_ms[s] = a;
        if (readout_ms) readout_ms[s] = b;
    }
    *count = n;
    t.used = 0;
    return SML_OK;
}

namespace {
// one member's begin (sml_res_step_begin; sml_res_step_begin_members at one member)
int begin_single(sml_reservoirs *c, const double *d_feedback, hipStream_t st) {
    return c->advance(true, [&](const double *xo, double *xn) {
        StepTimer timer(c, st);
        if (int rc = timer.stamp(0)) return rc;
        if (c->shape.begin_fused) {  // one launch: the update's time is inside the readout's (update_ms 0)
            if (int rc = timer.stamp(1)) return rc;
            if (int rc = launch_begin(c, xo, xn, d_feedback, st)) return rc;
        } else {
            if (int rc = launch_update(c, xo, xn, d_feedback, st)) return rc;  // beside SPEEDY's window
            if (int rc = timer.stamp(1)) return rc;
            launch_readout<kReadML>(c, xn, nullptr, nullptr, st);
        }
        SML_HIP(hipGetLastError());
        return timer.stamp(2);
    });
}
}  // namespace

extern "C" int sml_res_step_begin(sml_reservoirs *c, const double *d_feedback, void *stream) {
    SML_REQUIRE(c, "null context");
    if (int rc = check_single(c, "sml_res_step_begin")) return rc;
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_feedback, "null device buffer");
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_begin called twice without sml_res_step_finish");
    if (int rc = check_loaded(c)) return rc;
    return begin_single(c, d_feedback, (hipStream_t)stream);
}

// discard a begun step (sml_res_step_begin without its finish): wait for it, then
// roll the state back -- the begin read x from one buffer and wrote the update into
// the other, so the old state is intact; x_aug and the v_ml partial sums are scratch
// that the next begin rewrites.  A no-op when no step is begun.
extern "C" int sml_res_step_cancel(sml_reservoirs *c) {
    SML_REQUIRE(c, "null context");
    if (!c->is_begun()) return SML_OK;
    SML_HIP(hipDeviceSynchronize());
    c->close(true);
    return SML_OK;
}

extern "C" int sml_res_step_begun(const sml_reservoirs *c, int *begun) {
    SML_REQUIRE(c && begun, "null argument");
    *begun = c->is_begun() ? 1 : 0;
    return SML_OK;
}

extern "C" int sml_res_step_finish(sml_reservoirs *c, const double *d_local_model, double *d_outvec, void *stream) {
    SML_REQUIRE(c, "null context");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_outvec, "null device buffer");
    SML_REQUIRE(c->ncs == 0 || d_local_model, "hybrid context needs d_local_model");
    if (!c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_finish without sml_res_step_begin");
    if (int rc = check_single(c, "sml_res_step_finish")) return rc;  // (it would finish member 0 alone and close the step)
    hipStream_t st = (hipStream_t)stream;
    launch_readout<kReadFinish>(c, nullptr, d_local_model, d_outvec, st);
    SML_HIP(hipGetLastError());
    c->close();
    return SML_OK;
}

// predict_slab (src/mod_slab_ocean_reservoir.f90:1201-1249) for every local region
// of a generic context: x = tanh(A x + W_in feedback) (leakage as created; the
// reference's slab update has none, i.e. 1), outvec = W_out [local_model; x~], the
// raw outvec as the next local model (:1235), then x*std + mean per output slot.
// d_local_model_next must not alias d_local_model (the host ping-pongs them).
extern "C" int sml_res_step_slab(sml_reservoirs *c, const double *d_feedback, const double *d_local_model,
                                 double *d_local_model_next, double *d_outvec, void *stream) {
    SML_REQUIRE(c, "null context");
    if (int rc = check_single(c, "sml_res_step_slab")) return rc;
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_feedback && d_outvec && d_local_model_next && (c->ncs == 0 || d_local_model), "null device buffer");
    SML_REQUIRE(d_local_model_next != d_local_model, "d_local_model_next must not alias d_local_model");
    SML_REQUIRE(c->ncs == c->nout, "predict_slab feeds its outvec back: chunk_speedy (%d) must equal nout (%d)",
                c->ncs, c->nout);
    if (int rc = sml_res_step_begin(c, d_feedback, stream)) return rc;
    launch_readout<kReadFinish>(c, nullptr, d_local_model, d_outvec, (hipStream_t)stream, d_local_model_next);
    SML_HIP(hipGetLastError());
    c->close();
    return SML_OK;
}

int sml::res_finish_wait(sml_reservoirs *c, const uint64_t *flag, uint64_t value, unsigned *late,
                         long long timeout) {
    SML_REQUIRE(c && flag && late, "null argument");
    SML_REQUIRE(c->ncs <= 256, "the in-kernel wait needs ncs <= the finish block");
    c->fin_wflag = flag;
    c->fin_wval = value;
    c->fin_wlate = late;
    c->fin_wtimeout = timeout;
    return SML_OK;
}

extern "C" int sml_res_step_finish_grid(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d,
                                        double *d_local_model, double *d_outvec, void *stream) {
    SML_REQUIRE(c, "null context");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_outvec && (c->ncs == 0 || (d_fc4d && d_fc2d)), "null device buffer");
    SML_REQUIRE(!c->generic || c->ncs == 0, "a generic (slab) context has no local-model tiling");
    SML_REQUIRE(c->ncs <= kMaxNcs, "ncs %d exceeds %d", c->ncs, kMaxNcs);
    if (!c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_finish_grid without sml_res_step_begin");
    if (int rc = check_single(c, "sml_res_step_finish_grid")) return rc;  // (it would finish member 0 alone and close the step)
    launch_finish_grid<false>(c, d_fc4d, d_fc2d, d_local_model, d_outvec, nullptr, nullptr, nullptr,
                              (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    c->close();
    return SML_OK;
}

bool sml::res_in_global_order(const sml_reservoirs *c) {
    if (!c || c->generic || c->nlocal != c->numregions) return false;
    for (int i = 0; i < c->nlocal; ++i)
        if (c->region_ids[i] != i) return false;
    return true;
}

extern "C" int sml_res_step_finish_assemble(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d,
                                            double *d_local_model, double *d_outvec, double *d_grid4d,
                                            double *d_grid2d, double *d_precip, void *stream) {
    SML_REQUIRE(c, "null context");
    SML_REQUIRE(sml::res_in_global_order(c), "the fused assembly needs every region on this rank, in global order");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_outvec && d_grid4d && d_grid2d && d_precip && (c->ncs == 0 || (d_fc4d && d_fc2d)),
                "null device buffer");
    SML_REQUIRE(c->ncs <= kMaxNcs, "ncs %d exceeds %d", c->ncs, kMaxNcs);
    if (!c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_finish_assemble without sml_res_step_begin");
    if (int rc = check_single(c, "sml_res_step_finish_assemble")) return rc;  // (it would finish member 0 alone and close the step)
    launch_finish_grid<true>(c, d_fc4d, d_fc2d, d_local_model, d_outvec, d_grid4d, d_grid2d, d_precip,
                             (hipStream_t)stream);
    SML_HIP(hipGetLastError());
    c->close();
    return SML_OK;
}

extern "C" int sml_res_step(sml_reservoirs *c, const double *d_feedback, const double *d_local_model,
                            double *d_outvec, void *stream) {
    SML_REQUIRE(c, "null context");
    if (int rc = check_single(c, "sml_res_step")) return rc;
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_feedback && d_outvec, "null device buffer");
    SML_REQUIRE(c->ncs == 0 || d_local_model, "hybrid context needs d_local_model");
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step inside a begun step");
    if (int rc = check_loaded(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    return c->advance(false, [&](const double *xo, double *xn) {
        StepTimer timer(c, st);
        if (int rc = timer.stamp(0)) return rc;
        if (int rc = launch_update(c, xo, xn, d_feedback, st)) return rc;
        if (int rc = timer.stamp(1)) return rc;
        launch_readout<kReadFull>(c, xn, d_local_model, d_outvec, st);
        SML_HIP(hipGetLastError());
        return timer.stamp(2);
    });
}

// synchronize (src/mod_reservoir.f90:1352-1378): `length` reservoir updates driven
// by a sequence of inputs, no readout -- the spin-up of start_prediction (:938-959).
// d_inputs: length blocks of the packed feedback layout (sml_res_feedback_offsets),
// block i at d_inputs + i * stride doubles.
extern "C" int sml_res_synchronize(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride,
                                   void *stream) {
    SML_REQUIRE(c && length >= 0, "bad argument");
    if (int rc = check_single(c, "sml_res_synchronize")) return rc;
    if (c->nlocal == 0 || length == 0) return SML_OK;
    SML_REQUIRE(d_inputs && stride >= (int64_t)c->tot_fb, "stride smaller than the packed feedback size");
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_synchronize inside a begun step");
    if (int rc = check_loaded(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < length; ++t) {
        const double *u = d_inputs + (size_t)t * stride;
        if (int rc = c->advance(false, [&](const double *xo, double *xn) { return launch_update(c, xo, xn, u, st); }))
            return rc;
    }
    return SML_OK;
}

// sml_res_step for every member of the context in one stream of the weights: member e's
// feedback, local model and outvecs at e * fb_stride / lm_stride / ov_stride doubles.
// One member takes sml_res_step's own kernels.  All members advance together: one swap.
extern "C" int sml_res_step_members(sml_reservoirs *c, const double *d_feedback, int64_t fb_stride,
                                    const double *d_local_model, int64_t lm_stride, double *d_outvec,
                                    int64_t ov_stride, void *stream) {
    SML_REQUIRE(c, "null context");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_feedback && d_outvec, "null device buffer");
    SML_REQUIRE(c->ncs == 0 || d_local_model, "hybrid context needs d_local_model");
    SML_REQUIRE(fb_stride >= c->tot_fb, "fb_stride %lld smaller than the packed feedback size %lld",
                (long long)fb_stride, (long long)c->tot_fb);
    SML_REQUIRE(c->ncs == 0 || lm_stride >= (int64_t)c->nlocal * c->ncs,
                "lm_stride %lld smaller than nlocal * chunk_speedy", (long long)lm_stride);
    SML_REQUIRE(ov_stride >= (int64_t)c->nlocal * c->ov_ld, "ov_stride %lld smaller than nlocal * the outvec row stride",
                (long long)ov_stride);
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_members inside a begun step");
    if (int rc = check_loaded(c)) return rc;
    if (c->ncs == 0) {
        d_local_model = nullptr;
        lm_stride = 0;
    }
    hipStream_t st = (hipStream_t)stream;
    return c->advance(false, [&](const double *xo, double *xn) {
        StepTimer timer(c, st);
        if (int rc = timer.stamp(0)) return rc;
        if (c->members == 1) {
            if (int rc = launch_update(c, xo, xn, d_feedback, st)) return rc;
            if (int rc = timer.stamp(1)) return rc;
            launch_readout<kReadFull>(c, xn, d_local_model, d_outvec, st);
            SML_HIP(hipGetLastError());
        } else {
            if (int rc = launch_update_mem(c, xo, xn, d_feedback, fb_stride, st)) return rc;
            if (int rc = timer.stamp(1)) return rc;
            if (int rc = launch_readout_mem<kReadFull>(c, xn, d_local_model, lm_stride, d_outvec, ov_stride, st)) return rc;
        }
        return timer.stamp(2);
    });
}

// sml_res_synchronize for every member: block t of member e at d_inputs + t * stride +
// e * member_stride doubles
extern "C" int sml_res_synchronize_members(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride,
                                           int64_t member_stride, void *stream) {
    SML_REQUIRE(c && length >= 0, "bad argument");
    if (c->nlocal == 0 || length == 0) return SML_OK;
    SML_REQUIRE(d_inputs && stride >= (int64_t)c->tot_fb, "stride smaller than the packed feedback size");
    SML_REQUIRE(c->members == 1 || member_stride >= (int64_t)c->tot_fb,
                "member_stride smaller than the packed feedback size");
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_synchronize_members inside a begun step");
    if (int rc = check_loaded(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for (int t = 0; t < length; ++t) {
        const double *u = d_inputs + (size_t)t * stride;
        if (int rc = c->advance(false, [&](const double *xo, double *xn) {
                return c->members == 1 ? launch_update(c, xo, xn, u, st)
                                       : launch_update_mem(c, xo, xn, u, member_stride, st);
            }))
            return rc;
    }
    return SML_OK;
}

// ---- the split step for every member (sml_res_members.hpp): sml_res_step_begin_members
// updates every member and leaves every member's v_ml in c->d_part; the three finishes add
// each member's v_p.  At one member they are the single-member calls.
namespace {
int check_fb_stride(const sml_reservoirs *c, int64_t fb_stride) {
    SML_REQUIRE(fb_stride >= c->tot_fb, "fb_stride %lld smaller than the packed feedback size %lld",
                (long long)fb_stride, (long long)c->tot_fb);
    return SML_OK;
}
int check_lm_ov_strides(const sml_reservoirs *c, int64_t lm_stride, int64_t ov_stride) {
    SML_REQUIRE(c->ncs == 0 || lm_stride >= (int64_t)c->nlocal * c->ncs,
                "lm_stride %lld smaller than nlocal * chunk_speedy", (long long)lm_stride);
    SML_REQUIRE(ov_stride >= (int64_t)c->nlocal * c->ov_ld, "ov_stride %lld smaller than nlocal * the outvec row stride",
                (long long)ov_stride);
    return SML_OK;
}

// the grid finishes' common part; on success the step is closed
template <bool kAsm>
int finish_grid_members(sml_reservoirs *c, const char *what, const double *d_fc4d, int64_t fc4_stride,
                        const double *d_fc2d, int64_t fc2_stride, double *d_local_model, int64_t lm_stride,
                        double *d_outvec, int64_t ov_stride, double *d_grid4d, int64_t g4_stride, double *d_grid2d,
                        double *d_precip, int64_t g2_stride, void *stream) {
    SML_REQUIRE(c, "null context");
    if (kAsm)
        SML_REQUIRE(sml::res_in_global_order(c), "the fused assembly needs every region on this rank, in global order");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_outvec && (c->ncs == 0 || (d_fc4d && d_fc2d)), "null device buffer");
    SML_REQUIRE(!kAsm || (d_grid4d && d_grid2d && d_precip), "null device buffer");
    SML_REQUIRE(!c->generic || c->ncs == 0, "a generic (slab) context has no local-model tiling");
    SML_REQUIRE(c->ncs <= kMaxNcs, "ncs %d exceeds %d", c->ncs, kMaxNcs);
    SML_REQUIRE(c->ncs == 0 || fc4_stride >= kGrid4d, "fc4_stride %lld smaller than the 4-d grid's %d doubles",
                (long long)fc4_stride, kGrid4d);
    SML_REQUIRE(c->ncs == 0 || fc2_stride >= kGrid2d, "fc2_stride %lld smaller than the 2-d grid's %d doubles",
                (long long)fc2_stride, kGrid2d);
    if (int rc = check_lm_ov_strides(c, d_local_model ? lm_stride : (int64_t)c->nlocal * c->ncs, ov_stride)) return rc;
    if (kAsm) {
        SML_REQUIRE(g4_stride >= kGrid4d, "g4_stride %lld smaller than the 4-d grid's %d doubles", (long long)g4_stride,
                    kGrid4d);
        SML_REQUIRE(g2_stride >= kGrid2d, "g2_stride %lld smaller than the 2-d grid's %d doubles", (long long)g2_stride,
                    kGrid2d);
    }
    if (!c->is_begun()) return fail(SML_ERR_STATE, "%s without sml_res_step_begin_members", what);
    hipStream_t st = (hipStream_t)stream;
    if (c->members == 1) {  // the single-member kernel itself
        launch_finish_grid<kAsm>(c, d_fc4d, d_fc2d, d_local_model, d_outvec, d_grid4d, d_grid2d, d_precip, st);
        SML_HIP(hipGetLastError());
    } else {
        const FinMemArgs a{c->members, c->mfin.tile, c->mfin.tiles, fc4_stride, fc2_stride, lm_stride, ov_stride,
                           part_stride(c), g4_stride, g2_stride};
        if (int rc = launch_finish_grid_mem<kAsm>(c, d_fc4d, d_fc2d, d_local_model, d_outvec, d_grid4d, d_grid2d,
                                                  d_precip, a, st))
            return rc;
    }
    c->close();
    return SML_OK;
}
}  // namespace

extern "C" int sml_res_step_begin_members(sml_reservoirs *c, const double *d_feedback, int64_t fb_stride,
                                          void *stream) {
    SML_REQUIRE(c, "null context");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_feedback, "null device buffer");
    if (int rc = check_fb_stride(c, fb_stride)) return rc;
    if (c->is_begun())
        return fail(SML_ERR_STATE, "sml_res_step_begin_members called twice without a members finish");
    if (int rc = check_loaded(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (c->members == 1) return begin_single(c, d_feedback, st);  // sml_res_step_begin's kernels, the fused begin too
    // two launches; one swap covers all members (and one roll-back: sml_res_step_cancel)
    return c->advance(true, [&](const double *xo, double *xn) {
        StepTimer timer(c, st);
        if (int rc = timer.stamp(0)) return rc;
        if (int rc = launch_update_mem(c, xo, xn, d_feedback, fb_stride, st)) return rc;
        if (int rc = timer.stamp(1)) return rc;
        if (int rc = launch_readout_mem<kReadML>(c, xn, nullptr, 0, nullptr, 0, st)) return rc;
        return timer.stamp(2);
    });
}

extern "C" int sml_res_step_finish_members(sml_reservoirs *c, const double *d_local_model, int64_t lm_stride,
                                           double *d_outvec, int64_t ov_stride, void *stream) {
    SML_REQUIRE(c, "null context");
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(d_outvec, "null device buffer");
    SML_REQUIRE(c->ncs == 0 || d_local_model, "hybrid context needs d_local_model");
    if (int rc = check_lm_ov_strides(c, lm_stride, ov_stride)) return rc;
    if (!c->is_begun()) return fail(SML_ERR_STATE, "sml_res_step_finish_members without sml_res_step_begin_members");
    hipStream_t st = (hipStream_t)stream;
    if (c->ncs == 0) {
        d_local_model = nullptr;
        lm_stride = 0;
    }
    if (c->members == 1) {
        launch_readout<kReadFinish>(c, nullptr, d_local_model, d_outvec, st);
        SML_HIP(hipGetLastError());
    } else if (int rc = launch_finish_mem(c, d_local_model, lm_stride, d_outvec, ov_stride, st)) {
        return rc;
    }
    c->close();
    return SML_OK;
}

extern "C" int sml_res_step_finish_grid_members(sml_reservoirs *c, const double *d_fc4d, int64_t fc4_stride,
                                                const double *d_fc2d, int64_t fc2_stride, double *d_local_model,
                                                int64_t lm_stride, double *d_outvec, int64_t ov_stride,
                                                void *stream) {
    return finish_grid_members<false>(c, "sml_res_step_finish_grid_members", d_fc4d, fc4_stride, d_fc2d, fc2_stride,
                                      d_local_model, lm_stride, d_outvec, ov_stride, nullptr, 0, nullptr, nullptr, 0,
                                      stream);
}

extern "C" int sml_res_step_finish_assemble_members(sml_reservoirs *c, const double *d_fc4d, int64_t fc4_stride,
                                                    const double *d_fc2d, int64_t fc2_stride, double *d_local_model,
                                                    int64_t lm_stride, double *d_outvec, int64_t ov_stride,
                                                    double *d_grid4d, int64_t g4_stride, double *d_grid2d,
                                                    double *d_precip, int64_t g2_stride, void *stream) {
    return finish_grid_members<true>(c, "sml_res_step_finish_assemble_members", d_fc4d, fc4_stride, d_fc2d,
                                     fc2_stride, d_local_model, lm_stride, d_outvec, ov_stride, d_grid4d, g4_stride,
                                     d_grid2d, d_precip, g2_stride, stream);
}

// the members one block of the grid finish serves (member_finish; 1 at members > 1: the
// single-member kernel once per member)
extern "C" int sml_res_member_finish_tile(const sml_reservoirs *c, int *finish_tile) {
    SML_REQUIRE(c && finish_tile, "null argument");
    *finish_tile = c->mfin.tile;
    return SML_OK;
}

// a measurement's choice of that tile (tools/probe_members_split.py; not in the public
// header): 0 the build's, 1 the looped single-member kernel, 2 .. kFinTileMax
extern "C" int sml_res_dbg_set_finish_tile(sml_reservoirs *c, int tile) {
    SML_REQUIRE(c && tile >= 0 && tile <= kFinTileMax, "bad argument");
    c->fin_tile_want = tile;
    reshape(c);
    return SML_OK;
}

// the training drive (k_res_drive): "record, then advance" over one batch of m
// columns for every local region.  Stream-ordered, no host synchronisation.
// d_tin: the series the targets are read from (sml_res_train_drive_from), or NULL: the
// driving series' own blocks, as each kernel holds them.
namespace {

int train_drive(sml_reservoirs *c, const char *what, const double *d_inputs, int m, int64_t stride,
                const double *d_tin, int64_t tstride, const double *d_model, int64_t model_stride, double *d_states,
                double *d_targets, void *stream) {
    SML_REQUIRE(c && m >= 0, "bad argument");
    if (int rc = check_single(c, what)) return rc;
    if (c->nlocal == 0 || m == 0) return SML_OK;
    SML_REQUIRE(d_inputs && stride >= (int64_t)c->tot_fb, "stride smaller than the packed feedback size");
    SML_REQUIRE(d_states, "null device buffer");
    SML_REQUIRE(c->ncs == 0 || (d_model && model_stride >= (int64_t)c->nlocal * c->ncs),
                "model_stride smaller than nlocal * chunk_speedy (or d_model null)");
    // (a generic context has a target table once sml_res_set_target_index has given it one)
    SML_REQUIRE(!d_targets || !c->generic || c->d_tgt_idx,
                "a generic (slab) context has no target geometry: d_targets must be NULL");
    if (c->is_begun()) return fail(SML_ERR_STATE, "%s inside a begun step", what);
    if (int rc = check_loaded(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (c->ncs == 0) {
        d_model = nullptr;
        model_stride = 0;
    }
    const StepShape &s = c->shape;
    if (!s.drive_fused) {
        const int chunks = (c->ncs + c->maxn + 255) / 256;
        for (int t = 0; t < m; ++t) {
            const double *u = d_inputs + (size_t)t * stride;
            const double *tu = d_tin ? d_tin + (size_t)t * tstride : u;
            if (int rc = c->advance(false, [&](const double *xo, double *xn) {
                    hipLaunchKernelGGL(k_drive_record, dim3(c->nlocal, chunks), dim3(256), 0, st, c->d_rd, c->d_row0,
                                       xo, tu, d_model + (size_t)t * model_stride, c->d_tgt_idx, d_states, d_targets,
                                       t, m, c->ncs, c->nout);
                    return launch_update(c, xo, xn, u, st);
                }))
                return rc;
        }
        SML_HIP(hipGetLastError());
        return SML_OK;
    }
    const Ell ell = make_ell(c);
    return c->advance(false, [&](const double *xo, double *xn) {
        with_wt(c, [&](auto tag) {
            using WT = decltype(tag);
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(c->nlocal), dim3(kUpdThreads), s.lds_drive, st, c->d_rd, c->d_row0,
                                   c->d_a_rp, c->d_a_col, (const WT *)c->d_a_val, c->d_w_rp, c->d_w_col,
                                   (const WT *)c->d_w_val, ell, xo, xn, d_inputs, stride, d_tin, tstride, d_model,
                                   model_stride, c->d_tgt_idx, d_states, d_targets, m, c->ncs, c->nout, c->leakage,
                                   s.lds_x, c->maxninp);
            };
            if (d_tin && d_targets)
                launch(k_res_drive<WT, true>);
            else
                launch(k_res_drive<WT, false>);
        });
        SML_HIP(hipGetLastError());
        return (int)SML_OK;
    });
}

}  // namespace

extern "C" int sml_res_train_drive(sml_reservoirs *c, const double *d_inputs, int m, int64_t stride,
                                   const double *d_model, int64_t model_stride, double *d_states,
                                   double *d_targets, void *stream) {
    return train_drive(c, "sml_res_train_drive", d_inputs, m, stride, nullptr, 0, d_model, model_stride, d_states,
                       d_targets, stream);
}

// sml_res_train_drive with column c's targets read from d_target_inputs + c * target_stride
// (global memory), the states driven by d_inputs: the clean series beside the noised one
extern "C" int sml_res_train_drive_from(sml_reservoirs *c, const double *d_inputs, int m, int64_t stride,
                                        const double *d_target_inputs, int64_t target_stride, const double *d_model,
                                        int64_t model_stride, double *d_states, double *d_targets, void *stream) {
    SML_REQUIRE(c && m >= 0, "bad argument");
    if (c->nlocal && m && d_targets) {
        SML_REQUIRE(d_target_inputs, "sml_res_train_drive_from: d_target_inputs is null");
        SML_REQUIRE(target_stride >= (int64_t)c->tot_fb,
                    "sml_res_train_drive_from: target_stride %lld smaller than the packed feedback size %lld",
                    (long long)target_stride, (long long)c->tot_fb);
    } else {
        d_target_inputs = nullptr;  // nothing reads it
    }
    return train_drive(c, "sml_res_train_drive_from", d_inputs, m, stride, d_target_inputs, target_stride, d_model,
                       model_stride, d_states, d_targets, stream);
}

// the targets of a generic context (the slab: sml_slab_target_index): the table the two
// drive forms gather u_c[idx] through, which the geometry gives every other context.
// Every index is checked before anything changes; the upload waits for the device, since
// a drive in flight may read the table it replaces.
extern "C" int sml_res_set_target_index(sml_reservoirs *c, const int32_t *idx) {
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(idx, "idx is null");
    SML_REQUIRE(c->generic, "sml_res_set_target_index on a context with a geometry: its table stays the only one");
    SML_REQUIRE(c->members == 1, "sml_res_set_target_index on a context of %d members", c->members);
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_set_target_index inside a begun step");
    for (int i = 0; i < c->nlocal; ++i)
        for (int o = 0; o < c->nout; ++o) {
            const int32_t v = idx[(size_t)i * c->nout + o];
            SML_REQUIRE(v >= 0 && v < c->ninp[i], "target index %d of local region %d, output %d: outside [0, %d)", v, i,
                        o, c->ninp[i]);
        }
    if (!c->nlocal) return SML_OK;
    if (!c->d_tgt_idx)
        if (int rc = pool(c, &c->d_tgt_idx, (int64_t)c->nlocal * c->nout)) return rc;
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(c->d_tgt_idx, idx, (size_t)c->nlocal * c->nout * sizeof(int32_t), hipMemcpyHostToDevice));
    return SML_OK;
}

// the spectral radius of every local region's A (k_res_radius): one launch, then
// the host waits for the stream -- a set-up call, not part of the step
extern "C" int sml_res_spectral_radius(sml_reservoirs *c, double tol, int max_iter, double *lo, double *hi,
                                       int *iters, int *info, void *stream) {
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(tol > 0.0, "sml_res_spectral_radius: tol must be positive");  // (a NaN fails it too)
    SML_REQUIRE(max_iter >= 1, "sml_res_spectral_radius: max_iter = %d < 1", max_iter);
    if (c->nlocal == 0) return SML_OK;
    SML_REQUIRE(lo && hi && iters && info, "sml_res_spectral_radius: null output array");
    if (int rc = check_loaded(c)) return rc;
    // x and y of a region in LDS where they fit (and the scratch is not forced); the
    // kernel keeps no static LDS, but what the compiler reports is taken off the limit
    hipFuncAttributes fa;
    SML_HIP(with_wt(c, [&](auto tag) {
        return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_res_radius<decltype(tag)>));
    }));
    const size_t lds_limit = c->radius_global || fa.sharedSizeBytes > c->max_lds ? 0 : c->max_lds - fa.sharedSizeBytes;
    size_t lds = 0;
    bool scratch = false;
    for (int i = 0; i < c->nlocal; ++i) {
        const size_t b = 2 * (size_t)c->n[i] * sizeof(double);
        if (b <= lds_limit)
            lds = std::max(lds, b);
        else
            scratch = true;
    }
    if (!c->d_rad_out) {  // the partials and the results: both or neither
        pool(c, &c->d_rad_part, (int64_t)c->nlocal * 3 * kRadWaves);
        if (int rc = pool(c, &c->d_rad_out, c->nlocal)) {
            c->mem.release(&c->d_rad_part);
            return rc;
        }
    }
    if (scratch && !c->d_rad_xy)
        if (int rc = pool(c, &c->d_rad_xy, 2 * (int64_t)c->row0_h[c->nlocal])) return rc;
    hipStream_t st = (hipStream_t)stream;
    with_wt(c, [&](auto tag) {
        using WT = decltype(tag);
        hipLaunchKernelGGL(k_res_radius<WT>, dim3(c->nlocal), dim3(kUpdThreads), lds, st, c->d_rd, c->d_row0,
                           c->d_a_rp, c->d_a_col, (const WT *)c->d_a_val, c->d_rad_xy, c->d_rad_part, c->d_rad_out, tol,
                           max_iter, lds_limit);
    });
    SML_HIP(hipGetLastError());
    SML_HIP(hipStreamSynchronize(st));
    std::vector<RadiusOut> out(c->nlocal);
    SML_HIP(hipMemcpy(out.data(), c->d_rad_out, out.size() * sizeof(RadiusOut), hipMemcpyDeviceToHost));
    for (int i = 0; i < c->nlocal; ++i) {
        lo[i] = out[i].lo;
        hi[i] = out[i].hi;
        iters[i] = out[i].iters;
        info[i] = out[i].info;
    }
    return SML_OK;
}

// start_prediction (src/mod_reservoir.f90:938-959): synchronize_print (:1381-1414,
// the same update loop as synchronize) over the first `length` input blocks, then
// the next block becomes the feedback (reservoir%feedback = predictiondata(:, L+1))
extern "C" int sml_res_start_prediction(sml_reservoirs *c, const double *d_inputs, int length, int64_t stride,
                                        double *d_feedback, void *stream) {
    SML_REQUIRE(c && d_inputs && d_feedback && length >= 0, "bad argument");
    if (int rc = check_single(c, "sml_res_start_prediction")) return rc;
    if (int rc = sml_res_synchronize(c, d_inputs, length, stride, stream)) return rc;
    if (c->tot_fb)
        SML_HIP(hipMemcpyAsync(d_feedback, d_inputs + (size_t)length * stride, (size_t)c->tot_fb * 8,
                               hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SML_OK;
}

extern "C" int sml_res_step_host(sml_reservoirs *c, const double *feedback, const double *local_model,
                                 double *outvec) {
    SML_REQUIRE(c && feedback && outvec, "null argument");
    SML_REQUIRE(c->ncs == 0 || local_model, "hybrid context needs local_model");
    if (int rc = check_single(c, "sml_res_step_host")) return rc;
    const size_t nfb = c->tot_fb, nlm = (size_t)c->nlocal * c->ncs, nov = (size_t)c->nlocal * c->ov_ld;
    if (c->d_io_n != nfb + nlm + nov) {  // sized for the current outvec stride
        c->mem.release(&c->d_io);
        c->d_io_n = 0;
        if (int rc = pool(c, &c->d_io, (int64_t)(nfb + nlm + nov))) return rc;
        c->d_io_n = nfb + nlm + nov;
    }
    double *dfb = c->d_io, *dlm = dfb + nfb, *dov = dlm + nlm;
    SML_HIP(hipMemcpy(dfb, feedback, nfb * 8, hipMemcpyHostToDevice));
    if (nlm) SML_HIP(hipMemcpy(dlm, local_model, nlm * 8, hipMemcpyHostToDevice));
    if (int rc = sml_res_step(c, dfb, dlm, dov, nullptr)) return rc;
    SML_HIP(hipMemcpy2D(outvec, (size_t)c->nout * 8, dov, (size_t)c->ov_ld * 8, (size_t)c->nout * 8, c->nlocal,
                        hipMemcpyDeviceToHost));
    return SML_OK;
}

extern "C" int sml_res_footprint(const sml_reservoirs *c, int64_t *weight_bytes, int64_t *algo_bytes) {
    SML_REQUIRE(c, "null context");
    footprint(c->nlocal, c->n.data(), c->k.data(), c->ninp.data(), c->ncs, c->nout, (int64_t)wbytes(c), weight_bytes,
              algo_bytes);
    return SML_OK;
}

extern "C" int sml_exchange_assemble(sml_reservoirs *c, const double *d_outvec_all, double *d_grid4d,
                                     double *d_grid2d, double *d_precip, void *stream) {
    SML_REQUIRE(c && d_outvec_all && d_grid4d && d_grid2d && d_precip, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    const int total = c->numregions * c->nout;
    hipLaunchKernelGGL(k_assemble, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->d_asm_dst,
                       d_outvec_all, d_grid4d, d_grid2d, d_precip, total, c->nout, c->ov_ld);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_res_tile_feedback(sml_reservoirs *c, const double *d_grid4d, const double *d_grid2d,
                                     const double *d_precip, const double *d_tisr, double *d_feedback, void *stream) {
    SML_REQUIRE(c && d_grid4d && d_grid2d && d_precip && d_feedback, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    if (c->tot_fb) {
        const int total = (int)c->tot_fb;
        hipLaunchKernelGGL(k_tile_feedback, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream, c->d_fb_src,
                           c->d_fb_l, c->d_fb_reg, c->d_meanstd, d_grid4d, d_grid2d, d_precip, d_tisr, d_feedback,
                           total);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

extern "C" int sml_res_tile_tisr_field(sml_reservoirs *c, const double *d_tisr_grid, double *d_feedback,
                                       void *stream) {
    SML_REQUIRE(c && d_tisr_grid && d_feedback, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    if (c->tot_tisr) {
        hipLaunchKernelGGL(k_tile_tisr, dim3((c->tot_tisr + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                           c->d_tisr_fb, c->d_tisr_grid, c->d_tisr_reg, c->d_meanstd, d_tisr_grid, d_feedback,
                           c->tot_tisr);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

// the two feedback tilings for every member of the context, one launch each (at one member:
// the single-member calls)
extern "C" int sml_res_tile_feedback_members(sml_reservoirs *c, const double *d_grid4d, int64_t g4_stride,
                                             const double *d_grid2d, const double *d_precip, int64_t g2_stride,
                                             const double *d_tisr, double *d_feedback, int64_t fb_stride,
                                             void *stream) {
    SML_REQUIRE(c && d_grid4d && d_grid2d && d_precip && d_feedback, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    SML_REQUIRE(g4_stride >= kGrid4d, "g4_stride %lld smaller than the 4-d grid's %d doubles", (long long)g4_stride,
                kGrid4d);
    SML_REQUIRE(g2_stride >= kGrid2d, "g2_stride %lld smaller than the 2-d grid's %d doubles", (long long)g2_stride,
                kGrid2d);
    if (int rc = check_fb_stride(c, fb_stride)) return rc;
    if (c->members == 1) return sml_res_tile_feedback(c, d_grid4d, d_grid2d, d_precip, d_tisr, d_feedback, stream);
    if (c->tot_fb) {
        const int total = (int)c->tot_fb;
        hipLaunchKernelGGL(k_tile_feedback_mem, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                           c->d_fb_src, c->d_fb_l, c->d_fb_reg, c->d_meanstd, d_grid4d, d_grid2d, d_precip, d_tisr,
                           d_feedback, total, c->members, g4_stride, g2_stride, fb_stride);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

extern "C" int sml_res_tile_tisr_field_members(sml_reservoirs *c, const double *d_tisr_grid, double *d_feedback,
                                               int64_t fb_stride, void *stream) {
    SML_REQUIRE(c && d_tisr_grid && d_feedback, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    if (int rc = check_fb_stride(c, fb_stride)) return rc;
    if (c->members == 1) return sml_res_tile_tisr_field(c, d_tisr_grid, d_feedback, stream);
    if (c->tot_tisr) {
        hipLaunchKernelGGL(k_tile_tisr_mem, dim3((c->tot_tisr + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                           c->d_tisr_fb, c->d_tisr_grid, c->d_tisr_reg, c->d_meanstd, d_tisr_grid, d_feedback,
                           c->tot_tisr, c->members, fb_stride);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

extern "C" int sml_res_tile_local_model(sml_reservoirs *c, const double *d_fc4d, const double *d_fc2d,
                                        double *d_local_model, void *stream) {
    SML_REQUIRE(c && d_fc4d && d_fc2d && d_local_model, "null argument");
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    if (c->ncs && c->nlocal) {
        const int total = c->nlocal * c->ncs;
        hipLaunchKernelGGL(k_tile_local_model, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                           c->d_lm_src, c->d_lm_l, c->d_meanstd, d_fc4d, d_fc2d, d_local_model, c->ncs, total);
        SML_HIP(hipGetLastError());
    }
    return SML_OK;
}

extern "C" int sml_res_tile_inputs(sml_reservoirs *c, const double *d_grid4d, const double *d_grid2d,
                                   const double *d_precip, const double *d_fc4d, const double *d_fc2d,
                                   const double *d_tisr, double *d_feedback, double *d_local_model, void *stream) {
    if (int rc = sml_res_tile_feedback(c, d_grid4d, d_grid2d, d_precip, d_tisr, d_feedback, stream)) return rc;
    if (c->ncs && d_fc4d && c->nlocal) return sml_res_tile_local_model(c, d_fc4d, d_fc2d, d_local_model, stream);
    return SML_OK;
}

// ---------------------------------------------------------------- series of grids
namespace {

// the series calls' tables, at the first of them (ordered before every launch: synchronous uploads)
int ensure_series_tables(sml_reservoirs *c) {
    if (c->d_ser_src) return SML_OK;
    const TablesIn in{c->numregions, c->nlocal, c->ncs, c->nout, c->geom.data(), c->sst.data(), c->ninp.data(),
                      c->rd.data(), c->tot_fb, nullptr};
    SeriesTables t;
    if (int rc = build_series_tables(in, &t)) return rc;
    auto mk = [c](auto **d, const auto &v) {
        const int rc = pool(c, d, (int64_t)v.size());
        return rc ? rc : upload(*d, v);
    };
    int rc;
    if ((rc = mk(&c->d_ser_l, t.l)) || (rc = mk(&c->d_ser_pt_off, t.pt_off)) ||
        (rc = mk(&c->d_ser_pt_grid, t.pt_grid)) || (rc = mk(&c->d_ser_sst, c->sst)) || (rc = mk(&c->d_ser_src, t.src)))
        return rc;
    return SML_OK;
}

// what the two series calls check of their common arguments, before anything is enqueued
int check_series_args(const sml_reservoirs *c, const double *d_g4, int64_t g4_stride, const double *d_g2,
                      const double *d_pr, int64_t g2_stride, int T) {
    SML_REQUIRE(T >= 1, "T = %d: a series holds one step at least", T);
    SML_REQUIRE(g4_stride >= kGrid4d, "g4_stride %lld smaller than the 4-d grid's %d doubles", (long long)g4_stride,
                kGrid4d);
    SML_REQUIRE(g2_stride >= kGrid2d, "g2_stride %lld smaller than a 2-d grid's %d doubles", (long long)g2_stride,
                kGrid2d);
    SML_REQUIRE(g4_stride % 2 == 0, "g4_stride %lld is odd: every step's 4-d grid must be 16-byte aligned",
                (long long)g4_stride);
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(d_g4 && d_g2 && d_pr, "null argument (d_g4, d_g2 and d_pr are needed)");
    SML_REQUIRE((uintptr_t)d_g4 % 16 == 0, "d_g4 %p is not 16-byte aligned", (const void *)d_g4);
    SML_REQUIRE(!c->generic, "a generic (slab) context has no exchange tables");
    return SML_OK;
}

}  // namespace

extern "C" int sml_res_series_stats(sml_reservoirs *c, const double *d_g4, int64_t g4_stride, const double *d_g2,
                                    const double *d_pr, const double *d_sst, const double *d_tisr,
                                    int64_t g2_stride, int T, double *d_meanstd, int *d_sst_change, void *stream) {
    if (int rc = check_series_args(c, d_g4, g4_stride, d_g2, d_pr, g2_stride, T)) return rc;
    SML_REQUIRE(d_meanstd, "d_meanstd is null");
    bool any_sst = false;
    for (int i = 0; i < c->nlocal; ++i) any_sst = any_sst || c->sst[i];
    SML_REQUIRE(d_sst || !any_sst, "d_sst is null on a context with sst regions");
    if (!c->nlocal) return SML_OK;
    if (int rc = ensure_series_tables(c)) return rc;
    if (!c->d_ser_work)
        if (int rc = pool(c, &c->d_ser_work, (int64_t)(2 * kSerSplitMax + 1) * kSerPoints)) return rc;
    const SeriesSplit sp = series_split(T);
    const SeriesIn in{d_g4, {d_g2, d_pr, any_sst ? d_sst : nullptr, d_tisr}, g4_stride, g2_stride};
    const SeriesWork w{c->d_ser_work, c->d_ser_work + (size_t)kSerSplitMax * kSerPoints,
                       c->d_ser_work + (size_t)(kSerSplitMax + 1) * kSerPoints};
    const dim3 grid(kSerQuadBlocks + kSerFields2d * kSerPointBlocks, sp.S);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_series_sum, grid, dim3(kSerThreads), 0, st, in, w, T, sp.len);
    hipLaunchKernelGGL(k_series_m2, grid, dim3(kSerThreads), 0, st, in, w, T, sp.len, sp.S);
    const int total = c->nlocal * kMeanStd;
    hipLaunchKernelGGL(k_series_combine, dim3((total + 63) / 64), dim3(64), 0, st, c->d_ser_pt_off, c->d_ser_pt_grid,
                       c->d_ser_sst, w, any_sst ? 1 : 0, d_tisr ? 1 : 0, T, sp.S, c->nlocal, d_meanstd, d_sst_change);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

extern "C" int sml_res_set_mean_std_device(sml_reservoirs *c, const double *d_meanstd, void *stream) {
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(d_meanstd, "d_meanstd is null");
    SML_REQUIRE(!c->is_begun(), "sml_res_set_mean_std_device inside a begun step");
    SML_REQUIRE(c->members == 1, "sml_res_set_mean_std_device on a context of %d members", c->members);
    if (!c->nlocal) return SML_OK;
    const size_t bytes = (size_t)c->nlocal * 2 * kMeanStd * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    SML_HIP(hipMemcpyAsync(c->d_meanstd, d_meanstd, bytes, hipMemcpyDeviceToDevice, st));
    SML_HIP(hipMemcpyAsync(c->meanstd_h.data(), d_meanstd, bytes, hipMemcpyDeviceToHost, st));
    SML_HIP(hipStreamSynchronize(st));
    return SML_OK;
}

extern "C" int sml_res_tile_series(sml_reservoirs *c, const double *d_g4, int64_t g4_stride, const double *d_g2,
                                   const double *d_pr, const double *d_sst, const double *d_tisr, int64_t g2_stride,
                                   const double *d_fc4, int64_t fc4_stride, const double *d_fc2, int64_t fc2_stride,
                                   int T, double *d_inputs, int64_t in_stride, double *d_model,
                                   int64_t model_stride, void *stream) {
    if (int rc = check_series_args(c, d_g4, g4_stride, d_g2, d_pr, g2_stride, T)) return rc;
    SML_REQUIRE(d_inputs, "d_inputs is null");
    SML_REQUIRE(in_stride >= c->tot_fb, "in_stride %lld smaller than the packed feedback's %lld doubles",
                (long long)in_stride, (long long)c->tot_fb);
    const int nmod = (d_fc4 ? 1 : 0) + (d_fc2 ? 1 : 0) + (d_model ? 1 : 0);
    SML_REQUIRE(nmod == 0 || nmod == 3, "d_fc4, d_fc2 and d_model are given together or not at all");
    SML_REQUIRE(nmod == 0 || c->ncs > 0, "model blocks on a context with chunk_speedy 0");
    if (nmod) {
        SML_REQUIRE(fc4_stride >= kGrid4d, "fc4_stride %lld smaller than the 4-d grid's %d doubles",
                    (long long)fc4_stride, kGrid4d);
        SML_REQUIRE(fc2_stride >= kGrid2d, "fc2_stride %lld smaller than a 2-d grid's %d doubles",
                    (long long)fc2_stride, kGrid2d);
        SML_REQUIRE(model_stride >= (int64_t)c->nlocal * c->ncs,
                    "model_stride %lld smaller than the packed model block's %lld doubles", (long long)model_stride,
                    (long long)c->nlocal * c->ncs);
    }
    if (!c->nlocal) return SML_OK;
    if (int rc = ensure_series_tables(c)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (c->tot_fb) {
        const SeriesIn in{d_g4, {d_g2, d_pr, d_sst, d_tisr}, g4_stride, g2_stride};
        const int total = (int)c->tot_fb;
        hipLaunchKernelGGL(k_tile_series, dim3((total + 255) / 256), dim3(256), 0, st, c->d_ser_src, c->d_ser_l,
                           c->d_fb_reg, c->d_meanstd, in, d_inputs, in_stride, total, T);
    }
    if (nmod) {
        const int total = c->nlocal * c->ncs;
        hipLaunchKernelGGL(k_tile_series_model, dim3((total + 255) / 256), dim3(256), 0, st, c->d_lm_src, c->d_lm_l,
                           c->d_meanstd, d_fc4, fc4_stride, d_fc2, fc2_stride, d_model, model_stride, c->ncs, total,
                           T);
    }
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// the slab training series' view of the atmo context (sml_internal.hpp)
int sml::res_slab_series(sml_reservoirs *c, const SlabLayoutIn &in, SlabSeriesDev *out) {
    SML_REQUIRE(c && out, "null argument");
    SML_REQUIRE(!c->generic, "the atmo context is generic: a generic (slab) context has no exchange tables");
    SML_REQUIRE(c->members == 1, "sml_slab_train_series on an atmo context of %d members", c->members);
    if (c->sls_tot < 0) {
        const TablesIn tin{c->numregions, c->nlocal, c->ncs, c->nout, c->geom.data(), c->sst.data(), c->ninp.data(),
                           c->rd.data(), c->tot_fb, nullptr};
        SeriesTables ser;
        if (int rc = build_series_tables(tin, &ser)) return rc;
        SlabSeriesTables t;
        if (int rc = build_slab_series_tables(in, ser.src.data(), ser.l.data(), (int64_t)ser.src.size(), &t)) return rc;
        auto mk = [c](auto **d, const auto &v) {
            const int rc = pool(c, d, (int64_t)v.size());
            return rc ? rc : upload(*d, v);
        };
        int rc;
        if ((rc = mk(&c->d_sls_src, t.src)) || (rc = mk(&c->d_sls_l, t.l)) || (rc = mk(&c->d_sls_row, t.row))) {
            c->mem.release(&c->d_sls_src);
            c->mem.release(&c->d_sls_l);
            c->mem.release(&c->d_sls_row);
            return rc;
        }
        c->sls_tot = (int)t.src.size();
    } else {  // the table is the atmo context's alone; the slab context is checked at every call
        SlabTables tb;
        if (int rc = build_slab_tables(in, &tb)) return rc;
    }
    *out = {c->d_sls_src, c->d_sls_l, c->d_sls_row, c->d_meanstd, c->sls_tot};
    return SML_OK;
}

// ---------------------------------------------------------------- input noise
// The configuration of sml_res_input_noise.  ids [nlocal] (host) or NULL:
// the regions' noise ids -- the context's region ids, the local index on a generic context.
// The tables are the context's from the first call on; a later call replaces their contents
// after waiting for the device (a launch in flight may read them).
extern "C" int sml_res_set_input_noise(sml_reservoirs *c, double noisemag, uint64_t seed, double precip_epsilon,
                                       const int32_t *ids) {
    SML_REQUIRE(std::isfinite(noisemag) && noisemag >= 0.0, "sml_res_set_input_noise: noisemag = %g is negative or not finite",
                noisemag);
    SML_REQUIRE(std::isfinite(precip_epsilon) && precip_epsilon >= 0.0,
                "sml_res_set_input_noise: precip_epsilon = %g is negative or not finite", precip_epsilon);
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(c->members == 1, "sml_res_set_input_noise on a context of %d members", c->members);
    if (c->is_begun()) return fail(SML_ERR_STATE, "sml_res_set_input_noise inside a begun step");
    std::vector<uint64_t> key(2 * (size_t)c->nlocal);
    for (int i = 0; i < c->nlocal; ++i) {
        const int id = ids ? ids[i] : c->generic ? i : c->region_ids[i];
        SML_REQUIRE(id >= 0, "sml_res_set_input_noise: noise id %d of local region %d is negative", id, i);
        SML_REQUIRE(c->ninp[i] < kNoiseEntryMax, "sml_res_set_input_noise: local region %d has ninp = %d >= 2^20", i,
                    c->ninp[i]);
        key[2 * i] = stream_key(seed, id, kNoiseStreamU1);
        key[2 * i + 1] = stream_key(seed, id, kNoiseStreamU2);
    }
    if (c->nlocal) {
        // the precip branch reads the series tables' slots: a context with a geometry only
        if (precip_epsilon > 0.0 && !c->generic)
            if (int rc = ensure_series_tables(c)) return rc;
        if (c->generic && !c->d_nz_reg) {
            std::vector<uint16_t> reg((size_t)c->tot_fb);
            for (int i = 0; i < c->nlocal; ++i)
                for (int j = 0; j < c->ninp[i]; ++j) reg[(size_t)c->rd[i].fb + j] = (uint16_t)i;
            if (int rc = pool(c, &c->d_nz_reg, (int64_t)reg.size())) return rc;
            if (int rc = upload(c->d_nz_reg, reg)) return rc;
        }
        if (!c->d_nz_key)
            if (int rc = pool(c, &c->d_nz_key, (int64_t)key.size())) return rc;
        SML_HIP(hipDeviceSynchronize());
        if (int rc = upload(c->d_nz_key, key)) return rc;
    }
    c->noise_mag = noisemag;
    c->noise_eps = precip_epsilon;
    c->noise_set = true;
    return SML_OK;
}

// blocks t0 .. t0 + m - 1 of the packed feedback layout, noised (k_input_noise): block j read
// at d_in + j * in_stride, written at d_out + j * out_stride.  Stream-ordered.
extern "C" int sml_res_input_noise(sml_reservoirs *c, const double *d_in, int64_t in_stride, double *d_out,
                                   int64_t out_stride, int64_t t0, int m, void *stream) {
    SML_REQUIRE(m >= 0, "sml_res_input_noise: m = %d is negative", m);
    SML_REQUIRE(t0 >= 0 && t0 <= kNoiseStepMax - (int64_t)m, "sml_res_input_noise: steps t0 = %lld .. + %d outside [0, 2^43)",
                (long long)t0, m);
    SML_REQUIRE(c != nullptr, "null reservoir context");
    SML_REQUIRE(c->members == 1, "sml_res_input_noise on a context of %d members", c->members);
    if (!c->noise_set) return fail(SML_ERR_STATE, "sml_res_input_noise before sml_res_set_input_noise");
    if (c->nlocal == 0 || c->tot_fb == 0 || m == 0) return SML_OK;
    SML_REQUIRE(d_out, "sml_res_input_noise: d_out is null");
    SML_REQUIRE(out_stride >= (int64_t)c->tot_fb, "sml_res_input_noise: out_stride %lld smaller than the packed feedback size %lld",
                (long long)out_stride, (long long)c->tot_fb);
    SML_REQUIRE(!d_in || in_stride >= (int64_t)c->tot_fb,
                "sml_res_input_noise: in_stride %lld smaller than the packed feedback size %lld", (long long)in_stride,
                (long long)c->tot_fb);
    SML_REQUIRE(d_in != d_out || in_stride == out_stride, "sml_res_input_noise: in place with two strides");
    if (d_in == d_out && c->noise_mag == 0.0) return SML_OK;  // the copy of a block onto itself
    const bool precip = c->noise_eps > 0.0 && !c->generic;
    const NoiseDev nz{c->generic ? c->d_nz_reg : c->d_fb_reg, c->d_nz_key, precip ? c->d_ser_l : nullptr, c->d_meanstd,
                      c->noise_mag, c->noise_eps};
    const int total = (int)c->tot_fb;
    const int tiles = std::min((m + kTileMem - 1) / kTileMem, 65535);
    hipLaunchKernelGGL(k_input_noise, dim3((total + kNoiseThreads - 1) / kNoiseThreads, tiles), dim3(kNoiseThreads), 0,
                       (hipStream_t)stream, c->d_rd, nz, d_in, in_stride, d_out, out_stride, t0, m, total);
    SML_HIP(hipGetLastError());
    return SML_OK;
}

// ---------------------------------------------------------------- CU-range streams
extern "C" int sml_stream_create_cu_range(int first_cu, int num_cus, void **out) {
    SML_REQUIRE(out && first_cu >= 0 && num_cus > 0, "bad argument");
    int dev = 0, ncu = 0;
    SML_HIP(hipGetDevice(&dev));
    SML_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    SML_REQUIRE(first_cu + num_cus <= ncu, "CU range [%d, %d) exceeds the device's %d CUs", first_cu,
                first_cu + num_cus, ncu);
    std::vector<uint32_t> mask((ncu + 31) / 32, 0u);
    for (int c = first_cu; c < first_cu + num_cus; ++c) mask[c / 32] |= 1u << (c % 32);
    hipStream_t s = nullptr;
    SML_HIP(hipExtStreamCreateWithCUMask(&s, (uint32_t)mask.size(), mask.data()));
    *out = s;
    return SML_OK;
}

extern "C" int sml_stream_destroy(void *stream) {
    SML_REQUIRE(stream, "bad argument");
    SML_HIP(hipStreamDestroy((hipStream_t)stream));
    return SML_OK;
}
