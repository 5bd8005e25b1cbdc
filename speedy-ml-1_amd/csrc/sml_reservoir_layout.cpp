// sml_reservoir_layout.cpp -- host side of the reservoir context (sml_reservoir.hip):
// pool offsets, one region's weights in their device layouts, the exchange / tiling
// index tables.  No HIP here: the caller allocates and uploads what these return.
#include "sml_reservoir_layout.hpp"

#include <algorithm>

namespace sml {

PoolPlan plan_pools(const PoolPlanIn &in) {
    PoolPlan p;
    p.rd.resize(in.nlocal);
    p.ld.resize(in.nlocal);
    for (int i = 0; i < in.nlocal; ++i) {
        const int n = in.n[i];
        // W_out rows (and x_aug) padded to 32 columns: with the streamed columns starting
        // at ncs & ~31, every 1 KB load of a wave is whole 128-B lines (no line fetched
        // by two neighbouring loads)
        p.ld[i] = (in.ncs + n + kLdAlign - 1) / kLdAlign * kLdAlign;
        RegionDev &r = p.rd[i];
        r.n = n;
        r.ninp = in.ninp[i];
        r.ld = p.ld[i];
        r.a_rp = p.tot_a_rp;
        p.tot_a_rp += n + 1;
        r.a_nz = p.tot_a_nz;
        p.tot_a_nz += in.k[i];
        r.w_rp = p.tot_w_rp;
        p.tot_w_rp += n + 1;
        r.w_nz = p.tot_w_nz;
        p.tot_w_nz += n;
        r.wout = p.tot_wout;
        p.tot_wout += (int64_t)in.nout_pad * p.ld[i];
        r.wlm = p.tot_wlm;
        p.tot_wlm += (int64_t)in.ncs * in.nout_pad;
        // the state's slot is the x~ column block of the region's ld-wide row (column
        // ncs on, 32-column aligned start, zero padding after n): the readout streams
        // x~ straight from the state the update wrote, squaring the even-numbered
        // entries as it loads them, so the update writes 8 B per row less
        r.xaug = p.tot_xaug;
        p.tot_xaug += p.ld[i];
        r.x = r.xaug + in.ncs;
        r.fb = p.tot_fb;
        p.tot_fb += in.ninp[i];
        p.maxn = std::max(p.maxn, n);
        p.maxninp = std::max(p.maxninp, in.ninp[i]);
        p.a_ell_cap.push_back(ell_cap_a(n, in.k[i], in.csr_only));
        p.w_ell_cap.push_back(ell_cap_w(in.csr_only));
        r.a_w = r.w_w = r.a_ov = r.w_q = 0;
        r.w_magic = 0;
        r.a_ell = p.tot_a_ell;
        p.tot_a_ell += (int64_t)p.a_ell_cap.back() * n;
        r.w_ell = p.tot_w_ell;
        p.tot_w_ell += (int64_t)p.w_ell_cap.back() * n;
        r.a_om = p.tot_a_om;
        p.tot_a_om += p.a_ell_cap.back() ? (n + 63) / 64 : 0;
        r.a_oe = p.tot_a_oe;
        p.tot_a_oe += p.a_ell_cap.back() ? n : 0;
    }
    return p;
}

StepShape step_shape(const StepShapeIn &in) {
    StepShape s;
    s.lds_x = (in.maxn + 1) / 2 * 2;
    s.lds_buf = s.lds_x + in.maxninp;
    s.lds_region = (size_t)s.lds_buf * sizeof(double);
    s.lds_bal = 2 * s.lds_region;
    s.lds_drive = 2 * s.lds_region;
    s.region_lds = s.lds_region <= kRegionLdsMax;
    // parts per region: enough blocks to fill the 512 resident 1024-thread block slots
    // (2 per CU with ~54 KB LDS each) once, each part at least one 1024-row pass.  Every
    // part stages the region's whole x, so more parts cost HBM traffic: measured on
    // 1152 regions, 1 part 119 us, 2 parts 128 us, 4 parts 165 us (profiles/r01m)
    const int max_parts = std::max(1, (in.maxn + kUpdThreads - 1) / kUpdThreads);
    s.parts = in.nlocal > 0 ? std::max(1, std::min(max_parts, (512 + in.nlocal - 1) / in.nlocal)) : 1;
    s.wide = in.nout_pad % kRowsWide == 0 && in.nout_pad / kRowsWide <= kWideMax;
    s.rows = s.wide ? kRowsWide : kRows;
    s.groups = in.nout_pad / s.rows;
    s.wpb = s.wide ? kWideWaves : 4;
    // the balanced update needs every region in ELL form, a segment's x and u within one
    // staging round (kStageX entries of x, one of u, per thread) and two buffers in LDS
    s.balanced = !in.per_region && in.nlocal > 0 && in.ell_ok && in.maxn <= kStageX * kUpdThreads &&
                 in.maxninp <= kUpdThreads && s.lds_bal <= in.max_lds;
    // the fused begin needs the wide readout (a wave per item of a region in one block)
    // and the update's LDS staging (2 blocks per CU)
    s.begin_fused = in.begin_mode > 0 && s.wide && s.region_lds;
    // the grouped finish: outputs in quads, kFinGroups column groups of kFinGsz at most,
    // a thread per (quad, group) in a block of 256
    s.finish_grouped = in.ncs > 0 && in.nout_pad % 4 == 0 && in.nout_pad <= kFinOutMax &&
                       in.nout_pad / 4 * kFinGroups <= 256 && (in.ncs + kFinGroups - 1) / kFinGroups <= kFinGsz &&
                       !in.finish_ungrouped;
    s.drive_fused = !in.stepwise_drive && s.lds_drive <= in.max_lds;
    return s;
}

MemberShape member_shape(const MemberShapeIn &in) {
    MemberShape m;
    m.update_lds = in.region_lds;
    m.update_tile = std::min(in.members, kMemberTile);
    // staged: the tile's x and u side by side within the device's LDS per workgroup
    // (an empty context stages nothing: no bound)
    if (m.update_lds && in.lds_region > 0)
        m.update_tile = (int)std::min<size_t>((size_t)m.update_tile, in.max_lds / in.lds_region);
    m.lds = m.update_lds ? (size_t)m.update_tile * in.lds_region : 0;
    m.readout_tile = std::min(in.members, kMemberTile);
    m.readout_streams = (in.members + m.readout_tile - 1) / m.readout_tile;
    return m;
}

MemberFinish member_finish(int members, int want) {
    MemberFinish f;
    const int cap = want >= 1 && want <= kFinTileMax ? want : kFinTile;
    f.tile = std::max(1, std::min(members, cap));
    f.tiles = (std::max(members, 1) + f.tile - 1) / f.tile;
    f.looped = f.tile == 1 && members > 1;
    // slm[tile][kMaxNcs] and red[tile][kFinGroups][kFinOutMax] doubles
    f.lds = (size_t)f.tile * (kMaxNcs + (size_t)kFinGroups * kFinOutMax) * sizeof(double);
    return f;
}

template <typename SrcT, typename StoT>
int pack_region(const PackIn &in, const RegionDev &rg, const int *rows, const int *cols, const SrcT *vals,
                const SrcT *win, const SrcT *wout, PackedRegion<StoT> *out) {
    const int i = in.i, n = rg.n, k = in.k, ninp = rg.ninp, ld = rg.ld, ncs = in.ncs, nout = in.nout;
    *out = PackedRegion<StoT>();
    PackedRegion<StoT> &p = *out;
    // --- A: COO (1-based) -> CSR, stable in file order (mklsparse, mod_linalg.f90:10-25)
    std::vector<int32_t> &rp = p.rp;
    rp.assign(n + 1, 0);
    for (int e = 0; e < k; ++e) {
        SML_REQUIRE(rows[e] >= 1 && rows[e] <= n && cols[e] >= 1 && cols[e] <= n,
                    "region %d: A entry %d out of range (row %d col %d, n %d)", i, e, rows[e], cols[e], n);
        rp[rows[e]]++;
    }
    for (int r = 0; r < n; ++r) rp[r + 1] += rp[r];
    std::vector<int32_t> fill(rp.begin(), rp.end() - 1);
    std::vector<uint16_t> &acol = p.acol;
    std::vector<StoT> &aval = p.aval;
    acol.resize(k);
    aval.resize(k);
    for (int e = 0; e < k; ++e) {
        const int at = fill[rows[e] - 1]++;
        acol[at] = (uint16_t)(cols[e] - 1);
        aval[at] = (StoT)vals[e];
        SML_REQUIRE((SrcT)aval[at] == vals[e], "region %d: A value %d not representable in the storage dtype", i, e);
    }
    // --- W_in: dense win(n, ninp) column-major -> CSR by row, columns ascending
    std::vector<int32_t> &wrp = p.wrp;
    wrp.assign(n + 1, 0);
    for (int col = 0; col < ninp; ++col)
        for (int r = 0; r < n; ++r)
            if (win[(size_t)col * n + r] != (SrcT)0) wrp[r + 1]++;
    for (int r = 0; r < n; ++r) wrp[r + 1] += wrp[r];
    const int64_t wnz = p.wnz = wrp[n];
    std::vector<int32_t> wfill(wrp.begin(), wrp.end() - 1);
    std::vector<uint16_t> &wcol = p.wcol;
    std::vector<StoT> &wval = p.wval;
    wcol.resize(wnz);
    wval.resize(wnz);
    for (int col = 0; col < ninp; ++col)
        for (int r = 0; r < n; ++r) {
            const SrcT v = win[(size_t)col * n + r];
            if (v == (SrcT)0) continue;
            const int at = wfill[r]++;
            wcol[at] = (uint16_t)col;
            wval[at] = (StoT)v;
            SML_REQUIRE((SrcT)wval[at] == v, "region %d: W_in value not representable in the storage dtype", i);
        }
    // --- W_out: wout(nout, ncs+n) column-major -> [nout_pad][ld] row-major
    std::vector<StoT> &wt = p.wt;
    wt.assign((size_t)in.nout_pad * ld, (StoT)0);
    for (int j = 0; j < ncs + n; ++j)
        for (int o = 0; o < nout; ++o) {
            const SrcT v = wout[(size_t)j * nout + o];
            StoT s = (StoT)v;
            SML_REQUIRE((SrcT)s == v || v != v, "region %d: W_out value not representable in the storage dtype", i);
            wt[(size_t)o * ld + j] = s;
        }
    if (ncs > 0) {  // W_out(:, 1:ncs) as [ncs][nout_pad]: the file's own order (outputs fastest), padded
        p.wl.assign((size_t)ncs * in.nout_pad, (StoT)0);
        for (int j = 0; j < ncs; ++j)
            for (int o = 0; o < nout; ++o) p.wl[(size_t)j * in.nout_pad + o] = (StoT)wout[(size_t)j * nout + o];
    }
    // --- ELL copies (RegionDev): A pair-major with the main width that moves the fewest
    // bytes, W_in one slot per row -- file order within a row, zero-padded after the
    // row's entries; a region whose rows do not fit keeps the CSR copies only
    const size_t wb = sizeof(StoT);
    if (in.a_ell_cap > 0) {
        int maxlen = 0, nmax = 0;
        for (int r = 0; r < n; ++r) maxlen = std::max(maxlen, rp[r + 1] - rp[r]);
        for (int r = 0; r < n; ++r) nmax += (rp[r + 1] - rp[r]) == maxlen;
        if (maxlen >= 1 && maxlen <= in.a_ell_cap) {
            // bytes per row: the pairs (odd widths padded), + for an overflow list its bit
            // words / counts (12 B per 64 rows) and an entry per row of maxlen entries
            const double eb = 2.0 + (double)wb;
            auto cost = [&](int w, bool ov) {
                return 2 * ((w + 1) / 2) * eb * n + (ov ? 12.0 * ((n + 63) / 64) + eb * nmax : 0.0);
            };
            int w = maxlen;
            bool ov = false;
            if (maxlen >= 2 && cost(maxlen - 1, true) < cost(maxlen, false)) {
                w = maxlen - 1;
                ov = true;
            }
            const int np = (w + 1) / 2;
            std::vector<uint16_t> &ec = p.a_ec;
            std::vector<StoT> &ev = p.a_ev;
            ec.assign((size_t)2 * np * n, 0);
            ev.assign((size_t)2 * np * n, (StoT)0);
            const int nw = (n + 63) / 64;
            p.om.assign(ov ? nw : 0, 0ull);
            p.ob.assign(ov ? nw : 0, 0u);
            for (int r = 0; r < n; ++r) {
                if (ov && (r & 63) == 0) p.ob[r >> 6] = (uint32_t)p.oc.size();
                for (int e = rp[r]; e < rp[r + 1]; ++e) {
                    const int s = e - rp[r];
                    if (s < w) {  // pair s / 2, half s % 2 of row r
                        const size_t at = (size_t)(s >> 1) * 2 * n + 2 * (size_t)r + (s & 1);
                        ec[at] = acol[e];
                        ev[at] = aval[e];
                    } else {  // s == w: the overflow entry
                        p.om[r >> 6] |= 1ull << (r & 63);
                        p.oc.push_back(acol[e]);
                        p.ovv.push_back(aval[e]);
                    }
                }
            }
            p.a_w = w;
            p.a_ov = ov ? 1 : 0;
        }
    }
    if (in.w_ell_cap > 0) {
        bool one = true;  // exactly one entry per row (train_reservoir's W_in, mod_reservoir.f90:260-278)
        for (int r = 0; r < n && one; ++r) one = wrp[r + 1] - wrp[r] == 1;
        if (one) {
            std::vector<uint16_t> &ec = p.w_ec;
            std::vector<StoT> &ev = p.w_ev;
            ec.resize(n);
            ev.resize(n);
            for (int r = 0; r < n; ++r) {
                ec[r] = wcol[wrp[r]];
                ev[r] = wval[wrp[r]];
            }
            // block-diagonal (rows (j-1) q + 1 .. j q read input j, q = n / ninp): the
            // column is i / q, computed as umulhi(i, magic), so only the value is read
            const int q = ninp > 0 && n % ninp == 0 ? n / ninp : 0;
            bool implicit = q > 0;
            const uint32_t magic = q > 0 ? win_magic(q) : 0u;
            for (int r = 0; r < n && implicit; ++r)
                implicit = ec[r] == r / q && (uint32_t)(((uint64_t)r * magic) >> 32) == (uint32_t)(r / q);
            p.w_w = 1;
            if (implicit) {
                p.w_q = q;
                p.w_magic = magic;
            }
        }
    }
    return SML_OK;
}

#define SML_PACK_INST(S, D)                                                                                      \
    template int pack_region<S, D>(const PackIn &, const RegionDev &, const int *, const int *, const S *, const S *, \
                                   const S *, PackedRegion<D> *);
SML_PACK_INST(float, float)
SML_PACK_INST(float, double)
SML_PACK_INST(double, float)
SML_PACK_INST(double, double)
#undef SML_PACK_INST

int out_std_index(int o, const RegionGeom &g) {
    const int res2d = g.resx * g.resy, natmo = kVars * res2d * kZGrid;
    if (o < natmo) {
        const int v = o % kVars, z = o / (kVars * res2d);
        return v * kZGrid + z;
    }
    if (o < natmo + res2d) return 32;
    if (o < natmo + 2 * res2d) return 34;
    return -1;
}

int build_region_tables(const TablesIn &in, RegionTables *out) {
    *out = RegionTables();
    if (in.out_l) {  // generic: no exchange / tiling tables, only the unstandardize slots
        out->outl.assign(in.out_l, in.out_l + in.nout);
        return SML_OK;
    }
    const int nlocal = in.nlocal, ncs = in.ncs, nout = in.nout;
    // assemble: every region of the decomposition (outvec_all is global)
    std::vector<int32_t> &dst = out->asm_dst;
    dst.assign((size_t)in.numregions * nout, -1);
    for (int r = 0; r < in.numregions; ++r) {
        RegionGeom g{};
        region_geom(in.numregions, r, &g);
        const int rx = g.resx, ry = g.resy, natmo = kVars * rx * ry * kZGrid;
        for (int o = 0; o < nout; ++o) {
            int d = -1;
            if (o < natmo) {
                const int v = o % kVars, x = (o / kVars) % rx, y = (o / (kVars * rx)) % ry, z = o / (kVars * rx * ry);
                d = g4(v, g.res_xstart - 1 + x, g.res_ystart - 1 + y, z);
            } else if (o < natmo + rx * ry) {
                const int p = o - natmo;
                d = kGrid4d + g2(g.res_xstart - 1 + p % rx, g.res_ystart - 1 + p / rx);
            } else if (o < natmo + 2 * rx * ry) {
                const int p = o - natmo - rx * ry;
                d = kGrid4d + kGrid2d + g2(g.res_xstart - 1 + p % rx, g.res_ystart - 1 + p / rx);
            }
            dst[(size_t)r * nout + o] = d;
        }
    }
    // feedback tiles of the local regions (tile_4d_and_logp_to_local_state_input +
    // standardize_state_vec_input + precip standardisation + tisr + sst)
    std::vector<int32_t> &fsrc = out->fb_src, &lsrc = out->lm_src, &tfb = out->tisr_fb, &tgi = out->tisr_grid;
    std::vector<uint8_t> &fl = out->fb_l, &ll = out->lm_l;
    std::vector<uint16_t> &freg = out->fb_reg, &treg = out->tisr_reg;
    fsrc.resize(in.tot_fb);
    fl.assign(in.tot_fb, 0);
    freg.resize(in.tot_fb);
    lsrc.assign((size_t)nlocal * std::max(ncs, 1), 0);
    ll.assign((size_t)nlocal * std::max(ncs, 1), 0);
    for (int i = 0; i < nlocal; ++i) {
        const RegionGeom &g = in.geom[i];
        const int ix = g.inx, iy = g.iny, in2d = ix * iy, natmo = kVars * in2d * kZGrid;
        const int64_t base = in.rd[i].fb;
        auto gx = [&](int lx) { return input_x(g, lx + 1) - 1; };
        for (int z = 0; z < kZGrid; ++z)
            for (int ly = 0; ly < iy; ++ly)
                for (int lx = 0; lx < ix; ++lx)
                    for (int v = 0; v < kVars; ++v) {
                        const int64_t e = base + v + kVars * (lx + ix * (ly + iy * z));
                        fsrc[e] = g4(v, gx(lx), g.in_ystart - 1 + ly, z);
                        fl[e] = (uint8_t)(v * kZGrid + z);
                    }
        for (int ly = 0; ly < iy; ++ly)
            for (int lx = 0; lx < ix; ++lx) {
                const int p = lx + ix * ly;
                fsrc[base + natmo + p] = kGrid4d + g2(gx(lx), g.in_ystart - 1 + ly);
                fl[base + natmo + p] = 32;  // logp (l = 33)
                fsrc[base + natmo + in2d + p] = kGrid4d + kGrid2d + g2(gx(lx), g.in_ystart - 1 + ly);
                fl[base + natmo + in2d + p] = 34;  // precip (l = 35)
            }
        int64_t off = base + natmo + 2 * in2d;
        if (in.sst[i]) {
            for (int p = 0; p < in2d; ++p) fsrc[off + p] = kSrcKeep;
            off += in2d;
        }
        for (int p = 0; p < in2d; ++p) {
            fsrc[off + p] = -2 - (i * kTisrStride + p);
            tfb.push_back((int32_t)(off + p));
            tgi.push_back(g2(gx(p % ix), g.in_ystart - 1 + p / ix));
            treg.push_back((uint16_t)i);
        }
        for (int64_t e = base; e < base + in.ninp[i]; ++e) freg[e] = (uint16_t)i;
        // local_model: the region's own points of the SPEEDY forecast grids
        const int rx = g.resx, ry = g.resy, na = kVars * rx * ry * kZGrid;
        for (int cidx = 0; cidx < ncs; ++cidx) {
            int s = 0, l = 0;
            if (cidx < na) {
                const int v = cidx % kVars, x = (cidx / kVars) % rx, y = (cidx / (kVars * rx)) % ry,
                          z = cidx / (kVars * rx * ry);
                s = g4(v, g.res_xstart - 1 + x, g.res_ystart - 1 + y, z);
                l = v * kZGrid + z;
            } else {
                const int p = cidx - na;
                s = kGrid4d + g2(g.res_xstart - 1 + p % rx, g.res_ystart - 1 + (p / rx) % ry);
                l = 32;
            }
            lsrc[(size_t)i * ncs + cidx] = s;
            ll[(size_t)i * ncs + cidx] = (uint8_t)l;
        }
    }
    out->outl.resize(nout);
    for (int o = 0; o < nout; ++o) out->outl[o] = (int8_t)out_std_index(o, nlocal ? in.geom[0] : RegionGeom{});
    // the training targets' positions in each local region's feedback (the drive's gather)
    std::vector<int32_t> &tidx = out->tgt_idx;
    tidx.assign((size_t)nlocal * nout, 0);
    for (int i = 0; i < nlocal; ++i) {
        std::vector<int32_t> t((size_t)(kVars * kZGrid + 2) * in.geom[i].inx * in.geom[i].iny);
        const int cnt = region_target_index(in.geom[i], t.data());
        SML_REQUIRE(cnt == nout, "region %d: %d training targets, nout %d", i, cnt, nout);
        std::copy(t.begin(), t.begin() + cnt, tidx.begin() + (size_t)i * nout);
    }
    return SML_OK;
}

int build_series_tables(const TablesIn &in, SeriesTables *out) {
    *out = SeriesTables();
    SML_REQUIRE(!in.out_l, "a generic (slab) context has no exchange tables");
    out->src.assign(in.tot_fb, 0);
    out->l.assign(in.tot_fb, 0);
    out->pt_off.assign(in.nlocal + 1, 0);
    for (int i = 0; i < in.nlocal; ++i) {
        const RegionGeom &g = in.geom[i];
        const int ix = g.inx, iy = g.iny, in2d = ix * iy, natmo = kVars * in2d * kZGrid;
        const int64_t base = in.rd[i].fb;
        SML_REQUIRE(base + region_ninp(g, in.sst[i] != 0) <= in.tot_fb, "region %d: feedback past the pool", i);
        // the 2-d blocks behind the atmosphere's, in the feedback's order (region_ninp)
        int blocks = 0, field[4], slot[4];
        field[blocks] = kSerLogp, slot[blocks++] = 32;
        field[blocks] = kSerPrecip, slot[blocks++] = 34;
        if (in.sst[i]) field[blocks] = kSerSst, slot[blocks++] = 35;
        field[blocks] = kSerTisr, slot[blocks++] = 33;
        for (int ly = 0; ly < iy; ++ly)
            for (int lx = 0; lx < ix; ++lx) {
                const int gx = input_x(g, lx + 1) - 1, gy = g.in_ystart - 1 + ly, p = lx + ix * ly;
                out->pt_grid.push_back(g2(gx, gy));
                for (int z = 0; z < kZGrid; ++z)
                    for (int v = 0; v < kVars; ++v) {
                        const int64_t e = base + v + kVars * (p + in2d * z);
                        out->src[e] = g4(v, gx, gy, z);
                        out->l[e] = (uint8_t)(v * kZGrid + z);
                    }
                for (int b = 0; b < blocks; ++b) {
                    const int64_t e = base + natmo + (int64_t)b * in2d + p;
                    out->src[e] = kGrid4d + field[b] * kGrid2d + g2(gx, gy);
                    out->l[e] = (uint8_t)slot[b];
                }
            }
        out->pt_off[i + 1] = (int32_t)out->pt_grid.size();
    }
    return SML_OK;
}

std::vector<int32_t> block_first_regions(const std::vector<int32_t> &row0, int G) {
    const int64_t total = row0.back();
    std::vector<int32_t> r0(G);
    for (int b = 0; b < G; ++b) {
        const int64_t g0 = total * b / G;
        r0[b] = (int32_t)(std::upper_bound(row0.begin(), row0.end(), (int32_t)g0) - row0.begin() - 1);
    }
    return r0;
}

void footprint(int nlocal, const int *nn, const int *kk, const int *ni, int ncs, int nout, int64_t wb,
               int64_t *weight_bytes, int64_t *algo_bytes) {
    int64_t w = 0, a = 0;
    for (int i = 0; i < nlocal; ++i) {
        const int64_t n = nn[i], k = kk[i], ninp = ni[i];
        const int64_t wout = wb * nout * (ncs + n);       // unpadded W_out
        const int64_t amat = 4 * (n + 1) + (2 + wb) * k;  // CSR row ptr + col + val
        const int64_t winm = 4 * (n + 1) + (2 + wb) * n;  // CSR, one entry per row
        w += wout + amat + winm;
        // minimal traffic: weights once, state in + out, feedback, local model, outvec
        a += wout + amat + winm + 8 * n + 8 * n + 8 * ninp + 8 * ncs + 8 * nout;
    }
    if (weight_bytes) *weight_bytes = w;
    if (algo_bytes) *algo_bytes = a;
}

}  // namespace sml
