// reservoir_layout_check.cpp -- CPU check of the reservoir context's layout unit
// (speedy-ml-1_amd/csrc/sml_reservoir_layout.cpp): every vector the context uploads is
// compared with its plain definition, written out here without the unit's own code.
// Stand-alone (tests/test_reservoir_layout_cpu.py builds it plain and under ASan/UBSan).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "sml_reservoir_layout.hpp"

using namespace sml;

static int g_fail = 0, g_checks = 0;
static std::string g_case;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        ++g_checks;                                                   \
        if (!(cond)) {                                                \
            if (++g_fail <= 40) {                                     \
                std::printf("FAIL [%s] %s:%d %s -- ", g_case.c_str(), __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                             \
                std::printf("\n");                                    \
            }                                                         \
        }                                                             \
    } while (0)

// ---------------------------------------------------------------- cases
enum Win { kBlockDiag, kPermuted, kZeroAndTwo, kDense, kOnePerRowNoBlock };

struct Case {
    std::string name;
    int n = 1, ninp = 1, ncs = 0, nout = 5;
    std::vector<int> rows, cols;  // A as COO, 1-based, file order
    Win win = kBlockDiag;
};

// A with lens[r] entries in row r, in a file order that interleaves the rows (last row
// first), so the CSR conversion has to be stable; columns repeat when n is small
static void fill_a(Case &c, const std::vector<int> &lens) {
    int maxlen = 0;
    for (int l : lens) maxlen = std::max(maxlen, l);
    for (int s = 0; s < maxlen; ++s)
        for (int r = c.n - 1; r >= 0; --r)
            if (s < lens[r]) {
                c.rows.push_back(r + 1);
                c.cols.push_back((r * 7 + s * 3) % c.n + 1);
            }
}

static Case make(const std::string &name, int n, int ninp, const std::vector<int> &lens, Win win = kBlockDiag,
                 int ncs = 0, int nout = 5) {
    Case c;
    c.name = name;
    c.n = n;
    c.ninp = ninp;
    c.ncs = ncs;
    c.nout = nout;
    c.win = win;
    fill_a(c, lens);
    return c;
}

// values: small multiples of 1/4, exact in float, never zero, distinct along a row
static double aval_of(int e) { return 0.25 * (e % 97 + 1) * ((e & 1) ? -1 : 1); }
static double wout_of(size_t idx) { return 0.5 * (double)(idx % 251 + 1) * ((idx & 2) ? -1 : 1); }

template <typename SrcT>
static std::vector<SrcT> make_win(const Case &c) {
    std::vector<SrcT> w((size_t)c.n * c.ninp, (SrcT)0);
    auto at = [&](int r, int col) -> SrcT & { return w[(size_t)col * c.n + r]; };
    const int q = c.n % c.ninp == 0 ? c.n / c.ninp : 1;
    for (int r = 0; r < c.n; ++r) switch (c.win) {
            case kBlockDiag: at(r, r / q) = (SrcT)(0.5 * (r % 31 + 1)); break;
            case kPermuted: at(r, c.ninp - 1 - r / q) = (SrcT)(0.5 * (r % 31 + 1)); break;
            case kOnePerRowNoBlock: at(r, r % c.ninp) = (SrcT)(0.5 * (r % 31 + 1)); break;
            case kZeroAndTwo:
                if (r == c.n / 2) break;  // a row with no entry
                at(r, r / q) = (SrcT)(0.5 * (r % 31 + 1));
                if (r == c.n - 1) at(r, (r / q + 1) % c.ninp) = (SrcT)-1.5;  // a row with two
                break;
            case kDense:
                for (int col = 0; col < c.ninp; ++col) at(r, col) = (SrcT)(0.25 * (1 + (r + 3 * col) % 17));
                break;
        }
    return w;
}

// ---------------------------------------------------------------- one region
template <typename T>
static bool same(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <typename SrcT, typename StoT>
static void check_region(const Case &c, bool csr_only = false) {
    g_case = c.name + (sizeof(SrcT) == 4 ? " src32" : " src64") + (sizeof(StoT) == 4 ? " sto32" : " sto64") +
             (csr_only ? " csr" : "");
    const int n = c.n, ninp = c.ninp, ncs = c.ncs, nout = c.nout, k = (int)c.rows.size();
    const int nout_pad = (nout + 7) / 8 * 8;
    std::vector<SrcT> vals(k);
    for (int e = 0; e < k; ++e) vals[e] = (SrcT)aval_of(e);
    const std::vector<SrcT> win = make_win<SrcT>(c);
    std::vector<SrcT> wout((size_t)(ncs + n) * nout);
    for (size_t e = 0; e < wout.size(); ++e) wout[e] = (SrcT)wout_of(e);

    const PoolPlan plan = plan_pools({1, &n, &k, &ninp, ncs, nout_pad, csr_only});
    const RegionDev &rg = plan.rd[0];
    const int ld = rg.ld;
    CHECK(ld % 32 == 0 && ld >= ncs + n && ld < ncs + n + 32, "ld %d", ld);
    CHECK(plan.a_ell_cap[0] == ((!csr_only && k / n + 1 <= 8) ? 8 : 0), "A cap %d", plan.a_ell_cap[0]);
    CHECK(plan.w_ell_cap[0] == (csr_only ? 0 : 1), "W_in cap %d", plan.w_ell_cap[0]);
    PackedRegion<StoT> p;
    const PackIn in{0, k, ncs, nout, nout_pad, plan.a_ell_cap[0], plan.w_ell_cap[0]};
    const int rc = pack_region(in, rg, c.rows.data(), c.cols.data(), vals.data(), win.data(), wout.data(), &p);
    CHECK(rc == SML_OK, "pack_region: %s", sml_last_error());
    if (rc != SML_OK) return;

    // ---- A: the rows' entries in file order
    std::vector<std::vector<std::pair<int, StoT>>> arow(n);
    for (int e = 0; e < k; ++e) arow[c.rows[e] - 1].push_back({c.cols[e] - 1, (StoT)vals[e]});
    CHECK((int)p.rp.size() == n + 1 && (int)p.acol.size() == k && (int)p.aval.size() == k, "CSR sizes");
    int maxlen = 0, nmax = 0;
    for (int r = 0; r < n; ++r) maxlen = std::max(maxlen, (int)arow[r].size());
    for (int r = 0; r < n; ++r) nmax += (int)arow[r].size() == maxlen;
    for (int r = 0, at = 0; r < n; ++r) {
        CHECK(p.rp[r] == at && p.rp[r + 1] == at + (int)arow[r].size(), "rp[%d]", r);
        for (size_t s = 0; s < arow[r].size(); ++s, ++at)
            CHECK(p.acol[at] == arow[r][s].first && same(p.aval[at], arow[r][s].second), "CSR row %d entry %zu", r, s);
    }
    // the width: none without a reserved slot, an entry, or past 8; else the cheaper of
    // (maxlen, no list) and (maxlen - 1, list) in bytes: a slot pair is 2 u16 + 2 values per
    // row, a list is a u64 + a u32 per 64 rows and a u16 + a value per longest row
    const long wb = sizeof(StoT), nw = (n + 63) / 64;
    int want_w = 0, want_ov = 0;
    if (plan.a_ell_cap[0] > 0 && maxlen >= 1 && maxlen <= 8) {
        const long plain = (long)((maxlen + 1) / 2) * n * (4 + 2 * wb);
        const long list = (long)(maxlen / 2) * n * (4 + 2 * wb) + nw * 12 + (long)nmax * (2 + wb);
        want_ov = maxlen >= 2 && list < plain;
        want_w = want_ov ? maxlen - 1 : maxlen;
    }
    CHECK(p.a_w == want_w && p.a_ov == want_ov, "(a_w, a_ov) = (%d, %d), cheaper is (%d, %d); maxlen %d nmax %d",
          p.a_w, p.a_ov, want_w, want_ov, maxlen, nmax);
    if (maxlen > 8 || k == 0) CHECK(p.a_w == 0, "a_w %d with maxlen %d k %d", p.a_w, maxlen, k);
    if (p.a_w == 0) {
        CHECK(p.a_ec.empty() && p.a_ev.empty() && p.om.empty() && p.ob.empty() && p.oc.empty() && p.ovv.empty(),
              "ELL vectors of a CSR region");
    } else {
        const int w = p.a_w, np = (w + 1) / 2;
        CHECK(p.a_ec.size() == (size_t)2 * np * n && p.a_ev.size() == p.a_ec.size(), "ELL size %zu", p.a_ec.size());
        CHECK((int64_t)p.a_ec.size() <= (int64_t)plan.a_ell_cap[0] * n, "ELL copy exceeds its pool share");
        CHECK(p.om.size() == (size_t)(p.a_ov ? nw : 0) && p.ob.size() == p.om.size(), "overflow words %zu", p.om.size());
        CHECK(p.oc.size() == p.ovv.size() && p.oc.size() <= (size_t)n, "overflow entries %zu", p.oc.size());
        if (p.a_ec.size() != (size_t)2 * np * n || p.om.size() != (size_t)(p.a_ov ? nw : 0)) return;
        size_t before = 0;  // overflow entries in the rows before r
        for (int r = 0; r < n; ++r) {
            const int len = (int)arow[r].size();
            if (p.a_ov && r % 64 == 0) CHECK(p.ob[r / 64] == before, "ob[%d] = %u, %zu rows before", r / 64, p.ob[r / 64], before);
            for (int s = 0; s < 2 * np; ++s) {
                const size_t at = (size_t)(s >> 1) * 2 * n + 2 * (size_t)r + (s & 1);
                if (s < len && s < w)
                    CHECK(p.a_ec[at] == arow[r][s].first && same(p.a_ev[at], arow[r][s].second), "ELL row %d slot %d", r, s);
                else
                    CHECK(p.a_ec[at] == 0 && same(p.a_ev[at], (StoT)0), "ELL padding row %d slot %d", r, s);
            }
            CHECK(len <= w + p.a_ov, "row %d holds %d entries, width %d", r, len, w);
            const bool bit = p.a_ov && ((p.om[r / 64] >> (r % 64)) & 1);
            CHECK(bit == (len == w + 1), "overflow bit of row %d (%d entries, width %d)", r, len, w);
            if (len == w + 1 && before < p.oc.size()) {
                CHECK(p.oc[before] == arow[r][w].first && same(p.ovv[before], arow[r][w].second), "overflow entry of row %d", r);
                ++before;
            }
        }
        CHECK(before == p.oc.size(), "%zu overflow entries, %zu rows one longer", p.oc.size(), before);
        for (size_t q = 0; q < p.om.size(); ++q)  // no bit past the last row
            if (q == p.om.size() - 1 && n % 64) CHECK((p.om[q] >> (n % 64)) == 0, "overflow bits past row n");
    }

    // ---- W_in: the rows' entries, columns ascending
    std::vector<std::vector<std::pair<int, StoT>>> wrow(n);
    for (int r = 0; r < n; ++r)
        for (int col = 0; col < ninp; ++col)
            if (win[(size_t)col * n + r] != (SrcT)0) wrow[r].push_back({col, (StoT)win[(size_t)col * n + r]});
    bool one = true;
    int64_t wnz = 0;
    for (int r = 0; r < n; ++r) {
        one = one && wrow[r].size() == 1;
        wnz += (int64_t)wrow[r].size();
    }
    CHECK(p.wnz == wnz && (int64_t)p.wcol.size() == wnz && (int64_t)p.wval.size() == wnz && (int)p.wrp.size() == n + 1, "W_in CSR sizes");
    for (int r = 0, at = 0; r < n; ++r) {
        CHECK(p.wrp[r] == at && p.wrp[r + 1] == at + (int)wrow[r].size(), "wrp[%d]", r);
        for (size_t s = 0; s < wrow[r].size(); ++s, ++at) {
            CHECK(p.wcol[at] == wrow[r][s].first && same(p.wval[at], wrow[r][s].second), "W_in CSR row %d entry %zu", r, s);
            if (s) CHECK(p.wcol[at] > p.wcol[at - 1], "W_in CSR row %d columns not ascending", r);
        }
    }
    CHECK(p.w_w == (one && !csr_only ? 1 : 0), "W_in ELL %d, one entry per row %d", p.w_w, (int)one);
    bool block = one && !csr_only && n % ninp == 0;
    for (int r = 0; r < n && block; ++r) block = wrow[r][0].first == r / (n / ninp);
    // (blocks of one row, q = 1, have no 32-bit magic: ceil(2^32 / 1) does not fit, so
    // past n = 1 such a region keeps its stored columns)
    const uint32_t magic = block ? (uint32_t)(((1ull << 32) + n / ninp - 1) / (n / ninp)) : 0u;
    for (int r = 0; r < n && block; ++r) block = (((uint64_t)r * magic) >> 32) == (uint64_t)(r / (n / ninp));
    CHECK(p.w_q == (block ? n / ninp : 0) && p.w_magic == (block ? magic : 0u), "w_q %d w_magic %u, block diagonal %d", p.w_q,
          p.w_magic, (int)block);
    if (n > 1 && ninp == n) CHECK(p.w_q == 0, "q = 1 taken as implicit");
    if (p.w_w) {
        CHECK((int)p.w_ec.size() == n && (int)p.w_ev.size() == n, "W_in ELL size");
        for (int r = 0; r < n && (int)p.w_ec.size() == n; ++r)
            CHECK(p.w_ec[r] == wrow[r][0].first && same(p.w_ev[r], wrow[r][0].second), "W_in ELL row %d", r);
    } else {
        CHECK(p.w_ec.empty() && p.w_ev.empty(), "W_in ELL vectors of a CSR region");
    }
    for (int i = 0; i < n && p.w_q; ++i)
        CHECK((uint32_t)(((uint64_t)i * p.w_magic) >> 32) == (uint32_t)(i / p.w_q), "umulhi(%d, magic) != %d / %d", i, i, p.w_q);

    // ---- W_out transposed and padded, and its local-model block
    CHECK(p.wt.size() == (size_t)nout_pad * ld, "wt size %zu", p.wt.size());
    if (p.wt.size() == (size_t)nout_pad * ld)
        for (int o = 0; o < nout_pad; ++o)
            for (int j = 0; j < ld; ++j) {
                const StoT want = o < nout && j < ncs + n ? (StoT)wout[(size_t)j * nout + o] : (StoT)0;
                CHECK(same(p.wt[(size_t)o * ld + j], want), "wt[%d][%d]", o, j);
            }
    CHECK(p.wl.size() == (size_t)ncs * nout_pad, "wl size %zu", p.wl.size());
    if (p.wl.size() == (size_t)ncs * nout_pad)
        for (int j = 0; j < ncs; ++j)
            for (int o = 0; o < nout_pad; ++o) {
                const StoT want = o < nout ? (StoT)wout[(size_t)j * nout + o] : (StoT)0;
                CHECK(same(p.wl[(size_t)j * nout_pad + o], want), "wl[%d][%d]", j, o);
            }
}

static void check_region_all(const Case &c) {
    check_region<float, float>(c);
    check_region<double, float>(c);
    check_region<float, double>(c);
    check_region<double, double>(c);
}

// ---------------------------------------------------------------- rejected loads
template <typename SrcT, typename StoT>
static void check_reject(const char *what, int where, SrcT bad, bool accepted, const char *msg) {
    g_case = std::string("reject ") + what + (sizeof(SrcT) == 4 ? " src32" : " src64") + (sizeof(StoT) == 4 ? " sto32" : " sto64");
    const int n = 3, ninp = 3, ncs = 2, nout = 5, nout_pad = 8, k = 3;
    int rows[3] = {1, 2, 3}, cols[3] = {2, 3, 1};
    SrcT vals[3] = {(SrcT)0.5, (SrcT)-1, (SrcT)2};
    std::vector<SrcT> win(n * ninp, (SrcT)0), wout((ncs + n) * nout, (SrcT)0.25);
    for (int r = 0; r < n; ++r) win[r * n + r] = (SrcT)1;
    if (where == 0) vals[1] = bad;
    if (where == 1) win[1 * n + 1] = bad;
    if (where == 2) wout[7] = bad;
    if (where == 3) cols[2] = n + 1;
    const PoolPlan plan = plan_pools({1, &n, &k, &ninp, ncs, nout_pad, false});
    PackedRegion<StoT> p;
    const int rc = pack_region({0, k, ncs, nout, nout_pad, 8, 1}, plan.rd[0], rows, cols, vals, win.data(), wout.data(), &p);
    if (accepted) {
        CHECK(rc == SML_OK, "rejected: %s", sml_last_error());
        if (where == 2 && rc == SML_OK) CHECK(p.wt[(7 % nout) * plan.ld[0] + 7 / nout] != p.wt[(7 % nout) * plan.ld[0] + 7 / nout], "NaN not kept");
    } else {
        CHECK(rc == SML_ERR_ARG && std::strstr(sml_last_error(), msg), "rc %d, message '%s'", rc, sml_last_error());
    }
}

// ---------------------------------------------------------------- plan, blocks
static void check_plan(int ncs, int nout_pad, bool csr_only) {
    g_case = "plan ncs " + std::to_string(ncs) + (csr_only ? " csr" : "");
    const std::vector<int> n = {1, 63, 64, 65, 6048, 130}, k = {0, 100, 64 * 2, 65 * 8, 6048 * 3, 130 * 7},
                           ninp = {1, 7, 64, 13, 1152, 65535};
    const int nl = (int)n.size();
    const PoolPlan p = plan_pools({nl, n.data(), k.data(), ninp.data(), ncs, nout_pad, csr_only});
    CHECK((int)p.rd.size() == nl && (int)p.ld.size() == nl && (int)p.a_ell_cap.size() == nl && (int)p.w_ell_cap.size() == nl, "sizes");
    int64_t at[12] = {0};
    int maxn = 0, maxninp = 0;
    for (int i = 0; i < nl; ++i) {
        const RegionDev &r = p.rd[i];
        const int ld = p.ld[i], ca = (!csr_only && k[i] / n[i] + 1 <= 8) ? 8 : 0, cw = csr_only ? 0 : 1;
        CHECK(r.n == n[i] && r.ninp == ninp[i] && r.ld == ld, "region %d sizes", i);
        CHECK(ld % 32 == 0 && ld >= ncs + n[i] && ld < ncs + n[i] + 32, "region %d ld %d", i, ld);
        CHECK(p.a_ell_cap[i] == ca && p.w_ell_cap[i] == cw, "region %d caps", i);
        CHECK(r.a_w == 0 && r.w_w == 0 && r.a_ov == 0 && r.w_q == 0 && r.w_magic == 0, "region %d layout not cleared", i);
        CHECK(r.x == r.xaug + ncs, "region %d x", i);
        // each pool: this region starts where the one before it ended
        const int64_t off[12] = {r.a_rp, r.a_nz, r.w_rp, r.w_nz, r.wout, r.wlm, r.xaug, r.fb, r.a_ell, r.w_ell, r.a_om, r.a_oe};
        const int64_t len[12] = {n[i] + 1, k[i], n[i] + 1, n[i], (int64_t)nout_pad * ld, (int64_t)ncs * nout_pad, ld, ninp[i],
                                 (int64_t)ca * n[i], (int64_t)cw * n[i], ca ? (n[i] + 63) / 64 : 0, ca ? n[i] : 0};
        for (int q = 0; q < 12; ++q) {
            CHECK(off[q] == at[q], "region %d pool %d offset %lld, expected %lld", i, q, (long long)off[q], (long long)at[q]);
            at[q] += len[q];
        }
        maxn = std::max(maxn, n[i]);
        maxninp = std::max(maxninp, ninp[i]);
    }
    const int64_t tot[12] = {p.tot_a_rp, p.tot_a_nz, p.tot_w_rp, p.tot_w_nz, p.tot_wout, p.tot_wlm, p.tot_xaug, p.tot_fb,
                             p.tot_a_ell, p.tot_w_ell, p.tot_a_om, p.tot_a_oe};
    for (int q = 0; q < 12; ++q) CHECK(tot[q] == at[q], "pool %d total %lld, expected %lld", q, (long long)tot[q], (long long)at[q]);
    CHECK(p.maxn == maxn && p.maxninp == maxninp, "maxn %d maxninp %d", p.maxn, p.maxninp);
}

static void check_blocks() {
    const std::vector<int> n = {1, 63, 64, 65, 300, 2};
    std::vector<int32_t> row0(1, 0);
    for (int v : n) row0.push_back(row0.back() + v);
    const int total = row0.back();
    for (int G : {1, 2, total, 256}) {
        g_case = "blocks G " + std::to_string(G);
        const std::vector<int32_t> r0 = block_first_regions(row0, G);
        CHECK((int)r0.size() == G, "size %zu", r0.size());
        for (int b = 0; b < G && (int)r0.size() == G; ++b) {
            const long g0 = (long)total * b / G;  // the block's first row: in region i, row0[i] <= g0 < row0[i + 1]
            int i = 0;
            while (g0 >= row0[i + 1]) ++i;
            CHECK(r0[b] == i, "block %d (row %ld) starts in region %d, expected %d", b, g0, r0[b], i);
        }
    }
}

// ---------------------------------------------------------------- tables
static void check_tables() {
    const int numregions = 1152, nout = 136, ncs = 132, nl = 4;
    const int ids[nl] = {0, 5, 30, 1151};  // pole + wrap, wrap, interior, pole + wrap
    const unsigned char sst[nl] = {0, 1, 0, 1};
    RegionGeom geom[nl];
    int ninp[nl], n[nl], k[nl];
    for (int i = 0; i < nl; ++i) {
        region_geom(numregions, ids[i], &geom[i]);
        ninp[i] = geom[i].inx * geom[i].iny * (kVars * kZGrid + 3 + sst[i]);
        n[i] = 8;
        k[i] = 8;
    }
    const PoolPlan plan = plan_pools({nl, n, k, ninp, ncs, nout, false});
    RegionTables t;
    g_case = "tables";
    const int rc = build_region_tables({numregions, nl, ncs, nout, geom, sst, ninp, plan.rd.data(), plan.tot_fb, nullptr}, &t);
    CHECK(rc == SML_OK, "build_region_tables: %s", sml_last_error());
    if (rc != SML_OK) return;
    CHECK(geom[0].pole && geom[0].periodic && !geom[1].pole && geom[1].periodic && !geom[2].pole && !geom[2].periodic &&
              geom[3].pole && geom[3].periodic, "the regions' kinds");
    CHECK((int64_t)t.fb_src.size() == plan.tot_fb && t.fb_l.size() == t.fb_src.size() && t.fb_reg.size() == t.fb_src.size(), "feedback sizes");
    CHECK(t.lm_src.size() == (size_t)nl * ncs && t.lm_l.size() == t.lm_src.size(), "local-model sizes");
    CHECK(t.asm_dst.size() == (size_t)numregions * nout && t.outl.size() == (size_t)nout && t.tgt_idx.size() == (size_t)nl * nout, "sizes");
    // the region's own point p (x fastest) of a 2 x 2 tile, and output o's grid element
    auto own = [&](const RegionGeom &g, int o) {
        if (o < 128) return g4(o % 4, g.res_xstart - 1 + (o / 4) % 2, g.res_ystart - 1 + (o / 8) % 2, o / 16);
        const int p = (o - 128) % 4;
        return kGrid4d + (o >= 132 ? kGrid2d : 0) + g2(g.res_xstart - 1 + p % 2, g.res_ystart - 1 + p / 2);
    };
    for (int o = 0; o < nout; ++o) CHECK(t.outl[o] == (o < 128 ? (o % 4) * 8 + o / 16 : o < 132 ? 32 : 34), "outl[%d] = %d", o, t.outl[o]);
    int64_t base = 0;
    size_t tt = 0;
    for (int i = 0; i < nl; ++i) {
        g_case = "tables region " + std::to_string(ids[i]);
        const RegionGeom &g = geom[i];
        const int ix = g.inx, iy = g.iny, in2d = ix * iy, natmo = 4 * in2d * 8;
        CHECK(plan.rd[i].fb == base, "fb offset");
        auto gx = [&](int lx) { return input_x(g, lx + 1) - 1; };
        for (int rel = 0; rel < ninp[i]; ++rel) {
            const int64_t e = base + rel;
            int src, l = 0;
            if (rel < natmo) {
                const int v = rel % 4, lx = (rel / 4) % ix, ly = (rel / (4 * ix)) % iy, z = rel / (4 * ix * iy);
                src = g4(v, gx(lx), g.in_ystart - 1 + ly, z);
                l = v * 8 + z;
            } else if (rel < natmo + 2 * in2d) {
                const int p = (rel - natmo) % in2d, second = (rel - natmo) / in2d;
                src = kGrid4d + second * kGrid2d + g2(gx(p % ix), g.in_ystart - 1 + p / ix);
                l = second ? 34 : 32;
            } else if (sst[i] && rel < natmo + 3 * in2d) {
                src = -1;
            } else {
                const int p = rel - natmo - (2 + sst[i]) * in2d;
                src = -2 - (i * 16 + p);
                CHECK(tt < t.tisr_fb.size() && t.tisr_fb[tt] == e && t.tisr_grid[tt] == g2(gx(p % ix), g.in_ystart - 1 + p / ix) &&
                          t.tisr_reg[tt] == i, "tisr entry %zu", tt);
                ++tt;
            }
            CHECK(t.fb_src[e] == src && t.fb_l[e] == l && t.fb_reg[e] == i, "feedback %d: src %d l %d reg %d, expected %d %d %d", rel,
                  t.fb_src[e], t.fb_l[e], t.fb_reg[e], src, l, i);
        }
        for (int cidx = 0; cidx < ncs; ++cidx)
            CHECK(t.lm_src[(size_t)i * ncs + cidx] == own(g, cidx) && t.lm_l[(size_t)i * ncs + cidx] == (cidx < 128 ? (cidx % 4) * 8 + cidx / 16 : 32),
                  "local model %d", cidx);
        for (int o = 0; o < nout; ++o) {
            CHECK(t.asm_dst[(size_t)ids[i] * nout + o] == own(g, o), "assembly of output %d", o);
            // a training target is the feedback element read from the output's own grid point
            const int ti = t.tgt_idx[(size_t)i * nout + o];
            CHECK(ti >= 0 && ti < ninp[i] && t.fb_src[base + ti] == own(g, o), "training target %d at %d", o, ti);
        }
        base += ninp[i];
    }
    CHECK(tt == t.tisr_fb.size() && tt == t.tisr_grid.size() && tt == t.tisr_reg.size(), "tisr entries %zu", tt);
    // every grid element is written by exactly one (region, output) of the assembly
    std::vector<int> hits(kGrid4d + 2 * kGrid2d, 0);
    for (int32_t d : t.asm_dst)
        if (d >= 0 && d < (int)hits.size()) ++hits[d];
    int bad = 0;
    for (int h : hits) bad += h != 1;
    g_case = "tables assembly";
    CHECK(bad == 0, "%d grid elements not written exactly once", bad);

    g_case = "tables generic";
    std::vector<int8_t> out_l = {3, -1, 35, 0, 7};
    RegionTables gt;
    const int rcg = build_region_tables({numregions, nl, ncs, 5, geom, sst, ninp, plan.rd.data(), plan.tot_fb, out_l.data()}, &gt);
    CHECK(rcg == SML_OK && gt.outl == out_l, "outl");
    CHECK(gt.asm_dst.empty() && gt.fb_src.empty() && gt.fb_l.empty() && gt.fb_reg.empty() && gt.lm_src.empty() && gt.lm_l.empty() &&
              gt.tisr_fb.empty() && gt.tisr_grid.empty() && gt.tisr_reg.empty() && gt.tgt_idx.empty(), "a generic context has only outl");
}

// ---------------------------------------------------------------- the step's shape
// step_shape against the predicates as the launchers used to spell them, each where it
// was used, with their numbers written out (1024 threads, 7 staged entries, 17 rows and
// 8 waves, 7 groups of 19, 64 KiB): on both sides of every edge, then a random sweep.
struct WantShape {
    int lds_x, lds_buf, parts, rows, groups, wpb;
    size_t lds_region, lds_bal, lds_drive;
    bool region_lds, wide, balanced, begin_fused, finish_grouped, drive_fused;
};

static WantShape want_shape(const StepShapeIn &in) {
    WantShape w;
    // launch_update
    const int max_parts = std::max(1, (in.maxn + 1024 - 1) / 1024);
    w.parts = in.nlocal ? std::max(1, std::min(max_parts, (512 + in.nlocal - 1) / in.nlocal)) : 1;
    w.lds_x = (in.maxn + 1) / 2 * 2;
    w.lds_buf = w.lds_x + in.maxninp;
    w.lds_region = (size_t)(w.lds_x + in.maxninp) * sizeof(double);
    w.region_lds = w.lds_region <= 64 * 1024;
    // bal_usable / launch_update_bal
    w.lds_bal = 2 * (size_t)((in.maxn + 1) / 2 * 2 + in.maxninp) * sizeof(double);
    w.balanced = !in.per_region && in.nlocal != 0 && in.ell_ok && in.maxn <= 7 * 1024 && in.maxninp <= 1024 &&
                 w.lds_bal <= in.max_lds;
    // begin_fusable (kBeginThreads / 64 = 512 / 64)
    w.begin_fused = in.begin_mode > 0 && in.nout_pad % 17 == 0 && in.nout_pad / 17 <= 512 / 64 &&
                    (size_t)(w.lds_x + in.maxninp) * sizeof(double) <= 64 * 1024;
    // launch_readout
    w.wide = in.nout_pad % 17 == 0 && in.nout_pad / 17 <= 8;
    w.rows = w.wide ? 17 : 8;
    w.groups = in.nout_pad / w.rows;
    w.wpb = w.wide ? 2 : 4;
    // launch_finish_grid
    w.finish_grouped = in.ncs > 0 && in.nout_pad % 4 == 0 && in.nout_pad <= 144 && in.nout_pad / 4 * 7 <= 256 &&
                       (in.ncs + 7 - 1) / 7 <= 19 && !in.finish_ungrouped;
    // drive_lds / sml_res_train_drive
    w.lds_drive = 2 * (size_t)((in.maxn + 1) / 2 * 2 + in.maxninp) * sizeof(double);
    w.drive_fused = !(in.stepwise_drive || w.lds_drive > in.max_lds);
    return w;
}

static void check_shape_one(const StepShapeIn &in) {
    const StepShape s = step_shape(in);
    const WantShape w = want_shape(in);
    CHECK(s.lds_x == w.lds_x && s.lds_buf == w.lds_buf, "lds_x %d %d lds_buf %d %d", s.lds_x, w.lds_x, s.lds_buf,
          w.lds_buf);
    CHECK(s.lds_region == w.lds_region && s.lds_bal == w.lds_bal && s.lds_drive == w.lds_drive,
          "lds %zu %zu / %zu %zu / %zu %zu", s.lds_region, w.lds_region, s.lds_bal, w.lds_bal, s.lds_drive,
          w.lds_drive);
    CHECK(s.parts == w.parts, "parts %d %d", s.parts, w.parts);
    CHECK(s.region_lds == w.region_lds, "region_lds %d %d", s.region_lds, w.region_lds);
    CHECK(s.wide == w.wide && s.rows == w.rows && s.groups == w.groups && s.wpb == w.wpb,
          "readout %d %d %d %d, want %d %d %d %d", s.wide, s.rows, s.groups, s.wpb, w.wide, w.rows, w.groups, w.wpb);
    CHECK(s.balanced == w.balanced, "balanced %d %d", s.balanced, w.balanced);
    CHECK(s.begin_fused == w.begin_fused, "begin_fused %d %d", s.begin_fused, w.begin_fused);
    CHECK(s.finish_grouped == w.finish_grouped, "finish_grouped %d %d", s.finish_grouped, w.finish_grouped);
    CHECK(s.drive_fused == w.drive_fused, "drive_fused %d %d", s.drive_fused, w.drive_fused);
}

static void check_shape() {
    // the T30L8 hybrid context: n 6048, ninp 804 with sst, nout 136, ncs 132, 1152 regions
    const StepShapeIn base{6048, 804, 136, 132, 1152, 163840, true, 0, false, false, false};
    auto with = [&](const char *name, auto set) {
        g_case = std::string("shape ") + name;
        StepShapeIn in = base;
        set(in);
        check_shape_one(in);
        return step_shape(in);
    };
    {   // the values the GPU tests pin (test_reservoir_edges_gpu.py), and the default's forms
        const StepShape s = with("base", [](StepShapeIn &) {});
        CHECK(s.balanced && !s.begin_fused && s.finish_grouped && s.drive_fused && s.wide && s.groups == 8 &&
                  s.parts == 1 && s.lds_x == 6048,
              "the default context's forms");
    }
    // maxn at kStageX * kUpdThreads, and the odd count below it (lds_x rounds up)
    CHECK(with("maxn 7168", [](StepShapeIn &in) { in.maxn = 7168; }).balanced, "balanced at 7168");
    CHECK(!with("maxn 7169", [](StepShapeIn &in) { in.maxn = 7169; }).balanced, "per region at 7169");
    CHECK(with("maxn 7167", [](StepShapeIn &in) { in.maxn = 7167; }).lds_x == 7168, "odd maxn");
    CHECK(with("maxninp 1024", [](StepShapeIn &in) { in.maxninp = 1024; }).balanced, "balanced at 1024");
    CHECK(!with("maxninp 1025", [](StepShapeIn &in) { in.maxninp = 1025; }).balanced, "per region at 1025");
    // the balanced and the drive LDS (2 (lds_x + maxninp) doubles) at max_lds and one row over
    for (size_t max_lds : {(size_t)65536, (size_t)163840}) {
        const int rows = (int)(max_lds / 16);  // lds_x + maxninp at the limit
        for (int over : {0, 1}) {
            const StepShape s = with("lds edge", [&](StepShapeIn &in) {
                in.max_lds = max_lds;
                in.maxninp = 500;
                in.maxn = rows - 500 + 2 * over;  // (even: lds_x = maxn)
            });
            CHECK(s.lds_bal == max_lds + 32 * (size_t)over, "lds_bal %zu", s.lds_bal);
            // (at 163840 the rows alone pass kStageX * kUpdThreads, so only the drive shows this edge)
            CHECK(s.balanced == (!over && rows - 500 <= 7168), "balanced %d at max_lds %zu + %d", s.balanced,
                  max_lds, over);
            CHECK(s.drive_fused == !over, "drive_fused %d at max_lds %zu + %d", s.drive_fused, max_lds, over);
        }
        // the balanced edge below the row bound: more inputs than rows
        for (int over : {0, 1}) {
            const StepShape s = with("lds edge, wide u", [&](StepShapeIn &in) {
                in.max_lds = max_lds;
                in.maxninp = 1024;
                in.maxn = std::min(rows - 1024, 7168) + 2 * over;
            });
            CHECK(s.balanced == !over, "balanced %d at max_lds %zu + %d", s.balanced, max_lds, over);
        }
    }
    // the per-region LDS at 64 KiB and 8 bytes over
    CHECK(with("region 64 KiB", [](StepShapeIn &in) { in.maxn = 8192 - 804; }).region_lds, "staged at 64 KiB");
    CHECK(!with("region 64 KiB + 8", [](StepShapeIn &in) { in.maxn = 8192 - 804; in.maxninp = 805; }).region_lds,
          "global at 64 KiB + 8");
    for (int mode : {1, 2}) {
        CHECK(with("fused 64 KiB", [&](StepShapeIn &in) { in.begin_mode = mode; in.maxn = 8192 - 804; }).begin_fused,
              "fused at 64 KiB");
        CHECK(!with("fused 64 KiB + 8", [&](StepShapeIn &in) {
                   in.begin_mode = mode;
                   in.maxn = 8192 - 804;
                   in.maxninp = 805;
               }).begin_fused,
              "split at 64 KiB + 8");
    }
    // nout_pad: 17 * 8, 17 * 9 (a multiple of 17 past the waves; rounded to kRows it is 160, not wide
    // either), a multiple of kRows that is none of 17
    CHECK(with("nout_pad 136", [](StepShapeIn &in) { in.nout_pad = 136; in.begin_mode = 1; }).begin_fused, "136");
    {
        const StepShape s = with("nout_pad 153", [](StepShapeIn &in) { in.nout_pad = 153; in.begin_mode = 1; });
        CHECK(!s.wide && !s.begin_fused && s.rows == 8, "153");
    }
    {
        const StepShape s = with("nout_pad 144", [](StepShapeIn &in) { in.nout_pad = 144; in.begin_mode = 2; });
        CHECK(!s.wide && !s.begin_fused && s.rows == 8 && s.groups == 18 && s.wpb == 4, "144");
    }
    CHECK(with("nout_pad 17", [](StepShapeIn &in) { in.nout_pad = 17; }).groups == 1, "17");
    // the grouped finish
    CHECK(with("ncs 133", [](StepShapeIn &in) { in.ncs = 133; }).finish_grouped, "ncs 133");
    CHECK(!with("ncs 134", [](StepShapeIn &in) { in.ncs = 134; }).finish_grouped, "ncs 134");
    CHECK(!with("ncs 0", [](StepShapeIn &in) { in.ncs = 0; }).finish_grouped, "ncs 0");
    CHECK(with("finish 144", [](StepShapeIn &in) { in.nout_pad = 144; }).finish_grouped, "nout_pad 144");
    CHECK(!with("finish 148", [](StepShapeIn &in) { in.nout_pad = 148; }).finish_grouped, "nout_pad 148");
    CHECK(!with("finish 152", [](StepShapeIn &in) { in.nout_pad = 152; }).finish_grouped, "nout_pad 152");
    CHECK(!with("ungrouped", [](StepShapeIn &in) { in.finish_ungrouped = true; }).finish_grouped, "the switch");
    // parts: 512 block slots over the regions, a 1024-row pass each at least
    CHECK(with("nlocal 1", [](StepShapeIn &in) { in.nlocal = 1; }).parts == 6, "nlocal 1");
    CHECK(with("nlocal 1 small", [](StepShapeIn &in) { in.nlocal = 1; in.maxn = 1024; }).parts == 1, "one pass");
    CHECK(with("nlocal 1 1025", [](StepShapeIn &in) { in.nlocal = 1; in.maxn = 1025; }).parts == 2, "two passes");
    CHECK(with("nlocal 256", [](StepShapeIn &in) { in.nlocal = 256; }).parts == 2, "nlocal 256");
    CHECK(with("nlocal 512", [](StepShapeIn &in) { in.nlocal = 512; }).parts == 1, "nlocal 512");
    CHECK(with("nlocal 513", [](StepShapeIn &in) { in.nlocal = 513; }).parts == 1, "nlocal 513");
    CHECK(with("nlocal 511", [](StepShapeIn &in) { in.nlocal = 511; }).parts == 2, "nlocal 511");
    CHECK(!with("nlocal 0", [](StepShapeIn &in) { in.nlocal = 0; }).balanced, "nlocal 0");
    // the begin modes, the reference-path switches alone, a region out of ELL form
    CHECK(!with("mode 0", [](StepShapeIn &in) { in.begin_mode = 0; }).begin_fused, "mode 0");
    CHECK(with("mode 1", [](StepShapeIn &in) { in.begin_mode = 1; }).begin_fused, "mode 1");
    CHECK(with("mode 2", [](StepShapeIn &in) { in.begin_mode = 2; }).begin_fused, "mode 2");
    {
        const StepShape s = with("per region", [](StepShapeIn &in) { in.per_region = true; });
        CHECK(!s.balanced && s.finish_grouped && s.drive_fused, "per_region alone");
    }
    {
        const StepShape s = with("ungrouped alone", [](StepShapeIn &in) { in.finish_ungrouped = true; });
        CHECK(s.balanced && !s.finish_grouped && s.drive_fused, "finish_ungrouped alone");
    }
    {
        const StepShape s = with("stepwise", [](StepShapeIn &in) { in.stepwise_drive = true; });
        CHECK(s.balanced && s.finish_grouped && !s.drive_fused, "stepwise_drive alone");
    }
    CHECK(!with("csr", [](StepShapeIn &in) { in.ell_ok = false; }).balanced, "a region in CSR form");
    // a sweep around every edge at once
    g_case = "shape sweep";
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    auto next = [&](int n) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        return (int)((rng >> 33) % (uint64_t)n);
    };
    const int maxns[] = {1, 2, 1023, 1024, 1025, 6048, 7167, 7168, 7169, 7388, 9216, 10240, 65535};
    const int ninps[] = {1, 804, 805, 1023, 1024, 1025, 4096, 65535};
    const int nouts[] = {8, 16, 17, 34, 136, 144, 148, 152, 153, 160, 272, 280};
    const int ncss[] = {0, 1, 7, 19, 132, 133, 134, 256};
    const int nlocals[] = {0, 1, 2, 255, 256, 511, 512, 513, 1152};
    const size_t ldss[] = {0, 65536, 163840};
    for (int t = 0; t < 6000; ++t) {
        StepShapeIn in;
        in.maxn = next(2) ? maxns[next(13)] : 1 + next(12000);
        in.maxninp = next(2) ? ninps[next(8)] : 1 + next(2000);
        in.nout_pad = next(2) ? nouts[next(12)] : 1 + next(300);
        in.ncs = next(2) ? ncss[next(8)] : next(300);
        in.nlocal = next(2) ? nlocals[next(9)] : next(1300);
        in.max_lds = next(4) ? ldss[next(3)] : (size_t)16 * (in.maxn + in.maxninp + next(5) - 2);
        in.ell_ok = next(4) != 0;
        in.begin_mode = next(3);
        in.per_region = next(4) == 0;
        in.finish_ungrouped = next(4) == 0;
        in.stepwise_drive = next(4) == 0;
        check_shape_one(in);
    }
}

int main() {
    std::vector<Case> cases;
    auto lens = [](int n, int base) { return std::vector<int>(n, base); };
    cases.push_back(make("n1", 1, 1, lens(1, 1)));
    cases.push_back(make("n1 duplicates", 1, 1, lens(1, 3)));
    cases.push_back(make("k0", 65, 5, lens(65, 0)));
    for (int n : {63, 64, 65}) {
        for (int pos : {0, n - 1, 63, 64}) {  // one row longer: first, last, word edges
            if (pos >= n) continue;
            std::vector<int> l = lens(n, 2);
            l[pos] = 3;
            cases.push_back(make("n" + std::to_string(n) + " long row " + std::to_string(pos), n, 1, l));
        }
        cases.push_back(make("n" + std::to_string(n) + " hybrid sizes", n, 1, lens(n, 2), kBlockDiag, 132, 136));
    }
    for (int m = 1; m <= 9; ++m) {  // each side of the cost choice, odd and even widths, the cap and past it
        for (int n : {1, 2, 3, 130}) cases.push_back(make("equal " + std::to_string(m) + " n" + std::to_string(n), n, 1, lens(n, m)));
        std::vector<int> few = lens(130, m - 1), many = lens(130, m);
        few[64] = m;
        many[129] = m - 1;
        cases.push_back(make("few rows of " + std::to_string(m), 130, 1, few));
        cases.push_back(make("most rows of " + std::to_string(m), 130, 1, many));
    }
    // a longest row past the 8 reserved slots in a region that has them (k / n + 1 <= 8):
    // only pack_region's own comparison keeps a 9-wide copy out of an 8 n pool share
    for (int base : {2, 7}) {
        std::vector<int> l = lens(131, base);
        l[64] = 9;
        cases.push_back(make("one row of 9 among rows of " + std::to_string(base), 131, 1, l));
        g_case = cases.back().name;
        CHECK((int)cases.back().rows.size() / 131 + 1 <= 8, "the case reserves no ELL slots");
    }
    {
        Case c;
        c.name = "duplicate entries";
        c.n = 4;
        c.ninp = 2;
        c.rows = {1, 1, 3, 1, 4, 3};
        c.cols = {2, 2, 1, 2, 4, 1};
        cases.push_back(c);
    }
    cases.push_back(make("win block q11", 66, 6, lens(66, 2), kBlockDiag, 132, 5));
    cases.push_back(make("win block q1", 66, 66, lens(66, 2)));
    cases.push_back(make("win permuted", 66, 6, lens(66, 2), kPermuted));
    cases.push_back(make("win one per row, n % ninp != 0", 65, 6, lens(65, 2), kOnePerRowNoBlock));
    cases.push_back(make("win zero and two", 66, 6, lens(66, 2), kZeroAndTwo));
    cases.push_back(make("win dense", 7, 5, lens(7, 2), kDense, 0, 136));
    for (const Case &c : cases) check_region_all(c);
    const Case csr = make("n65 long row 63", 65, 1, [&] {  // a CSR-only context: no ELL copy
        std::vector<int> l = lens(65, 2);
        l[63] = 3;
        return l;
    }());
    check_region<float, float>(csr, true);
    check_region<double, double>(csr, true);
    check_region<float, float>(make("n65535 q65535", 65535, 1, lens(65535, 1), kBlockDiag, 0, 1));

    // the magic of every block length at the largest n (a dense 65535 x 21845 W_in is not held)
    for (int q : {1, 3, 65535}) {
        g_case = "magic q " + std::to_string(q);
        const uint32_t magic = win_magic(q);
        // q = 1: ceil(2^32 / 1) wraps to 0 in 32 bits, which pack_region's own comparison
        // rejects ("win block q1" above: stored columns); every other q must divide exactly
        if (q == 1) CHECK(magic == 0, "magic %u", magic);
        for (int i = 0; i < 65535 && q > 1; ++i)
            CHECK((uint32_t)(((uint64_t)i * magic) >> 32) == (uint32_t)(i / q), "umulhi(%d, %u) != %d / %d", i, magic, i, q);
    }

    // a double that float does not hold; NaN (A and W_in reject it, W_out keeps it)
    const double nan = std::numeric_limits<double>::quiet_NaN();
    check_reject<double, float>("A", 0, 0.1, false, "A value 1 not representable in the storage dtype");
    check_reject<double, float>("W_in", 1, 0.1, false, "W_in value not representable in the storage dtype");
    check_reject<double, float>("W_out", 2, 0.1, false, "W_out value not representable in the storage dtype");
    check_reject<double, double>("0.1 in double storage", 0, 0.1, true, "");
    check_reject<double, double>("A NaN", 0, nan, false, "A value 1 not representable");
    check_reject<float, float>("W_in NaN", 1, (float)nan, false, "W_in value not representable");
    check_reject<double, float>("W_out NaN", 2, nan, true, "");
    check_reject<float, double>("W_out NaN", 2, (float)nan, true, "");
    check_reject<float, float>("A column", 3, 0.f, false, "A entry 2 out of range (row 3 col 4, n 3)");

    for (int ncs : {0, 132})
        for (bool csr : {false, true}) check_plan(ncs, ncs ? 136 : 8, csr);
    check_blocks();
    check_tables();
    check_shape();
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail != 0;
}
