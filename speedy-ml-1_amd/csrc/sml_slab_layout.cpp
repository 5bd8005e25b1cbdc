// sml_slab_layout.cpp -- the slab ocean's index tables (sml_slab_layout.hpp).  Host only.
#include "sml_slab_layout.hpp"

namespace sml {

int check_slab_cadence(int timestep, int timestep_slab) {
    SML_REQUIRE(timestep > 0 && timestep_slab % timestep == 0 && timestep_slab / timestep >= 2,
                "timestep_slab (%d) must be a multiple >= 2 of timestep (%d)", timestep_slab, timestep);
    return SML_OK;
}

int build_slab_tables(const SlabLayoutIn &in, SlabTables *out) {
    SML_REQUIRE(out && in.nlocal >= 0 && in.nslab >= 0 && (in.nlocal == 0 || (in.ids && in.ninp && in.off)) &&
                    (in.nslab == 0 || (in.sids && in.sninp && in.soff)),
                "bad argument");
    SML_REQUIRE(in.snum == in.numregions && in.sncs == 0, "the slab context must be ML-only (chunk_speedy 0) over the "
                "same %d regions", in.numregions);
    RegionGeom g0{};
    SML_REQUIRE(region_geom(in.numregions, 0, &g0) && in.snout == g0.resx * g0.resy,
                "the slab reservoirs predict the sst of the region's %d points, not %d", g0.resx * g0.resy, in.snout);
    *out = SlabTables();
    // the slab reservoirs are those of the rank's regions with an sst input, in order
    // (trained_ocean_reservoir_prediction: sst_bool_prediction <=> sst input)
    int j = 0;
    for (int i = 0; i < in.nlocal; ++i) {
        RegionGeom g{};
        SML_REQUIRE(region_geom(in.numregions, in.ids[i], &g), "local region %d: %d is no region of %d", i, in.ids[i],
                    in.numregions);
        const int in2d = g.inx * g.iny, natmo = kVars * in2d * kZGrid;
        const bool sst = in.ninp[i] == region_ninp(g, true);
        if (!sst) continue;
        SML_REQUIRE(j < in.nslab && in.sids[j] == in.ids[i],
                    "slab reservoir %d is not the rank's sst region %d (local %d)", j, in.ids[i], i);
        SML_REQUIRE(in.sninp[j] == 7 * in2d && in.soff[j + 1] - in.soff[j] == in.sninp[j],
                    "slab reservoir of region %d: %d inputs, the atmo subset has %d", in.ids[i], in.sninp[j], 7 * in2d);
        // atmo_training_data_idx (mod_slab_ocean_reservoir.f90:1550-1563): the lowest
        // level's 4 variables and logp, the sst, the tisr of the atmo feedback
        for (int e = natmo - kVars * in2d; e < natmo + in2d; ++e) out->ring_src.push_back((int32_t)(in.off[i] + e));
        for (int e = natmo + 2 * in2d; e < natmo + 4 * in2d; ++e) out->ring_src.push_back((int32_t)(in.off[i] + e));
        out->row.push_back(i);
        for (int p = 0; p < in2d; ++p) {  // the sst entries of the atmo feedback
            const int lx = p % g.inx, ly = p / g.inx;
            out->sfb.push_back((int32_t)(in.off[i] + natmo + 2 * in2d + p));
            out->sgrid.push_back(g2(input_x(g, lx + 1) - 1, g.in_ystart - 1 + ly));
            out->sreg.push_back((uint16_t)j);
        }
        ++j;
    }
    SML_REQUIRE(j == in.nslab, "%d slab reservoirs for %d sst regions", in.nslab, j);
    // wholegrid_sst point -> its region's exchange row and sst column
    const int xw = in.nout + in.snout;
    out->xw = xw;
    out->src.assign(kGrid2d, -1);
    for (int r = 0; r < in.numregions; ++r) {
        RegionGeom g{};
        region_geom(in.numregions, r, &g);
        for (int ly = 0; ly < g.resy; ++ly)
            for (int lx = 0; lx < g.resx; ++lx) {
                int32_t &s = out->src[g2(g.res_xstart - 1 + lx, g.res_ystart - 1 + ly)];
                SML_REQUIRE(s < 0, "grid point (%d, %d) belongs to two regions", g.res_xstart + lx, g.res_ystart + ly);
                s = r * xw + in.nout + lx + g.resx * ly;
            }
    }
    for (int p = 0; p < kGrid2d; ++p) SML_REQUIRE(out->src[p] >= 0, "grid point %d belongs to no region", p);
    return SML_OK;
}

int build_slab_series_tables(const SlabLayoutIn &in, const int32_t *ser_src, const uint8_t *ser_l, int64_t ser_len,
                             SlabSeriesTables *out) {
    SML_REQUIRE(out, "bad argument");
    *out = SlabSeriesTables();
    SlabTables tb;
    if (int rc = build_slab_tables(in, &tb)) return rc;
    const int64_t tot_fb = in.nlocal ? in.off[in.nlocal] : 0;
    SML_REQUIRE(ser_len == tot_fb && (tot_fb == 0 || (ser_src && ser_l)),
                "the series tables hold %lld entries, the atmo feedback %lld", (long long)ser_len, (long long)tot_fb);
    const size_t n = tb.ring_src.size();
    out->src.resize(n);
    out->l.resize(n);
    out->row.resize(n);
    size_t e = 0;
    for (size_t j = 0; j < tb.row.size(); ++j) {
        const int i = tb.row[j];
        for (int64_t k = in.soff[j]; k < in.soff[j + 1]; ++k, ++e) {
            const int32_t a = tb.ring_src[e];
            SML_REQUIRE(a >= in.off[i] && a < in.off[i + 1], "slab entry %zu leaves its region's feedback", e);
            out->src[e] = ser_src[a];
            out->l[e] = ser_l[a];
            out->row[e] = (uint16_t)i;
        }
    }
    SML_REQUIRE(e == n, "the slab feedback holds %zu entries, the atmo subsets %zu", e, n);
    return SML_OK;
}

}  // namespace sml

// the slab's training targets inside the slab feedback of a region (slab_target_index,
// sml_slab_layout.hpp): idx holds resx * resy entries, 4 at 1152 regions
extern "C" int sml_slab_target_index(int numregions, int region, int32_t *idx, int *count) {
    SML_REQUIRE(idx && count, "null argument");
    sml::RegionGeom r;
    SML_REQUIRE(sml::region_geom(numregions, region, &r), "region %d of %d does not decompose the grid", region,
                numregions);
    *count = sml::slab_target_index(r, idx);
    return SML_OK;
}
