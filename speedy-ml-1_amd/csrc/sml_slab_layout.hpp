// sml_slab_layout.hpp -- the slab ocean's index tables (sendrecievegrid's sst half,
// mpires.f90:288-478, 575-767): what sml_hybrid_set_slab and sml_slab_create upload,
// computed on the host with no HIP call in between, so the index arithmetic and its
// consistency checks run (and are sanitised) on a CPU: tests/slab_layout_check.cpp.
#pragma once

#include <cstdint>
#include <vector>

#include "sml_internal.hpp"

namespace sml {

// the atmo context's local regions and the slab context's reservoirs, as sml_res_info,
// sml_res_ninp and sml_res_feedback_offsets report them
struct SlabLayoutIn {
    int numregions, nlocal, nout;  // the atmo context
    const int *ids;                // [nlocal] region ids
    const int *ninp;               // [nlocal] feedback lengths
    const int64_t *off;            // [nlocal + 1] feedback offsets
    int snum, nslab, sncs, snout;  // the slab context: its decomposition, reservoirs, chunk_speedy, nout
    const int *sids;               // [nslab] region ids
    const int *sninp;              // [nslab] feedback lengths
    const int64_t *soff;           // [nslab + 1] feedback offsets
};

struct SlabTables {
    // atmo_training_data_idx (mod_slab_ocean_reservoir.f90:1550-1563) of every sst region:
    // the slab feedback's entry e is the atmo feedback's entry ring_src[e] (7 * in2d a region)
    std::vector<int32_t> ring_src;
    std::vector<int32_t> row;  // [nslab] the slab reservoir's local atmo row
    // the atmo feedback's sst entries: feedback index, grid2d index of the overlap-tile
    // point, slab reservoir
    std::vector<int32_t> sfb, sgrid;
    std::vector<uint16_t> sreg;
    // wholegrid_sst point (96 x 48) -> its region's exchange row and sst column
    // (region * xw + nout + lx + resx * ly)
    std::vector<int32_t> src;
    int xw = 0;  // the exchange row: nout + resx * resy
};

// timestep_slab a multiple >= 2 of timestep (the ring holds timestep_slab / timestep - 1 columns)
int check_slab_cadence(int timestep, int timestep_slab);

// The tables above, after the checks of sml_hybrid_set_slab: an ML-only slab context over
// the same regions, nout = resx * resy, the slab reservoirs are the local sst regions in
// order, 7 * in2d inputs each.
int build_slab_tables(const SlabLayoutIn &in, SlabTables *out);

// The slab training series' table (sml_slab_train_series): slab feedback entry e's source in
// the index space of one step of a training series (SeriesTables::src: the 4-d grid's
// kGrid4d doubles, then logp, precip, sst, tisr of kGrid2d points each), the mean / std slot
// of that source (SeriesTables::l) and the local atmo row whose statistics standardise it,
// composed through ring_src:  src[e] = ser_src[ring_src[e]], l[e] = ser_l[ring_src[e]],
// row[e] = the atmo region holding feedback entry ring_src[e].
struct SlabSeriesTables {
    std::vector<int32_t> src;   // [slab feedback]
    std::vector<uint8_t> l;     // [slab feedback]
    std::vector<uint16_t> row;  // [slab feedback]
};

// ser_src / ser_l: the atmo context's SeriesTables::src / l, ser_len = its packed feedback
// size.  The checks are build_slab_tables' (its refusals carry through), then the series
// tables' length.
int build_slab_series_tables(const SlabLayoutIn &in, const int32_t *ser_src, const uint8_t *ser_l, int64_t ser_len,
                             SlabSeriesTables *out);

// sml_slab_target_index: the training targets' positions in the slab feedback of a region
// [ 4 variables of the lowest level (v, x, y) | logp | sst | tisr ], each over the input tile:
// entry 5 * in2d + the input-tile position of resolved point o -- the sst section's inner
// tile (tile_full_input_to_target_data2d_ocean_model, res_domain.f90:691-716), in the order
// of the slab outvec (x fastest).  Returns their count, resx * resy.
inline int slab_target_index(const RegionGeom &g, int32_t *idx) {
    std::vector<int32_t> t((size_t)(kVars * kZGrid + 2) * g.inx * g.iny);
    region_target_index(g, t.data());  // its logp block: the inner tile's points, x fastest
    const int in2d = g.inx * g.iny, natmo = kVars * in2d * kZGrid, res2d = g.resx * g.resy;
    for (int o = 0; o < res2d; ++o) idx[o] = 5 * in2d + (t[(size_t)kVars * res2d * kZGrid + o] - natmo);
    return res2d;
}

}  // namespace sml
