// sml_hybrid_layout.cpp -- the hybrid loop's host arithmetic (sml_hybrid_layout.hpp): the
// exchange plan, the reference's calendar, the loop's calendar and schedule, and the
// res_domain wrappers of the C ABI.  No HIP, no RCCL.
#include "sml_hybrid_layout.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace sml;

// ------------------------------------------------------------- exchange plan
// The all-gather's layout for `world` ranks of processor_decomposition
// (res_domain.f90:31-62): every rank sends its outvecs zero-padded to the largest
// share maxc, so the receive buffer is [world][maxc][nout]; region r (0-based) sits
// at slab row perm[r] = rank * maxc + (position of r in the rank's list).  With even
// shares (numregions % world == 0) the slabs are already global region order
// (*contiguous = 1); else rank q in 1..left also owns region numregions - left + q - 1
// at the end of its list and k_gather_rows applies perm.  perm may be NULL.
extern "C" int sml_exchange_plan(int numregions, int world, int *maxc, int *contiguous, int32_t *perm) {
    SML_REQUIRE(numregions > 0 && world >= 1 && world <= numregions && maxc && contiguous, "bad argument");
    std::vector<int> all(numregions);
    int mc = 0, c0 = -1;
    bool contig = true;
    for (int r = 0; r < world; ++r) mc = std::max(mc, processor_regions(numregions, world, r, all.data()));
    std::vector<int32_t> p(numregions, -1);
    for (int r = 0; r < world; ++r) {
        const int c = processor_regions(numregions, world, r, all.data());
        if (c0 < 0) c0 = c;
        if (c != c0) contig = false;
        for (int i = 0; i < c; ++i) {
            SML_REQUIRE(p[all[i]] < 0, "region %d owned twice", all[i]);
            p[all[i]] = r * mc + i;
            if (all[i] != r * c0 + i) contig = false;
        }
    }
    for (int r = 0; r < numregions; ++r) SML_REQUIRE(p[r] >= 0, "region %d owned by no rank", r);
    *maxc = mc;
    *contiguous = contig ? 1 : 0;
    if (perm) std::memcpy(perm, p.data(), sizeof(int32_t) * numregions);
    return SML_OK;
}

// ------------------------------------------------------------------ calendar
// The reference's calendar arithmetic (src/mod_calendar.f90), restated with its
// quirks: get_current_time_delta_hour (:24-92) counts years of 8760 h from the
// start year (start month / day / hour unused), subtracts the leap days of the
// elapsed years, walks a 365-day month table whose February it sets to 29 in a leap
// year -- the table is a SAVEd local, so once a leap year is met February keeps 29
// days for the rest of the run (*feb29 carries that state) -- and an exact month
// boundary falls to December 31 of the year before; numof_hours_into_year
// (:133-175) counts whole months, days, the hour, and 0 -> 1.  get_tisr_by_date
// (mpires.f90:1665-1671) then wraps indices past 8760 by 8760.
namespace {
bool leap_year(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }  // leap_year_check :94-106
}  // namespace

// get_current_time_delta_hour (mod_calendar.f90:24-92): date[4] = currentyear,
// currentmonth, currentday, currenthour after hours_elapsed hours from startyear
extern "C" int sml_calendar_delta_hour(int startyear, int64_t hours_elapsed, int *feb29, int *date) {
    SML_REQUIRE(feb29 && date && hours_elapsed >= 0, "bad argument");
    const int64_t hours_in_year = 8760, hours_in_a_day = 24;
    const int64_t years = hours_elapsed / hours_in_year;
    int year = (int)(years + startyear);
    int leap_days = 0;
    for (int64_t i = 0; i < years; ++i)
        if (leap_year(startyear + (int)i)) ++leap_days;
    if (leap_year(year)) *feb29 = 1;
    const int ncal[12] = {31, *feb29 ? 29 : 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    const int64_t day_of_year = (hours_elapsed % hours_in_year) / hours_in_a_day - leap_days;
    int64_t counter = day_of_year;
    int month = 1;
    while (counter > 0) {
        counter -= ncal[month - 1];
        ++month;
    }
    month -= 1;
    if (month <= 0) {
        month = 12;
        year -= 1;
    }
    date[0] = year;
    date[1] = month;
    date[2] = (int)(ncal[month - 1] + counter);
    date[3] = (int)(hours_elapsed % hours_in_a_day);
    return SML_OK;
}

extern "C" int sml_tisr_date_index(int startyear, int64_t hours_elapsed, int *feb29, int *index) {
    SML_REQUIRE(feb29 && index && hours_elapsed >= 0, "bad argument");
    int d[4];
    if (int rc = sml_calendar_delta_hour(startyear, hours_elapsed, feb29, d)) return rc;
    const int year = d[0], month = d[1], day = d[2], hour = d[3];
    // numof_hours_into_year(year, month, day, hour) with the year's own leap table
    const bool ly = leap_year(year);
    const int nmon[12] = {31, ly ? 29 : 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    int64_t n = 0;
    for (int i = 1; i < month; ++i) n += 24 * nmon[i - 1];
    for (int i = 1; i < day; ++i) n += 24;
    n += hour;
    if (n == 0) n = 1;
    if (n > 24 * 365) n -= 24 * 365;
    *index = (int)n;
    return SML_OK;
}

// ------------------------------------------------------------ the loop's calendar
void LoopCalendar::set_calendar(int startyear_, int64_t hours_base, int step_hours_) {
    startyear = startyear_;
    base = hours_base;
    step_hours = step_hours_;
    feb29 = 0;
    t = 0;
    cal_on = true;
}

void LoopCalendar::set_tisr_table(int nhours_, int startyear_, int64_t hours_base, int step_hours_) {
    nhours = nhours_;
    startyear = startyear_;
    base = hours_base;
    step_hours = step_hours_;
    feb29 = 0;
    t = 0;
}

int LoopCalendar::window_date(int *date) const {
    int latch = feb29;
    return sml_calendar_delta_hour(startyear, base + (t + 1) * step_hours, &latch, date);
}

int LoopCalendar::next_date(int *date) {
    return sml_calendar_delta_hour(startyear, base + (t + 1) * step_hours, &feb29, date);
}

int LoopCalendar::tisr_index(int *index) {
    int idx = 0;
    if (int rc = sml_tisr_date_index(startyear, base + (t - 1) * step_hours, &feb29, &idx)) return rc;
    if (idx < 1 || idx > nhours) return fail(SML_ERR_ARG, "tisr hour %d outside the table's %d hours", idx, nhours);
    *index = idx;
    return SML_OK;
}

// ------------------------------------------------------------ the loop's schedule
LoopSchedule sml::loop_schedule(const LoopScheduleIn &in) {
    LoopSchedule s;
    // hop mode: SML_HOP_AUTO (kernel hops on CU-disjoint streams, event hops when dispatch
    // is serialised or SML_HYBRID_EVENTS=1, wait-value hops otherwise), SML_HOP_WAIT_VALUE,
    // SML_HOP_EVENTS, SML_HOP_KERNEL
    if (in.hop_mode == SML_HOP_AUTO) {
        // kernel hops only when the two streams run on disjoint CUs (res_cus > 0): a
        // waiting finish's blocks then never occupy a CU the window (their producer)
        // needs; not when dispatch is serialised (a waiting kernel would hold its queue
        // ahead of its producer) or SML_HYBRID_EVENTS=1 asks for event hops (the PMC
        // passes of profiles/collect.sh)
        s.use_events = in.env_events || in.serialised;
        s.use_kernels = !s.use_events && in.cu_split;
    } else {
        s.use_events = in.hop_mode == SML_HOP_EVENTS;
        s.use_kernels = in.hop_mode == SML_HOP_KERNEL;
    }
    s.hop_effective = s.use_events ? SML_HOP_EVENTS : s.use_kernels ? SML_HOP_KERNEL : SML_HOP_WAIT_VALUE;
    // the step's serial chain (finish -> exchange -> assembly -> tiling): on the main
    // stream between two cross-stream hops (SML_CHAIN_TWO_STREAMS), or on SPEEDY's stream
    // right after the window (SML_CHAIN_SPEEDY).  SML_CHAIN_AUTO is the two-stream form:
    // measured same-box (r04a), the chain on SPEEDY's stream was 19-20 us per step SLOWER
    // at world 1 and in the 8-rank share -- its two remaining stream operations
    // (hipStreamWaitValue64 / WriteValue64 run as blit kernels, ~6 us each, satisfied or
    // not) stay on the critical path, and the finish and assembly get 64 CUs instead of
    // 192.  With kernel hops it has no hop kernel on SPEEDY's stream at all (the finish
    // waits for its begin in-kernel, the entry specx signals the grid) and still loses
    // (r04, profiles/r04/chain_nohop: N = 1 1104 / 1109 vs 1123 / 1123 steps/s, 8-rank
    // share 1185 / 1186 vs 1194 / 1195): the finish and assembly on 64 CUs cost more than
    // the two signal kernels.
    s.chain = in.chain_mode == SML_CHAIN_SPEEDY && in.overlap && in.two_streams;
    s.chain_effective = s.chain ? SML_CHAIN_SPEEDY : SML_CHAIN_TWO_STREAMS;
    s.chain_on_side = s.chain;
    s.hops = in.overlap && !s.chain;
    // chain on SPEEDY's stream with kernel hops: the next run_model's entry specx signals
    // the assembled grid as it starts (no signal kernel in front of the window); run_model
    // is then enqueued before the main stream's wait for that signal -- every in-kernel
    // wait is enqueued after its producer, so no wait can hold a hardware queue that its
    // producer sits behind
    s.entry_sig = in.overlap && s.chain && s.use_kernels;
    // two streams with kernel hops: the entry's specx waits for the assembled grid
    // in-kernel, and the forecast's signal is a store that run_model issues right behind
    // its exit (sml_hybrid_advance)
    s.entry_wait = s.exit_store = s.hops && s.use_kernels;
    // the finish follows the begin (chain: on SPEEDY's stream, once the main stream's
    // begin is done) or SPEEDY's forecast of the previous window (two streams); with
    // kernel hops it waits inside the finish kernel, whose weights load meanwhile
    if (in.overlap) {
        s.finish_hop = s.chain ? kHopBegun : kHopLm;
        s.finish_in_kernel = s.use_kernels;
    }
    return s;
}

// ------------------------------------------------------------ res_domain wrappers
// region geometry of the res_domain decomposition (getxyresextent, getoverlapindices;
// res_domain.f90:123-204), 1-based like the reference:
// g[12] = res_xstart, res_xend, res_ystart, res_yend, resx, resy, in_xstart, in_xend,
//         in_ystart, in_yend, inx, iny
extern "C" int sml_region_geometry(int numregions, int region, int *g) {
    SML_REQUIRE(g, "null argument");
    RegionGeom r;
    SML_REQUIRE(region_geom(numregions, region, &r), "region %d of %d does not decompose the grid", region,
                numregions);
    const int v[12] = {r.res_xstart, r.res_xend, r.res_ystart, r.res_yend, r.resx, r.resy,
                       r.in_xstart,  r.in_xend,  r.in_ystart,  r.in_yend,  r.inx,  r.iny};
    std::memcpy(g, v, sizeof v);
    return SML_OK;
}

// the training targets' 0-based positions inside the region's feedback vector
// (region_target_index, csrc/sml_internal.hpp): idx holds 34 resx resy entries, 136 at
// 1152 regions.  The sst block sits after precip, so the flag moves none of them.
extern "C" int sml_region_target_index(int numregions, int region, int sst, int32_t *idx, int *count) {
    SML_REQUIRE(idx && count, "null argument");
    (void)sst;
    RegionGeom r;
    SML_REQUIRE(region_geom(numregions, region, &r), "region %d of %d does not decompose the grid", region,
                numregions);
    *count = region_target_index(r, idx);
    return SML_OK;
}

// processor_decomposition (res_domain.f90:31-62): the regions (0-based) rank irank of
// numprocs owns; returns their count in *count (regions may be NULL to ask only)
extern "C" int sml_processor_decomposition(int numregions, int numprocs, int irank, int *regions, int *count) {
    SML_REQUIRE(count && numregions > 0 && numprocs > 0 && irank >= 0 && irank < numprocs, "bad argument");
    std::vector<int> r(numregions);
    *count = processor_regions(numregions, numprocs, irank, r.data());
    if (regions) std::memcpy(regions, r.data(), sizeof(int) * *count);
    return SML_OK;
}
