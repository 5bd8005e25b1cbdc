// sml_hybrid_layout.hpp -- the hybrid loop's host arithmetic, with no HIP or RCCL call in
// it, so it runs (and is sanitised) on a CPU: tests/hybrid_layout_check.cpp.  The
// all-gather's plan (sml_exchange_plan), the reference's calendar (sml_calendar_delta_hour,
// sml_tisr_date_index) and the res_domain wrappers of the C ABI live in
// sml_hybrid_layout.cpp; the two value types below are what the loop (sml_hybrid.hip)
// holds instead of loose fields.
#pragma once

#include <cstdint>

#include "sml_internal.hpp"

namespace sml {

// the loop's cross-stream hops (sml_hops.hpp): the assembled grid, SPEEDY's forecast
// (the local model), the reservoir's begin
enum { kHopGrid = 0, kHopLm = 1, kHopBegun = 2, kHops = 3 };

// The loop's calendar.  get_tisr_by_date (mpires.f90:1644-1676): a table of hourly global
// tisr fields [nhours][48][96], the calendar's start year, the hours before the first
// prediction step and the hours per step; t = steps advanced so far.  The window's date
// (run_model, mpires.f90:1545): with the calendar on every advance hands SPEEDY the date
// of hour base + t * step_hours and the window's forcing follows it (sml_dyn_fordate).
// Within a step the date is taken first, then ++t, then the tisr index: the two lookups
// share the February latch (feb29), as the reference's calls share its SAVEd month table.
struct LoopCalendar {
    int startyear = 0, feb29 = 0, nhours = 0;
    int64_t base = 0, step_hours = 6, t = 0;
    bool cal_on = false;
    // both reset the step count and the latch; only set_calendar turns the date on
    void set_calendar(int startyear_, int64_t hours_base, int step_hours_);
    void set_tisr_table(int nhours_, int startyear_, int64_t hours_base, int step_hours_);
    // date[4] of step t + 1: window_date leaves the latch alone (a query), next_date moves
    // it (the advance's own lookup)
    int window_date(int *date) const;
    int next_date(int *date);
    // after ++t: the table's hour (1-based) of step t - 1, get_tisr_by_date(..., timestep - 1,
    // ...) for the next feedback (mpires.f90:726-728); refused outside the table
    int tisr_index(int *index);
};

// What decides the step's schedule; the two environment facts are read by the caller
// (SML_HYBRID_EVENTS; dispatch serialised by AMD_SERIALIZE_KERNEL or
// ROCPROF_COUNTER_COLLECTION).
struct LoopScheduleIn {
    bool overlap;      // SPEEDY's window beside the reservoir's begin
    bool two_streams;  // the side stream is a stream of its own
    int chain_mode;    // SML_CHAIN_*
    int hop_mode;      // SML_HOP_*
    bool cu_split;     // the two streams run on disjoint CUs (res_cus > 0)
    bool env_events, serialised;
};

// The step's schedule, stated once: it changes only when a mode is set
// (sml_hybrid_create / _set_hop_mode / _set_chain, which drain both streams first);
// predict, advance, step and sync only read it.  Every in-kernel wait it asks for is
// enqueued after its producer, so no wait can hold a hardware queue that its producer
// sits behind (loop_schedule states each case).
struct LoopSchedule {
    bool chain = false;                            // the serial chain runs on SPEEDY's stream
    bool use_events = false, use_kernels = false;  // the hops' flavour (neither: CP wait-value)
    bool hops = false;        // two hops around every window (grid_t main -> side, lm_t side -> main)
    bool entry_sig = false;   // run_model's entry specx signals the assembled grid (chain, kernel hops)
    bool entry_wait = false;  // run_model's entry specx waits for the assembled grid in-kernel
    bool exit_store = false;  // run_model's exit is followed by the forecast's store
    int finish_hop = -1;      // the hop the v_p finish waits for (-1: none, the one-pass step)
    // ... inside the finish kernel (a loop with no local region has no finish: it takes
    // Hops::wait), else through Hops::wait in front of it
    bool finish_in_kernel = false;
    bool chain_on_side = false;  // the chain's (finish, exchange, assembly) stream is the side stream
    int hop_effective = SML_HOP_WAIT_VALUE, chain_effective = SML_CHAIN_TWO_STREAMS;
};

LoopSchedule loop_schedule(const LoopScheduleIn &in);

}  // namespace sml
