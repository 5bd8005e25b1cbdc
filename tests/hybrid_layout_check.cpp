// hybrid_layout_check.cpp -- CPU check of the hybrid loop's host arithmetic
// (speedy-ml-1_amd/csrc/sml_hybrid_layout.cpp): the reference's calendar against known
// answers and a statement-by-statement restatement of mod_calendar.f90, the loop's
// calendar against direct calls in the loop's order, the exchange plan against
// processor_regions, and the step's schedule against the expressions the loop used to
// evaluate inline, over every combination of its inputs.  Stand-alone
// (tests/test_hybrid_layout_cpu.py builds it plain and under ASan/UBSan).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sml_hybrid_layout.hpp"

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

static void refuse(const char *what, int rc, const char *needle) {
    g_case = what;
    CHECK(rc != SML_OK, "accepted");
    CHECK(std::strstr(sml_last_error(), needle) != nullptr, "message '%s' lacks '%s'", sml_last_error(), needle);
}

// ---- mod_calendar.f90 get_current_time_delta_hour + numof_hours_into_year, statement by
// statement; ncal is the SAVEd month table
static bool leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }

static int ref_index(int startyear, long long hours, int *ncal) {
    const long long years = hours / 8760;
    int year = (int)years + startyear;
    int leap_days = 0;
    for (long long i = 0; i < years; ++i)
        if (leap(startyear + (int)i)) ++leap_days;
    const long long day_of_year = (hours % 8760) / 24 - leap_days;
    if (leap(year)) ncal[1] = 29;
    long long c = day_of_year;
    int month = 1;
    while (c > 0) {
        c -= ncal[month - 1];
        ++month;
    }
    month -= 1;
    if (month <= 0) {
        month = 12;
        year -= 1;
    }
    const int day = (int)(ncal[month - 1] + c);
    const int hour = (int)(hours % 24);
    const int tab[12] = {31, leap(year) ? 29 : 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    long long n = 0;
    for (int i = 0; i < month - 1; ++i) n += 24 * tab[i];
    n += 24 * std::max(0, day - 1) + hour;
    if (n == 0) n = 1;
    if (n > 8760) n -= 8760;
    return (int)n;
}

static void check_calendar() {
    // the known answers of tests/test_calendar.py and the dates behind them
    struct Known { int start; long long hours; int index, date[4]; } known[] = {
        {1981, 0, 8760, {1980, 12, 31, 0}},  // hour 0 of 1981: Dec 31 of the year before
        {1981, 24, 1, {1981, 1, 1, 0}},
        {1981, 30, 6, {1981, 1, 1, 6}},
        {1981, 24 * 32 + 12, 31 * 24 + 12, {1981, 2, 1, 12}},
        {1984, 8760 + 24, 8760, {1984, 12, 31, 0}},
    };
    g_case = "known answers";
    for (const Known &k : known) {
        int feb = 0, idx = 0, d[4] = {0, 0, 0, 0};
        CHECK(sml_tisr_date_index(k.start, k.hours, &feb, &idx) == SML_OK, "%s", sml_last_error());
        CHECK(idx == k.index, "(%d, %lld): index %d, want %d", k.start, k.hours, idx, k.index);
        feb = 0;
        CHECK(sml_calendar_delta_hour(k.start, k.hours, &feb, d) == SML_OK, "%s", sml_last_error());
        CHECK(std::equal(d, d + 4, k.date), "(%d, %lld): %d-%d-%d %d h", k.start, k.hours, d[0], d[1], d[2], d[3]);
    }
    g_case = "an exact month boundary";
    {
        int feb = 0, d[4];
        CHECK(sml_calendar_delta_hour(1981, 24 * 31, &feb, d) == SML_OK, "%s", sml_last_error());
        CHECK(d[0] == 1981 && d[1] == 1 && d[2] == 31 && d[3] == 0, "%d-%d-%d %d h", d[0], d[1], d[2], d[3]);
        CHECK(sml_calendar_delta_hour(1981, 24 * (31 + 28 + 31), &feb, d) == SML_OK, "%s", sml_last_error());
        CHECK(d[0] == 1981 && d[1] == 3 && d[2] == 31 && feb == 0, "%d-%d-%d", d[0], d[1], d[2]);
    }
    g_case = "the February latch";
    {
        // day 60 of 1985 (after 1984's leap day): March 1 for a calendar that has met no leap
        // year, February 29 once 1984 was met
        const long long h85 = 4 * 8760 + 24 * 61;
        int feb = 0, d[4];
        CHECK(sml_calendar_delta_hour(1981, h85, &feb, d) == SML_OK && feb == 0, "latch %d", feb);
        CHECK(d[0] == 1985 && d[1] == 3 && d[2] == 1, "%d-%d-%d", d[0], d[1], d[2]);
        CHECK(sml_calendar_delta_hour(1981, 3 * 8760 + 24 * 40, &feb, d) == SML_OK && feb == 1, "latch %d", feb);
        CHECK(d[0] == 1984, "year %d", d[0]);
        CHECK(sml_calendar_delta_hour(1981, h85, &feb, d) == SML_OK && feb == 1, "latch %d", feb);
        CHECK(d[0] == 1985 && d[1] == 2 && d[2] == 29, "%d-%d-%d", d[0], d[1], d[2]);
        // window_date works on a copy of the latch, next_date moves it
        LoopCalendar c;
        c.set_calendar(1981, 3 * 8760 + 24 * 40, 6);
        CHECK(c.window_date(d) == SML_OK && d[0] == 1984 && c.feb29 == 0, "latch %d after window_date", c.feb29);
        int e[4];
        CHECK(c.next_date(e) == SML_OK && std::equal(d, d + 4, e) && c.feb29 == 1, "latch %d after next_date", c.feb29);
    }
    for (int start : {1981, 1990, 2000}) {
        g_case = "the restatement from " + std::to_string(start);
        int ncal[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
        int feb = 0, bad = 0;
        for (long long h = 0; h < 30 * 8760; h += 6) {
            int idx = 0;
            if (sml_tisr_date_index(start, h, &feb, &idx) != SML_OK) ++bad;
            const int want = ref_index(start, h, ncal);
            if (idx != want || idx < 1 || idx > 8784) {
                if (++bad <= 5) CHECK(false, "hour %lld: %d, want %d", h, idx, want);
            }
            if (feb != (ncal[1] == 29)) ++bad;
        }
        CHECK(bad == 0, "%d hours differ", bad);
    }
    int feb = 0, d[4], idx = 0;
    refuse("negative hours", sml_calendar_delta_hour(1981, -1, &feb, d), "bad argument");
    refuse("null latch", sml_tisr_date_index(1981, 0, nullptr, &idx), "bad argument");
}

static void check_loop_calendar() {
    g_case = "LoopCalendar";
    // 6000 steps of 12 h from early 1983: through the leap years 1984 and 1988
    const int sy = 1981, sh = 12;
    const long long base = 2 * 8760 + 24 * 20 + 6;
    LoopCalendar c;
    c.set_tisr_table(8784, sy, base, sh);
    CHECK(!c.cal_on && c.t == 0 && c.feb29 == 0, "set_tisr_table");
    c.set_calendar(sy, base, sh);
    CHECK(c.cal_on && c.t == 0 && c.feb29 == 0 && c.nhours == 8784, "set_calendar");
    int feb = 0, bad = 0, leaps = 0, last_year = 0;
    long long t = 0;
    for (int step = 0; step < 6000; ++step) {
        // the loop's order: the date of t + 1, ++t, the table's hour of t - 1, one latch
        int want_d[4], want_i = 0, d[4], w[4], i = 0;
        const int before = c.feb29;
        if (c.window_date(w) != SML_OK || c.feb29 != before) ++bad;
        if (sml_calendar_delta_hour(sy, base + (t + 1) * sh, &feb, want_d) != SML_OK) ++bad;
        if (c.next_date(d) != SML_OK || !std::equal(d, d + 4, want_d) || !std::equal(w, w + 4, want_d)) ++bad;
        ++t;
        ++c.t;
        if (sml_tisr_date_index(sy, base + (t - 1) * sh, &feb, &want_i) != SML_OK) ++bad;
        if (c.tisr_index(&i) != SML_OK || i != want_i || c.feb29 != feb || c.t != t) ++bad;
        if (d[0] != last_year && leap(d[0])) ++leaps;
        last_year = d[0];
    }
    CHECK(bad == 0, "%d steps differ from the direct calls", bad);
    CHECK(leaps >= 2 && c.feb29 == 1, "%d leap years crossed", leaps);
    // the resets: both clear t and the latch; set_tisr_table leaves cal_on alone
    c.set_tisr_table(100, sy, 24 * 200, 6);
    CHECK(c.t == 0 && c.feb29 == 0 && c.cal_on && c.nhours == 100, "set_tisr_table after a run");
    ++c.t;
    int i = -1;
    refuse("a table too short", c.tisr_index(&i), "outside the table's 100 hours");
    CHECK(std::strstr(sml_last_error(), "tisr hour ") != nullptr && i == -1, "'%s', index %d", sml_last_error(), i);
    g_case = "LoopCalendar resets";
    c.feb29 = 1;
    c.set_calendar(1990, 5, 3);
    CHECK(c.t == 0 && c.feb29 == 0 && c.cal_on && c.startyear == 1990 && c.base == 5 && c.step_hours == 3, "set_calendar");
    LoopCalendar off;
    off.set_tisr_table(8760, 1981, 0, 6);
    CHECK(!off.cal_on, "set_tisr_table turned the calendar on");
}

static void check_plan() {
    for (int n : {1, 6, 7, 288, 1152}) {
        std::vector<int> worlds;
        for (int w = 1; w <= std::min(n, 16); ++w) worlds.push_back(w);
        if (n > 16) worlds.push_back(n);
        for (int world : worlds) {
            g_case = "plan " + std::to_string(n) + " regions, world " + std::to_string(world);
            int maxc = -1, contig = -1;
            std::vector<int32_t> perm(n, -7);
            CHECK(sml_exchange_plan(n, world, &maxc, &contig, perm.data()) == SML_OK, "%s", sml_last_error());
            std::vector<int> mine(n);
            int largest = 0;
            std::vector<char> hit((size_t)world * std::max(maxc, 1), 0);
            int bad = 0;
            for (int r = 0; r < world; ++r) {
                const int c = processor_regions(n, world, r, mine.data());
                largest = std::max(largest, c);
                for (int i = 0; i < c; ++i)
                    if (perm[mine[i]] != r * maxc + i) ++bad;
            }
            CHECK(maxc == largest, "maxc %d, the largest share is %d", maxc, largest);
            CHECK(bad == 0, "%d regions not at rank * maxc + position", bad);
            for (int r = 0; r < n; ++r) {
                if (perm[r] < 0 || perm[r] >= world * maxc || hit[perm[r]]) ++bad;
                else hit[perm[r]] = 1;
            }
            CHECK(bad == 0, "perm is not injective into [0, %d)", world * maxc);
            CHECK(contig == (n % world == 0 ? 1 : 0), "contiguous %d", contig);
            int maxc2 = -1, contig2 = -1;
            CHECK(sml_exchange_plan(n, world, &maxc2, &contig2, nullptr) == SML_OK && maxc2 == maxc && contig2 == contig,
                  "a null perm");
        }
    }
    int maxc = 0, contig = 0;
    refuse("world 0", sml_exchange_plan(6, 0, &maxc, &contig, nullptr), "bad argument");
    refuse("more ranks than regions", sml_exchange_plan(6, 7, &maxc, &contig, nullptr), "bad argument");
    refuse("null maxc", sml_exchange_plan(6, 2, nullptr, &contig, nullptr), "bad argument");
    refuse("null contiguous", sml_exchange_plan(6, 2, &maxc, nullptr, nullptr), "bad argument");
    refuse("no regions", sml_exchange_plan(0, 1, &maxc, &contig, nullptr), "bad argument");
}

static void check_schedule() {
    int n = 0;
    for (int overlap = 0; overlap < 2; ++overlap)
    for (int two = 0; two < 2; ++two)
    for (int chain_mode : {SML_CHAIN_AUTO, SML_CHAIN_TWO_STREAMS, SML_CHAIN_SPEEDY})
    for (int hop_mode : {SML_HOP_AUTO, SML_HOP_WAIT_VALUE, SML_HOP_EVENTS, SML_HOP_KERNEL})
    for (int split = 0; split < 2; ++split)
    for (int env = 0; env < 2; ++env)
    for (int ser = 0; ser < 2; ++ser) {
        ++n;
        char name[128];
        std::snprintf(name, sizeof name, "schedule overlap %d two %d chain %d hop %d split %d env %d ser %d", overlap,
                      two, chain_mode, hop_mode, split, env, ser);
        g_case = name;
        const LoopSchedule s = loop_schedule({overlap != 0, two != 0, chain_mode, hop_mode, split != 0, env != 0, ser != 0});
        // the expressions of the loop before the schedule was a value: sml_hybrid_set_hop_mode, ...
        bool use_events, use_kernels;
        if (hop_mode == SML_HOP_AUTO) {
            use_events = env || ser;
            use_kernels = !use_events && split;
        } else {
            use_events = hop_mode == SML_HOP_EVENTS;
            use_kernels = hop_mode == SML_HOP_KERNEL;
        }
        // ... sml_hybrid_set_chain (side != main: a second stream), ...
        const bool chain = chain_mode == SML_CHAIN_SPEEDY && overlap && two;
        // ... sml_hybrid_advance, ...
        const bool hops = overlap && !chain;
        const bool entry_sig = overlap && chain && use_kernels;
        const bool exit_store = hops && use_kernels;
        // ... and predict_impl: the chain's finish waits for the begin, the two-stream one
        // for the forecast; inside the kernel with kernel hops
        const int finish_hop = !overlap ? -1 : chain ? kHopBegun : kHopLm;
        const bool finish_in_kernel = overlap && use_kernels;
        CHECK(s.use_events == use_events && s.use_kernels == use_kernels, "events %d kernels %d", s.use_events, s.use_kernels);
        CHECK(s.chain == chain && s.chain_on_side == chain, "chain %d on side %d", s.chain, s.chain_on_side);
        CHECK(s.hops == hops, "hops %d", s.hops);
        CHECK(s.entry_sig == entry_sig, "entry_sig %d", s.entry_sig);
        CHECK(s.exit_store == exit_store && s.entry_wait == exit_store, "exit_store %d entry_wait %d", s.exit_store, s.entry_wait);
        CHECK(s.finish_hop == finish_hop && s.finish_in_kernel == finish_in_kernel, "finish hop %d in kernel %d",
              s.finish_hop, s.finish_in_kernel);
        // the modes sml_hybrid_hop_mode and sml_hybrid_chain report
        CHECK(s.hop_effective == (use_events ? SML_HOP_EVENTS : use_kernels ? SML_HOP_KERNEL : SML_HOP_WAIT_VALUE),
              "effective hop mode %d", s.hop_effective);
        CHECK(s.chain_effective == (chain ? SML_CHAIN_SPEEDY : SML_CHAIN_TWO_STREAMS), "effective chain %d", s.chain_effective);
        // what makes the schedule safe, whatever the expressions are
        CHECK(!s.chain || (overlap && two), "a chain without overlap or without a second stream");
        if (!overlap)
            CHECK(!s.hops && !s.finish_in_kernel && !s.entry_wait && !s.entry_sig && !s.exit_store && s.finish_hop < 0 &&
                      !s.chain_on_side,
                  "a hop or an in-kernel wait without overlap");
        CHECK(!(s.entry_sig && s.hops), "entry_sig and hops");
        CHECK(!s.exit_store || (s.hops && s.use_kernels), "exit_store without hops and kernel hops");
        CHECK(!s.entry_wait || (s.hops && s.use_kernels), "entry_wait without hops and kernel hops");
        CHECK(!s.finish_in_kernel || s.use_kernels, "an in-kernel finish wait without kernel hops");
        CHECK(!(s.use_events && s.use_kernels), "events and kernels");
        if (hop_mode == SML_HOP_AUTO && ser) CHECK(s.use_events && !s.use_kernels, "serialised dispatch without event hops");
        if (overlap) CHECK(s.finish_hop == (s.chain ? kHopBegun : kHopLm), "finish hop %d", s.finish_hop);
    }
    g_case = "schedule";
    CHECK(n == 384, "%d combinations", n);
}

int main() {
    check_calendar();
    check_loop_calendar();
    check_plan();
    check_schedule();
    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    return g_fail ? 1 : 0;
}
