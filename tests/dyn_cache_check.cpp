// The dynamics context's host caches (csrc/sml_dyn_cache.hpp) on a CPU: a stand-alone
// program that includes that header alone (tests/test_dyn_cache_cpu.py builds it plain
// and with ASan/UBSan).  It pins the slot cache's eviction against a restatement of
// the rule it replaced, the pins that keep a window's three table slots apart, the
// window cache's releases, and every field of the keys.
#include "sml_dyn_cache.hpp"

#include <cstdio>
#include <functional>
#include <map>
#include <vector>

using namespace sml;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            if (++g_failed <= 20) {                       \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

using Slots = RoundRobinCache<ImpintKey, NoValue, 4>;

// the rule the slot cache replaced: a hit changes nothing; a miss takes `next` and
// advances it mod 4
struct PlainSlots {
    double key[4][2] = {};
    bool used[4] = {};
    int next = 0;
    int request(double dt, double alph, bool *hit) {
        for (int i = 0; i < 4; ++i)
            if (used[i] && key[i][0] == dt && key[i][1] == alph) {
                *hit = true;
                return i;
            }
        *hit = false;
        const int i = next;
        next = (i + 1) % 4;
        key[i][0] = dt;
        key[i][1] = alph;
        used[i] = true;
        return i;
    }
};

static ImpintKey key_of(int k) { return ImpintKey{60.0 * (k + 1), 0.5}; }

// every request sequence of length <= 6 over 6 keys, without pins
static void slots_follow_the_plain_rule() {
    long sequences = 0;
    for (int len = 1; len <= 6; ++len) {
        long total = 1;
        for (int i = 0; i < len; ++i) total *= 6;
        for (long code = 0; code < total; ++code) {
            Slots c;
            PlainSlots p;
            long rest = code;
            bool same = true;
            for (int i = 0; i < len && same; ++i, rest /= 6) {
                const ImpintKey k = key_of((int)(rest % 6));
                bool hit = false, phit = false;
                const int w = c.acquire(k, 0, &hit);
                const int pw = p.request(k.dt, k.alph, &phit);
                same = w == pw && hit == phit && c.find(k) == w;
            }
            CHECK(same, "sequence %ld of length %d departs from the plain rule", code, len);
            ++sequences;
        }
    }
    CHECK(sequences == 6 + 36 + 216 + 1296 + 7776 + 46656, "%ld sequences", sequences);
}

// ways [X, A, Y, Z] with next == 1, then a window that hits A and misses twice
static void window_slots(bool pinning, int out[3]) {
    Slots c;
    bool hit = false;
    const int fill[5] = {0, 1, 2, 3, 0};
    for (int i = 0; i < 5; ++i) {  // five keys: the fifth wraps to way 0 and leaves next == 1
        const int w = c.acquire(key_of(i), 0, &hit);
        CHECK(!hit && w == fill[i], "fill %d went to way %d", i, w);
    }
    unsigned taken = 0;
    const int keys[3] = {1, 6, 7};  // A, then two keys the cache has never seen
    for (int i = 0; i < 3; ++i) {
        out[i] = c.acquire(key_of(keys[i]), pinning ? taken : 0u, &hit);
        CHECK(hit == (i == 0), "request %d: hit %d", i, (int)hit);
        if (out[i] >= 0) taken |= Slots::pin(out[i]);
    }
}

static void pins_keep_a_window_apart() {
    int w[3];
    window_slots(true, w);
    CHECK(w[0] == 1 && w[1] == 2 && w[2] == 3, "pinned: ways %d %d %d", w[0], w[1], w[2]);
    CHECK(w[0] != w[1] && w[1] != w[2] && w[0] != w[2], "pinned: three distinct ways");
    // the rule before the pins, on record: the first miss lands on the way just hit
    window_slots(false, w);
    CHECK(w[0] == 1 && w[1] == 1 && w[2] == 2, "unpinned: ways %d %d %d", w[0], w[1], w[2]);

    // two ways pinned, whatever `next` is: a miss returns a way, and never a pinned one
    for (int start = 0; start < 4; ++start)
        for (int a = 0; a < 4; ++a)
            for (int b = a + 1; b < 4; ++b) {
                Slots c;
                bool hit = false;
                for (int i = 0; i < 4 + start; ++i) c.acquire(key_of(i), 0, &hit);  // next == start
                const unsigned pinned = Slots::pin(a) | Slots::pin(b);
                for (int i = 0; i < 6; ++i) {
                    const int w1 = c.acquire(key_of(100 + i), pinned, &hit);
                    CHECK(!hit && w1 >= 0 && w1 < 4 && w1 != a && w1 != b, "start %d pins %d %d: way %d", start, a, b,
                          w1);
                }
            }
    Slots c;
    bool hit = false;
    CHECK(c.acquire(key_of(0), 0xfu, &hit) == -1 && !hit, "every way pinned: no way");
}

// a release callback that counts, per value
struct CountRelease {
    std::map<int, int> *released;
    void operator()(int &v) const { ++(*released)[v]; }
};

static WindowKey window_key(int n) {
    WindowKey k;
    k.nleap = n;
    k.delt = 2400.0;
    return k;
}

static void window_cache_releases() {
    std::map<int, int> released;
    {
        using Cache = RoundRobinCache<WindowKey, int, 4, CountRelease>;
        Cache cls[4] = {Cache(CountRelease{&released}), Cache(CountRelease{&released}),
                        Cache(CountRelease{&released}), Cache(CountRelease{&released})};
        bool hit = false;
        for (int c = 0; c < 4; ++c)
            for (int i = 0; i < 4; ++i) {
                const int w = cls[c].acquire(window_key(i), 0, &hit);
                CHECK(!hit && w == i, "class %d key %d: way %d", c, i, w);
                cls[c].value(w) = 100 * c + i;
            }
        CHECK(released.empty(), "nothing released while every way was free");
        const int w = cls[2].acquire(window_key(4), 0, &hit);  // a fifth key in class 2
        CHECK(!hit && w == 0, "the fifth key takes the class's oldest way, got %d", w);
        cls[2].value(w) = 204;
        CHECK(released.size() == 1 && released[200] == 1, "the evicted value released exactly once");
        for (int c = 0; c < 4; ++c)
            for (int i = (c == 2 ? 1 : 0); i < 4; ++i) {
                const int f = cls[c].find(window_key(i));
                CHECK(f == i && cls[c].value(f) == 100 * c + i, "class %d key %d survives", c, i);
            }
        CHECK(cls[2].find(window_key(0)) == -1 && cls[2].find(window_key(4)) == 0, "class 2 after the eviction");
        // a way dropped after a failed fill: released once, gone, and not released again
        const int w5 = cls[3].acquire(window_key(5), 0, &hit);
        cls[3].value(w5) = 305;
        cls[3].drop(w5);
        CHECK(released[300] == 1 && released[305] == 1 && cls[3].find(window_key(5)) == -1, "a dropped way");
    }
    int values = 0;
    bool once = true;
    for (const auto &r : released) {
        ++values;
        once = once && r.second == 1;
    }
    CHECK(values == 18 && once, "%d values released, each once: %d", values, (int)once);
}

template <class Key>
static void every_field_matters(const char *what, const Key &base,
                                const std::vector<std::function<void(Key &)>> &flips) {
    RoundRobinCache<Key, NoValue, 2> c;
    bool hit = false;
    c.acquire(base, 0, &hit);
    CHECK(c.find(base) == 0 && base == Key(base), "%s: the key finds itself", what);
    int i = 0;
    for (const auto &flip : flips) {
        Key k = base;
        flip(k);
        CHECK(!(k == base) && !(base == k) && c.find(k) == -1, "%s: flipping field %d still hits", what, i);
        ++i;
    }
}

static void keys_compare_every_field() {
    static const int obj[32] = {};
    auto other = [](const void *&p) { p = p ? (const char *)p + 1 : (const void *)&obj[1]; };

    every_field_matters<ImpintKey>("ImpintKey", ImpintKey{1200.0, 0.5},
                                   {[](ImpintKey &k) { k.dt = 2400.0; }, [](ImpintKey &k) { k.alph = 0.0; }});

    LeapfrogKey lf{4800.0, 0.5, 0.05, 0.53, &obj[2], &obj[3], true};
    every_field_matters<LeapfrogKey>(
        "LeapfrogKey", lf,
        {[](LeapfrogKey &k) { k.dt = 1.0; }, [](LeapfrogKey &k) { k.alph = 1.0; }, [](LeapfrogKey &k) { k.rob = 1.0; },
         [](LeapfrogKey &k) { k.wil = 1.0; }, [&](LeapfrogKey &k) { other(k.phys); },
         [](LeapfrogKey &k) { k.phys = nullptr; }, [&](LeapfrogKey &k) { other(k.tab); },
         [](LeapfrogKey &k) { k.phys_on = false; }});

    WindowKey w;
    w.nleap = 8;
    w.delt = 2400.0;
    w.alph = 0.5;
    w.rob = 0.05;
    w.wil = 0.53;
    w.phys_on = true;
    w.fused = true;
    w.prepared = true;
    w.tab = {&obj[4], &obj[5], &obj[6]};
    w.has_exit = true;
    w.exit = {&obj[7], &obj[8], &obj[9], &obj[10], &obj[11], &obj[12], &obj[13], 1000, &obj[14]};
    w.has_entry = true;
    w.entry = {&obj[15], &obj[16], &obj[17], 2000, &obj[18], &obj[19]};
    using F = std::function<void(WindowKey &)>;
    std::vector<F> flips = {
        [](WindowKey &k) { k.nleap = 9; },       [](WindowKey &k) { k.delt = 1.0; },
        [](WindowKey &k) { k.alph = 1.0; },      [](WindowKey &k) { k.rob = 1.0; },
        [](WindowKey &k) { k.wil = 1.0; },       [](WindowKey &k) { k.phys_on = false; },
        [](WindowKey &k) { k.fused = false; },   [](WindowKey &k) { k.prepared = false; },
        [&](WindowKey &k) { other(k.tab[0]); },  [&](WindowKey &k) { other(k.tab[1]); },
        [&](WindowKey &k) { other(k.tab[2]); },  [](WindowKey &k) { k.has_exit = false; },
        [&](WindowKey &k) { other(k.exit.varm); }, [&](WindowKey &k) { other(k.exit.fc4); },
        [&](WindowKey &k) { other(k.exit.fc2); },  [&](WindowKey &k) { other(k.exit.mm); },
        [&](WindowKey &k) { other(k.exit.in4); },  [&](WindowKey &k) { other(k.exit.inlp); },
        [&](WindowKey &k) { other(k.exit.cnt); },  [](WindowKey &k) { k.exit.timeout = 1; },
        [&](WindowKey &k) { other(k.exit.store); }, [](WindowKey &k) { k.exit.store = nullptr; },
        [](WindowKey &k) { k.has_entry = false; },
        [&](WindowKey &k) { other(k.entry.flag); }, [](WindowKey &k) { k.entry.flag = nullptr; },
        [&](WindowKey &k) { other(k.entry.late); }, [&](WindowKey &k) { other(k.entry.sig); },
        [](WindowKey &k) { k.entry.timeout = 1; },  [&](WindowKey &k) { other(k.entry.vptr); },
        [&](WindowKey &k) { other(k.entry.go); }};
    every_field_matters<WindowKey>("WindowKey", w, flips);

    // "has exit" / "has entry" alone: whatever the other fields are, even all empty
    for (int filled = 0; filled < 2; ++filled) {
        WindowKey a = filled ? w : WindowKey(), b = a;
        b.has_exit = !a.has_exit;
        CHECK(!(a == b) && !(b == a), "keys that differ in has_exit alone compare equal (filled %d)", filled);
        b = a;
        b.has_entry = !a.has_entry;
        CHECK(!(a == b) && !(b == a), "keys that differ in has_entry alone compare equal (filled %d)", filled);
    }
}

int main() {
    slots_follow_the_plain_rule();
    pins_keep_a_window_apart();
    window_cache_releases();
    keys_compare_every_field();
    std::printf("dyn_cache_check: %d checks, %d failed\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
