// sml_dyn_cache.hpp -- the dynamics context's host-side caches: one small N-way,
// round-robin cache template and the typed keys of its three uses (the impint table
// slots, the leapfrog step graphs, the window graphs).  Host only: no HIP type, no
// kernel, no launch; a cached value is released through the Release functor its owner
// gives (tests/dyn_cache_check.cpp builds this header alone).
#pragma once
#include <array>
#include <tuple>

namespace sml {

// a cache whose ways hold nothing to release (the impint slots: the way is the value)
struct NoValue {};
struct NoRelease {
    template <class V>
    void operator()(V &) const {}
};

// Ways entries, looked up by ==.  A miss evicts round robin: it takes the first way
// from `next` on that the caller has not pinned, and `next` moves behind it.  Without
// pins that is "take next, advance it mod Ways".
template <class Key, class Value, int Ways, class Release = NoRelease>
class RoundRobinCache {
    static_assert(Ways >= 1 && Ways <= 32, "pins are a 32-bit mask of ways");

public:
    explicit RoundRobinCache(Release release = Release()) : release_(release) {}
    RoundRobinCache(const RoundRobinCache &) = delete;
    RoundRobinCache &operator=(const RoundRobinCache &) = delete;
    ~RoundRobinCache() {
        for (int w = 0; w < Ways; ++w) drop(w);
    }

    static constexpr unsigned pin(int way) { return 1u << way; }

    // the way that holds key, or -1; a lookup changes nothing
    int find(const Key &key) const {
        for (int w = 0; w < Ways; ++w)
            if (used_[w] && key_[w] == key) return w;
        return -1;
    }

    // The way of key.  A hit (*hit = true) changes nothing.  A miss releases the value
    // of the way it evicts -- never one of `pinned` -- and leaves a default value there
    // for the caller to fill (or to drop(), if it cannot).  -1: every way is pinned.
    int acquire(const Key &key, unsigned pinned, bool *hit) {
        int w = find(key);
        *hit = w >= 0;
        if (w >= 0) return w;
        for (int i = 0; i < Ways && w < 0; ++i)
            if (const int c = (next_ + i) % Ways; !(pinned & pin(c))) w = c;
        if (w < 0) return -1;
        next_ = (w + 1) % Ways;
        drop(w);
        key_[w] = key;
        used_[w] = true;
        return w;
    }

    Value &value(int way) { return value_[way]; }

    // way holds nothing any more: its value released (once), its key forgotten
    void drop(int way) {
        if (used_[way]) release_(value_[way]);
        value_[way] = Value();
        used_[way] = false;
    }

private:
    Key key_[Ways] = {};
    Value value_[Ways] = {};
    bool used_[Ways] = {};
    int next_ = 0;  // where the next miss starts to look for a way to evict
    Release release_;
};

// ---- keys: plain fields, compared with ==.  Pointers are identities (device or host
// buffers the launches were captured with), never dereferenced here.

// an impint table slot: build_dyn_impint(dt, alph)
struct ImpintKey {
    double dt = 0, alph = 0;
    auto tie() const { return std::tie(dt, alph); }
    bool operator==(const ImpintKey &o) const { return tie() == o.tie(); }
};

// a captured step(2, 2, dt, alph, rob, wil): its class is the step's lradsw
struct LeapfrogKey {
    double dt = 0, alph = 0, rob = 0, wil = 0;
    const void *phys = nullptr;  // the caller's physics tendencies, or null
    const void *tab = nullptr;   // the impint slot
    bool phys_on = false;
    auto tie() const { return std::tie(dt, alph, rob, wil, phys, tab, phys_on); }
    bool operator==(const LeapfrogKey &o) const { return tie() == o.tie(); }
};

// A captured window: its class is (stepone's lradsw, prepared).  The fixed arguments of
// run_model's exit behind the window, and of its entry in front of it, are part of the
// key only where has_exit / has_entry say the graph holds them; the per-launch values
// (counts, hop values) are not: they travel through device memory.
struct WindowKey {
    int nleap = 0;
    double delt = 0, alph = 0, rob = 0, wil = 0;
    bool phys_on = false, fused = false, prepared = false;
    std::array<const void *, 3> tab = {};  // the impint slots of delt / 2, delt, 2 delt
    bool has_exit = false;
    struct Exit {
        const void *varm = nullptr, *fc4 = nullptr, *fc2 = nullptr, *mm = nullptr, *in4 = nullptr, *inlp = nullptr,
                   *cnt = nullptr;
        long long timeout = 0;
        const void *store = nullptr;  // the hop's flag behind the exit, or null
        auto tie() const { return std::tie(varm, fc4, fc2, mm, in4, inlp, cnt, timeout, store); }
    } exit;
    bool has_entry = false;
    struct Entry {
        const void *flag = nullptr, *late = nullptr, *sig = nullptr;
        long long timeout = 0;
        const void *vptr = nullptr, *go = nullptr;
        auto tie() const { return std::tie(flag, late, sig, timeout, vptr, go); }
    } entry;
    auto tie() const {
        return std::tie(nleap, delt, alph, rob, wil, phys_on, fused, prepared, tab, has_exit, has_entry);
    }
    bool operator==(const WindowKey &o) const {
        return tie() == o.tie() && exit.tie() == o.exit.tie() && entry.tie() == o.entry.tie();
    }
};

}  // namespace sml
