// sml_hops.hpp -- Hops: the cross-stream dependencies of the hybrid loop's overlapped
// schedule (grid_t: main -> side, lm_t: side -> main; the chain on SPEEDY's stream,
// SML_CHAIN_SPEEDY, hops the other way: grid_t, side -> main, before the re-tiling;
// begun_t, main -> side, before the finish).  Each is a sequence number in device memory
// that the producer's stream writes and the consumer's waits for (CP stream memory
// operations: 3.9 us from the producer's end to the consumer's start on gfx950, 10 us for
// an event record + wait; tools/probe_hop.hip).  A wait-value packet blocks its queue
// until the producer's write lands, so under serialised dispatch (rocprofv3 counter
// passes, AMD_SERIALIZE_KERNEL) it can stall ahead of that producer: SML_HOP_AUTO then
// takes event hops (loop_schedule, sml_hybrid_layout.cpp).
// SML_HOP_KERNEL (the default unless dispatch is serialised): the same sequence numbers,
// stored by a one-lane kernel behind the producer (k_hop_signal) and polled by the
// consumer -- inside the v_p finish and run_model's entry specx, which load everything
// else first, or by a one-lane k_hop_wait elsewhere.  The CP's stream operations run as
// blit kernels of ~6 us each with a ~6 us boundary in front; measured in an 8-rank share,
// the chain around the window 45.7 -> 34.8 us.
// Included by sml_hybrid.hip behind its SML_TL_DEFINE (k_hop_signal is on the step timeline).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sml_devmem.hpp"
#include "sml_hybrid_layout.hpp"
#include "sml_timeline.hpp"

namespace {
using namespace sml;

// SML_HOP_KERNEL's two kernels.  The producer's data is released by its own kernel's
// end (the dispatch after it on the same stream starts behind that release), so the
// signal is one relaxed agent-scope store of the sequence number (a vector store,
// write-through: MI355X_MICROARCH.md inter-workgroup visibility), and the consumer's
// next dispatch acquires at its start like any kernel's.  The wait polls with relaxed
// agent loads and s_sleep from one lane; it never spins forever: after ~4 s it marks
// the late word (sml_hybrid_sync reports it) and lets the stream go on.
__global__ void k_hop_signal(uint64_t *flag, uint64_t v) {
    SML_TL_SCOPE(sml::tl::kHopSignal);
    if (threadIdx.x == 0) __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_hop_wait(const uint64_t *flag, uint64_t v, unsigned *late, long long timeout) {
    if (threadIdx.x != 0) return;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) {
        __builtin_amdgcn_s_sleep(1);
        if (wall_clock64() - t0 > timeout) {  // default ~4 s at wall_clock64's 100 MHz
            __hip_atomic_store(late, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
    }
}

struct Hops {
    enum Flavour { kWaitValue, kEvents, kKernel };
    Flavour flavour = kWaitValue;
    // the waits' give-up time (wall_clock64 ticks)
    long long timeout = 400000000ll;

    // the events, the sequence words (device, the loop's DevMem) and the late word: a
    // kernel hop that gave up waiting (its consumer read NaN instead of stale data) marks
    // a pinned host word, stored at system scope and read without a copy by late_check
    int create(DevMem &mem) {
        for (hipEvent_t &e : ev_)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return fail(SML_ERR_HIP, "event");
        mem.device(&d_seq_, (size_t)kHops * kSeqStride);
        mem.pinned(&h_late_, 1, hipHostMallocCoherent);
        if (mem.status()) return fail(SML_ERR_HIP, "sequence counters");
        return SML_OK;
    }
    // after both streams are drained (the words and the late word go with the DevMem)
    void destroy_events() {
        for (hipEvent_t &e : ev_) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
    }

    uint64_t *word(int k) const { return d_seq_ + k * kSeqStride; }
    uint64_t seq(int k) const { return seq_[k]; }
    unsigned *late_word() const { return h_late_; }
    // the two moves a producer other than signal() makes: run_model's entry specx added
    // `adds` to the word; run_model's exit store of `v` is enqueued
    void add_seq(int k, uint64_t adds) { seq_[k] += adds; }
    void set_seq(int k, uint64_t v) { seq_[k] = v; }

    // producer side of hop `k`: ordered after everything issued on `s` so far
    int signal(int k, hipStream_t s) {
        if (flavour == kEvents) {
            SML_HIP(hipEventRecord(ev_[k], s));
        } else if (flavour == kKernel) {
            hipLaunchKernelGGL(k_hop_signal, dim3(1), dim3(64), 0, s, word(k), ++seq_[k]);
            SML_HIP(hipGetLastError());
        } else {
            SML_HIP(hipStreamWriteValue64(s, word(k), ++seq_[k], 0));
        }
        return SML_OK;
    }

    // consumer side: `s` waits for the latest signal of hop `k`
    int wait(int k, hipStream_t s) {
        if (flavour == kEvents) {
            SML_HIP(hipStreamWaitEvent(s, ev_[k], 0));
        } else if (flavour == kKernel) {
            hipLaunchKernelGGL(k_hop_wait, dim3(1), dim3(64), 0, s, word(k), seq_[k], h_late_, timeout);
            SML_HIP(hipGetLastError());
        } else {
            SML_HIP(hipStreamWaitValue64(s, word(k), seq_[k], hipStreamWaitValueGte, ~0ull));
        }
        return SML_OK;
    }

    // a hop that timed out since the last report: SML_ERR_STATE once (the word is reset)
    int late_check(const char *where) {
        if (h_late_ && __atomic_load_n(h_late_, __ATOMIC_ACQUIRE)) {
            __atomic_store_n(h_late_, 0u, __ATOMIC_RELEASE);
            return fail(SML_ERR_STATE, "%s: a cross-stream hop (SML_HOP_KERNEL) timed out -- its consumer read NaN, "
                                       "the steps since are invalid", where);
        }
        return SML_OK;
    }

private:
    static constexpr int kSeqStride = 16;  // one 128-B line per hop's word
    hipEvent_t ev_[kHops] = {nullptr, nullptr, nullptr};
    uint64_t *d_seq_ = nullptr, seq_[kHops] = {0, 0, 0};
    unsigned *h_late_ = nullptr;
};

}  // namespace
