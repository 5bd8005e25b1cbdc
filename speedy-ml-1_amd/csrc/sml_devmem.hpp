// sml_devmem.hpp -- DevMem: the one owner of a context's device and pinned memory
// (sml_dynamics.hip, sml_reservoir.hip, sml_train.hip, sml_hybrid.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "sml_internal.hpp"

namespace sml {

// Every device and pinned allocation of a context.  A buffer is named once, where it is
// allocated, with its size; all of them are freed together when the context goes.
// Memory comes zero-filled, and the fill is complete when the request returns (a buffer
// asked for in mid-run is then safe on any stream); zero = false leaves that out for a
// buffer whose every word is written before it is read.  The first failure sticks: later requests do nothing and
// status() reports it, so a list of allocations needs one check at its end.
class DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() {
        for (void *p : dev_) (void)hipFree(p);
        for (void *p : pinned_) (void)hipHostFree(p);
    }
    template <typename T>
    int device(T **p, size_t count, bool zero = true) {
        *p = nullptr;
        if (rc_) return rc_;
        void *v = nullptr;
        if (hipError_t e = hipMalloc(&v, count * sizeof(T)); e != hipSuccess) return fail_hip(e);
        dev_.push_back(v);
        if (zero) {
            if (hipError_t e = hipMemset(v, 0, count * sizeof(T)); e != hipSuccess) return fail_hip(e);
            if (hipError_t e = hipDeviceSynchronize(); e != hipSuccess) return fail_hip(e);
        }
        *p = static_cast<T *>(v);
        return SML_OK;
    }
    template <typename T>
    int pinned(T **p, size_t count, unsigned flags) {
        *p = nullptr;
        if (rc_) return rc_;
        void *v = nullptr;
        if (hipHostMalloc(&v, count * sizeof(T), flags) != hipSuccess)
            return rc_ = fail(SML_ERR_NOMEM, "pinned allocation of %zu bytes failed", count * sizeof(T));
        pinned_.push_back(v);
        std::memset(v, 0, count * sizeof(T));
        *p = static_cast<T *>(v);
        return SML_OK;
    }
    // one device buffer given back before the context goes (a pool or a table that is
    // re-laid larger): freed, forgotten, the pointer nulled.  The caller has made sure
    // that nothing in flight still reads it.
    template <typename T>
    void release(T **p) {
        const auto it = std::find(dev_.begin(), dev_.end(), static_cast<void *>(*p));
        if (it != dev_.end()) {
            (void)hipFree(*it);
            dev_.erase(it);
        }
        *p = nullptr;
    }
    int status() const { return rc_; }

private:
    int fail_hip(hipError_t e) { return rc_ = fail(SML_ERR_HIP, "device allocation: %s", hipGetErrorString(e)); }
    std::vector<void *> dev_, pinned_;
    int rc_ = SML_OK;
};

}  // namespace sml
