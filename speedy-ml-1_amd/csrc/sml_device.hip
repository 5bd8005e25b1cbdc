// sml_device.hip -- device plumbing that belongs to no unit: memory and copies for hosts
// without a GPU runtime binding of their own (the Fortran host), and the step
// timeline's debug entry.
#include <hip/hip_runtime.h>

#include "sml_internal.hpp"
#include "sml_timeline.hpp"

using namespace sml;

// ------------------------------------------------------------- diagnostics
// The step-accounting timeline (sml_timeline.hpp; profiling build only, -DSML_TL): a
// device buffer of per-(launch, block) start / end times of the step's kernels,
// attached to every translation unit; reset != 0 zeroes it (after the device is idle).
// *d_buf = the buffer (sml::tl::Buf), *bytes its size; SML_ERR_STATE in a build
// without the timeline.  Not in the public header (tools/probe_step_accounting.py).
extern "C" int sml_dbg_timeline(void **d_buf, int64_t *bytes, int reset) {
    SML_REQUIRE(d_buf && bytes, "null argument");
    static sml::tl::Buf *buf = nullptr;
    if (!buf) {
        sml::tl::Buf *b = nullptr;
        SML_HIP(hipMalloc(&b, sizeof(sml::tl::Buf)));
        if (sml::tl_attach_dynamics(b) || sml::tl_attach_spectral(b) || sml::tl_attach_reservoir(b) ||
            sml::tl_attach_hybrid(b)) {
            (void)hipFree(b);
            return fail(SML_ERR_STATE, "this build has no step timeline (compile with -DSML_TL)");
        }
        buf = b;
        reset = 1;
    }
    if (reset) {
        SML_HIP(hipDeviceSynchronize());
        SML_HIP(hipMemset(buf, 0, sizeof(sml::tl::Buf)));
        SML_HIP(hipDeviceSynchronize());
    }
    *d_buf = buf;
    *bytes = (int64_t)sizeof(sml::tl::Buf);
    return SML_OK;
}

// ------------------------------------------------------------- device memory
// zeroed device allocations and synchronous copies
extern "C" int sml_device_alloc(int64_t bytes, void **d_ptr) {
    SML_REQUIRE(d_ptr && bytes >= 0, "bad argument");
    *d_ptr = nullptr;
    SML_HIP(hipMalloc(d_ptr, bytes > 0 ? (size_t)bytes : 16));
    SML_HIP(hipMemset(*d_ptr, 0, bytes > 0 ? (size_t)bytes : 16));
    return SML_OK;
}

extern "C" int sml_device_free(void *d_ptr) {
    if (d_ptr) SML_HIP(hipFree(d_ptr));
    return SML_OK;
}

extern "C" int sml_copy_to_device(void *d_dst, const void *src, int64_t bytes) {
    SML_REQUIRE(d_dst && src && bytes >= 0, "bad argument");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(d_dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return SML_OK;
}

extern "C" int sml_copy_to_host(void *dst, const void *d_src, int64_t bytes) {
    SML_REQUIRE(dst && d_src && bytes >= 0, "bad argument");
    SML_HIP(hipDeviceSynchronize());
    SML_HIP(hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost));
    return SML_OK;
}
