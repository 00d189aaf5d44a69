// ndt_buffer.hpp -- DeviceBuffer: a grow-only device allocation that a context keeps for the next frame (host code only).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ndt_hip.h"

namespace ndt_impl {

// sets the calling thread's ndt_hip_last_error() text and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// "Make this buffer hold at least N bytes and keep it for the next frame": every such buffer of the context and of its sinks.
// Deliberately not built on it: ndt_kd.hip's kd_grow, which keeps the old contents and doubles (another contract), and the ray
// workspace (ws_alloc, ws_allocs, sa_allocs in ndt_frame.hip), a set of allocations that is replaced together.
struct DeviceBuffer {
    void *p = nullptr;
    size_t bytes = 0;           // of the allocation; 0: nothing is held, whatever p says
    template <typename T> T *as() const { return (T *)p; }
    // At least `want` bytes (want 0 counts as 1); the contents are NOT kept when it grows.  Large enough already: a compare and a
    // return.  Otherwise `drain` is synchronised before the old allocation is freed (an empty buffer has nothing to wait for), and
    // after a failed hipMalloc the buffer is empty (null, 0), HIP's sticky error is dropped and NDT_E_NOMEM comes back.  With
    // head_room the allocation is a quarter larger than asked for.  The caller has set the current device.
    int reserve(size_t want, hipStream_t drain, const char *who, bool head_room = false)
    {
        if (want == 0) want = 1;
        return bytes >= want ? NDT_OK : grow(want, drain, who, head_room);
    }
    // hipFree if held; null / 0 afterwards; harmless on an empty buffer
    void release()
    {
        if (bytes) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }

private:
    int grow(size_t want, hipStream_t drain, const char *who, bool head_room)
    {
        if (bytes) {
            const hipError_t e = hipStreamSynchronize(drain);
            if (e != hipSuccess) return fail(NDT_E_DEVICE, "%s: hipStreamSynchronize: %s", who, hipGetErrorString(e));
            (void)hipFree(p);
        }
        p = nullptr;
        bytes = 0;
        const size_t size = head_room ? want + want / 4 : want;
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, size);
        if (e != hipSuccess) {
            (void)hipGetLastError();        // a failed allocation must not surface behind a later launch
            return fail(NDT_E_NOMEM, "%s: hipMalloc of %zu bytes: %s", who, size, hipGetErrorString(e));
        }
        p = q;
        bytes = size;
        return NDT_OK;
    }
};

} // namespace ndt_impl
