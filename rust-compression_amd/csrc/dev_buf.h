// dev_buf.h -- a block of device memory that is freed with the object that holds it: an engine's or a workspace's
// DevBuf members go with its `delete`, one on the stack goes on every way out of its scope.
// No DevBuf may have static storage duration, directly or inside a static object: hipFree after the HIP runtime has
// been torn down is not safe.  What outlives a call (the cached engines of dec_engine.hip) is held by pointer and
// freed by bz_release_cached_resources.
#pragma once
#include "../../include/bz2_mi355x.h"
#ifdef BZ_HOST_PIPELINE_TEST
#include "hip_shim.h" // tests/host_stub: the HIP calls on the host (tests/test_devbuf_host.py)
#else
#include <hip/hip_runtime.h>
#endif

#include <utility>

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) {
            release(); // (what the target held is freed)
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return BZ_OK;
        release(); // (free before grow: the old and the new block never exist side by side)
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) {
            if (hipMalloc(&p, bytes) != hipSuccess) {
                p = nullptr; // (whatever the failed call left there is not ours to free)
                return BZ_E_NOMEM;
            }
            want = bytes;
        }
        cap = want;
        return BZ_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
