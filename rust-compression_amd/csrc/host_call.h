// host_call.h -- what every host-to-host entry point does around its device work, in one place: the caller's HIP
// device (CallerDevice), the engine a call borrows from the per-process cache (EngineLease: THE keep-or-destroy rule),
// the packing of a batch's entries into one image (BatchLayout), HIPCHK and the host clock (now_ms).
// Host only; of HIP it uses hipGetDevice and hipSetDevice, and bz_gpu_engine stays an incomplete type.  Compiled as it
// is by a host compiler against tests/host_stub/hip_shim.h (tests/test_host_call_host.py).
#pragma once
#include "../../include/bz2_mi355x.h"
#ifdef BZ_HOST_PIPELINE_TEST
#include "hip_shim.h"
#else
#include <hip/hip_runtime.h>
#endif

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define HIPCHK(x)                                                                                     \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "bz2_mi355x: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__,   \
                    __LINE__);                                                                        \
            return BZ_E_UNEXPECTED;                                                                   \
        }                                                                                             \
    } while (0)

// the host's steady clock in milliseconds: the spans the *_timings and the traces report
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The engines that host-to-host calls and streaming contexts of BOTH codecs park between uses (engine_cache.hip).
// prefer: 1 = an engine that holds a bzip2 decode workspace, 2 = one that holds a Deflate workspace.
struct bz_gpu_engine *dec_cache_take(int device, int prefer = 0);
void dec_cache_put(int device, struct bz_gpu_engine *g);
void dec_release_cached();

// The calling thread's current HIP device is the caller's business: the entry points switch devices (lanes of a
// multi-device context live on different GPUs) and put the caller's device back when they return.  Worker threads
// keep their own.
struct CallerDevice {
    int dev = -1;
    CallerDevice() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~CallerDevice() { if (dev >= 0) (void)hipSetDevice(dev); }
    CallerDevice(const CallerDevice &) = delete;
    CallerDevice &operator=(const CallerDevice &) = delete;
};

// An engine of `device` for the length of a call, and the device selected.  The call reports its INFRASTRUCTURE status
// with settle(); the destructor parks the engine for the next call when that status is BZ_OK and destroys it otherwise
// (a sticky HIP error, a half-grown workspace), and an engine nobody settled is destroyed.  A decoder's data verdict (a
// truncated or corrupt stream) is no such status: the engine is sound, settle(BZ_OK).  Then the caller's device is put
// back, also when no engine could be made.
// A streaming context holds its engine across calls: it takes it out with release() and ends it through a lease that
// adopts it, settled with the context's own notion of "good".
class EngineLease {
    CallerDevice caller_; // (a member: restored behind the destructor's body, on every path)
    int device_;
    bz_gpu_engine *g_;
    int status_ = BZ_OK, settled_ = BZ_E_UNEXPECTED;

public:
    EngineLease(int device, int prefer, size_t max_blocks_for_create) : device_(device), g_(dec_cache_take(device, prefer))
    {
        if (!g_) status_ = bz_gpu_engine_create(&g_, device, max_blocks_for_create);
        if (status_ != BZ_OK) g_ = nullptr;
        else if (hipSetDevice(device) != hipSuccess) status_ = BZ_E_UNEXPECTED;
    }
    EngineLease(int device, bz_gpu_engine *held) : device_(device), g_(held)
    {
        if (hipSetDevice(device) != hipSuccess) status_ = BZ_E_UNEXPECTED;
    }
    ~EngineLease()
    {
        if (!g_) return;
        if (settled_ == BZ_OK) dec_cache_put(device_, g_);
        else bz_gpu_engine_destroy(g_);
    }
    int status() const { return status_; } // BZ_OK: engine() is there and its device is selected
    bz_gpu_engine *engine() const { return g_; }
    void settle(int rc) { settled_ = rc; }
    bz_gpu_engine *release()
    {
        bz_gpu_engine *g = g_;
        g_ = nullptr;
        return g;
    }
};

// The entries of a batch call side by side in one image: entry i at in_off[i], a multiple of `align` (a power of two),
// `total` bytes in all.  status: BZ_E_PARAM when an entry announces bytes without a pointer.
struct BatchLayout {
    std::vector<uint64_t> in_off, in_len;
    uint64_t total = 0;
    int status = BZ_OK;
    const uint8_t *const *ins;

    BatchLayout(const uint8_t *const *ins_, const size_t *lens, size_t count, uint64_t align) : in_off(count), in_len(count), ins(ins_)
    {
        for (size_t i = 0; i < count; ++i) {
            if (lens[i] && !ins[i]) status = BZ_E_PARAM;
            in_off[i] = total;
            in_len[i] = lens[i];
            total += ((uint64_t)lens[i] + align - 1) & ~(align - 1);
        }
    }
    // the bytes between the entries are left as they are: `dst` is a zeroed image, or one whose padding nobody reads
    template <class Copy> void pack_into(uint8_t *dst, Copy copy) const
    {
        for (size_t i = 0; i < in_len.size(); ++i)
            if (in_len[i]) copy(dst + in_off[i], ins[i], (size_t)in_len[i]);
    }
    void pack_into(uint8_t *dst) const
    {
        pack_into(dst, [](uint8_t *d, const uint8_t *s, size_t n) { memcpy(d, s, n); });
    }
};
