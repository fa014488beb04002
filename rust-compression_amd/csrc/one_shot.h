// one_shot.h -- the round trip of a host-to-host call that makes ONE device call: bytes up into the leased engine's
// dec_in, the device call, `total` bytes of its oneshot_out down into a malloc'ed block.  df_encode_batch_dict,
// df_bgzf_encode_buffer, df_decode_batch_dict, df_decode_members_buffer, df_bgzf_read_buffer, bz_lzh_decode_batch,
// bz_lzh_encode_batch and bz_lha_read_buffer are their own parameter checks, their device call and their way of finding
// `total` around it.  (The calls that overlap copies with kernels -- CopyPool, the pinned ring -- are not this shape.)
// Every such entry point reports in this order: parameter errors; the empty result, which touches no device
// (one_shot_empty); BZ_E_NOGPU; the lease's status.  one_shot() answers the last two.
// Host only, as host_call.h; it wants bz_gpu_engine complete, with its DevBuf members dec_in and oneshot_out
// (engine_state.h includes it behind the engine; tests/host_stub/host_call_check.cpp behind a stand-in).
#pragma once
#include "dev_buf.h"
#include "host_call.h"

#include <cstdlib>

// A device number out of range is BZ_E_NOGPU for the entry points that ask here first (the one-shot calls, df_enc_create);
// the others pass on what bz_gpu_engine_create answers (BZ_E_PARAM).
inline int device_in_range(int device)
{
    int ndev = 0;
    return hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && device >= 0 && device < ndev ? BZ_OK : BZ_E_NOGPU;
}

// the result of no bytes: one byte, so that the caller has something to bz_free
inline int one_shot_empty(uint8_t **out)
{
    *out = (uint8_t *)malloc(1);
    return *out ? BZ_OK : BZ_E_NOMEM;
}

// the result: `total` bytes of device memory in a malloc'ed block (bz_free), one byte for none; *out is stored only with BZ_OK
inline int one_shot_download(uint8_t **out, const void *d_src, size_t total)
{
    uint8_t *h = (uint8_t *)malloc(total ? total : 1);
    if (!h) return BZ_E_NOMEM;
    if (total && hipMemcpy(h, d_src, total, hipMemcpyDeviceToHost) != hipSuccess) {
        free(h);
        return BZ_E_UNEXPECTED;
    }
    *out = h;
    return BZ_OK;
}

// What goes up: the entries of a batch packed into one image (BatchLayout), or one span of the caller's bytes.
struct OneShotIn {
    const BatchLayout *lay = nullptr;
    const uint8_t *p = nullptr;
    size_t n = 0;
    OneShotIn(const BatchLayout &l) : lay(&l), n((size_t)l.total) {}
    OneShotIn(const uint8_t *p_, size_t n_) : p(p_), n(n_) {}
};

constexpr size_t kOutGrown = ~(size_t)0; // out_bound: the device call grows g->oneshot_out itself, between its launches
enum OneShotSettle {
    kSettleStatus, // the engine is parked when the call ends BZ_OK and destroyed otherwise
    kSettleParamSound, // ... and parked after BZ_E_PARAM too: a call the sizes launch refused leaves a sound engine
};

// prefer: dec_cache_take's (2 for Deflate, 0 for LZHUF and LHA).  out_bound: oneshot_out holds that many bytes (+ 64)
// before the call, or kOutGrown.  call(g, &total): the device call, from g->dec_in.p into g->oneshot_out; its status, and in
// `total` the bytes of the result.  A decoder's data verdict is not its status.
template <class Call>
int one_shot(int device, int prefer, const OneShotIn &in, size_t out_bound, OneShotSettle rule, uint8_t **out, Call call)
{
    if (device_in_range(device) != BZ_OK) return BZ_E_NOGPU;
    EngineLease lease(device, prefer, 1);
    if (lease.status() != BZ_OK) return lease.status();
    bz_gpu_engine *g = lease.engine();
    std::vector<uint8_t> packed;
    const uint8_t *src = in.p;
    if (in.lay) {
        packed.resize(in.n + 16);
        in.lay->pack_into(packed.data());
        src = packed.data();
    }
    size_t total = 0;
    int rc = g->dec_in.ensure(in.n + 64);
    if (rc == BZ_OK && out_bound != kOutGrown) rc = g->oneshot_out.ensure(out_bound + 64);
    if (rc == BZ_OK && in.n && hipMemcpy(g->dec_in.p, src, in.n, hipMemcpyHostToDevice) != hipSuccess) rc = BZ_E_UNEXPECTED;
    if (rc == BZ_OK) rc = call(g, &total);
    if (rc == BZ_OK) rc = one_shot_download(out, g->oneshot_out.p, total);
    lease.settle(rule == kSettleParamSound && rc == BZ_E_PARAM ? BZ_OK : rc);
    return rc;
}
