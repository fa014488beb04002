// lzhuf_engine.hip -- the driver of the LZHUF decoder (include/bz2_mi355x.h section 9; kernel: k_lzhuf.hip): the device
// call with its two launches, its figures, and the host-to-host forms on an engine of the per-process cache (host_call.h).
#include "engine_state.h"
#include "k_lzhuf.h"

#include <cstdlib>
#include <vector>

using namespace lzhgpu;

struct LzhWorkspace {
    DevBuf in, olen, ooff, rec; // the entries' ranges, their known lengths, their outputs' places, their records
    u64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void lzh_workspace_free(LzhWorkspace *w) { delete w; }

// dictionary_bits and offset_bits of a method (src/lzhuf/mod.rs:22-38); false: no such method
static bool lzh_method(int method, u32 &dbits, u32 &pbits)
{
    switch (method) {
    case BZ_LZH_LH4: dbits = 12, pbits = 4; return true;
    case BZ_LZH_LH5: dbits = 13, pbits = 4; return true;
    case BZ_LZH_LH6: dbits = 15, pbits = 5; return true;
    case BZ_LZH_LH7: dbits = 16, pbits = 5; return true;
    }
    return false;
}
static bool lzh_params_ok(int method, int prefill)
{
    u32 d, p;
    return lzh_method(method, d, p) && prefill >= -1 && prefill <= 255;
}

extern "C" int bz_gpu_last_lzh_decode_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->lzh ? g->lzh->stats[i] : 0;
    return BZ_OK;
}

// grow != nullptr: the output is the engine's own buffer, sized between the two launches (the host forms)
static int lzh_decode_batch_core(bz_gpu_engine *g, int method, int prefill, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                                 const uint64_t *h_orig_len, size_t count, void *d_out, size_t cap, DevBuf *grow, uint64_t *h_out_off,
                                 uint64_t *h_out_len, int32_t *h_verdict)
{
    u32 dbits = 0, pbits = 0;
    if (!g || !lzh_method(method, dbits, pbits) || prefill < -1 || prefill > 255) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !h_verdict || count > 0x7FFFFFFFu) return BZ_E_PARAM;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return BZ_E_PARAM;
    u64 in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 3u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i] || h_in_len[i] > 0xFFFFFFFFull) return BZ_E_PARAM;
        in_end = h_in_off[i] + h_in_len[i];
    }
    if (in_end && !d_in) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    if (!g->lzh) g->lzh = new LzhWorkspace();
    LzhWorkspace *w = g->lzh;
    for (u64 &s : w->stats) s = 0;
    int rc = w->in.ensure(2 * count * sizeof(u64));
    if (rc == BZ_OK) rc = w->olen.ensure(count * sizeof(u64));
    if (rc == BZ_OK) rc = w->ooff.ensure(count * sizeof(u64));
    if (rc == BZ_OK) rc = w->rec.ensure(count * sizeof(LzhRec));
    if (rc != BZ_OK) return rc;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    u64 *d_off = w->in.as<u64>(), *d_len = d_off + count, *d_ooff = w->ooff.as<u64>();
    u64 *d_olen = h_orig_len ? w->olen.as<u64>() : nullptr;
    LzhRec *d_rec = w->rec.as<LzhRec>();
    HIPCHK(hipMemcpyAsync(d_off, h_in_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(d_len, h_in_len, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    if (d_olen) HIPCHK(hipMemcpyAsync(d_olen, h_orig_len, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    // ---- the sizes
    if (lzh_launch_decode(g->st, false, in8, d_off, d_len, d_olen, (u32)count, dbits, pbits, prefill, nullptr, nullptr, d_rec) != 0)
        return BZ_E_UNEXPECTED;
    std::vector<LzhRec> rec(count);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, count * sizeof(LzhRec), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    // the outputs' places: input order, each at a multiple of 16
    u64 cursor = 0, need = 0;
    for (size_t i = 0; i < count; ++i) {
        if (rec[i].flags & 1u) return BZ_E_PARAM; // an entry of 4 GiB or more of output
        h_out_off[i] = cursor;
        h_out_len[i] = rec[i].len;
        h_verdict[i] = rec[i].verdict;
        need = cursor + rec[i].len;
        cursor += ((u64)rec[i].len + 15u) & ~(u64)15;
    }
    u8 *out8 = static_cast<u8 *>(d_out);
    if (grow) {
        rc = grow->ensure((size_t)need + 64);
        if (rc != BZ_OK) return rc;
        out8 = grow->as<u8>();
    } else if (d_out && need > cap) return BZ_E_CAPACITY;
    // ---- the bytes
    if (out8) {
        HIPCHK(hipMemcpyAsync(d_ooff, h_out_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
        if (lzh_launch_decode(g->st, true, in8, d_off, d_len, d_olen, (u32)count, dbits, pbits, prefill, out8, d_ooff, d_rec) != 0)
            return BZ_E_UNEXPECTED;
        HIPCHK(hipStreamSynchronize(g->st));
        w->stats[7] = 2;
    } else w->stats[7] = 1;
    for (size_t i = 0; i < count; ++i) {
        const LzhRec &q = rec[i];
        w->stats[q.verdict == BZ_OK ? 0 : 1] += 1;
        w->stats[2] += q.nblk;
        w->stats[3] += q.nlit;
        w->stats[4] += q.nmatch;
        w->stats[5] += q.len;
        if (q.verdict == BZ_OK) w->stats[6] += (q.end_bit + 7u) >> 3;
    }
    return BZ_OK;
}

extern "C" int bz_gpu_lzh_decode_batch_device(bz_gpu_engine *g, int method, int prefill, const void *d_in, const uint64_t *h_in_off,
                                              const uint64_t *h_in_len, const uint64_t *h_orig_len, size_t count, void *d_out, size_t cap,
                                              uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict)
{
    return lzh_decode_batch_core(g, method, prefill, d_in, h_in_off, h_in_len, h_orig_len, count, d_out, cap, nullptr, h_out_off, h_out_len,
                                 h_verdict);
}

// Many streams: packed at 4-byte-aligned offsets (BatchLayout), one upload, one device call (the engine's output buffer
// sized between its two launches), one download.
extern "C" int bz_lzh_decode_batch(int method, int prefill, int device, const uint8_t *const *ins, const size_t *lens, const uint64_t *orig_lens,
                                   size_t count, uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (!lzh_params_ok(method, prefill)) return BZ_E_PARAM;
    if (count && (!ins || !lens || !out_off || !out_len || !verdict)) return BZ_E_PARAM;
    const BatchLayout lay(ins, lens, count, 4);
    if (lay.status != BZ_OK) return lay.status;
    for (size_t i = 0; i < count; ++i)
        if (lens[i] > 0xFFFFFFFFull) return BZ_E_PARAM;
    if (count == 0) {
        *out = (uint8_t *)malloc(1);
        return *out ? BZ_OK : BZ_E_NOMEM;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BZ_E_NOGPU;
    EngineLease lease(device, 0, 1);
    if (lease.status() != BZ_OK) return lease.status();
    bz_gpu_engine *g = lease.engine();
    std::vector<uint8_t> packed((size_t)lay.total + 16);
    lay.pack_into(packed.data());
    int rc = g->dec_in.ensure((size_t)lay.total + 64);
    if (rc == BZ_OK && lay.total && hipMemcpy(g->dec_in.p, packed.data(), (size_t)lay.total, hipMemcpyHostToDevice) != hipSuccess)
        rc = BZ_E_UNEXPECTED;
    if (rc == BZ_OK)
        rc = lzh_decode_batch_core(g, method, prefill, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), orig_lens, count, nullptr, 0,
                                   &g->oneshot_out, out_off, out_len, verdict);
    if (rc == BZ_OK) {
        const size_t total = (size_t)(out_off[count - 1] + out_len[count - 1]);
        uint8_t *h = (uint8_t *)malloc(total ? total : 1);
        if (!h) rc = BZ_E_NOMEM;
        else if (total && hipMemcpy(h, g->oneshot_out.p, total, hipMemcpyDeviceToHost) != hipSuccess) {
            free(h);
            rc = BZ_E_UNEXPECTED;
        } else *out = h;
    }
    // a call the sizes launch refused (an entry of 4 GiB of output) leaves a sound engine; so do the entries' verdicts
    lease.settle(rc == BZ_E_PARAM ? BZ_OK : rc);
    return rc;
}

// The batch of one: BZ_OK with the bytes, or the entry's verdict with the bytes in front of it (as df_decode_buffer).
extern "C" int bz_lzh_decode_buffer(int method, int prefill, int device, const uint8_t *in, size_t in_len, uint64_t orig_len, uint8_t **out,
                                    size_t *out_len)
{
    if (!out || !out_len || (in_len && !in)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    uint64_t off = 0, len = 0;
    int32_t verdict = BZ_OK;
    const uint8_t *ins[1] = {in};
    const size_t lens[1] = {in_len};
    const uint64_t ol[1] = {orig_len};
    const int rc = bz_lzh_decode_batch(method, prefill, device, ins, lens, ol, 1, out, &off, &len, &verdict);
    if (rc != BZ_OK) return rc;
    *out_len = (size_t)len; // (the one entry lies at offset 0)
    return verdict;
}
