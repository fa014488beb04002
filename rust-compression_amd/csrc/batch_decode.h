// batch_decode.h -- the frame of a two-phase batch decode (sizes, then bytes) that df_decode_batch_core and
// lzh_decode_batch_core share: the check of the entries' ranges, the outputs' places and the buffer they need, the one
// reservation all entries that go across many waves share, and the tail of such an entry's writing (pointer jumping, the
// gather).  Plain functions; what differs between the codecs (the search, the candidate and chain rules, repair, the
// checksum fold, the window, known lengths) stays with them.
// Host only, as host_call.h: of the kernels it knows the two launchers of the tail by declaration.
#pragma once
#include "dev_buf.h"
#include "host_call.h"

#include <algorithm>

namespace dfgpu { // k_deflate.h
int df_launch_split_jump(hipStream_t st, uint32_t *src, uint32_t n, uint32_t *cnt);
int df_launch_split_gather(hipStream_t st, uint8_t *out, const uint32_t *src, uint32_t n);
} // namespace dfgpu

// The entries' ranges in d_in: offsets that are multiples of 4, ascending and disjoint, no off + len that wraps, no entry
// of 4 GiB or more, at most 2^31 - 1 entries, bytes only where there is a pointer, both pointers 16-byte aligned.
inline bool batch_ranges_ok(const void *d_in, const void *d_out, const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count)
{
    if (count > 0x7FFFFFFFu || ((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return false;
    uint64_t in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 3u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i] || h_in_len[i] > 0xFFFFFFFFull) return false;
        in_end = h_in_off[i] + h_in_len[i];
    }
    return !in_end || d_in;
}

// The outputs' places from the sizes phase's records (Rec: len, verdict, flags): input order, each at a multiple of 16, or
// where h_place says.  *need: the largest off + len (the offsets ascend when no places are given, so the last entry's,
// empty or not).  BZ_E_PARAM: an entry of 4 GiB or more of output.
template <class Rec>
int batch_place(const Rec *rec, size_t count, const uint64_t *h_place, uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict, uint64_t *need)
{
    uint64_t cursor = 0;
    *need = 0;
    for (size_t i = 0; i < count; ++i) {
        if (rec[i].flags & 1u) return BZ_E_PARAM;
        h_out_off[i] = h_place ? h_place[i] : cursor;
        h_out_len[i] = rec[i].len;
        h_verdict[i] = rec[i].verdict;
        *need = std::max(*need, h_out_off[i] + rec[i].len);
        cursor += ((uint64_t)rec[i].len + 15u) & ~(uint64_t)15;
    }
    return BZ_OK;
}

// Where the bytes go: the engine's own buffer grown to need + 64 (the host forms), or the caller's d_out when `need` fits
// its cap (BZ_E_CAPACITY); *out8 stays null for a call that wants the sizes alone.
inline int batch_output(uint64_t need, void *d_out, size_t cap, DevBuf *grow, uint8_t **out8)
{
    *out8 = static_cast<uint8_t *>(d_out);
    if (grow) {
        const int rc = grow->ensure((size_t)need + 64);
        if (rc != BZ_OK) return rc;
        *out8 = grow->as<uint8_t>();
    } else if (d_out && need > cap) return BZ_E_CAPACITY;
    return BZ_OK;
}

// The entries that go across many waves (Entry: index, rec.len) are written one after the other, so ONE source map (four
// bytes per output byte of the largest) and one counter serve all of them: sized here when a writing phase follows, before
// any entry is committed to the split path.  If they cannot be had, every entry takes the one-wave path (and the failed
// allocation's error is not the next launch's).  len_small: the entries' lengths with the split entries as entries of no
// bytes, which they are in the launches over all entries (empty: none is split).  Returns the entries sent back.
template <class Entry>
size_t split_reserve(std::vector<Entry> &splits, bool will_write, DevBuf &map, DevBuf &counter, const uint64_t *h_in_len, size_t count,
                     std::vector<uint64_t> &len_small)
{
    size_t dropped = 0;
    if (!splits.empty() && will_write) {
        size_t map_bytes = 0;
        for (const Entry &e : splits) map_bytes = std::max(map_bytes, (size_t)e.rec.len * 4 + 64);
        if (map.ensure(map_bytes) != BZ_OK || counter.ensure(64) != BZ_OK) {
            (void)hipGetLastError();
            dropped = splits.size();
            splits.clear();
        }
    }
    len_small.clear();
    if (!splits.empty()) {
        len_small.assign(h_in_len, h_in_len + count);
        for (const Entry &e : splits) len_small[e.index] = 0;
    }
    return dropped;
}

// The tail of a split entry's writing, behind the launch that wrote its n bytes and their source map: pointer jumping until
// a round moves nothing (none when !jump), then the gather if round 0 found bytes left to fetch.  The callers count the
// figures into their own slots.
struct SplitTail {
    uint32_t rounds = 0, left = 0, launches = 0;
    double jump_ms = 0, gather_ms = 0; // host clock around launches that are waited for
};
inline int split_jump_gather(hipStream_t st, bool jump, uint32_t *map, uint32_t n, uint32_t *cnt, uint8_t *eout, SplitTail &t)
{
    const double t0 = now_ms();
    while (jump) {
        uint32_t h[2] = {0, 0}; // what round 0 found left to fetch, what this round moved
        HIPCHK(hipMemsetAsync(cnt, 0, 8, st));
        if (dfgpu::df_launch_split_jump(st, map, n, cnt) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        t.launches += 1;
        if (t.rounds++ == 0) t.left = h[0];
        if (h[1] == 0) break;
    }
    const double t1 = now_ms();
    t.jump_ms = t1 - t0;
    if (t.left) {
        if (dfgpu::df_launch_split_gather(st, eout, map, n) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipStreamSynchronize(st));
        t.launches += 1;
    }
    t.gather_ms = now_ms() - t1;
    return BZ_OK;
}
