// bgzf_index.h -- reading BGZF (include/bz2_mi355x.h section 8, DESIGN_deflate.md "Reading BGZF"): the rule that says what a
// block header is, and the chain that walks a file from block to block by BSIZE and sums ISIZE.  They exist here only:
// df_bgzf_index_buffer walks host memory with them, k_bgzf_search / k_bgzf_block_info (k_bgzf_read.hip) run the header rule
// with one byte position per lane and df_gpu_bgzf_index_device walks the list they leave, k_bgzf_inflate checks the
// header of every block it decodes with the same words.
//
// A BLOCK HEADER at byte p is htslib's rule with FLG exact: in[p .. p + 16) == 1f 8b 08 04 ?? ?? ?? ?? ?? ?? 06 00 42 43 02 00
// (MTIME, XFL and OS may be anything; FLG is exactly 4; XLEN is exactly 6 with the BC subfield first and alone).  BSIZE is
// the u16 at p + 16, the block is BSIZE + 1 bytes, ISIZE is the u32 in its last four bytes.
//
// Plain C++17 without HIP headers (tests/host_stub/bgzf_index_check.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifndef BZ_HD
#ifdef __HIPCC__
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif
#endif

namespace bgzf {

constexpr uint32_t kHeader = 18;       // bytes in front of the Deflate bytes
constexpr uint32_t kTrailer = 8;       // CRC-32, ISIZE
constexpr uint32_t kMinBlock = 28;     // 18 + a 2-byte empty final block + 8: the EOF marker
constexpr uint32_t kMaxBlock = 65536;  // BSIZE + 1 at most, and ISIZE at most
constexpr uint32_t kTile = 4096;       // byte positions per workgroup of the search
constexpr uint32_t kBatch = 65536;     // candidates per list window, blocks per decode launch (BZ_DF_BGZF_BATCH)
constexpr int kOk = 0, kData = -1, kEof = -2; // BZ_OK, BZ_E_DATA, BZ_E_EOF (static_assert'ed where the public header is in sight)

// the header rule on the sixteen bytes at p as four little-endian words (bytes 4 .. 9, all of w1 and half of w2, are free)
BZ_HD inline bool header_words(uint32_t w0, uint32_t w2, uint32_t w3)
{
    return w0 == 0x04088B1Fu && (w2 >> 16) == 0x0006u && w3 == 0x00024342u;
}

BZ_HD inline uint32_t le32(const uint8_t *b) { return (uint32_t)b[0] | (uint32_t)b[1] << 8 | (uint32_t)b[2] << 16 | (uint32_t)b[3] << 24; }

// the sixteen bytes at p (all inside the caller's buffer)
BZ_HD inline bool header_at(const uint8_t *p) { return header_words(le32(p), le32(p + 8), le32(p + 12)); }

// A position the search lists: the header rule holds and at least kHeader bytes lie behind p.
BZ_HD inline bool candidate_at(const uint8_t *in, uint64_t len, uint64_t p)
{
    return p <= len && len - p >= kHeader && header_at(in + p);
}

// One step of the chain at a position with `left` > 0 bytes behind it, from what the first 18 bytes say: header_ok and
// bsize1 = BSIZE + 1 are looked at only when left >= kHeader.  kOk: the block lies whole inside the file, ISIZE is next.
BZ_HD inline int head_verdict(uint64_t left, bool header_ok, uint32_t bsize1)
{
    if (left < kHeader) return kEof;   // a cut header, whatever its bytes are
    if (!header_ok) return kData;
    if (bsize1 < kMinBlock) return kData;
    if (bsize1 > left) return kEof;
    return kOk;
}
BZ_HD inline int isize_verdict(uint32_t isize) { return isize > kMaxBlock ? kData : kOk; }

// THE CHAIN over a file of `len` bytes.  look(pos, &header_ok, &bsize1, &isize) is asked at every position with at least
// kHeader bytes behind it: whether the header rule holds there, BSIZE + 1 if it does, and ISIZE if the block then lies whole
// inside the file (else anything); it returns 0, or a status that ends the walk and is returned as it is.  block(coff, uoff)
// is told every block in order.  *end_c / *end_u: the end of the last complete block, the index's last pair.  Zero padding
// is not skipped, the 28-byte EOF marker is an ordinary block with ISIZE 0.
template <class Look, class Block>
inline int chain(uint64_t len, Look &&look, Block &&block, uint64_t *end_c, uint64_t *end_u, int *verdict)
{
    uint64_t pos = 0, upos = 0;
    int v = kOk;
    while (pos != len) {
        const uint64_t left = len - pos;
        bool ok = false;
        uint32_t bsize1 = 0, isize = 0;
        if (left >= kHeader) {
            const int rc = look(pos, &ok, &bsize1, &isize);
            if (rc != 0) return rc;
        }
        v = head_verdict(left, ok, bsize1);
        if (v == kOk) v = isize_verdict(isize);
        if (v != kOk) break;
        block(pos, upos);
        pos += bsize1;
        upos += isize;
    }
    *end_c = pos;
    *end_u = upos;
    *verdict = v;
    return 0;
}

// ... over host memory: nothing at or behind in + len is read
template <class Block>
inline int chain_host(const uint8_t *in, uint64_t len, Block &&block, uint64_t *end_c, uint64_t *end_u, int *verdict)
{
    return chain(
        len,
        [&](uint64_t pos, bool *ok, uint32_t *bsize1, uint32_t *isize) {
            *ok = header_at(in + pos);
            *bsize1 = ((uint32_t)in[pos + 16] | (uint32_t)in[pos + 17] << 8) + 1u;
            if (*ok && *bsize1 >= kMinBlock && *bsize1 <= len - pos) *isize = le32(in + pos + *bsize1 - 4);
            return 0;
        },
        block, end_c, end_u, verdict);
}

// ---- a range of the uncompressed bytes over an index of `count` blocks (count + 1 ascending pairs): the blocks it touches.
// The range is [ustart, uend) with ustart < uend <= uoff[count].  first: the block that holds byte ustart; last: the block
// that holds byte uend - 1.  Empty blocks between them are touched too (they are decoded and checked: no bytes), empty
// blocks in front of `first` or behind `last` are not.
inline void touched(const uint64_t *uoff, uint64_t count, uint64_t ustart, uint64_t uend, uint64_t *first, uint64_t *last)
{
    uint64_t lo = 0, hi = count; // the last k with uoff[k] <= ustart
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (uoff[mid] <= ustart) lo = mid;
        else hi = mid;
    }
    *first = lo;
    lo = *first, hi = count; // the last k with uoff[k] < uend
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (uoff[mid] < uend) lo = mid;
        else hi = mid;
    }
    *last = lo;
}

} // namespace bgzf
