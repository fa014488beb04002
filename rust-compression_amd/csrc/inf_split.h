// inf_split.h -- one large Deflate stream decoded by many waves (include/bz2_mi355x.h section 5, DESIGN_deflate.md "One
// large stream across many waves"): the rules that say where a piece of the stream MAY start (a candidate) and the rule
// that says whether it DOES (the chain).  They exist here only: k_df_split_search (k_inflate.hip) runs the candidate rules
// with one bit offset per lane, the host loop of df_split_sizes (deflate_engine.hip) runs the chain.
//
// A candidate is a bit position at which a NON-FINAL block header is valid under every rule k_df_inflate enforces:
//   mode 0, a dynamic header at that bit: HLIT <= 286, HDIST <= 30, a complete code-length code, no repeat without a
//           predecessor, no run past HLIT + HDIST, an end-of-block code, a complete literal/length set, a complete distance
//           set or one of the two accepted exceptions (no distance code, one code of length 1);
//   mode 1, the LEN field of a stored block at that bit (a multiple of 8): LEN ^ NLEN == 0xFFFF, three zero header bits
//           inside the ten bits in front, the payload inside the entry, and behind the payload a block header that can be
//           CHECKED and holds: a stored block's LEN ^ NLEN or a whole dynamic header, final or not.  LEN / NLEN alone match
//           at one byte position in 65 536, and a fixed block behind the payload has nothing to check: counting it as
//           "decodable" lets one such position in four through, and a 64 MiB stream then used up its four repair rounds
//           and decoded half its bytes in the serial tail (profiles/r14_inflate_split.md, run 1).  So a stored block in
//           front of a fixed one is no candidate: the piece in front of it decodes through it.
// Nothing here needs an array: the code lengths are looked at once, as they are decoded, and only their Kraft sums are kept.
//
// Plain C++17 without HIP headers (tests/host_stub/inf_split_check.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifndef BZ_HD
#ifdef __HIPCC__
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif
#endif

namespace infsplit {

constexpr uint32_t kRepairRounds = 4;        // pieces decoded one at a time behind false candidates, before the serial tail
constexpr uint64_t kNoStop = ~0ull;          // a piece that runs to the end of the stream
constexpr uint32_t kBaseUnknown = 0xFFFFFFFFu; // a piece that does not know where its output starts

// the entry's bytes; bits behind its end read as zero and are never touched
struct BitSrc {
    const uint8_t *base;
    uint64_t len;
    BZ_HD uint64_t nbits() const { return 8ull * len; }
    // at least 57 bits from `bit` on, bit 0 first
    BZ_HD uint64_t bits(uint64_t bit) const
    {
        const uint64_t b = bit >> 3;
        uint64_t v = 0;
        for (uint32_t k = 0; k < 8; ++k)
            if (b + k < len) v |= (uint64_t)base[b + k] << (8 * k);
        return v >> (bit & 7u);
    }
};

// ---- the register-only prefilter of a dynamic header: lo = bits [0, 64) from the position, hi = bits [64, 128)
BZ_HD inline bool dyn_prefilter(uint64_t lo, uint64_t hi)
{
    if ((lo & 7u) != 4u) return false; // BFINAL 0, BTYPE 2
    if (((lo >> 3) & 31u) > 29u || ((lo >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = (uint32_t)((lo >> 13) & 15u) + 4u;
    const uint64_t v = (lo >> 17) | (hi << 47); // the up to 19 three-bit lengths
    uint32_t kraft = 0;                         // in units of 2^-7
    for (uint32_t k = 0; k < 19; ++k) {
        const uint32_t l = (uint32_t)(v >> (3 * k)) & 7u;
        if (k < hclen && l) kraft += 128u >> l;
    }
    return kraft == 128u;
}

// c_cl_order of k_inflate.hip, five bits per entry
BZ_HD inline uint32_t cl_order(uint32_t k)
{
    constexpr uint64_t a = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                           11ull << 50 | 4ull << 55;
    constexpr uint64_t b = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12 ? a >> (5 * k) : b >> (5 * (k - 12))) & 31u);
}

// A dynamic block header at `bit`, whole: every rule of k_df_inflate between the three header bits and the block's first
// code.  final_ok: a final block counts too (the header behind a stored candidate's payload).
BZ_HD inline bool dyn_header_ok(const BitSrc &s, uint64_t bit, bool final_ok)
{
    const uint64_t total = s.nbits();
    if (bit + 17 > total) return false;
    uint64_t x = s.bits(bit);
    if (((x >> 1) & 3u) != 2u || ((x & 1u) && !final_ok)) return false;
    const uint32_t hlit = (uint32_t)((x >> 3) & 31u) + 257u, hdist = (uint32_t)((x >> 8) & 31u) + 1u, hclen = (uint32_t)((x >> 13) & 15u) + 4u;
    if (hlit > 286u || hdist > 30u) return false;
    uint64_t pos = bit + 17;
    if (pos + 3ull * hclen > total) return false;
    x = s.bits(pos);
    uint64_t cl = 0;  // the code-length code: three bits per symbol
    uint64_t cnt = 0; // codes per length, five bits each
    uint32_t kraft = 0;
    for (uint32_t k = 0; k < hclen; ++k) {
        const uint64_t l = (x >> (3 * k)) & 7u;
        cl |= l << (3 * cl_order(k));
        if (l) {
            cnt += 1ull << (5 * l);
            kraft += 128u >> l;
        }
    }
    if (kraft != 128u) return false;
    pos += 3ull * hclen;
    const uint32_t ncl = hlit + hdist;
    uint32_t i = 0, prev = 0, eob = 0, kl = 0, kd = 0, nd = 0, maxd = 0;
    while (i < ncl) {
        x = s.bits(pos);
        // one code of the (complete) code-length code: the canonical walk
        uint32_t code = 0, first = 0, sy = 0, l = 1;
        for (; l <= 7u; ++l) {
            code |= (uint32_t)(x >> (l - 1)) & 1u;
            const uint32_t c = (uint32_t)(cnt >> (5 * l)) & 31u;
            if (code < first + c) break;
            first = (first + c) << 1;
            code <<= 1;
        }
        if (l > 7u) return false; // (cannot happen with a complete code)
        for (uint32_t k = code - first, q = 0; q < 19; ++q)
            if (((cl >> (3 * q)) & 7u) == l) {
                if (k == 0) {
                    sy = q;
                    break;
                }
                --k;
            }
        x >>= l;
        pos += l;
        uint32_t rep = 1, val = sy;
        if (sy == 16) {
            if (i == 0) return false;
            rep = 3u + (uint32_t)(x & 3u);
            val = prev;
            pos += 2;
        } else if (sy == 17) {
            rep = 3u + (uint32_t)(x & 7u);
            val = 0;
            pos += 3;
        } else if (sy == 18) {
            rep = 11u + (uint32_t)(x & 127u);
            val = 0;
            pos += 7;
        }
        if (pos > total || i + rep > ncl) return false;
        if (val) {
            const uint32_t nl = (i + rep < hlit ? i + rep : hlit) - (i < hlit ? i : hlit);
            kl += nl * (32768u >> val);
            kd += (rep - nl) * (32768u >> val);
            if (rep - nl) {
                nd += rep - nl;
                if (val > maxd) maxd = val;
            }
            if (i <= 256u && 256u < i + rep) eob = val;
            if (kl > 32768u || kd > 32768u) return false; // over-subscribed
        }
        prev = val;
        i += rep;
    }
    if (eob == 0 || kl != 32768u) return false;
    return kd == 32768u || nd == 0 || (nd == 1 && maxd == 1);
}

// LEN ^ NLEN at byte `b`, the payload inside the entry
BZ_HD inline bool stored_fields_ok(const BitSrc &s, uint64_t b, uint32_t &ln)
{
    if (b + 4 > s.len) return false;
    const uint32_t v = (uint32_t)s.bits(8 * b);
    ln = v & 0xFFFFu;
    return (ln ^ (v >> 16)) == 0xFFFFu && b + 4 + ln <= s.len;
}

// a stored or dynamic block header at `bit`, final or not, that k_df_inflate would get past (a fixed block has nothing to check)
BZ_HD inline bool checked_header_ok(const BitSrc &s, uint64_t bit)
{
    if (bit + 3 > s.nbits()) return false;
    const uint32_t btype = (uint32_t)(s.bits(bit) >> 1) & 3u;
    uint32_t ln;
    if (btype == 0) return stored_fields_ok(s, (bit + 3 + 7) >> 3, ln);
    return btype == 2 && dyn_header_ok(s, bit, true);
}

// the LEN field of a non-final stored block at `bit` (a multiple of 8)
BZ_HD inline bool stored_ok(const BitSrc &s, uint64_t bit)
{
    uint32_t ln;
    if ((bit & 7u) || bit < 3 || !stored_fields_ok(s, bit >> 3, ln)) return false;
    bool head = false;
    for (uint64_t h = bit >= 10 ? bit - 10 : 0; h + 3 <= bit; ++h) head = head || (s.bits(h) & 7u) == 0;
    return head && checked_header_ok(s, 8 * ((bit >> 3) + 4 + ln));
}

// ---- the chain
struct Cand {
    uint64_t pos;  // the bit (mode 0: of the header, mode 1: of LEN); kNoStop: the piece has none
    uint32_t mode;
    uint32_t pad;
};
// where a piece ended: at the first block boundary at or behind its stop (for a non-final stored block that follows, at
// its LEN field: mode 1), or with the stream (the final block, an error, the entry's end)
struct PieceEnd {
    uint64_t pos;
    uint32_t mode;
    bool ended;
};
enum class Next {
    Done,      // the stream ended in the piece
    Confirmed, // candidate j starts exactly where the piece ended: its piece is the next of the chain
    Repair,    // no candidate there (those the piece ran over were false): a new piece from the end to `stop`
    Tail,      // ... and the repair rounds are used up: one piece from the end to the end of the stream
};
// c[0 .. n) ascending by pos, without the pieces that have none; j: the first candidate not yet behind the chain (in and out)
BZ_HD inline Next chain_next(const Cand *c, uint64_t n, const PieceEnd &e, uint32_t repairs, uint64_t &j, uint64_t &stop)
{
    if (e.ended) return Next::Done;
    while (j < n && c[j].pos < e.pos) ++j;
    if (j < n && c[j].pos == e.pos) {
        if (c[j].mode == e.mode) return Next::Confirmed;
        ++j; // (a header bit and a LEN field at the same position: not the same start)
    }
    if (repairs >= kRepairRounds) {
        stop = kNoStop;
        return Next::Tail;
    }
    stop = j < n ? c[j].pos : kNoStop;
    return Next::Repair;
}

} // namespace infsplit
