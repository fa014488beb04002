// lzh_split.h -- one large LZHUF stream decoded by many waves (include/bz2_mi355x.h section 9 (g), DESIGN_lzhuf.md section
// 11): the rule that says where a piece of the stream MAY start (a candidate) and the rule that says whether it DOES (the
// chain).  They exist here only: k_lzh_split_search (k_lzhuf.hip) runs the candidate rule with one bit offset per lane, the
// host loop of lzh_split_sizes (lzhuf_engine.hip) runs the chain.
//
// A candidate is a bit position at which a whole block header is valid under every rule of section 9 (d) that k_lzh_decode
// enforces between a block's first bit and its first code, and lies inside the entry:
//   the 16-bit count N is not 0;
//   t-table: a count <= 19, or the constant form with a symbol <= 18; the skip field behind the third length not past the
//            count; no length above 16; Kraft sum exactly 1;
//   c-table, read with that t-code: a count <= 510, or the constant form with a symbol <= 509; no zero run past the count;
//            Kraft sum exactly 1;
//   p-table: a count <= dictionary_bits + 1, or the constant form with a symbol <= dictionary_bits; no length above 16;
//            Kraft sum exactly 1;
//   no field uses a bit behind the entry's end (such a header is BZ_E_EOF for the piece that runs into it).
// These are the decoder's own rules, so every true block start is a candidate; a false one is found at about one bit offset
// in 300 000 of noise (lh5) and is sorted out by the chain.  Nothing here needs an array: the 19 t-lengths are packed into
// two words, the c- and p-sets only leave their Kraft sums.
//
// Plain C++17 without HIP headers (tests/host_stub/lzh_split_check.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifndef BZ_HD
#ifdef __HIPCC__
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif
#endif
#define LZH_FI __attribute__((always_inline)) inline // (a call would cost the search kernel a stack)

namespace lzhsplit {

constexpr uint64_t kNoStop = ~0ull;            // a piece with no candidate behind it
constexpr uint32_t kBaseUnknown = 0xFFFFFFFFu; // a piece that does not know where its output starts
constexpr uint32_t kNoLimit = 0xFFFFFFFFu;     // a piece without a byte limit
constexpr uint32_t kOne = 1u << 16;            // a Kraft sum of exactly 1, in units of 2^-16

// ---- two readers with one interface: take(n) for 1 <= n <= 16, bits MSB first, zeros behind what they hold (the host is
// little-endian, as the device is)
// the entry's bytes from a bit on; `pos` may pass the end, the caller looks at it once
struct MemBits {
    const uint8_t *base;
    uint64_t len;   // bytes
    uint64_t buf;   // the next bits at the top
    uint32_t cnt;   // valid bits in buf
    uint64_t nextw; // the next 32-bit word of the entry to enter buf
    uint64_t pos;   // bits taken, from the entry's first
    BZ_HD MemBits(const uint8_t *b, uint64_t n, uint64_t bit) : base(b), len(n), buf(0), cnt(0), nextw(bit >> 5), pos(bit & ~31ull)
    {
        if (bit & 31u) (void)take((uint32_t)bit & 31u);
    }
    // bytes 4w .. 4w + 3 as the bit stream has them; a word that lies whole inside the entry is one load (a header check is a
    // chain of dependent loads: byte by byte it took four times as long), its last, partial word is read byte by byte
    BZ_HD LZH_FI uint32_t word(uint64_t w) const
    {
        const uint64_t b = 4u * w;
        uint32_t v = 0;
        if (b + 4u <= len) {
            __builtin_memcpy(&v, base + b, 4);
            return __builtin_bswap32(v);
        }
        for (uint32_t k = 0; k < 4u && b + k < len; ++k) v |= (uint32_t)base[b + k] << (24u - 8u * k);
        return v;
    }
    BZ_HD LZH_FI uint32_t take(uint32_t n) // 1 <= n <= 31
    {
        while (cnt <= 32u) {
            buf |= (uint64_t)word(nextw) << (32u - cnt);
            cnt += 32u;
            ++nextw;
        }
        const uint32_t v = (uint32_t)(buf >> (64u - n));
        buf <<= n;
        cnt -= n;
        pos += n;
        return v;
    }
    BZ_HD bool undecided() const { return false; }
};
// 128 bits in two registers (the prefilter); behind them nothing is known
struct RegBits {
    uint64_t a, b;
    uint32_t used;
    BZ_HD RegBits(uint64_t first, uint64_t second) : a(first), b(second), used(0) {}
    BZ_HD LZH_FI uint32_t take(uint32_t n)
    {
        const uint32_t v = (uint32_t)(a >> (64u - n));
        a = a << n | b >> (64u - n);
        b <<= n;
        used += n;
        return v;
    }
    BZ_HD bool undecided() const { return used > 128u; }
};

// the code of the c-table's lengths: 19 lengths of five bits, codes per length 1 .. 16 of five bits (at most 19 each)
struct TCode {
    uint64_t len_lo, len_hi; // symbols 0 .. 11, 12 .. 18
    uint64_t cnt_lo, cnt_hi; // lengths 1 .. 12 at 5 * (l - 1), 13 .. 16 at 5 * (l - 13)
    int constant;            // >= 0: the constant form
    BZ_HD uint32_t len(uint32_t s) const { return (uint32_t)((s < 12 ? len_lo >> (5 * s) : len_hi >> (5 * (s - 12))) & 31u); }
    BZ_HD uint32_t count(uint32_t l) const { return (uint32_t)((l < 13 ? cnt_lo >> (5 * (l - 1)) : cnt_hi >> (5 * (l - 13))) & 31u); }
};

// one code length: 3 bits, 7 extended by a unary run of ones that a zero ends; 17: a length above 16
template <class R> BZ_HD LZH_FI uint32_t read_len(R &r)
{
    uint32_t c = r.take(3);
    if (c == 7u)
        while (r.take(1))
            if (++c > 16u) return 17u;
    return c;
}

// The 16-bit count and the t-table.  false: refused.  true with r.undecided(): the reader ran out, nothing is known.
template <class R> BZ_HD LZH_FI bool t_table_ok(R &r, TCode &t)
{
    if (r.take(16) == 0) return false;
    t.len_lo = t.len_hi = t.cnt_lo = t.cnt_hi = 0;
    t.constant = -1;
    const uint32_t n = r.take(5);
    if (n == 0) {
        const uint32_t s = r.take(5);
        t.constant = (int)s;
        return s <= 18u;
    }
    if (n > 19u) return false;
    uint32_t kraft = 0, i = 0;
    while (i < n) {
        if (i == 3u) {
            i += r.take(2);
            if (r.undecided()) return true;
            if (i > n) return false;
            if (i == n) break;
        }
        const uint32_t l = read_len(r);
        if (l > 16u) return false;
        if (r.undecided()) return true;
        if (l) {
            kraft += kOne >> l;
            if (kraft > kOne) return false;
            if (i < 12u) t.len_lo |= (uint64_t)l << (5 * i);
            else t.len_hi |= (uint64_t)l << (5 * (i - 12u));
            if (l < 13u) t.cnt_lo += 1ull << (5 * (l - 1u));
            else t.cnt_hi += 1ull << (5 * (l - 13u));
        }
        ++i;
    }
    return r.undecided() || kraft == kOne;
}

// one code of a complete t-code: the canonical walk (shorter lengths first, equal lengths by ascending symbol)
template <class R> BZ_HD LZH_FI uint32_t t_symbol(R &r, const TCode &t)
{
    uint32_t code = 0, first = 0;
    for (uint32_t l = 1; l <= 16u; ++l) {
        code = code << 1 | r.take(1);
        const uint32_t c = t.count(l);
        if (code - first < c) {
            uint32_t k = code - first;
            for (uint32_t s = 0; s < 19u; ++s)
                if (t.len(s) == l) {
                    if (k == 0) return s;
                    --k;
                }
        }
        first = (first + c) << 1;
    }
    return 0; // (cannot happen with a complete code)
}

// the register-only prefilter: bits [0, 64) and [64, 128) from the position, MSB first.  false: no candidate here.
BZ_HD LZH_FI bool prefilter(uint64_t first, uint64_t second)
{
    RegBits r(first, second);
    TCode t;
    return t_table_ok(r, t);
}

// A whole block header at `bit` of the entry (base, len): every rule between a block's first bit and its first code.
BZ_HD LZH_FI bool header_ok(const uint8_t *base, uint64_t len, uint64_t bit, uint32_t dbits, uint32_t pbits)
{
    const uint64_t total = 8ull * len;
    if (bit + 16u + 10u + 18u + 2u * pbits > total) return false; // (the shortest header: three constant tables)
    MemBits r(base, len, bit);
    TCode t;
    if (!t_table_ok(r, t)) return false;
    { // the c-table
        const uint32_t n = r.take(9);
        if (n == 0) {
            if (r.take(9) > 509u) return false;
        } else {
            if (n > 510u) return false;
            uint32_t kraft = 0, i = 0;
            while (i < n) {
                const uint32_t k = t.constant >= 0 ? (uint32_t)t.constant : t_symbol(r, t);
                uint32_t run = 1;
                if (k == 1u) run = 3u + r.take(4);
                else if (k == 2u) run = 20u + r.take(9);
                if (i + run > n) return false;
                if (k >= 3u) {
                    kraft += kOne >> (k - 2u);
                    if (kraft > kOne) return false;
                }
                i += run;
                if (r.pos > total) return false;
            }
            if (kraft != kOne) return false;
        }
    }
    { // the p-table
        const uint32_t n = r.take(pbits);
        if (n == 0) {
            if (r.take(pbits) > dbits) return false;
        } else {
            if (n > dbits + 1u) return false;
            uint32_t kraft = 0;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t l = read_len(r);
                if (l > 16u) return false;
                if (l) {
                    kraft += kOne >> l;
                    if (kraft > kOne) return false;
                }
            }
            if (kraft != kOne) return false;
        }
    }
    return r.pos <= total; // a header that needs a bit behind the entry's end is none
}

// ---- the chain
// Piece j starts at candidate c[j] (piece 0 at bit 0) and ends at the first block boundary at or behind the next candidate
// whose header it has read and found valid, or with the stream.  So where a piece stopped at bit e, e IS a candidate: the
// header there is valid and inside the entry.  The walk takes that candidate's piece next; if it is not in the list the rule
// is broken and the entry falls back to one wave.
struct PieceEnd {
    uint64_t pos; // the boundary where the piece stopped
    bool ended;   // the stream ended in the piece: the end (a), an error, the known length
};
enum class Next { Done, Confirmed, Broken };
// c[0 .. n) ascending; j: the first candidate not yet behind the chain (in and out; Confirmed: c[j] starts the next piece)
BZ_HD inline Next chain_next(const uint64_t *c, uint64_t n, const PieceEnd &e, uint64_t &j)
{
    if (e.ended) return Next::Done;
    while (j < n && c[j] < e.pos) ++j;
    return j < n && c[j] == e.pos ? Next::Confirmed : Next::Broken;
}

} // namespace lzhsplit
