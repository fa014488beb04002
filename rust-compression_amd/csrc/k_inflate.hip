// k_inflate.hip -- Deflate / zlib / gzip DECODE of many independent streams (include/bz2_mi355x.h section 5,
// DESIGN_deflate.md "Decoding many streams in one call").  The standard is RFC 1951 / 1950 / 1952, not the reference's
// decoder (src/deflate/decoder.rs), which swallows errors; the container header checks are the reference's
// (src/zlib/decoder.rs:78-90, src/gzip/decoder.rs:92-108, 175-191).
//
// ONE DECODE LOOP, three uses.  inf_decode<USE, WRITE, DICT> is the block loop -- block header, stored block, fixed and dynamic
// tables, codes, copies, the end -- written once; the comment at it lists the places where the uses differ, each settled at
// compile time.  A kernel keeps what is its own: how the reader is positioned and which header is checked, the call, the
// record written.  k_df_inflate: a whole entry per wave; k_df_inflate_piece: a piece of a split entry per wave (inf_split.h);
// k_bgzf_inflate: a BGZF block per wave.  What follows describes the loop by its first use.
//
// k_df_inflate<WRITE, DICT>: one 64-lane workgroup (one wave) per entry, from the entry's first bit to its last.  Everything that
// steers the decode -- bit buffer, positions, the symbol just decoded -- is wave-uniform; the lanes share the work that
// has width: building the tables, staging the input, storing literals, copying matches.
//   <false> sums the output length and writes nothing but the entry's record;
//   <true>  decodes again and writes the bytes at the place the driver gave the entry (never at or behind the length the
//           first launch reported: `limit`).
//
// INPUT.  The bit buffer (64 bits) is refilled in 32-bit words.  A word comes from a 64-word stage the lanes load together
// (lane l holds word cbase + l; the word wanted is read with readlane).  Words that lie whole inside the entry are loaded
// as words (d_in is 16-byte aligned, every offset a multiple of 4); the entry's last, partial word is put together from
// byte loads, so no byte behind in_off + in_len is ever touched; every word behind that is zero.  The bits consumed are
// 32 * nextw - cnt; having consumed more than 8 * in_len bits is the BZ_E_EOF condition, looked at behind every code and
// header field before its result is used (so a failure that padding bits caused is an EOF, never a data error).
//
// TABLES (LDS, 4.6 KiB per workgroup; no per-thread arrays): a first-level table indexed by the next 10 (literal/length),
// 9 (distance) or 7 (code-length code) bits, entry = symbol << 4 | length, 0 = "not here"; behind a miss the canonical walk
// over the per-length counts and the symbols sorted by (length, symbol) (codes of up to 15 bits).  Built by the wave:
// counts with LDS atomics, first codes and offsets in a serial sweep over the 15 lengths held in lanes 1..15, ranks by one
// ballot per length and 64 symbols, fill in parallel.
//
// LITERALS wait in a register (lane k holds the k-th pending byte) and leave with one store instruction per 64 bytes or
// when a match or a stored block needs the position settled.
//
// MATCHES are copied by the whole wave: byte i of the copy is out[p - d + (i mod d)] -- for d >= length that is the plain
// out[p + i - d], for shorter distances the period of d bytes replicated -- so EVERY source byte lies in front of p and was
// stored before this code was decoded; no lane reads what another lane stores in the same copy, whatever d and the length
// are.  What it may read is a byte that another lane of this wave stored an instruction earlier (a literal flush, the
// previous copy).  Those stores and these loads are ordered by a fence at workgroup scope (__threadfence_block()): the
// workgroup is one wave on one CU, its stores and loads go through that CU's one L1 in program order, and workgroup scope
// is exactly the scope at which that L1 is coherent.  The fence is skipped when the source ends at or in front of the
// position up to which an earlier fence has already ordered the stores (`fenced`).
//
// A PRESET DICTIONARY (<.., DICT = true>; clause (c) of section 5; DESIGN_deflate.md "Decoding with a preset dictionary"): the
// last W <= 32768 bytes of it (`dictw`, global memory: read-only and shared by every wave of the launch, it lives in L2) are
// history in front of position 0 of the entry's output.  A distance d at position p is valid iff d <= p + W; source byte
// q = p - d + (i mod d) < 0 is dictw[W + q] -- a signed index per lane; out + (p - d) is never formed for p < d.  Nobody writes
// the window, so a read from it needs no fence: `fenced` concerns q >= 0 only.  The zlib header then wants FDICT and, as
// DICTID, the Adler-32 of the whole dictionary (`dict_adler`).  The DICT = false instantiations never look at the three
// trailing parameters.
#include <hip/hip_runtime.h>

#include "../../include/bz2_mi355x.h"
#include "bzgpu.h"
#include "k_deflate.h"
#include "k_df_fold.h"
#include "inf_split.h"
#include "bgzf_index.h"

namespace dfgpu {
using namespace bzgpu;

namespace {
constexpr u32 kLBits = 10, kDBits = 9, kCBits = 7;

__constant__ u8 c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// a length / distance code's base value and extra bits in ONE word (base | bits << 16): one load per code, so the value
// never waits for a second load behind the first
#define X(base, bits) ((base) | (bits) << 16)
__constant__ u32 c_len_code[29] = {X(3, 0), X(4, 0), X(5, 0), X(6, 0), X(7, 0), X(8, 0), X(9, 0), X(10, 0), X(11, 1), X(13, 1), X(15, 1), X(17, 1), X(19, 2), X(23, 2), X(27, 2), X(31, 2), X(35, 3), X(43, 3), X(51, 3), X(59, 3), X(67, 4), X(83, 4), X(99, 4), X(115, 4), X(131, 5), X(163, 5), X(195, 5), X(227, 5), X(258, 0)};
__constant__ u32 c_dist_code[30] = {X(1, 0), X(2, 0), X(3, 0), X(4, 0), X(5, 1), X(7, 1), X(9, 2), X(13, 2), X(17, 3), X(25, 3), X(33, 4), X(49, 4), X(65, 5), X(97, 5), X(129, 6), X(193, 6), X(257, 7), X(385, 7), X(513, 8), X(769, 8), X(1025, 9), X(1537, 9), X(2049, 10), X(3073, 10), X(4097, 11), X(6145, 11), X(8193, 12), X(12289, 12), X(16385, 13), X(24577, 13)};
#undef X

__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

struct InfIn {
    const u8 *base; // the entry's first byte (a multiple of 4 from a 16-byte-aligned pointer)
    u32 len;        // its bytes
    u64 buf;        // the next bits, bit 0 first; bits at and above cnt are zero
    u32 cnt;        // valid bits in buf
    u32 nextw;      // the next word to enter buf
    u32 cw;         // PER LANE: word cbase + lane of the entry
    u32 cbase;
};

__device__ __forceinline__ u32 inf_word(InfIn &r, u32 w, u32 lane)
{
    if (w - r.cbase >= 64u) { // (wave-uniform)
        r.cbase = w;
        const u64 byte = 4ull * ((u64)w + lane);
        u32 v = 0;
        if (byte + 4 <= r.len) v = *reinterpret_cast<const u32 *>(r.base + byte);
        else
            for (u32 k = 0; k < 4 && byte + k < r.len; ++k) v |= (u32)r.base[byte + k] << (8 * k);
        r.cw = v;
    }
    return (u32)__builtin_amdgcn_readlane((int)r.cw, (int)uni(w - r.cbase));
}
// at least 33 valid bits behind this (zeros behind the entry's end)
__device__ __forceinline__ void inf_fill(InfIn &r, u32 lane)
{
    while (r.cnt <= 32u) {
        r.buf |= (u64)inf_word(r, r.nextw, lane) << r.cnt;
        r.cnt += 32u;
        ++r.nextw;
    }
}
__device__ __forceinline__ u32 inf_take(InfIn &r, u32 n) // n <= 32 <= cnt
{
    const u32 v = (u32)(r.buf & ((1ull << n) - 1ull));
    r.buf >>= n;
    r.cnt -= n;
    return v;
}
__device__ __forceinline__ u64 inf_consumed(const InfIn &r) { return 32ull * r.nextw - r.cnt; }
__device__ __forceinline__ void inf_seek(InfIn &r, u32 bytepos, u32 lane)
{
    r.nextw = bytepos >> 2;
    r.buf = 0;
    r.cnt = 0;
    inf_fill(r, lane);
    (void)inf_take(r, 8u * (bytepos & 3u));
}

// One code: the symbol, or -1 when the next bits are no code of the set (an incomplete set's unused code).
__device__ __forceinline__ int inf_sym(InfIn &r, const u16 *tab, u32 tbits, const u32 *cnt, const u16 *syms)
{
    const u32 e = uni(tab[(u32)r.buf & ((1u << tbits) - 1u)]);
    if (e & 15u) {
        (void)inf_take(r, e & 15u);
        return (int)(e >> 4);
    }
    u32 code = 0, first = 0, index = 0;
    for (u32 l = 1; l <= 15u; ++l) {
        code |= (u32)(r.buf >> (l - 1)) & 1u;
        const u32 c = uni(cnt[l]);
        if (code < first + c) {
            (void)inf_take(r, l);
            return (int)uni(syms[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

// The decode tables of one code-length set: lens[0 .. n) in LDS -> tab (1 << tbits entries), cnt[16], syms.
// Returns 0, 1 (over-subscribed) or 2 (incomplete); nsyms = codes in use, maxlen = the longest.
__device__ __forceinline__ int inf_build(const u8 *lens, u32 n, u16 *tab, u32 tbits, u32 *cnt, u16 *syms, u32 lane, u32 &nsyms, u32 &maxlen)
{
    if (lane < 16u) cnt[lane] = 0;
    for (u32 i = lane; i < (1u << tbits); i += 64u) tab[i] = 0;
    __syncthreads();
    for (u32 i = lane; i < n; i += 64u) {
        const u32 l = lens[i];
        if (l) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    const u32 myc = (lane >= 1u && lane < 16u) ? cnt[lane] : 0u; // lane l: codes of length l
    u32 myoff = 0, myadj = 0; // lane l: where its symbols start in syms; first code of length l minus that
    int left = 1;
    u32 o = 0, code = 0, prev = 0;
    maxlen = 0;
    for (u32 l = 1; l <= 15u; ++l) {
        const u32 c = (u32)__builtin_amdgcn_readlane((int)myc, (int)l);
        left = (left << 1) - (int)c;
        if (left < 0) return 1;
        code = (code + prev) << 1;
        if (lane == l) {
            myoff = o;
            myadj = code - o;
        }
        o += c;
        prev = c;
        if (c) maxlen = l;
    }
    nsyms = o;
    for (u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        const u32 l = i < n ? lens[i] : 0u;
        u32 rank = 0, cd = 0;
        for (u32 ll = 1; ll <= maxlen; ++ll) {
            const u64 m = __ballot(l == ll);
            if (m == 0) continue;
            const u32 o2 = (u32)__builtin_amdgcn_readlane((int)myoff, (int)ll);
            const u32 adj = (u32)__builtin_amdgcn_readlane((int)myadj, (int)ll);
            if (l == ll) {
                rank = o2 + (u32)__popcll(m & ((1ull << lane) - 1ull));
                cd = rank + adj;
            }
            if (lane == ll) myoff += (u32)__popcll(m);
        }
        if (l) {
            syms[rank] = (u16)i;
            if (l <= tbits) {
                const u16 e = (u16)((i << 4) | l);
                for (u32 j = __brev(cd) >> (32u - l); j < (1u << tbits); j += 1u << l) tab[j] = e;
            }
        }
    }
    __syncthreads();
    return left > 0 ? 2 : 0;
}
// the tables of one wave (LDS)
struct InfTabs {
    u16 tl[1u << kLBits], td[1u << kDBits], tc[1u << kCBits];
    u16 sl[288], sd[32], sc[32];
    u32 nl[16], nd[16], nc[16];
    u8 cl[320], clen[32];
};
// what a decode leaves behind
struct InfOut {
    u64 end_bit;
    u32 p, nblk0, nblk1, nblk2, check, isize, flags;
    int verdict;
    u32 reach, end_mode, ended; // of a piece (k_df_inflate_piece)
};
// what only a piece has (kPiece below; the other uses pass InfPiece{})
struct InfPiece {
    u32 *smap;   // the source map of the piece's bytes (WRITE)
    u32 base;    // where the piece's output starts inside the entry's, or infsplit::kBaseUnknown
    u64 stop;    // the piece ends at the first block boundary at or behind this bit
    bool at_len; // the reader stands at the LEN field of a stored block
};

__device__ __forceinline__ InfIn inf_open(const u8 *base, u32 len)
{
    InfIn r;
    r.base = base;
    r.len = len;
    r.buf = 0;
    r.cnt = 0;
    r.nextw = 0;
    r.cw = 0;
    r.cbase = 0xFFFFFF00u;
    return r;
}

// The container header in front of the Deflate bits, zlib (kind 1) or gzip (kind 2): BZ_OK, BZ_E_EOF when it runs behind the
// input, else BZ_E_DATA.  Every field is looked at behind the test for the end, so what is wrong with it is a data error.
template <bool DICT>
__device__ __forceinline__ int inf_header(InfIn &r, const u32 lane, const int kind, const u32 dict_adler)
{
    const u64 total = 8ull * r.len;
#define INF_HEOF()                                                                    \
    do {                                                                              \
        if (inf_consumed(r) > total) return BZ_E_EOF;                                 \
    } while (0)
    if (kind == 1) {
        inf_fill(r, lane);
        const u32 cmf = inf_take(r, 8), flg = inf_take(r, 8);
        INF_HEOF();
        if (DICT) { // zlib/decoder.rs:62-101: FDICT first, then the six bytes, then what they hold
            if (!(flg & 0x20u)) return BZ_E_DATA;
            inf_fill(r, lane);
            const u32 v = inf_take(r, 32);
            INF_HEOF();
            const u32 id = (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
            if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || id != dict_adler) return BZ_E_DATA;
        } else if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return BZ_E_DATA;
    } else if (kind == 2) {
        u32 hc = 0xFFFFFFFFu, flg = 0, xlen = 0;
#define INF_HBYTE(v)                                                                  \
    do {                                                                              \
        inf_fill(r, lane);                                                            \
        (v) = inf_take(r, 8);                                                         \
        INF_HEOF();                                                                   \
        hc ^= (v);                                                                    \
        for (int k_ = 0; k_ < 8; ++k_) hc = (hc & 1u) ? (hc >> 1) ^ 0xEDB88320u : hc >> 1; \
    } while (0)
#pragma unroll 1
        for (u32 k = 0; k < 10; ++k) {
            u32 b;
            INF_HBYTE(b);
            if ((k == 0 && b != 0x1Fu) || (k == 1 && b != 0x8Bu) || (k == 2 && b != 8u) || (k == 3 && (b & 0xE0u))) return BZ_E_DATA;
            if (k == 3) flg = b;
        }
        if (flg & 4u) {
            u32 b0, b1;
            INF_HBYTE(b0);
            INF_HBYTE(b1);
            xlen = b0 | (b1 << 8);
            for (u32 k = 0; k < xlen; ++k) INF_HBYTE(b0);
        }
        for (u32 f = 8u; f <= 16u; f <<= 1) // FNAME, FCOMMENT: up to the zero byte
            if (flg & f) {
                u32 b;
                do INF_HBYTE(b);
                while (b != 0);
            }
        if (flg & 2u) {
            const u32 want = (hc ^ 0xFFFFFFFFu) & 0xFFFFu;
            inf_fill(r, lane);
            const u32 got = inf_take(r, 16);
            INF_HEOF();
            if (got != want) return BZ_E_DATA;
        }
#undef INF_HBYTE
    }
#undef INF_HEOF
    return BZ_OK;
}

// THE decode loop: the blocks of one Deflate stream from where the reader stands -- block header, stored block, fixed and
// dynamic tables, codes, copies -- and what ends it.  Written once and instantiated per use; the uses differ in the places
// below and nowhere else, each resolved at compile time (`if constexpr`), so no instantiation carries another's test:
//   kEntry (k_df_inflate): a whole entry.  Stores are clipped to `limit` while p runs on (the 4 GiB guard sets flags bit 0); a
//     fault is BZ_E_EOF when the bits looked at reach behind the input, else BZ_E_DATA; a distance may reach p bytes back, with
//     DICT p + W, and a source in front of position 0 is a window byte; the end is the container trailer by `kind`.
//   kPiece (k_df_inflate_piece, inf_split.h): a piece of a split entry, kEntry but for this: the reader may stand at a stored
//     block's LEN (pc.at_len); at every block boundary the piece ends if the block behind it starts at or behind pc.stop
//     (end_key, end_mode, ended; a non-final stored block is named by its LEN position); `pc.base` is where the piece's output
//     starts inside the entry's (infsplit::kBaseUnknown: not known yet, a distance that reaches in front of the piece is
//     recorded in `reach` and believed), else base + p (+ W) bounds a distance; with WRITE every byte i gets smap[i]: i itself
//     when out[i] holds its value, else the position inside the entry's output (in front of the piece) that does -- no byte is
//     written then.  DICT: a source in front of the ENTRY is a window byte: it is stored at once and is its own root, the
//     source map never points into the window.
//   kBgzf (k_bgzf_inflate): the Deflate bytes of one BGZF block, kind 0, always written.  Every fault is BZ_E_DATA, running out of
//     bits included (the cut is BSIZE's, not the file's: bits behind the Deflate bytes are zeros to the reader, having used one
//     is the block's fault); so is a byte too many, p > limit, looked at with the end test and behind a stored block and a
//     match; a distance may reach p bytes back; a clean block produces exactly `limit` bytes and uses every bit.
// `verdict` is what the use's own entrance found: anything but BZ_OK and nothing is decoded.  The reader and the piece's
// data come by value and the result leaves by value: everything that steers the loop is a local of this function.
enum InfUse { kEntry, kPiece, kBgzf };

template <InfUse USE, bool WRITE, bool DICT>
__device__ __forceinline__ InfOut inf_decode(InfTabs &t, InfIn r, const u32 lane, int verdict, const int kind, u8 *out, const u32 limit,
                                             const InfPiece pc, const u8 *__restrict__ dictw, const u32 W)
{
    static_assert(USE != kBgzf || (WRITE && !DICT), "a BGZF block is written in its one pass and has no dictionary");
    const u64 total = 8ull * r.len;
    const u32 base = pc.base;
    u32 p = 0;       // bytes produced, pending literals included
    u32 npend = 0;   // literals waiting in `lit`
    u32 lit = 0;     // PER LANE: pending literal number `lane`
    u32 fenced = 0;  // stores below this position are ordered before every later load
    u32 nblk0 = 0, nblk1 = 0, nblk2 = 0, check = 0, isize = 0, flags = 0;
    u32 reach = 0, end_mode = 0, ended = 1;
    u64 end_key = 0;
    bool at_len = pc.at_len;
    bool fixed_ready = false;
    u32 maxl = 0, maxd = 0;

#define INF_FLUSH()                                                                   \
    do {                                                                              \
        if (WRITE && npend) {                                                         \
            const u32 q_ = p - npend + lane;                                          \
            if (lane < npend && q_ < limit) {                                         \
                out[q_] = (u8)lit;                                                    \
                if constexpr (USE == kPiece) pc.smap[q_] = base + q_;                 \
            }                                                                         \
        }                                                                             \
        npend = 0;                                                                    \
    } while (0)
// a failure: BZ_E_EOF if the bits looked at (those consumed and `extra` more) reach behind the input, else BZ_E_DATA
#define INF_FAIL(extra)                                                               \
    do {                                                                              \
        verdict = USE != kBgzf && (inf_consumed(r) + (extra)) > total ? BZ_E_EOF : BZ_E_DATA; \
        goto done;                                                                    \
    } while (0)
#define INF_EOF_CHECK()                                                               \
    do {                                                                              \
        if (inf_consumed(r) > total || (USE == kBgzf && p > limit)) {                 \
            verdict = USE == kBgzf ? BZ_E_DATA : BZ_E_EOF;                            \
            goto done;                                                                \
        }                                                                             \
    } while (0)

    if (verdict != BZ_OK) goto done;
    for (;;) {
        u32 bfinal = 0, btype = 0;
        const bool from_len = USE == kPiece && at_len; // (the header bits of that stored block lie in front of the piece)
        at_len = false;
        if (!from_len) {
            inf_fill(r, lane);
            if constexpr (USE == kPiece) {
                // a boundary: the block behind it is the next piece's if it starts at or behind `stop`
                const u64 h = inf_consumed(r);
                const bool st0 = h + 3 <= total && ((u32)r.buf & 7u) == 0u; // a non-final stored block: known by its LEN
                const u64 key = st0 ? (h + 10) & ~7ull : h;
                if (key >= pc.stop) {
                    end_key = key;
                    end_mode = st0 ? 1u : 0u;
                    ended = 0;
                    goto done;
                }
            }
            bfinal = inf_take(r, 1);
            btype = inf_take(r, 2);
            INF_EOF_CHECK();
            if (btype == 3u) INF_FAIL(0);
        }
        if (btype == 0u) {
            if (!from_len) (void)inf_take(r, r.cnt & 7u);
            inf_fill(r, lane);
            const u32 ln = inf_take(r, 16), nl = inf_take(r, 16);
            INF_EOF_CHECK();
            if ((ln ^ nl) != 0xFFFFu) INF_FAIL(0);
            const u32 bytepos = (u32)(inf_consumed(r) >> 3);
            if ((u64)bytepos + ln > r.len) {
                verdict = USE == kBgzf ? BZ_E_DATA : BZ_E_EOF;
                goto done;
            }
            if (USE != kBgzf && p > 0xFFFFFFFFu - 0x10000u) {
                flags |= 1u;
                INF_FAIL(0);
            }
            INF_FLUSH();
            if (WRITE)
                for (u32 i = lane; i < ln; i += 64u)
                    if (p + i < limit) {
                        out[p + i] = r.base[bytepos + i];
                        if constexpr (USE == kPiece) pc.smap[p + i] = base + p + i;
                    }
            p += ln;
            if (USE == kBgzf && p > limit) INF_FAIL(0);
            inf_seek(r, bytepos + ln, lane);
            ++nblk0;
        } else {
            if (btype == 1u) {
                if (!fixed_ready) {
                    __syncthreads();
                    for (u32 i = lane; i < 320u; i += 64u) t.cl[i] = (u8)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
                    __syncthreads();
                    u32 ns;
                    (void)inf_build(t.cl, 288, t.tl, kLBits, t.nl, t.sl, lane, ns, maxl);
                    (void)inf_build(t.cl + 288, 32, t.td, kDBits, t.nd, t.sd, lane, ns, maxd);
                    fixed_ready = true;
                }
            } else {
                fixed_ready = false;
                const u32 hlit = inf_take(r, 5) + 257u, hdist = inf_take(r, 5) + 1u, hclen = inf_take(r, 4) + 4u;
                INF_EOF_CHECK();
                if (hlit > 286u || hdist > 30u) INF_FAIL(0);
                __syncthreads();
                if (lane < 19u) t.clen[lane] = 0;
                __syncthreads();
                for (u32 k = 0; k < hclen; ++k) {
                    inf_fill(r, lane);
                    const u32 v = inf_take(r, 3);
                    if (lane == 0) t.clen[c_cl_order[k]] = (u8)v;
                }
                INF_EOF_CHECK();
                __syncthreads();
                u32 ns, maxc;
                if (inf_build(t.clen, 19, t.tc, kCBits, t.nc, t.sc, lane, ns, maxc) != 0) INF_FAIL(0);
                const u32 ncl = hlit + hdist;
                u32 i = 0, prev = 0;
                while (i < ncl) {
                    inf_fill(r, lane);
                    const int sy = inf_sym(r, t.tc, kCBits, t.nc, t.sc);
                    if (sy < 0) INF_FAIL(maxc);
                    if (sy < 16) {
                        INF_EOF_CHECK();
                        if (lane == 0) t.cl[i] = (u8)sy;
                        prev = (u32)sy;
                        ++i;
                        continue;
                    }
                    u32 rep, val = 0;
                    if (sy == 16) {
                        rep = 3u + inf_take(r, 2);
                        val = prev;
                    } else if (sy == 17) rep = 3u + inf_take(r, 3);
                    else rep = 11u + inf_take(r, 7);
                    INF_EOF_CHECK();
                    if ((sy == 16 && i == 0) || i + rep > ncl) INF_FAIL(0);
                    for (u32 q = lane; q < rep; q += 64u) t.cl[i + q] = (u8)val;
                    prev = val;
                    i += rep;
                }
                __syncthreads();
                if (t.cl[256] == 0) INF_FAIL(0); // no end-of-block code
                // (one sequence of hlit + hdist lengths: a run may cross from one alphabet into the other)
                const int rl = inf_build(t.cl, hlit, t.tl, kLBits, t.nl, t.sl, lane, ns, maxl);
                if (rl != 0) INF_FAIL(0);
                const int rd = inf_build(t.cl + hlit, hdist, t.td, kDBits, t.nd, t.sd, lane, ns, maxd);
                if (rd == 1 || (rd == 2 && !(ns == 0u || (ns == 1u && maxd == 1u)))) INF_FAIL(0);
            }
            // ---- the codes of the block
            for (;;) {
                inf_fill(r, lane);
                const int sy = inf_sym(r, t.tl, kLBits, t.nl, t.sl);
                if (sy < 0) INF_FAIL(maxl);
                if (sy < 256) {
                    if constexpr (USE != kBgzf) INF_EOF_CHECK();
                    if (lane == npend) lit = (u32)sy;
                    ++npend;
                    ++p;
                    if constexpr (USE == kBgzf) INF_EOF_CHECK(); // (behind ++p: the byte too many is counted in len)
                    if (npend == 64u) INF_FLUSH();
                    continue;
                }
                if (sy == 256) {
                    INF_EOF_CHECK();
                    break;
                }
                if (sy > 285) INF_FAIL(0);
                const u32 lc = c_len_code[sy - 257];
                const u32 len = (lc & 0xFFFFu) + inf_take(r, lc >> 16);
                inf_fill(r, lane);
                const int ds = inf_sym(r, t.td, kDBits, t.nd, t.sd);
                if (ds < 0) INF_FAIL(maxd);
                if (ds > 29) INF_FAIL(0);
                const u32 dc = c_dist_code[ds];
                const u32 d = (dc & 0xFFFFu) + inf_take(r, dc >> 16);
                INF_EOF_CHECK();
                if constexpr (USE == kPiece) {
                    if (d > p) { // in front of the piece: inside the entry's output if the piece knows where it lies
                        if (base != infsplit::kBaseUnknown && (u64)d > (u64)base + p + (DICT ? W : 0u)) INF_FAIL(0);
                        if (d - p > reach) reach = d - p;
                    }
                } else if (DICT ? d > p && d - p > W : d > p) INF_FAIL(0); // in front of the first byte (of the window)
                if (USE != kBgzf && p > 0xFFFFFFFFu - 0x10000u) {
                    flags |= 1u;
                    INF_FAIL(0);
                }
                INF_FLUSH();
                if (WRITE) {
                    // The last source byte is p - d + span - 1, which may lie in front of position 0 (nobody writes there: it
                    // needs no fence): p - d + span > fenced, with fenced <= p and no term below zero.
                    const u32 span = d < len ? d : len;
                    if (p - fenced + span > d) {
                        __threadfence_block();
                        fenced = p;
                    }
                    if constexpr (USE == kPiece) {
                        for (u32 b = 0; b < len; b += 64u) {
                            const u32 i = b + lane;
                            if (i < len && p + i < limit) {
                                const long long q = (long long)p - d + (d >= len ? i : i % d);
                                if (DICT && (long long)base + q < 0) { // in front of the entry: a window byte, its own root
                                    out[p + i] = dictw[(long long)W + base + q];
                                    pc.smap[p + i] = base + p + i;
                                } else if (q < 0) pc.smap[p + i] = (u32)((long long)base + q); // (no byte: the gather brings it)
                                else {
                                    const u32 sv = pc.smap[q];
                                    out[p + i] = out[q];
                                    pc.smap[p + i] = sv == base + (u32)q ? base + p + i : sv;
                                }
                            }
                        }
                    } else if constexpr (DICT) { // source byte q < 0 is window byte W + q; out + (p - d) is never formed for p < d
                        const long long q0 = (long long)p - d;
                        for (u32 b = 0; b < len; b += 64u) {
                            const u32 i = b + lane;
                            if (i < len && p + i < limit) {
                                const long long q = q0 + (d >= len ? i : i % d);
                                out[p + i] = q < 0 ? dictw[(long long)W + q] : out[q];
                            }
                        }
                    } else {
                        const u8 *src = out + (p - d);
                        for (u32 b = 0; b < len; b += 64u) {
                            const u32 i = b + lane;
                            if (i < len && p + i < limit) out[p + i] = src[d >= len ? i : i % d];
                        }
                    }
                }
                p += len;
                if (USE == kBgzf && p > limit) INF_FAIL(0);
            }
            if (btype == 1u) ++nblk1;
            else ++nblk2;
        }
        if (bfinal) break;
    }
    // ---- the end
    (void)inf_take(r, r.cnt & 7u);
    if constexpr (USE == kBgzf) { // exactly `limit` bytes, and the stream ends in the last byte of the input
        if (p != limit || inf_consumed(r) != total) verdict = BZ_E_DATA;
    } else if (kind == 1) {
        inf_fill(r, lane);
        const u32 v = inf_take(r, 32);
        INF_EOF_CHECK();
        check = (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
    } else if (kind == 2) {
        inf_fill(r, lane);
        check = inf_take(r, 32);
        inf_fill(r, lane);
        isize = inf_take(r, 32);
        INF_EOF_CHECK();
    }
done:
    INF_FLUSH();
    InfOut o;
    o.end_bit = !ended ? end_key : inf_consumed(r) < total ? inf_consumed(r) : total;
    o.p = p;
    o.verdict = verdict;
    o.nblk0 = nblk0;
    o.nblk1 = nblk1;
    o.nblk2 = nblk2;
    o.check = check;
    o.isize = isize;
    o.flags = flags;
    o.reach = reach;
    o.end_mode = end_mode;
    o.ended = ended;
    return o;
#undef INF_FLUSH
#undef INF_FAIL
#undef INF_EOF_CHECK
}

__device__ __forceinline__ DfInfRec inf_record(const InfOut &o)
{
    DfInfRec q;
    q.end_bit = o.end_bit;
    q.len = o.p;
    q.verdict = o.verdict;
    q.nblk[0] = o.nblk0;
    q.nblk[1] = o.nblk1;
    q.nblk[2] = o.nblk2;
    q.check = o.check;
    q.isize = o.isize;
    q.flags = o.flags;
    q.pad[0] = q.pad[1] = 0;
    return q;
}
} // namespace

// One wave per entry: the container header, then the decode loop from the entry's first block to its trailer.
template <bool WRITE, bool DICT>
__global__ __launch_bounds__(64) void k_df_inflate(const u8 *__restrict__ in, const u64 *__restrict__ in_off, const u64 *__restrict__ in_len,
                                                   int kind, u8 *out_all, const u64 *__restrict__ out_off, DfInfRec *rec,
                                                   const u8 *__restrict__ dictw, u32 W, u32 dict_adler)
{
    __shared__ InfTabs t;
    const u32 lane = threadIdx.x, j = blockIdx.x;
    InfIn r = inf_open(in + in_off[j], (u32)in_len[j]);
    const int head = inf_header<DICT>(r, lane, kind, dict_adler);
    const InfOut o = inf_decode<kEntry, WRITE, DICT>(t, r, lane, head, kind, WRITE ? out_all + out_off[j] : nullptr, WRITE ? rec[j].len : 0u,
                                                     InfPiece{}, dictw, W);
    if (!WRITE && lane == 0) rec[j] = inf_record(o);
}

// ---- one large entry across many waves (inf_split.h; DESIGN_deflate.md "One large stream across many waves")
// The first candidate of every piece but the first: 64 bit offsets per step, one per lane.
__global__ __launch_bounds__(64) void k_df_split_search(const u8 *__restrict__ ebase, u32 elen, u32 piece_bytes, infsplit::Cand *cand)
{
    const u32 lane = threadIdx.x, k = blockIdx.x + 1;
    const infsplit::BitSrc src{ebase, elen};
    const u64 lo = 8ull * k * piece_bytes, total = 8ull * elen;
    const u64 hi = lo + 8ull * piece_bytes < total ? lo + 8ull * piece_bytes : total;
    infsplit::Cand c;
    c.pos = infsplit::kNoStop;
    c.mode = 0;
    c.pad = 0;
    for (u64 o = lo; o < hi; o += 64u) {
        const u64 bit = o + lane;
        u32 w[5]; // (unrolled: registers) the words that hold bits [bit, bit + 128)
#pragma unroll
        for (u32 q = 0; q < 5; ++q) {
            const u64 byte = 4ull * ((bit >> 5) + q);
            u32 v = 0;
            if (byte + 4 <= elen) v = *reinterpret_cast<const u32 *>(ebase + byte);
            else
                for (u32 b = 0; b < 4 && byte + b < elen; ++b) v |= (u32)ebase[byte + b] << (8 * b);
            w[q] = v;
        }
        const u32 sh = (u32)bit & 31u;
        const u64 a0 = (u64)w[0] | (u64)w[1] << 32, a1 = (u64)w[2] | (u64)w[3] << 32;
        const u64 blo = sh ? a0 >> sh | a1 << (64u - sh) : a0;
        const u64 bhi = sh ? a1 >> sh | (u64)w[4] << (64u - sh) : a1;
        u32 found = 0;
        if (bit < hi) {
            if (infsplit::dyn_prefilter(blo, bhi) && infsplit::dyn_header_ok(src, bit, false)) found = 1;
            else if ((bit & 7u) == 0 && (((u32)blo ^ (u32)(blo >> 16)) & 0xFFFFu) == 0xFFFFu && infsplit::stored_ok(src, bit)) found = 2;
        }
        const u64 m = __ballot(found != 0);
        if (m) {
            const u32 first = (u32)__ffsll((long long)m) - 1u;
            c.pos = o + first;
            c.mode = (u32)__builtin_amdgcn_readlane((int)found, (int)first) - 1u;
            break;
        }
    }
    if (lane == 0) cand[blockIdx.x] = c;
}

// One wave per piece.  <false>: what the piece is (DfPieceRec); <true>: its bytes and their source map, below pc.len.
template <bool WRITE, bool DICT>
__global__ __launch_bounds__(64) void k_df_inflate_piece(const u8 *__restrict__ ebase, u32 elen, int kind, const DfPiece *__restrict__ pc,
                                                         DfPieceRec *rec, u8 *eout, u32 *emap, const u8 *__restrict__ dictw, u32 W,
                                                         u32 dict_adler)
{
    __shared__ InfTabs t;
    const u32 lane = threadIdx.x, j = blockIdx.x;
    const DfPiece q = pc[j];
    InfIn r = inf_open(ebase, elen);
    const bool head = (q.mode & 2u) != 0, at_len = (q.mode & 1u) != 0;
    if (at_len) inf_seek(r, (u32)(q.start >> 3), lane);
    else if (!head) {
        r.nextw = (u32)(q.start >> 5);
        inf_fill(r, lane);
        (void)inf_take(r, (u32)q.start & 31u);
    }
    const int hv = head ? inf_header<DICT>(r, lane, kind, dict_adler) : BZ_OK; // (the entry's first piece)
    const InfOut o = inf_decode<kPiece, WRITE, DICT>(t, r, lane, hv, kind, WRITE ? eout + q.base : nullptr, WRITE ? q.len : 0u,
                                                     InfPiece{WRITE ? emap + q.base : nullptr, q.base, q.stop, at_len}, dictw, W);
    if (!WRITE && lane == 0) {
        DfPieceRec x;
        x.r = inf_record(o);
        x.reach = o.reach;
        x.end_mode = o.end_mode;
        x.ended = o.ended;
        x.pad = 0;
        rec[j] = x;
    }
}

// src[i] = src[src[i]] over the bytes whose value lies elsewhere; cnt[0] += such bytes, cnt[1] += pointers moved.  A racing
// read sees an older or a newer ancestor: both are valid, pointers only move toward the root.
__global__ __launch_bounds__(256) void k_df_split_jump(u32 *src, u32 n, u32 *cnt)
{
    __shared__ u32 s_n[2];
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
    __syncthreads();
    u32 un = 0, ch = 0;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
        const u32 s = __hip_atomic_load(&src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (s < i) {
            ++un;
            const u32 a = __hip_atomic_load(&src[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (a < s) {
                __hip_atomic_store(&src[i], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ++ch;
            }
        }
    }
    if (un) atomicAdd(&s_n[0], un);
    if (ch) atomicAdd(&s_n[1], ch);
    __syncthreads();
    if (threadIdx.x < 2 && s_n[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], s_n[threadIdx.x]);
}

// out[i] = out[src[i]]: every src[i] is a root by now, a byte that the writing launch stored and nothing overwrites
__global__ __launch_bounds__(256) void k_df_split_gather(u8 *out, const u32 *__restrict__ src, u32 n)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
        const u32 s = src[i];
        if (s < i) out[i] = out[s];
    }
}

// The container checksums of the decoded bytes, a workgroup per entry: thread t folds the t-th slice of the entry (a
// multiple of 16 bytes), the slices are combined as k_df_batch_wrap combines its pieces (k_df_fold.h).  A mismatch with the
// trailer -- Adler-32 (kind 1), CRC-32 or ISIZE (kind 2) -- turns the entry's verdict to BZ_E_DATA.
__global__ __launch_bounds__(256) void k_df_inflate_check(const u8 *__restrict__ out_all, const u64 *__restrict__ out_off, DfInfRec *rec, int kind)
{
    __shared__ u32 s_tab[256];
    __shared__ u64 s_a[256], s_b[256];
    __shared__ u32 s_c[256];
    const u32 tid = threadIdx.x, j = blockIdx.x;
    if (rec[j].verdict != BZ_OK) return;
    const u32 len = rec[j].len;
    {
        u32 c = tid;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        s_tab[tid] = c;
    }
    __syncthreads();
    const u8 *src = out_all + out_off[j]; // (a multiple of 16)
    const u64 slice = ((((u64)len + 255u) >> 8) + 15u) & ~15ull;
    const u64 lo = (u64)tid * slice < len ? (u64)tid * slice : len;
    const u64 hi = lo + slice < len ? lo + slice : len;
    u64 a = 0, b = 0;
    u32 c = 0;
    u64 i = lo;
    for (; i + 16 <= hi; i += 16) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t *>(src + i);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 k = 0; k < 16; ++k) df_fold_byte((w[k >> 2] >> (8 * (k & 3u))) & 0xFFu, hi - (i + k), s_tab, a, b, c);
    }
    for (; i < hi; ++i) df_fold_byte(src[i], hi - i, s_tab, a, b, c);
    const u64 after = len - hi;
    s_a[tid] = a % 65521u;
    s_b[tid] = (b % 65521u + (a % 65521u) * (after % 65521u)) % 65521u;
    s_c[tid] = df_gf_mul(c, df_gf_xpow8((u32)after));
    __syncthreads();
    if (tid != 0) return;
    u64 sa = 0, sb = 0;
    u32 raw = 0;
    for (u32 t = 0; t < 256; ++t) {
        sa += s_a[t];
        sb += s_b[t];
        raw ^= s_c[t];
    }
    bool ok;
    if (kind == 1) {
        const u32 A = (u32)((1 + sa) % 65521u), B = (u32)((len + sb) % 65521u); // adler32.rs:20-66 from (1, 0)
        ok = ((B << 16) | A) == rec[j].check;
    } else ok = df_crc_finish(raw, len) == rec[j].check && rec[j].isize == len;
    if (!ok) rec[j].verdict = BZ_E_DATA;
}

// ---- reading BGZF (include/bz2_mi355x.h section 8; DESIGN_deflate.md "Reading BGZF")
// One wave per block of the index, ONE pass: the block's length comes from BSIZE and its output's length from ISIZE, both
// checked against the index here, so the bytes go straight to their place.  The decode loop is inf_decode's kBgzf form (its
// rules are listed there); this kernel's own part is the entrance: the lanes check the header rule (bgzf_index.h) at the
// block's coff, which may have any byte phase (the reader starts at the 4-aligned byte in front of it, 18 + phase bytes in:
// inf_seek, and the loop's `total` counts from there to the byte in front of the trailer); `limit` is ISIZE; the output may
// start at any byte.  A distance that reaches in front of the block's first byte is a fault although the block in front lies
// right there.  An edge block (slot != 0) is decoded into its 64 KiB slot of the workspace instead.
__global__ __launch_bounds__(64) void k_bgzf_inflate(const u8 *__restrict__ in, const BgzfDesc *__restrict__ desc, u8 *out_all, u8 *slots,
                                                     BgzfRec *rec)
{
    __shared__ InfTabs t;
    const u32 lane = threadIdx.x, j = blockIdx.x;
    const BgzfDesc q = desc[j];
    u8 *const out = q.slot ? slots + (size_t)(q.slot - 1u) * bgzf::kMaxBlock : out_all + q.dst;
    const u32 phase = (u32)q.coff & 3u;
    InfIn r = inf_open(in + (q.coff - phase), phase + q.csize - bgzf::kTrailer);
    u32 check = 0;
    bool head_ok = false;
    if (q.csize >= bgzf::kMinBlock && q.csize <= bgzf::kMaxBlock) { // lanes 0 .. 17: the header's bytes, 18 .. 25: the trailer's
        u32 hb = 0;
        if (lane < bgzf::kHeader) hb = in[q.coff + lane];
        else if (lane < bgzf::kHeader + bgzf::kTrailer) hb = in[q.coff + q.csize - (bgzf::kHeader + bgzf::kTrailer) + lane];
#define BG_B(l) ((u32)__builtin_amdgcn_readlane((int)hb, (l)))
#define BG_W(l) (BG_B(l) | BG_B((l) + 1) << 8 | BG_B((l) + 2) << 16 | BG_B((l) + 3) << 24)
        const u32 bsize1 = (BG_B(16) | BG_B(17) << 8) + 1u, isize = BG_W(22);
        check = BG_W(18);
        head_ok = bgzf::header_words(BG_W(0), BG_W(8), BG_W(12)) && bsize1 == q.csize && isize == q.usize;
#undef BG_B
#undef BG_W
    }
    if (head_ok) inf_seek(r, phase + bgzf::kHeader, lane);
    const InfOut o = inf_decode<kBgzf, true, false>(t, r, lane, head_ok ? BZ_OK : BZ_E_DATA, 0, out, q.usize, InfPiece{}, nullptr, 0u);
    if (lane == 0) {
        BgzfRec x;
        x.verdict = o.verdict;
        x.len = o.p;
        x.check = check;
        x.nblk[0] = o.nblk0;
        x.nblk[1] = o.nblk1;
        x.nblk[2] = o.nblk2;
        x.pad[0] = x.pad[1] = 0;
        rec[j] = x;
    }
}

// The CRC-32 of every clean block's bytes against its trailer, a workgroup per block: k_df_inflate_check's fold for an
// output that starts at ANY byte -- thread 0 takes the bytes in front of the first multiple of 16 with its slice, every
// slice behind starts at a multiple of 16 and is read in 16-byte loads.  A mismatch turns the verdict to BZ_E_DATA.
__global__ __launch_bounds__(256) void k_bgzf_check(const BgzfDesc *__restrict__ desc, const u8 *__restrict__ out_all, const u8 *__restrict__ slots,
                                                    BgzfRec *rec)
{
    __shared__ u32 s_tab[256];
    __shared__ u32 s_c[256];
    const u32 tid = threadIdx.x, j = blockIdx.x;
    if (rec[j].verdict != BZ_OK) return;
    const BgzfDesc q = desc[j];
    const u32 len = q.usize;
    {
        u32 c = tid;
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        s_tab[tid] = c;
    }
    __syncthreads();
    const u8 *src = q.slot ? slots + (size_t)(q.slot - 1u) * bgzf::kMaxBlock : out_all + q.dst;
    const u32 head = (16u - (u32)((uintptr_t)src & 15u)) & 15u;
    const u32 slice = (((len + 255u) >> 8) + 15u) & ~15u;
    const u32 lo = tid == 0 ? 0u : (head + tid * slice < len ? head + tid * slice : len);
    const u32 hi = head + (tid + 1u) * slice < len ? head + (tid + 1u) * slice : len;
    u64 a = 0, b = 0; // (the Adler sums of df_fold_byte: not used)
    u32 c = 0;
    u32 i = lo;
    for (; i < hi && ((uintptr_t)(src + i) & 15u); ++i) df_fold_byte(src[i], 0, s_tab, a, b, c);
    for (; i + 16 <= hi; i += 16) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t *>(src + i);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (u32 k = 0; k < 16; ++k) df_fold_byte((w[k >> 2] >> (8 * (k & 3u))) & 0xFFu, 0, s_tab, a, b, c);
    }
    for (; i < hi; ++i) df_fold_byte(src[i], 0, s_tab, a, b, c);
    s_c[tid] = df_gf_mul(c, df_gf_xpow8(len - hi));
    __syncthreads();
    if (tid != 0) return;
    u32 raw = 0;
    for (u32 t = 0; t < 256; ++t) raw ^= s_c[t];
    if (df_crc_finish(raw, len) != rec[j].check) rec[j].verdict = BZ_E_DATA;
}

int df_launch_bgzf_inflate(hipStream_t st, const u8 *in, const BgzfDesc *desc, u32 count, u8 *out, u8 *slots, BgzfRec *rec)
{
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(count), dim3(64), 0, st, in, desc, out, slots, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_bgzf_check(hipStream_t st, const BgzfDesc *desc, u32 count, const u8 *out, const u8 *slots, BgzfRec *rec)
{
    hipLaunchKernelGGL(k_bgzf_check, dim3(count), dim3(256), 0, st, desc, out, slots, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_inflate(hipStream_t st, bool write, const u8 *in, const u64 *in_off, const u64 *in_len, u32 count, int kind, u8 *out,
                      const u64 *out_off, DfInfRec *rec, DfWindow win)
{
#define INF_LAUNCH(WR, DI)                                                                                                          \
    hipLaunchKernelGGL((k_df_inflate<WR, DI>), dim3(count), dim3(64), 0, st, in, in_off, in_len, kind, out, out_off, rec, win.p, win.W, \
                       win.adler)
    if (win.W) {
        if (write) INF_LAUNCH(true, true);
        else INF_LAUNCH(false, true);
    } else if (write) INF_LAUNCH(true, false);
    else INF_LAUNCH(false, false);
#undef INF_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_inflate_check(hipStream_t st, const u8 *out, const u64 *out_off, u32 count, DfInfRec *rec, int kind)
{
    hipLaunchKernelGGL(k_df_inflate_check, dim3(count), dim3(256), 0, st, out, out_off, rec, kind);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// cand: npieces - 1 infsplit::Cand, of pieces 1 .. npieces - 1
int df_launch_split_search(hipStream_t st, const u8 *ebase, u32 elen, u32 piece_bytes, u32 npieces, void *cand)
{
    if (npieces < 2) return 0;
    hipLaunchKernelGGL(k_df_split_search, dim3(npieces - 1), dim3(64), 0, st, ebase, elen, piece_bytes, static_cast<infsplit::Cand *>(cand));
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_inflate_piece(hipStream_t st, bool write, const u8 *ebase, u32 elen, int kind, const DfPiece *pc, u32 count, DfPieceRec *rec,
                            u8 *eout, u32 *emap, DfWindow win)
{
#define INF_LAUNCH(WR, DI)                                                                                                          \
    hipLaunchKernelGGL((k_df_inflate_piece<WR, DI>), dim3(count), dim3(64), 0, st, ebase, elen, kind, pc, rec, eout, emap, win.p, win.W, \
                       win.adler)
    if (win.W) {
        if (write) INF_LAUNCH(true, true);
        else INF_LAUNCH(false, true);
    } else if (write) INF_LAUNCH(true, false);
    else INF_LAUNCH(false, false);
#undef INF_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

static u32 df_split_grid(u32 n) { return n / 1024u + 1u < 8192u ? n / 1024u + 1u : 8192u; }

int df_launch_split_jump(hipStream_t st, u32 *src, u32 n, u32 *cnt)
{
    hipLaunchKernelGGL(k_df_split_jump, dim3(df_split_grid(n)), dim3(256), 0, st, src, n, cnt);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_split_gather(hipStream_t st, u8 *out, const u32 *src, u32 n)
{
    hipLaunchKernelGGL(k_df_split_gather, dim3(df_split_grid(n)), dim3(256), 0, st, out, src, n);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace dfgpu
