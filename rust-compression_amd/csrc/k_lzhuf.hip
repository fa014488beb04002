// k_lzhuf.hip -- LZHUF (-lh4- .. -lh7-) DECODE of many independent streams (include/bz2_mi355x.h section 9, DESIGN_lzhuf.md).
// The stream format is the reference's (src/lzhuf/decoder.rs, encoder.rs); the contract of section 9 decides what its
// decoder leaves open: the end, a known original length, EOF against data errors, the table rules, the bytes in front of
// position 0.
//
// k_lzh_decode<WRITE>: one 64-lane workgroup (one wave) per entry, the shape of k_df_inflate (k_inflate.hip).  Everything
// that steers the decode -- bit buffer, positions, the symbol just decoded -- is wave-uniform; the lanes share the work that
// has width: building the tables, staging the input, storing literals, copying matches.
//   <false> sums the output length and writes nothing but the entry's record;
//   <true>  decodes again and writes the bytes at the place the driver gave the entry, never at or behind the length the
//           first launch reported (`limit`).
// The loop itself is lzh_decode<USE, WRITE>, once: kEntry is the above; kPiece is k_lzh_decode_piece<WRITE>, one wave per
// PIECE of one large entry (DESIGN_lzhuf.md section 11; the rules: lzh_split.h), whose starts k_lzh_split_search finds.
//
// INPUT.  Bits are read MSB first: the bit buffer (64 bits) holds the next bits at its TOP, and is refilled in 32-bit words
// whose bytes are swapped on the way in.  A word comes from a 64-word stage the lanes load together (lane l holds word
// cbase + l; the word wanted is read with readlane).  Words that lie whole inside the entry are loaded as words (d_in is
// 16-byte aligned, every offset a multiple of 4); the entry's last, partial word is put together from byte loads, so no byte
// behind in_off + in_len is ever touched; every word behind that is zero.  The bits consumed are 32 * nextw - cnt; having
// consumed more than 8 * in_len bits is the BZ_E_EOF condition, looked at behind every code and header field BEFORE its
// value is judged (so a failure that padding bits caused is an EOF, never a data error).
//
// TABLES (LDS, 5.1 KiB per workgroup; no per-thread arrays).  Codes are canonical and written MSB first, so the first l bits
// of the buffer ARE a code of length l as a number: a first-level table indexed by the next 10 (c) or 8 (t, p) bits, entry
// = symbol << 5 | length, 0 = "not here", where a code of length l fills the 1 << (bits - l) consecutive entries behind
// code << (bits - l); behind a miss the canonical walk over the per-length counts and the symbols sorted by (length,
// symbol).  A set must be complete (Kraft sum exactly 1), so the walk always ends at a symbol.  Built by the wave as
// inf_build does: counts with LDS atomics, first codes and offsets in a serial sweep over the 16 lengths held in lanes
// 1..16, ranks by one ballot per length and 64 symbols, fill in parallel.  A table in its constant form is a register.
//
// LITERALS wait in a register (lane k holds the k-th pending byte) and leave with one store instruction per 64 bytes or
// when a match needs the position settled.
//
// MATCHES are copied by the whole wave: byte i of the copy is out[p - d + (i mod d)], so every source byte lies in front of
// p and was stored before this code was decoded; no lane reads what another lane stores in the same copy.  A source index
// below zero (prefill >= 0 only) is the prefill byte: a signed index per lane, out + (p - d) is never formed.  What a copy may
// read is a byte that another lane of this wave stored an instruction earlier; those stores and these loads are ordered by
// a fence at workgroup scope, skipped when the source ends at or in front of the position an earlier fence has covered
// (`fenced`) -- the discipline of k_inflate.hip, where it is argued.
#include <hip/hip_runtime.h>

#include "../../include/bz2_mi355x.h"
#include "bzgpu.h"
#include "k_lzhuf.h"
#include "lzh_split.h"

namespace lzhgpu {
using namespace bzgpu;

namespace {
constexpr u32 kCBits = 10, kSBits = 8;
constexpr u32 kMaxLen = 16;

__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

struct LzhIn {
    const u8 *base; // the entry's first byte (a multiple of 4 from a 16-byte-aligned pointer)
    u32 len;        // its bytes
    u64 buf;        // the next bits, bit 63 first; bits below 64 - cnt are zero
    u32 cnt;        // valid bits in buf
    u32 nextw;      // the next word to enter buf
    u32 cw;         // PER LANE: word cbase + lane of the entry, bytes swapped
    u32 cbase;
};

__device__ __forceinline__ u32 lzh_word(LzhIn &r, u32 w, u32 lane)
{
    if (w - r.cbase >= 64u) { // (wave-uniform)
        r.cbase = w;
        const u64 byte = 4ull * ((u64)w + lane);
        u32 v = 0;
        if (byte + 4 <= r.len) v = *reinterpret_cast<const u32 *>(r.base + byte);
        else
            for (u32 k = 0; k < 4 && byte + k < r.len; ++k) v |= (u32)r.base[byte + k] << (8 * k);
        r.cw = __builtin_bswap32(v);
    }
    return (u32)__builtin_amdgcn_readlane((int)r.cw, (int)uni(w - r.cbase));
}
// at least 33 valid bits behind this (zeros behind the entry's end)
__device__ __forceinline__ void lzh_fill(LzhIn &r, u32 lane)
{
    while (r.cnt <= 32u) {
        r.buf |= (u64)lzh_word(r, r.nextw, lane) << (32u - r.cnt);
        r.cnt += 32u;
        ++r.nextw;
    }
}
__device__ __forceinline__ u32 lzh_take(LzhIn &r, u32 n) // n <= 32 <= cnt; n == 0 gives 0
{
    const u32 v = (u32)((r.buf >> 32) >> (32u - n));
    r.buf <<= n;
    r.cnt -= n;
    return v;
}
__device__ __forceinline__ u64 lzh_consumed(const LzhIn &r) { return 32ull * r.nextw - r.cnt; }

// One code of a complete set: the symbol (-1 cannot happen behind lzh_build's Kraft test; it is kept as a failure).
__device__ __forceinline__ int lzh_sym(LzhIn &r, const u16 *tab, u32 tbits, const u32 *cnt, const u16 *syms)
{
    const u32 e = uni(tab[(u32)(r.buf >> (64u - tbits))]);
    if (e & 31u) {
        (void)lzh_take(r, e & 31u);
        return (int)(e >> 5);
    }
    u32 first = 0, index = 0;
    for (u32 l = 1; l <= kMaxLen; ++l) {
        const u32 code = (u32)(r.buf >> (64u - l));
        const u32 c = uni(cnt[l]);
        if (code - first < c) {
            (void)lzh_take(r, l);
            return (int)uni(syms[index + (code - first)]);
        }
        index += c;
        first = (first + c) << 1;
    }
    return -1;
}

// The decode tables of one code-length set: lens[0 .. n) in LDS, every one <= 16 -> tab (1 << tbits entries), cnt[17], syms.
// Returns 0, or 1 when the Kraft sum is not exactly 1.
__device__ __forceinline__ int lzh_build(const u8 *lens, u32 n, u16 *tab, u32 tbits, u32 *cnt, u16 *syms, u32 lane)
{
    if (lane <= kMaxLen) cnt[lane] = 0;
    for (u32 i = lane; i < (1u << tbits); i += 64u) tab[i] = 0;
    __syncthreads();
    for (u32 i = lane; i < n; i += 64u) {
        const u32 l = lens[i];
        if (l) atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    const u32 myc = (lane >= 1u && lane <= kMaxLen) ? cnt[lane] : 0u; // lane l: codes of length l
    u32 myoff = 0, myadj = 0; // lane l: where its symbols start in syms; first code of length l minus that
    int left = 1;
    u32 o = 0, code = 0, prev = 0, maxlen = 0;
    for (u32 l = 1; l <= kMaxLen; ++l) {
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
    if (left != 0) return 1;
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
                const u16 e = (u16)((i << 5) | l);
                const u32 lo = cd << (tbits - l), hi = (cd + 1u) << (tbits - l);
                for (u32 q = lo; q < hi; ++q) tab[q] = e;
            }
        }
    }
    __syncthreads();
    return 0;
}

// the tables of one wave (LDS)
struct LzhTabs {
    u16 tc[1u << kCBits], tp[1u << kSBits], tt[1u << kSBits];
    u16 sc[512], sp[32], st[32];
    u32 nc[20], np[20], nt[20];
    u8 cl[512], pl[32], tl[32];
};

// The decode loop, once.  kEntry: a whole entry from its first bit (k_lzh_decode).  kPiece: a piece of a split entry
// (k_lzh_decode_piece; lzh_split.h), which differs only where `if constexpr (USE == kPiece)` says so: it starts at any bit; at
// a block boundary at or behind `stop` whose header it has read and found valid it stops (so where a piece stops there is a
// candidate); a distance that reaches in front of the piece is believed while `base` is unknown and held against base + p
// once it is known, its excess d - p recorded in `reach`; with WRITE every byte i gets smap[i]: base + i itself when the
// byte is stored, else the position in the entry's output, in front of the piece, that holds its value.  A source in front
// of the ENTRY (prefill >= 0) is the constant: stored at once, its own root.
enum LzhUse { kEntry, kPiece };
struct LzhPieceArg {
    u32 *smap; // the source map of the piece's bytes (WRITE)
    u32 base;  // where the piece's output starts in the entry's (lzhsplit::kBaseUnknown: not known)
    u64 stop;  // the next candidate
};
// r: open at the first bit to decode; L: the byte limit (has_len: reaching the end (a) in front of it is BZ_E_EOF); out, limit:
// where the bytes go and how many of them (WRITE); rec (and prec, kPiece): what a sizes launch leaves
template <LzhUse USE, bool WRITE>
__device__ __forceinline__ void lzh_decode(const u8 *const ebase, const u32 elen, const u64 start, const u32 lane, const u32 L, const bool has_len,
                                             const u32 dbits, const u32 pbits, const int prefill, u8 *const out, const u32 limit,
                                           const LzhPieceArg pc, LzhRec *const rec, LzhPieceRec *const prec)
{
    __shared__ LzhTabs t;
    LzhIn r;
    r.base = ebase;
    r.len = elen;
    r.buf = 0;
    r.cnt = 0;
    r.nextw = 0;
    r.cw = 0;
    r.cbase = 0xFFFFFF00u;
    const u64 total = 8ull * r.len;
    if constexpr (USE == kPiece) { // any bit of the entry
        r.nextw = (u32)(start >> 5);
        lzh_fill(r, lane);
        (void)lzh_take(r, (u32)start & 31u);
    }
    const u32 window = 1u << dbits;
    [[maybe_unused]] const u32 base = pc.base;

    u32 p = 0;      // bytes produced, pending literals included
    u32 npend = 0;  // literals waiting in `lit`
    u32 lit = 0;    // PER LANE: pending literal number `lane`
    u32 fenced = 0; // stores below this position are ordered before every later load
    u32 nblk = 0, nlit = 0, nmatch = 0, flags = 0;
    [[maybe_unused]] u32 reach = 0;
    [[maybe_unused]] bool stopped = false;
    [[maybe_unused]] u64 boundary = 0;
    int verdict = BZ_OK;

#define LZH_FLUSH()                                                                   \
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
#define LZH_EOF_CHECK()                                                               \
    do {                                                                              \
        if (lzh_consumed(r) > total) {                                                \
            verdict = BZ_E_EOF;                                                       \
            goto done;                                                                \
        }                                                                             \
    } while (0)
// behind LZH_EOF_CHECK: every bit looked at lies inside the entry
#define LZH_DATA()                                                                    \
    do {                                                                              \
        verdict = BZ_E_DATA;                                                          \
        goto done;                                                                    \
    } while (0)
// one code length: 3 bits, 7 extended by a unary run of ones that a zero ends (at most 3 + 11 bits before it fails)
#define LZH_LEN(dst)                                                                  \
    do {                                                                              \
        u32 c_ = lzh_take(r, 3);                                                      \
        LZH_EOF_CHECK();                                                              \
        if (c_ == 7u)                                                                 \
            for (;;) {                                                                \
                const u32 b_ = lzh_take(r, 1);                                        \
                LZH_EOF_CHECK();                                                      \
                if (!b_) break;                                                       \
                if (++c_ > kMaxLen) LZH_DATA();                                       \
            }                                                                         \
        (dst) = c_;                                                                   \
    } while (0)

    for (;;) {
        if (p >= L) break; // (b): the known length is there
        lzh_fill(r, lane);
        if (total - lzh_consumed(r) < 16u) break; // (a): no room for a block length
        if constexpr (USE == kPiece) boundary = lzh_consumed(r);
        const u32 ncodes = lzh_take(r, 16);
        if (ncodes == 0) break; // (a)
        int tconst = -1, cconst = -1, pconst = -1;
        { // ---- the t-table: the code of the c-table's lengths
            const u32 n = lzh_take(r, 5);
            LZH_EOF_CHECK();
            if (n == 0) {
                const u32 s = lzh_take(r, 5);
                LZH_EOF_CHECK();
                if (s > 18u) LZH_DATA();
                tconst = (int)s;
            } else {
                if (n > 19u) LZH_DATA();
                __syncthreads();
                if (lane < 32u) t.tl[lane] = 0;
                __syncthreads();
                u32 i = 0;
                while (i < n) {
                    lzh_fill(r, lane);
                    if (i == 3u) {
                        i += lzh_take(r, 2);
                        LZH_EOF_CHECK();
                        if (i > n) LZH_DATA();
                        if (i == n) break;
                    }
                    u32 c;
                    LZH_LEN(c);
                    if (lane == 0) t.tl[i] = (u8)c;
                    ++i;
                }
                __syncthreads();
                if (lzh_build(t.tl, n, t.tt, kSBits, t.nt, t.st, lane) != 0) LZH_DATA();
            }
        }
        { // ---- the c-table: literals and lengths
            lzh_fill(r, lane);
            const u32 n = lzh_take(r, 9);
            LZH_EOF_CHECK();
            if (n == 0) {
                const u32 s = lzh_take(r, 9);
                LZH_EOF_CHECK();
                if (s > 509u) LZH_DATA();
                cconst = (int)s;
            } else {
                if (n > 510u) LZH_DATA();
                __syncthreads();
                for (u32 i = lane; i < 512u; i += 64u) t.cl[i] = 0;
                __syncthreads();
                u32 i = 0;
                while (i < n) {
                    lzh_fill(r, lane);
                    const int k = tconst >= 0 ? tconst : lzh_sym(r, t.tt, kSBits, t.nt, t.st);
                    if (k < 0) {
                        LZH_EOF_CHECK();
                        LZH_DATA();
                    }
                    u32 run = 1;
                    if (k == 1) run = 3u + lzh_take(r, 4);
                    else if (k == 2) run = 20u + lzh_take(r, 9);
                    LZH_EOF_CHECK();
                    if (i + run > n) LZH_DATA();
                    if (k >= 3 && lane == 0) t.cl[i] = (u8)(k - 2);
                    i += run;
                }
                __syncthreads();
                if (lzh_build(t.cl, n, t.tc, kCBits, t.nc, t.sc, lane) != 0) LZH_DATA();
            }
        }
        { // ---- the p-table: the distances' bit counts
            lzh_fill(r, lane);
            const u32 n = lzh_take(r, pbits);
            LZH_EOF_CHECK();
            if (n == 0) {
                const u32 s = lzh_take(r, pbits);
                LZH_EOF_CHECK();
                if (s > dbits) LZH_DATA();
                pconst = (int)s;
            } else {
                if (n > dbits + 1u) LZH_DATA();
                __syncthreads();
                if (lane < 32u) t.pl[lane] = 0;
                __syncthreads();
                for (u32 i = 0; i < n; ++i) {
                    lzh_fill(r, lane);
                    u32 c;
                    LZH_LEN(c);
                    if (lane == 0) t.pl[i] = (u8)c;
                }
                __syncthreads();
                if (lzh_build(t.pl, n, t.tp, kSBits, t.np, t.sp, lane) != 0) LZH_DATA();
            }
        }
        if constexpr (USE == kPiece) {
            if (boundary >= pc.stop) { // a valid header at or behind the next candidate: that candidate's piece goes on from here
                stopped = true;
                goto done;
            }
        }
        // ---- the codes of the block
        for (u32 k = 0; k < ncodes; ++k) {
            if (p >= L) goto done; // (b)
            if (USE == kPiece && base != lzhsplit::kBaseUnknown ? (u64)base + p > 0xFFFFFFFFu - 0x200u : p > 0xFFFFFFFFu - 0x200u) {
                flags |= 1u;
                LZH_DATA();
            }
            lzh_fill(r, lane);
            const int sy = cconst >= 0 ? cconst : lzh_sym(r, t.tc, kCBits, t.nc, t.sc);
            if (sy < 0) {
                LZH_EOF_CHECK();
                LZH_DATA();
            }
            if (sy < 256) {
                LZH_EOF_CHECK();
                if (lane == npend) lit = (u32)sy;
                ++npend;
                ++p;
                ++nlit;
                if (npend == 64u) LZH_FLUSH();
                continue;
            }
            u32 len = (u32)sy - 253u;
            lzh_fill(r, lane);
            const int v = pconst >= 0 ? pconst : lzh_sym(r, t.tp, kSBits, t.np, t.sp);
            if (v < 0) {
                LZH_EOF_CHECK();
                LZH_DATA();
            }
            const u32 pos = v > 1 ? (1u << (v - 1)) | lzh_take(r, (u32)v - 1u) : (u32)v;
            LZH_EOF_CHECK();
            const u32 d = pos + 1u;
            if constexpr (USE == kPiece) {
                if (d > window) LZH_DATA();
                if (d > p) { // in front of the piece: inside the entry's output if the piece knows where it lies
                    if (prefill < 0 && base != lzhsplit::kBaseUnknown && (u64)d > (u64)base + p) LZH_DATA();
                    if (d - p > reach) reach = d - p;
                }
            } else if (d > window || (prefill < 0 && d > p)) LZH_DATA();
            if (len > L - p) len = L - p; // (b): cut at the known length
            LZH_FLUSH();
            if (WRITE) {
                // the last source byte is p - d + span - 1; it needs a fence iff it lies at or behind `fenced` (no term below
                // zero: fenced <= p); a source in front of position 0 is the prefill byte, which nobody stores
                const u32 span = d < len ? d : len;
                if (p - fenced + span > d) {
                    __threadfence_block();
                    fenced = p;
                }
                const long long q0 = (long long)p - d;
                for (u32 b = 0; b < len; b += 64u) {
                    const u32 i = b + lane;
                    if (i < len && p + i < limit) {
                        const long long q = q0 + (d >= len ? i : i % d);
                        if constexpr (USE == kPiece) {
                            if ((long long)base + q < 0) { // in front of the entry: the constant, its own root
                                out[p + i] = (u8)prefill;
                                pc.smap[p + i] = base + p + i;
                            } else if (q < 0) pc.smap[p + i] = (u32)((long long)base + q); // (no byte: the gather brings it)
                            else {
                                const u32 sv = pc.smap[q];
                                out[p + i] = out[q];
                                pc.smap[p + i] = sv == base + (u32)q ? base + p + i : sv;
                            }
                        } else out[p + i] = q < 0 ? (u8)prefill : out[q];
                    }
                }
            }
            p += len;
            ++nmatch;
        }
        ++nblk;
    }
    if (has_len && p < L) verdict = BZ_E_EOF; // the end (a) in front of the known length
done:
    LZH_FLUSH();
    if (!WRITE && lane == 0) {
        LzhRec q;
        q.end_bit = lzh_consumed(r) < total ? lzh_consumed(r) : total;
        if constexpr (USE == kPiece) {
            if (stopped) q.end_bit = boundary;
        }
        q.len = p;
        q.verdict = verdict;
        q.nblk = nblk;
        q.nlit = nlit;
        q.nmatch = nmatch;
        q.flags = flags;
        *rec = q;
        if constexpr (USE == kPiece) {
            prec->reach = reach;
            prec->ended = stopped ? 0u : 1u;
            prec->pad[0] = prec->pad[1] = 0;
        }
    }
#undef LZH_FLUSH
#undef LZH_EOF_CHECK
#undef LZH_DATA
#undef LZH_LEN
}
} // namespace

template <bool WRITE>
__global__ __launch_bounds__(64) void k_lzh_decode(const u8 *__restrict__ in, const u64 *__restrict__ in_off, const u64 *__restrict__ in_len,
                                                   const u64 *__restrict__ orig_len, u32 dbits, u32 pbits, int prefill, u8 *out_all,
                                                   const u64 *__restrict__ out_off, LzhRec *rec)
{
    const u32 lane = threadIdx.x, j = blockIdx.x;
    const u8 *const ebase = in + in_off[j];
    const u32 elen = (u32)in_len[j];
    const u64 ol = orig_len ? orig_len[j] : kNoLen;
    const bool has_len = ol != kNoLen;
    const u32 L = ol > 0xFFFFFFFEull ? 0xFFFFFFFFu : (u32)ol; // (a length the 4 GiB guard comes in front of is as good as none)
    lzh_decode<kEntry, WRITE>(ebase, elen, 0, lane, L, has_len, dbits, pbits, prefill, WRITE ? out_all + out_off[j] : nullptr,
                              WRITE ? rec[j].len : 0u, LzhPieceArg{nullptr, 0, 0}, rec + j, nullptr);
}

// One wave per piece.  <false>: what the piece is (LzhPieceRec); <true>: its bytes and their source map, below pc.limit.
template <bool WRITE>
__global__ __launch_bounds__(64) void k_lzh_decode_piece(const u8 *__restrict__ ebase, u32 elen, u32 dbits, u32 pbits, int prefill,
                                                         const LzhPiece *__restrict__ pcs, LzhPieceRec *rec, u8 *eout, u32 *emap)
{
    const u32 lane = threadIdx.x, j = blockIdx.x;
    const LzhPiece q = pcs[j];
    // the writing launch knows its base: eout + base and emap + base are the piece's own ranges
    lzh_decode<kPiece, WRITE>(ebase, elen, q.start, lane, q.limit, !WRITE && q.has_len != 0, dbits, pbits, prefill, WRITE ? eout + q.base : nullptr,
                              WRITE ? q.limit : 0u, LzhPieceArg{WRITE ? emap + q.base : nullptr, q.base, q.stop}, WRITE ? nullptr : &rec[j].r,
                              WRITE ? nullptr : rec + j);
}

// ---- the candidates of one entry (lzh_split.h), all of them, ascending.  A wave looks at kSearchBits bit offsets, 64 per
// step, one per lane.  FILL false: cnt[wave] = its candidates; FILL true: it writes them behind first[wave], in order (the
// host has summed the counts in between: no atomic decides an order).
constexpr u32 kSearchBits = 1024;
template <bool FILL>
__global__ __launch_bounds__(64) void k_lzh_split_search(const u8 *__restrict__ ebase, u32 elen, u32 dbits, u32 pbits, u32 *cnt,
                                                         const u32 *__restrict__ first, u64 *cand, u32 ncand)
{
    const u32 lane = threadIdx.x;
    const u64 total = 8ull * elen, lo = (u64)blockIdx.x * kSearchBits;
    const u64 hi = lo + kSearchBits < total ? lo + kSearchBits : total;
    if (FILL && cnt[blockIdx.x] == 0) return; // (the count pass found nothing in this wave's bits)
    u32 n = 0;
    const u32 at = FILL ? first[blockIdx.x] : 0u;
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
            w[q] = __builtin_bswap32(v);
        }
        const u32 sh = (u32)bit & 31u;
        const u64 a0 = (u64)w[0] << 32 | w[1], a1 = (u64)w[2] << 32 | w[3], a2 = (u64)w[4] << 32;
        const u64 b0 = sh ? a0 << sh | a1 >> (64u - sh) : a0;
        const u64 b1 = sh ? a1 << sh | a2 >> (64u - sh) : a1;
        const bool found = bit < hi && lzhsplit::prefilter(b0, b1) && lzhsplit::header_ok(ebase, elen, bit, dbits, pbits);
        const u64 m = __ballot(found);
        if (FILL && found) {
            const u32 at_ = at + n + (u32)__popcll(m & ((1ull << lane) - 1ull));
            if (at_ < ncand) cand[at_] = bit; // (the counts were taken from the same bytes: always)
        }
        n += (u32)__popcll(m);
    }
    if (!FILL && lane == 0) cnt[blockIdx.x] = n;
}

int lzh_launch_decode(hipStream_t st, bool write, const u8 *in, const u64 *in_off, const u64 *in_len, const u64 *orig_len, u32 count,
                      u32 dbits, u32 pbits, int prefill, u8 *out, const u64 *out_off, LzhRec *rec)
{
    if (write)
        hipLaunchKernelGGL((k_lzh_decode<true>), dim3(count), dim3(64), 0, st, in, in_off, in_len, orig_len, dbits, pbits, prefill, out, out_off, rec);
    else
        hipLaunchKernelGGL((k_lzh_decode<false>), dim3(count), dim3(64), 0, st, in, in_off, in_len, orig_len, dbits, pbits, prefill, out, out_off, rec);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lzh_launch_decode_piece(hipStream_t st, bool write, const u8 *ebase, u32 elen, u32 dbits, u32 pbits, int prefill, const LzhPiece *pcs,
                            u32 count, LzhPieceRec *rec, u8 *eout, u32 *emap)
{
    if (write)
        hipLaunchKernelGGL((k_lzh_decode_piece<true>), dim3(count), dim3(64), 0, st, ebase, elen, dbits, pbits, prefill, pcs, rec, eout, emap);
    else
        hipLaunchKernelGGL((k_lzh_decode_piece<false>), dim3(count), dim3(64), 0, st, ebase, elen, dbits, pbits, prefill, pcs, rec, eout, emap);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

u32 lzh_split_search_waves(u32 elen) { return (u32)((8ull * elen + kSearchBits - 1) / kSearchBits); }
int lzh_launch_split_search(hipStream_t st, bool fill, const u8 *ebase, u32 elen, u32 dbits, u32 pbits, u32 *cnt, const u32 *first, u64 *cand,
                            u32 ncand)
{
    const u32 waves = lzh_split_search_waves(elen);
    if (fill) hipLaunchKernelGGL((k_lzh_split_search<true>), dim3(waves), dim3(64), 0, st, ebase, elen, dbits, pbits, cnt, first, cand, ncand);
    else hipLaunchKernelGGL((k_lzh_split_search<false>), dim3(waves), dim3(64), 0, st, ebase, elen, dbits, pbits, cnt, first, cand, ncand);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace lzhgpu
