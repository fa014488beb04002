// k_lzhuf.h -- what the LZHUF decode kernels (k_lzhuf.hip) and their driver (lzhuf_engine.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "bzgpu.h"

namespace lzhgpu {
using namespace bzgpu;

// what a launch leaves per entry (the sizes launch writes it, the writing launch reads len as its store limit)
struct LzhRec {
    u64 end_bit;  // bits consumed, at most 8 * in_len
    u32 len;      // bytes produced
    int verdict;  // BZ_OK, BZ_E_DATA, BZ_E_EOF
    u32 nblk;     // blocks decoded whole
    u32 nlit;     // literal codes
    u32 nmatch;   // match codes
    u32 flags;    // bit 0: the output would reach 4 GiB
};
static_assert(sizeof(LzhRec) == 32, "LzhRec is copied between host and device as it is");

constexpr u64 kNoLen = ~0ull; // orig_len: not known

// dbits: dictionary_bits, pbits: offset_bits of the method; orig_len: nullptr or one u64 per entry
int lzh_launch_decode(hipStream_t st, bool write, const u8 *in, const u64 *in_off, const u64 *in_len, const u64 *orig_len, u32 count,
                      u32 dbits, u32 pbits, int prefill, u8 *out, const u64 *out_off, LzhRec *rec);

// ---- one large entry across many waves (lzh_split.h): a piece runs from a bit of the entry to the first block boundary at
// or behind `stop` that holds a valid header, or to the stream's end
struct LzhPiece {
    u64 start;   // bit of the entry: a block header
    u64 stop;    // the next candidate (lzhsplit::kNoStop: none)
    u32 base;    // where its output starts inside the entry's (lzhsplit::kBaseUnknown: not known yet)
    u32 limit;   // the sizes launch: the bytes at which it ends (lzhsplit::kNoLimit: none); the writing launch: bytes to write
    u32 has_len; // the sizes launch: `limit` is what is left of the entry's known length
    u32 pad;
};
struct LzhPieceRec {
    LzhRec r;  // as of an entry; r.end_bit of a piece that stopped at a boundary: that boundary
    u32 reach; // the furthest a match reached in front of the piece's own output
    u32 ended; // the stream ended in the piece: the end (a), an error, the limit
    u32 pad[2];
};
static_assert(sizeof(LzhPiece) == 32 && sizeof(LzhPieceRec) == 48, "copied between host and device as they are");
int lzh_launch_decode_piece(hipStream_t st, bool write, const u8 *ebase, u32 elen, u32 dbits, u32 pbits, int prefill, const LzhPiece *pcs,
                            u32 count, LzhPieceRec *rec, u8 *eout, u32 *emap);
// the candidates of one entry in two launches: fill = false leaves cnt[w] per search wave, fill = true writes them, ascending,
// wave w's behind first[w]
u32 lzh_split_search_waves(u32 elen);
int lzh_launch_split_search(hipStream_t st, bool fill, const u8 *ebase, u32 elen, u32 dbits, u32 pbits, u32 *cnt, const u32 *first, u64 *cand,
                            u32 ncand);
} // namespace lzhgpu
