// k_deflate.h -- declarations shared by the Deflate kernels (k_deflate.hip) and their orchestration
// (deflate_engine.hip).  SURVEY.md rows f-2 (Inflater) and f-3 (zlib / gzip containers).
#pragma once
#include "bzgpu.h"

namespace dfgpu {
using bzgpu::u8;
using bzgpu::u16;
using bzgpu::u32;
using bzgpu::u64;
using bzgpu::i64;

constexpr u32 kWin = 0x8000;       // Inflater::new: window (deflate/encoder.rs:117)
constexpr u32 kMaxMatch = 258;     // LZSS_MAX_MATCH :110
constexpr u32 kMinMatch = 3;       // LZSS_MIN_MATCH :109
constexpr u32 kChain = 255;        // MATCH_SEARCH_COUNT - 1 (lzss/slidedict.rs:129, 232)
constexpr u32 kBlockMax = 0xFFFF;  // MAX_BLOCK_SIZE (deflate/encoder.rs:270)
#ifndef DF_CHUNK_LOG2
#define DF_CHUNK_LOG2 19
#endif
constexpr u32 kChunk = 1u << DF_CHUNK_LOG2; // positions per sort chunk (hash chains are built chunk by chunk)
constexpr u32 kChunkStride = kChunk + kWin;          // entries of one sort chunk: its positions and the 32 KiB in front
constexpr u32 kChunkTiles = kChunkStride / bzgpu::kSortTile; // 132 tiles of 8192 entries
constexpr u32 kPrevSpan = kChunkStride / 256;         // 256-entry slices of one sort chunk
constexpr u32 kMTile = 8192;       // positions per match workgroup
constexpr u32 kMThreads = 1024;
#ifndef DF_M2_THREADS
#define DF_M2_THREADS 256          // entries per workgroup of the match kernel (k_df_match2)
#endif
constexpr u32 kPTile = 4096;       // positions per parse tile
constexpr u32 kEntries = 260;      // a step advances by at most 258 + 2: entry offsets 0..259
constexpr u32 kFan = 64;           // tiles composed per level
#ifndef DF_BLOCK_THREADS
#define DF_BLOCK_THREADS 128
#endif
constexpr u32 kBThreads = DF_BLOCK_THREADS;
#ifndef DF_EMIT_THREADS
#define DF_EMIT_THREADS 64
#endif
constexpr u32 kEThreads = DF_EMIT_THREADS;
constexpr u32 kHdrWords = 160;     // bits of BFINAL + dynamic header: < 74 + 316 * 14
constexpr u32 kDfLmTable = 3 * 288 + 64 + 2 * 15 * (2 * 288 + 4); // scratch words of one length-limited table
constexpr u32 kDfLmWords = 2 * kDfLmTable;
constexpr u32 kSumPiece = 65536;   // bytes per checksum piece
constexpr u32 F_CODE = 0x80000000u; // code[q]: an LZSS code starts at q
constexpr u32 F_REF = 0x40000000u;  //          it is a reference: len | (dist - 1) << 9
constexpr u32 F_STEP = 0x20000000u; //          a step of the LZSS parse starts at q (lzss/encoder.rs:132-184: a step emits up
                                    //          to two literals and then a reference; only its first code is a step start)

struct DfBlock {
    u32 btype;     // 0 stored, 1 fixed, 2 dynamic
    u32 hdr_bits;  // BFINAL + BTYPE (+ dynamic header)
    u32 bytes;     // decompress_len
    u32 lm;        // tables that took the length-limited path
    u64 bits;      // whole block, btype 1 / 2
    u64 bit_off;   // where it starts in the stream
};

// what a part of a long stream tells the host when its kernels are over (k_df_part_keep, k_df_part_tail)
struct DfPartRes {
    u64 consumed;    // where the next part starts
    u64 last_bstart; // start of the last block written
    u32 skip, err, nb_all, end_byte;
    u32 st[5];       // blocks stored / fixed / dynamic, limited tables, dynamic blocks without distances
    u32 pad[3];
};
int df_launch_part_keep(hipStream_t st, const u64 *bstart, u32 *nb, u32 bcap, const u32 *code, u64 n, u64 guard, DfPartRes *res);
int df_launch_part_tail(hipStream_t st, const DfBlock *blocks, const u64 *bstart, const u32 *nb, const u64 *total_bits, const u8 *stream, DfPartRes *res);

u32 df_chunks(u64 n); // sort chunks of an input of n bytes
int df_launch_chains(hipStream_t st, const u8 *in, u64 n, u32 *v0, u32 *s, u16 *hs, u32 *hist, u32 *tbase, u32 *pe);
int df_launch_match(hipStream_t st, const u8 *in, const u32 *pe, u64 n, u32 *M);
int df_launch_match2(hipStream_t st, const u8 *in, u64 n, const u32 *s, u32 *M);
// the block chain taken in pieces beside the marking of the tiles (df_launch_parse with canon): a second stream,
// kCutPieces + 1 events, the arguments of df_launch_cuts and two words of device memory for the chain's state
constexpr u32 kCutPieces = 4;
struct DfPiecewiseCuts {
    hipStream_t st2;
    hipEvent_t ev[kCutPieces + 1];
    u64 *bstart;
    u32 *nb;
    u32 cap, dl0, first;
    u64 *state;
    // kdone != nullptr: piece i of the chain leaves the number of blocks it has closed in kdone[i + 1] (kdone[0] is
    // 0) and records evc[i]; the caller launches the blocks of every piece behind its event and df_launch_parse does
    // not make `st` wait for the chain
    u32 *kdone;
    hipEvent_t evc[kCutPieces];
};
u32 df_cut_pieces(u32 ntiles);
int df_launch_blocks_piece(hipStream_t st, const u8 *in, const u32 *code, u64 *bstart, u32 *nb, u32 cap, DfBlock *blocks, u8 *lens,
                           u32 *hdr, u32 *lm_scratch, u32 dl0, u32 last_is_final, const u32 *kr, u32 piece_last);
int df_launch_block_offsets(hipStream_t st, DfBlock *blocks, const u32 *nb, u64 *total_bits, u32 bit0);
// pc != nullptr (needs canon): the block starts are made on the way (no df_launch_cuts afterwards)
int df_launch_parse(hipStream_t st, const u32 *M, u64 n, u16 *step, u16 *const *tabs, u16 *const *ents, const u32 *counts,
                    u32 nlevels, u32 *code, u64 *bm, u64 *canon, const DfPiecewiseCuts *pc);
// dl0: decompress_len carried into the segment (0 unless it follows an Action::Flush); last_is_final: the
// segment ends the stream (Finish) rather than being flushed.  `in` is the segment's first byte; the dl0 bytes
// in front of it must be readable (a stored first block copies them).  The block chain (df_launch_cuts) is its
// own launch so that the host can drop the blocks at the end of a PART of a long stream (those whose cuts could
// still change with the input behind the part) before tables and offsets are made; bit0: the first block starts
// at this bit (0..7) of the output's first byte.
int df_launch_cuts(hipStream_t st, u64 n, u64 *bm, u64 *bstart, u32 *nb, u32 cap, u32 dl0, u32 first);
int df_launch_blocks(hipStream_t st, const u8 *in, const u32 *code, u64 *bstart, u32 *nb, u32 cap,
                     DfBlock *blocks, u8 *lens, u32 *hdr, u32 *lm_scratch, u64 *total_bits, u32 dl0, u32 last_is_final, u32 bit0);
int df_launch_emit(hipStream_t st, const u8 *in, const u32 *code, const u64 *bstart, const u32 *nb, u32 cap,
                   const DfBlock *blocks, const u8 *lens, const u32 *hdr, u32 *out);
// ---- many inputs in one pass (df_gpu_encode_batch_device): every input of at most kBlockMax bytes is one block of its own.
// The inputs of a sub-batch lie in one IMAGE, each in a SLOT that starts at a multiple of kPTile (an input of 0 bytes has
// one tile too); tile_slot[t] = the slot that tile t of the image belongs to.
// With a preset dictionary every slot has `wtiles` = ceil(W / kPTile) WINDOW TILES in front of `lo`, which belong to it in
// tile_slot: the dictionary's last W bytes at [lo - W, lo), zeros in front of them.  `win` (device memory) holds that window
// right-aligned in kWin bytes, zeros in front of it; win == nullptr, W == 0, wtiles == 0: no dictionary, the kernels of old.
struct DfSlot {
    u64 src;  // where the input lies, relative to the caller's buffer
    u32 lo;   // the input's first image position
    u32 len;  // bytes of the input: the rest of the slot's last tile is a gap of zeros
};
struct DfBatchOut { u32 off, len; }; // a stream inside the sub-batch's output (off: a multiple of 4)
int df_launch_gather(hipStream_t st, const u8 *d_in, const DfSlot *slots, const u32 *tile_slot, u32 ntiles, u8 *image, const u8 *win);
int df_launch_match2_batch(hipStream_t st, const u8 *image, u64 n, const u32 *s, u32 *M, const u32 *tile_slot, const DfSlot *slots, u32 W);
// the parse of every slot: entered at offset 0 of its first input tile, tile after tile (no entry crosses a slot)
int df_launch_parse_batch(hipStream_t st, const u32 *M, u64 n, u32 ntiles, const DfSlot *slots, u32 nslots, u32 wtiles, u16 *step,
                          u16 *tab, u16 *ent, u32 *code, u64 *bm, u64 *canon);
// bse: (start, end) of block j = slot j; every block is the final block of its stream
int df_launch_blocks_batch(hipStream_t st, const u8 *image, const u32 *code, const u64 *bse, const u32 *nb, u32 nslots, DfBlock *blocks,
                           u8 *lens, u32 *hdr, u32 *lm_scratch);
// byte offset of every stream (header + blocks + trailer, rounded up to 4) and the bit offset of its block; total[0] = bytes
int df_launch_batch_offsets(hipStream_t st, DfBlock *blocks, u32 nslots, u32 head, u32 tail, DfBatchOut *outs, u64 *total);
int df_launch_emit_batch(hipStream_t st, const u8 *image, const u32 *code, const u64 *bse, const u32 *nb, u32 nslots, const DfBlock *blocks,
                         const u8 *lens, const u32 *hdr, u32 *out);
struct DfCrcShifts { u32 x[8]; }; // x^(8 * 256 * 2^k) mod P, reflected: moves a CRC register over 256 * 2^k bytes
int df_launch_sums(hipStream_t st, const u8 *in, u64 n, u64 *asum, u64 *bsum, u32 *crc, u32 *last_sub, DfCrcShifts xk);
// container header and trailer of every stream, written on the device (kind 1: Adler-32, kind 2: CRC-32 + ISIZE), and
// what kinds of blocks there were: stats[0..4] += stored, fixed, dynamic, limited tables, dynamic without distances
// with_dict (kind 1): the six-byte header with FDICT and `dictid`, the Adler-32 of the whole dictionary
int df_launch_batch_wrap(hipStream_t st, const u8 *image, const DfSlot *slots, u32 nslots, const DfBlock *blocks, const DfBatchOut *outs,
                         int kind, DfCrcShifts xk, u8 *out, u32 *stats, bool with_dict, u32 dictid);
// ---- a BGZF file (df_gpu_bgzf_encode_device): the batch pipeline over cuts of one contiguous input.  The slots' sources
// start at any byte (df_launch_gather_cut); a dynamic block without any match is never written (df_launch_blocks_strict:
// stored or fixed instead, DfBlock::lm bit 9); the members lie byte against byte (df_launch_exact_offsets: outs[j].off is
// any byte offset); df_launch_bgzf_wrap writes the 18-byte header with BSIZE and the gzip trailer, and counts
// stats[0..4] += stored, fixed, dynamic, limited tables, blocks the strict rule replaced.
int df_launch_gather_cut(hipStream_t st, const u8 *d_in, const DfSlot *slots, const u32 *tile_slot, u32 ntiles, u8 *image);
int df_launch_blocks_strict(hipStream_t st, const u8 *image, const u32 *code, const u64 *bse, const u32 *nb, u32 nslots, DfBlock *blocks,
                            u8 *lens, u32 *hdr, u32 *lm_scratch);
int df_launch_exact_offsets(hipStream_t st, DfBlock *blocks, u32 nslots, u32 head, u32 tail, DfBatchOut *outs, u64 *total);
int df_launch_bgzf_wrap(hipStream_t st, const u8 *image, const DfSlot *slots, u32 nslots, const DfBlock *blocks, const DfBatchOut *outs,
                        DfCrcShifts xk, u8 *out, u32 *stats);
// ---- LZHUF encode (bz_gpu_lzh_encode_batch_device, lzhuf_engine.hip; DESIGN_lzhuf.md sections 7 to 9): the batch front end
// above with LZHUF's window (1 << dbits), its longest match (256) and 64 KiB of history in front of every sort chunk, then
// blocks of 65 535 CODES.  Block k of a sub-batch belongs to slot `slot`; the blocks of slot j are bbase[j] .. bbase[j + 1] - 1,
// as many as the input could need (ceil(len / 65535)); those its parse does not fill have ncodes == 0.
constexpr u32 kLzhHist = 0x10000;                 // positions sorted in front of a chunk: the window of lh7
constexpr u32 kLzhStride = kChunk + kLzhHist;     // entries of one sort chunk
constexpr u32 kLzhBlockCodes = 0xFFFF;            // lzhuf/encoder.rs: codes per block
constexpr u32 kLzhNC = 510, kLzhNP = 17, kLzhNT = 19;
constexpr u32 kLzhHdrWords = 288;                 // a block header is at most 8 665 bits (DESIGN_lzhuf.md section 8)
constexpr u32 kLzhLensBytes = 576;                // per block: 512 c-lengths, 32 p-lengths, 32 t-lengths
constexpr u32 kLzhLmWords = 3 * kLzhNC + 64 + 2 * 16 * (2 * kLzhNC + 4); // scratch of one length-limited c-table
constexpr u32 kLzhSerialTiles = 64;               // a sub-batch of ONE slot with more tiles composes its exit tables
struct LzhBlk {
    u64 start, end; // image positions: its first code, and one past its last code's position
    u64 bits;       // header and codes
    u64 bit_off;    // where it starts in the sub-batch's output
    u32 slot, ncodes, hdr_bits;
    u32 flags;      // bit 0: the c-table is a constant, bit 1: the p-table is (or there is no match), bit 2: the t-table is
    u32 nlit, nmatch, lm, pad;
};
static_assert(sizeof(LzhBlk) == 64, "LzhBlk is copied between host and device as it is");
struct LzhOut { u64 off, len; }; // a stream inside the sub-batch's output (off: a multiple of 4)
// v0, s: df_chunks(n) * kLzhStride + 16 words each (and at least n + 16: M and code take their place); hist:
// (df_chunks(n) * kLzhStride / kSortTile + 1) * 256 words; tbase: 2 * (df_chunks(n) + 1) * 256 words
int lzh_launch_front(hipStream_t st, u32 dbits, const u8 *image, u64 n, u32 ntiles, const DfSlot *slots, u32 nslots, const u32 *tile_slot,
                     u32 *v0, u32 *s, u32 *hist, u32 *tbase, u16 *step, u16 *tab, u16 *ent, u64 *bm, u64 *canon);
// tab: lzh_tab_entries(ntiles) u16, ent: lzh_ent_entries(ntiles) u16
size_t lzh_tab_entries(u32 ntiles);
size_t lzh_ent_entries(u32 ntiles);
int lzh_launch_cuts(hipStream_t st, const DfSlot *slots, u32 nslots, const u32 *bbase, const u64 *bm, LzhBlk *blks);
int lzh_launch_blocks(hipStream_t st, const u8 *image, const u32 *code, LzhBlk *blks, u32 nblks, u32 pbits, u8 *lens, u32 *hdr, u32 *lm_scratch);
int lzh_launch_offsets(hipStream_t st, LzhBlk *blks, const u32 *bbase, u32 nslots, LzhOut *outs, u64 *total);
int lzh_launch_emit(hipStream_t st, const u8 *image, const u32 *code, const LzhBlk *blks, u32 nblks, const u8 *lens, const u32 *hdr, u32 *out);
// the block stage's table builder on given counts (bz_gpu_lzh_debug_tables): lens as one block's, res[0] = header bits
// (the 16-bit code count included), res[1] = flags, res[2] = tables on the length-limited path
int lzh_launch_tables_debug(hipStream_t st, const u32 *cfreq, const u32 *pfreq, u32 pbits, u8 *lens, u32 *hdr, u32 *lm_scratch, u32 *res);
// ---- decode of many streams (df_gpu_decode_batch_device; k_inflate.hip): what the sizes launch leaves per entry
struct DfInfRec {
    u64 end_bit;  // bits of the entry consumed: to the end of the stream or its trailer, or to the failing code
    u32 len;      // bytes produced in front of the verdict
    int verdict;  // BZ_OK, BZ_E_DATA, BZ_E_EOF
    u32 nblk[3];  // stored, fixed, dynamic blocks decoded whole
    u32 check;    // the trailer's Adler-32 (kind 1) / CRC-32 (kind 2)
    u32 isize;    // the trailer's ISIZE (kind 2)
    u32 flags;    // bit 0: the output would reach 4 GiB
    u32 pad[2];
};
// A preset dictionary as the decoder sees it: the last W <= 32768 bytes of it on the device -- history in front of position 0 of
// every entry's output -- and the Adler-32 of the whole dictionary (the DICTID of a zlib header).  W == 0: no dictionary.
struct DfWindow {
    const u8 *p = nullptr;
    u32 W = 0;
    u32 adler = 0;
};
// write = false: sizes only (out, out_off unused); write = true: the bytes of entry i go to out + out_off[i], at most rec[i].len
int df_launch_inflate(hipStream_t st, bool write, const u8 *in, const u64 *in_off, const u64 *in_len, u32 count, int kind, u8 *out,
                      const u64 *out_off, DfInfRec *rec, DfWindow win);
int df_launch_inflate_check(hipStream_t st, const u8 *out, const u64 *out_off, u32 count, DfInfRec *rec, int kind);
// ---- one large entry across many waves (inf_split.h): a piece runs from a bit of the entry to the first block boundary at
// or behind `stop`
struct DfPiece {
    u64 start; // bit of the entry: a block header, or (mode bit 0) the LEN field of a stored block
    u64 stop;  // infsplit::kNoStop: to the end of the stream
    u32 mode;  // bit 0: starts at LEN; bit 1: the entry's first piece, the container header comes first
    u32 base;  // where its output starts inside the entry's (infsplit::kBaseUnknown: not known yet)
    u32 len;   // the writing launch: bytes to write
    u32 pad;
};
struct DfPieceRec {
    DfInfRec r;   // as of an entry; r.end_bit of a piece that stopped at a boundary: that boundary (see end_mode)
    u32 reach;    // the furthest a match reached in front of the piece's own output
    u32 end_mode; // the boundary is 0: a block header, 1: the LEN field of a non-final stored block
    u32 ended;    // the stream ended in the piece: the final block, an error, the entry's end
    u32 pad;
};
int df_launch_split_search(hipStream_t st, const u8 *ebase, u32 elen, u32 piece_bytes, u32 npieces, void *cand);
int df_launch_inflate_piece(hipStream_t st, bool write, const u8 *ebase, u32 elen, int kind, const DfPiece *pc, u32 count, DfPieceRec *rec,
                            u8 *eout, u32 *emap, DfWindow win);
int df_launch_split_jump(hipStream_t st, u32 *src, u32 n, u32 *cnt);
int df_launch_split_gather(hipStream_t st, u8 *out, const u32 *src, u32 n);
// ---- every member of a gzip file (gz_members.h; k_gz_members.hip)
struct GzSpan {
    u64 src; // where the bytes lie, relative to the source buffer
    u64 dst; // where they go, relative to the target buffer
    u32 len;
    u32 pad;
};
int df_launch_gz_search_count(hipStream_t st, const u8 *in, u32 len, u32 ntiles, u32 *cnt);
// the candidates numbered [first, first + n) of the input, found in the tiles [tile0, tile0 + ntiles); base: per tile of the
// INPUT, the candidates in front of it
int df_launch_gz_search_list(hipStream_t st, const u8 *in, u32 len, u32 tile0, u32 ntiles, const u32 *base, u32 first, u32 n, u32 *list);
int df_launch_gz_gather(hipStream_t st, const u8 *in, const GzSpan *spans, u32 count, u32 max_len, u8 *image);
int df_launch_gz_zero_skip(hipStream_t st, const u8 *in, const u32 *from, const u32 *bound, u32 count, u32 *out);
int df_launch_gz_compact(hipStream_t st, const u8 *staged, const GzSpan *spans, u32 count, u32 max_len, u8 *out);
// ---- reading BGZF (bgzf_index.h; k_bgzf_read.hip, k_bgzf_inflate and k_bgzf_check in k_inflate.hip)
struct BgzfInfo {
    u32 bsize1; // BSIZE + 1 of a candidate
    u32 isize;  // its ISIZE when the block lies whole inside the input and is at least 28 bytes, else 0
};
// the candidates per tile of bgzf::kTile positions; then, behind the host's exclusive sum (base: per tile of the INPUT, the
// candidates in front of it), the candidates numbered [first, first + n) found in the tiles [tile0, tile0 + ntiles)
int df_launch_bgzf_search_count(hipStream_t st, const u8 *in, u64 len, u32 ntiles, u32 *cnt);
int df_launch_bgzf_search_list(hipStream_t st, const u8 *in, u64 len, u32 tile0, u32 ntiles, const u64 *base, u64 first, u32 n, u64 *list);
int df_launch_bgzf_block_info(hipStream_t st, const u8 *in, u64 len, const u64 *list, u32 n, BgzfInfo *info);
// One block of a read as its wave is told it: the index's word about it, and where its bytes go.
struct BgzfDesc {
    u64 coff;  // where the block starts, relative to the input
    u64 dst;   // slot == 0: where its bytes go, relative to the output; else where its slice [lo, lo + n) goes
    u32 csize; // coff[k + 1] - coff[k]: 1 .. 65536
    u32 usize; // uoff[k + 1] - uoff[k]: 0 .. 65536
    u32 slot;  // 0: written in place; 1, 2: an edge block, decoded into that 64 KiB slot of the workspace
    u32 lo, n; // the slice of an edge block that belongs to the range
    u32 pad;
};
struct BgzfRec {
    int verdict;  // BZ_OK or BZ_E_DATA
    u32 len;      // bytes produced
    u32 check;    // the trailer's CRC-32
    u32 nblk[3];  // stored, fixed, dynamic Deflate blocks decoded whole
    u32 pad[2];
};
int df_launch_bgzf_inflate(hipStream_t st, const u8 *in, const BgzfDesc *desc, u32 count, u8 *out, u8 *slots, BgzfRec *rec);
int df_launch_bgzf_check(hipStream_t st, const BgzfDesc *desc, u32 count, const u8 *out, const u8 *slots, BgzfRec *rec);
// the slices of the edge blocks (descriptors with slot != 0; `count` of them, at most two) from their slots into the output
int df_launch_bgzf_edge_copy(hipStream_t st, const BgzfDesc *desc, u32 count, const u8 *slots, u8 *out);
} // namespace dfgpu
