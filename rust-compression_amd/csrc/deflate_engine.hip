// deflate_engine.hip -- orchestration and C ABI of the Deflate / zlib / gzip encode path
// (include/bz2_mi355x.h section 4).  Kernels: k_deflate.hip.
//
// Replaces, behind the reference's Encoder surface: Inflater (deflate/encoder.rs:92-260), ZlibEncoder
// (zlib/encoder.rs:55-157), GZipEncoder (gzip/encoder.rs:50-135) driven with Action::Finish (and
// Action::Run in front of it), with or without a preset dictionary (::with_dict), and -- for Inflater -- with
// Action::Flush in the middle of a stream (a stream is then a sequence of byte-aligned SEGMENTS, df_enc_end).
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "engine_state.h"
#include "batch_decode.h"
#include "copy_pool.h"

#include <sys/mman.h>
#include <functional>
#include "k_deflate.h"
#include "inf_split.h"
#include "gz_members.h"
#include "bgzf_index.h"

using namespace dfgpu;

struct DfWorkspace {
    DevBuf keys_in, keys_out, vals_in, vals_out, sort_tmp, prevd, est, segoff, concat, bitmap, canon, tabs, ents, bstart, nb, blocks, lens, hdr, lm, total,
        stream, asum, bsum, crc, part_res;
    DevBuf b_slots, b_tile_slot, b_bse, b_outs, b_stats; // a sub-batch of df_gpu_encode_batch_device: slot tables, block ends, streams' places
    DevBuf b_win;                                      // ... and the window of a call with a preset dictionary (uploaded per call)
    u64 batch_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // df_gpu_last_batch_stats
    u64 bgzf_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};      // df_gpu_last_bgzf_stats
    DevBuf i_in, i_ooff, i_rec;                        // df_gpu_decode_batch_device: the entries' ranges, their outputs' places, their records
    DevBuf i_dict;                                     // ... and the window of a call with a preset dictionary (uploaded per call)
    u64 inf_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // df_gpu_last_decode_batch_stats
    DevBuf s_cand, s_piece, s_prec, s_map, s_cnt;      // an entry across many waves: candidates, pieces, their records, the source map
    u64 split_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // df_gpu_last_decode_split_stats
    double split_ms[7] = {0, 0, 0, 0, 0, 0, 0};        // search, sizes, repair, writing, jump rounds, gather, checksum
    DevBuf m_cnt, m_base, m_cand, m_span, m_image, m_zs, m_stage; // every member of a gzip file: candidates per tile and in front of it, a
                                                       // window of the list, span tables, the batch image, zero skips, the members' bytes
    u64 mem_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // df_gpu_last_decode_members_stats
    double mem_ms[4] = {0, 0, 0, 0};                   // search, gather, zero skip, compaction
    DevBuf z_cnt, z_base, z_cand, z_info, z_desc, z_rec, z_slots; // reading BGZF: candidates per tile and in front of it, a window of the
                                                       // list and its blocks' sizes, a group's descriptors and records, the two edge slots
    u64 bgzf_read_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // df_gpu_last_bgzf_read_stats
    double bgzf_index_s = 0;                           // search and chain of the last index call
    double t_stage[6] = {0, 0, 0, 0, 0, 0}; // chains, matches, parse, blocks, emit, total
    u64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // blocks, stored, fixed, dynamic, limited tables, stream bytes, dynamic w/o distances
    hipEvent_t ev[7] = {};
    hipEvent_t evq[2 * kCutPieces + 1] = {}; // the pieces of the block chain beside the marking kernel
    bool ev_ready = false;
    // the blocks of the last call (or of its last part) for the debug entry points: fetched when one of them asks
    std::vector<DfBlock> h_blocks;
    std::vector<u64> h_bstart;
    u32 h_nb = 0;
    bool h_fetched = true;
};

void df_workspace_free(DfWorkspace *w)
{
    if (!w) return;
    if (w->ev_ready) {
        for (hipEvent_t e : w->ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : w->evq) (void)hipEventDestroy(e);
    }
    delete w;
}

// the engine's Deflate workspace with its events, made by the first call that needs it; selects the engine's device
static int df_workspace(bz_gpu_engine *g, DfWorkspace **out)
{
    HIPCHK(hipSetDevice(g->device));
    if (!g->df) g->df = new DfWorkspace();
    DfWorkspace *w = g->df;
    if (!w->ev_ready) {
        for (hipEvent_t &e : w->ev) HIPCHK(hipEventCreate(&e));
        for (hipEvent_t &e : w->evq) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        w->ev_ready = true;
    }
    *out = w;
    return BZ_OK;
}

// ev[0..6] as six stage times in seconds (five stages and the whole), assigned to t[] or added to it
static void df_stage_times(const DfWorkspace *w, double t[6], bool add)
{
    for (int i = 0; i < 6; ++i) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, w->ev[i < 5 ? i : 0], w->ev[i < 5 ? i + 1 : 6]);
        t[i] = (add ? t[i] : 0.0) + ms * 1e-3;
    }
}

// The buffers that one stream (df_encode_core) and a sub-batch of one-block inputs (df_batch_run) size alike: `positions`
// bytes go through the chain sort, the match kernel and the parse, in `tiles` tiles with a canonical orbit each (0: the
// parse by doubling has none), for at most `blocks` blocks and `stream_bytes` bytes of stream.
static int df_reserve_pipeline(DfWorkspace *w, u64 positions, u32 tiles, size_t blocks, size_t stream_bytes)
{
    const u64 npad = positions + 16, nchunks = df_chunks(positions);
    const u64 nsort = nchunks * kChunkStride + 16; // words of a sorted-position array
    int rc;
    if ((rc = w->keys_in.ensure(npad * 2)) != BZ_OK) return rc;                           // step[]
    if ((rc = w->vals_in.ensure((nsort > npad ? nsort : npad) * 4)) != BZ_OK) return rc;  // pass 0 output, later M[]
    if ((rc = w->vals_out.ensure((nsort > npad ? nsort : npad) * 4)) != BZ_OK) return rc; // sorted positions, later code[]
    if ((rc = w->sort_tmp.ensure((nchunks * kChunkTiles + 1) * 256 * 4)) != BZ_OK) return rc; // per-tile digit counts
    if ((rc = w->keys_out.ensure(2 * (nchunks + 1) * 256 * 4)) != BZ_OK) return rc;       // per-chunk digit bases, both passes
    if (tiles && (rc = w->canon.ensure((size_t)tiles * 64 * 8 + 64)) != BZ_OK) return rc; // a tile's canonical orbit, one bit per position
    if ((rc = w->bitmap.ensure((positions / 64 + 8) * 8)) != BZ_OK) return rc;
    if ((rc = w->nb.ensure(64)) != BZ_OK) return rc;
    if ((rc = w->blocks.ensure(blocks * sizeof(DfBlock))) != BZ_OK) return rc;
    if ((rc = w->lens.ensure(blocks * 320)) != BZ_OK) return rc;
    if ((rc = w->hdr.ensure(blocks * kHdrWords * 4)) != BZ_OK) return rc;
    if ((rc = w->lm.ensure(blocks * kDfLmWords * 4)) != BZ_OK) return rc;
    if ((rc = w->total.ensure(128)) != BZ_OK) return rc; // the stream's bit count, the chain's state, its pieces' block counts
    return w->stream.ensure(stream_bytes + 64);
}

extern "C" size_t df_encode_bound(size_t n)
{
    // stored blocks are the worst case: 5 bytes per 0xFFFF, plus container, plus word slack for the bit writer
    return n + 5 * (n / 0xFFFF + 2) + 64;
}

// ---- reflected CRC-32 arithmetic on the host (crc32.rs:40-55): polynomials with bit 31 = x^0
static u32 gf_mul_reflected(u32 a, u32 b)
{
    u32 p = 0;
    for (u32 m = 1u << 31; m != 0 && a != 0; m >>= 1) { // a: coefficients from x^0 (bit 31) upwards
        if (a & m) {
            p ^= b;
            a &= ~m;
        }
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1; // b * x
    }
    return p;
}
static u32 gf_xpow8_reflected(u64 nbytes) // x^(8 * nbytes) mod P
{
    u32 r = 1u << 31, sq = 1u << 23; // x^0, x^8
    while (nbytes) {
        if (nbytes & 1) r = gf_mul_reflected(r, sq);
        sq = gf_mul_reflected(sq, sq);
        nbytes >>= 1;
    }
    return r;
}
// Adler-32 (adler32.rs:20-66) of a preset dictionary: the DICTID of a zlib header
static u32 df_adler32_host(const uint8_t *p, size_t n)
{
    u32 a = 1, b = 0;
    for (size_t i = 0; i < n;) { // (5552 bytes keep b below 2^32: the largest n with 255 n (n + 1) / 2 + (n + 1) 65520 < 2^32)
        const size_t end = std::min(n, i + 5552);
        for (; i < end; ++i) {
            a += p[i];
            b += a;
        }
        a %= 65521;
        b %= 65521;
    }
    return (b << 16) | a;
}
// the parameter errors of a dictionary, the same in every batch form, encode and decode: a length without a pointer, and gzip
// (GZipEncoder and GZipDecoder have no with_dict)
static int df_dict_param(int kind, const uint8_t *dict, size_t dict_len)
{
    return dict_len && (!dict || kind == 2) ? BZ_E_PARAM : BZ_OK;
}
static DfCrcShifts df_crc_shifts() // x^(8 * 256 * 2^k): what the device folds a piece's sub-pieces with
{
    DfCrcShifts xk;
    for (u32 k = 0; k < 8; ++k) xk.x[k] = gf_xpow8_reflected(256ull << k);
    return xk;
}

// dict (host memory, may be NULL): Inflater::with_dict / ZlibEncoder::with_dict (deflate/encoder.rs:134-153,
// lzss/encoder.rs:104-130: the last 0x8000 bytes of it are history in front of the input)
// A SEGMENT of a stream (Action::Flush cuts a stream into segments: the LZSS stage is drained, the current block
// is closed WITHOUT the final bit and the bit string is padded to a byte, deflate/encoder.rs:170-195, :638-647,
// :236-246; the window and `decompress_len` live on).  d_in[0, n) is the segment; `prior` = stream bytes in
// front of it, readable at d_in[-prior, 0) (history of the match finder next to the dictionary's; a stored first
// block reaches back dl0 <= prior bytes); dl0 = decompress_len carried in; `final`: the segment ends the stream;
// head / tail: write the container's header / trailer (the trailer's checksums cover d_in[-prior, n)).
// *dl_out = decompress_len behind the segment.  A whole stream is the one segment (prior 0, dl0 0, final).
struct DfSeg {
    u64 prior = 0;
    u32 dl0 = 0;
    bool final = true, head = true, tail = true;
    // A PART of a long segment (one call handles < 2 GiB of positions): `more` = the input goes on behind
    // d_in[n) without a flush, and the n bytes handed in include look-ahead: only the blocks whose cuts and
    // codes cannot change with the bytes behind d_in[n) are written, *consumed tells where the next part
    // starts: at the STEP of the LZSS parse that holds the first block left out.  A block starts at a code,
    // but a step of the parse (lzss/encoder.rs:132-184) can emit one or two literals and then a reference, and
    // a block may be cut between them; the parse can only be taken up at the step's first byte, where the
    // decision was made.  skip = the literals of that step (0..2 bytes) that went out with the part before: the
    // first block of this part starts behind them.  bit0 / carry_byte: the bits (0..7) of the output's first
    // byte that the previous part has already filled.
    bool more = false;
    // Action::Run seen by a zlib / gzip wrapper (its container ends at the inner encoder's first None,
    // zlib/encoder.rs:146-150): write exactly the blocks the reference's Inflater has CLOSED once the iterator is dry.
    // The LZSS stage decides a step of its parse only with 258 + 3 bytes of look-ahead (lzss/encoder.rs:186-194), so
    // the codes of the steps that start at p <= n - 261 are out and are those of any longer input; a block is closed by
    // the arrival of the next block's first code (deflate/encoder.rs:585-593).  Only whole bytes leave the BitWriter.
    bool run = false;
    u32 skip = 0;
    u32 bit0 = 0;
    u8 carry_byte = 0;
    bool accumulate_stats = false;
};
struct DfPartOut {
    u64 consumed = 0;   // where the next part starts (the step that holds the first block left out)
    u32 skip = 0;       // bytes behind it that are already written (that step's literals)
    u32 end_bits = 0;   // bits (0..7) filled in the byte behind the bytes returned (more == true)
    u8 end_byte = 0;
};
// bytes at the end of a part that is not the last one whose codes or cuts may still change: a cut looks 0xFFFF
// bytes ahead, the code there another 258 + 2 + 258
constexpr u64 kPartGuard = 0x10000ull + 1024ull;
static int df_encode_core(bz_gpu_engine *g, int kind, const u8 *d_in, u64 n, const u8 *dict, size_t dict_len, u8 *d_out,
                          size_t cap, size_t *out_len, const DfSeg &seg = DfSeg(), u32 *dl_out = nullptr,
                          DfPartOut *part_out = nullptr)
{
    if (n >= (1ull << 31) - kWin) return BZ_E_PARAM; // positions and bit offsets are sized for < 2 GiB per call
    if (dict_len && kind == 2) return BZ_E_PARAM;    // GZipEncoder has no with_dict
    if (seg.dl0 > kBlockMax || seg.dl0 > seg.prior) return BZ_E_PARAM;
    int rc;
    DfWorkspace *w = nullptr;
    if ((rc = df_workspace(g, &w)) != BZ_OK) return rc;
    hipStream_t st = g->st;
    // history in front of the segment: the last 32 KiB of (dictionary, then the stream so far)
    const u64 hist_dev = seg.prior < kWin ? seg.prior : kWin;
    const u64 hist_dict = dict_len < kWin - hist_dev ? dict_len : kWin - hist_dev;
    const u64 hist = hist_dict + hist_dev;
    const u64 nall = hist + n;                           // positions the chain and match stages see
    const u64 npad = nall + 16;
    const u32 ntiles = (u32)((n + kPTile - 1) / kPTile) + (n == 0 ? 1u : 0u);
    std::vector<u32> counts;
    counts.push_back(ntiles);
    while (counts.back() > 1) counts.push_back((counts.back() + kFan - 1) / kFan);
    const u32 nlevels = (u32)counts.size();
    size_t tab_words = 0, ent_words = 0;
    for (u32 c : counts) { tab_words += (size_t)c * kEntries; ent_words += c + 8; }
    const u32 bcap = (u32)(n / (kBlockMax - 300) + 2);

    // BZ_DF_MATCH=walk: the chain-walking match kernel of rounds 1 and 2 (k_df_prev + k_df_match) instead of the one
    // that reads the candidates off the sorted order (k_df_match2); same match words either way
    const char *mv = getenv("BZ_DF_MATCH");
    const bool walk = mv && strcmp(mv, "walk") == 0;
    // BZ_DF_PARSE=doubling: the parse by pointer doubling of rounds 1 and 2 (k_df_tile_tab / k_df_mark) instead of
    // the canonical orbits (k_df_tile_orbit / k_df_mark2); same code words either way
    const char *pv = getenv("BZ_DF_PARSE");
    const bool doubling = pv && strcmp(pv, "doubling") == 0;
    const size_t bound = df_encode_bound(n);
    if ((rc = df_reserve_pipeline(w, nall, doubling ? 0u : ntiles, bcap, bound)) != BZ_OK) return rc;
    if (walk) {
        if ((rc = w->est.ensure((df_chunks(nall) * kChunkStride + 16) * 2)) != BZ_OK) return rc; // hashes of the sorted positions
        if ((rc = w->prevd.ensure(npad * 4)) != BZ_OK) return rc; // per position: chain distance | chain length << 16
    }
    if (hist && (rc = w->concat.ensure(nall + 64)) != BZ_OK) return rc;
    if ((rc = w->tabs.ensure(tab_words * 2 + 64)) != BZ_OK) return rc;
    if ((rc = w->ents.ensure(ent_words * 2 + 64)) != BZ_OK) return rc;
    if ((rc = w->bstart.ensure(((size_t)bcap + 2) * 8)) != BZ_OK) return rc;
    if ((rc = w->part_res.ensure(sizeof(DfPartRes))) != BZ_OK) return rc;
    const u64 ntot = seg.prior + n; // bytes the container's checksums cover
    const u32 npieces = (u32)((ntot + kSumPiece - 1) / kSumPiece);
    if (kind != 0) {
        if ((rc = w->asum.ensure((size_t)(npieces + 1) * 8)) != BZ_OK) return rc;
        if ((rc = w->bsum.ensure((size_t)(npieces + 1) * 8)) != BZ_OK) return rc;
        if ((rc = w->crc.ensure((size_t)(npieces + 1) * 4 + 256 * 4)) != BZ_OK) return rc; // per piece, + the last piece's sub-pieces
    }

    std::vector<u16 *> tabs(nlevels), ents(nlevels);
    {
        u16 *t = w->tabs.as<u16>(), *e = w->ents.as<u16>();
        for (u32 l = 0; l < nlevels; ++l) {
            tabs[l] = t; t += (size_t)counts[l] * kEntries;
            ents[l] = e; e += counts[l] + 8;
        }
    }
    u16 *step = w->keys_in.as<u16>();
    u32 *Mall = w->vals_in.as<u32>();
    u32 *M = Mall + hist; // match words of the input positions
    u32 *code = w->vals_out.as<u32>();
    const u8 *d_all = d_in;
    if (hist) { // history + input in one buffer for the chain and match stages
        if (hist_dict) HIPCHK(hipMemcpy(w->concat.p, dict + (dict_len - hist_dict), hist_dict, hipMemcpyHostToDevice));
        if (hist_dev + n)
            HIPCHK(hipMemcpyAsync(w->concat.as<u8>() + hist_dict, d_in - hist_dev, hist_dev + n, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(w->concat.as<u8>() + nall, 0, 64, st));
        d_all = w->concat.as<u8>();
    }

    HIPCHK(hipEventRecord(w->ev[0], st));
    HIPCHK(hipMemsetAsync(w->stream.p, 0, bound + 64, st));
    if (df_launch_chains(st, d_all, nall, w->vals_in.as<u32>(), w->vals_out.as<u32>(), w->est.as<u16>(), w->sort_tmp.as<u32>(), w->keys_out.as<u32>(),
                         walk ? w->prevd.as<u32>() : nullptr) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[1], st));
    if ((walk ? df_launch_match(st, d_all, w->prevd.as<u32>(), nall, Mall)
              : df_launch_match2(st, d_all, nall, w->vals_out.as<u32>(), Mall)) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[2], st));
    if (seg.skip > 2 || (seg.skip && seg.dl0)) return BZ_E_PARAM;
    // BZ_DF_CUTS=after: the chain of block starts behind the marking kernel (rounds 1 and 2) instead of in pieces
    // beside it on the engine's second stream
    const char *cv = getenv("BZ_DF_CUTS");
    const bool beside = n != 0 && !doubling && !(cv && strcmp(cv, "after") == 0); // (no tiles, no pieces)
    DfPiecewiseCuts pc;
    pc.st2 = g->st2;
    for (u32 i = 0; i <= kCutPieces; ++i) pc.ev[i] = w->evq[i];
    pc.bstart = w->bstart.as<u64>();
    pc.nb = w->nb.as<u32>();
    pc.cap = bcap; pc.dl0 = seg.dl0; pc.first = seg.skip;
    pc.state = w->total.as<u64>() + 2; // (spare words of the 64-byte buffer that takes the stream's bit count)
    // the blocks of a piece follow the chain's piece at once -- unless the host has to look at the chain first (a part
    // of a long stream, a wrapper ending under Action::Run: it drops blocks at the end)
    const bool blocks_follow = beside && !seg.more && !seg.run;
    pc.kdone = blocks_follow ? w->total.as<u32>() + 8 : nullptr;
    for (u32 i = 0; i < kCutPieces; ++i) pc.evc[i] = w->evq[kCutPieces + 1 + i];
    if (beside) HIPCHK(hipMemsetAsync(w->total.p, 0, 128, st));
    if (df_launch_parse(st, M, n, step, tabs.data(), ents.data(), counts.data(), nlevels, code, w->bitmap.as<u64>(),
                        doubling ? nullptr : w->canon.as<u64>(), beside ? &pc : nullptr) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[3], st));
    if (!beside && df_launch_cuts(st, n, w->bitmap.as<u64>(), w->bstart.as<u64>(), w->nb.as<u32>(), bcap, seg.dl0, seg.skip) != 0)
        return BZ_E_UNEXPECTED;
    u64 consumed = n;
    u32 next_skip = 0;
    HIPCHK(hipMemsetAsync(w->part_res.p, 0, sizeof(DfPartRes), st));
    if (seg.more) {
        // keep the blocks that START at or before n - guard: their ends (cuts) and codes are final; the next part starts at
        // the step of the parse that holds the first block left out.  Decided on the device (k_df_part_keep: rounds 1-4 read the
        // block starts and three code words back here, with the GPU idle meanwhile); the host learns it with the bit count.
        if (n <= kPartGuard) return BZ_E_UNEXPECTED;
        if (df_launch_part_keep(st, w->bstart.as<u64>(), w->nb.as<u32>(), bcap, code, n, kPartGuard, w->part_res.as<DfPartRes>()) != 0)
            return BZ_E_UNEXPECTED;
    }
    if (seg.run && !seg.more) {
        u32 nb_all = 0;
        HIPCHK(hipMemcpyAsync(&nb_all, w->nb.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (nb_all == 0xFFFFFFFFu || nb_all > bcap) return BZ_E_UNEXPECTED;
        std::vector<u64> hb((size_t)nb_all + 1);
        if (nb_all) HIPCHK(hipMemcpy(hb.data(), w->bstart.p, ((size_t)nb_all + 1) * 8, hipMemcpyDeviceToHost));
        // block j-1 is closed when the code at hb[j] has arrived: the step of the parse that holds it (at most two
        // literals in front of a reference) starts at or before n - 261.  (With a `skip` the first block starts
        // inside a step of the previous part; cuts further on are at least 0xFFFF - 257 bytes behind it.)
        u32 keep = 0;
        for (u32 j = nb_all; j-- > 1;) {
            const u64 bcut = hb[j];
            u32 cw[3] = {0, 0, 0};
            const u64 lo = bcut < 2 ? bcut : 2;
            HIPCHK(hipMemcpy(cw + (2 - lo), code + (bcut - lo), (size_t)(lo + 1) * 4, hipMemcpyDeviceToHost));
            if (!(cw[2] & F_CODE)) return BZ_E_UNEXPECTED;
            const u32 back = (cw[2] & F_STEP) ? 0u : ((cw[1] & F_STEP) ? 1u : 2u);
            if (back > lo || !(cw[2 - back] & F_STEP)) return BZ_E_UNEXPECTED;
            if (bcut - back + 261 <= n) {
                keep = j;
                break;
            }
        }
        HIPCHK(hipMemcpyAsync(w->nb.p, &keep, 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st)); // (`keep` lives on this stack frame)
    }
    if (blocks_follow) {
        const u32 np = df_cut_pieces(ntiles);
        for (u32 i = 0; i < np; ++i) {
            HIPCHK(hipStreamWaitEvent(st, pc.evc[i], 0));
            if (df_launch_blocks_piece(st, d_in, code, w->bstart.as<u64>(), w->nb.as<u32>(), bcap, w->blocks.as<DfBlock>(), w->lens.as<u8>(),
                                       w->hdr.as<u32>(), w->lm.as<u32>(), seg.dl0, seg.final ? 1u : 0u, pc.kdone + i, i + 1 == np ? 1u : 0u) != 0)
                return BZ_E_UNEXPECTED;
        }
        if (df_launch_block_offsets(st, w->blocks.as<DfBlock>(), w->nb.as<u32>(), w->total.as<u64>(), seg.bit0) != 0) return BZ_E_UNEXPECTED;
    } else if (df_launch_blocks(st, d_in, code, w->bstart.as<u64>(), w->nb.as<u32>(), bcap, w->blocks.as<DfBlock>(),
                                w->lens.as<u8>(), w->hdr.as<u32>(), w->lm.as<u32>(), w->total.as<u64>(), seg.dl0,
                                (seg.final && !seg.more && !seg.run) ? 1u : 0u, seg.bit0) != 0)
        return BZ_E_UNEXPECTED;
    if (seg.bit0) HIPCHK(hipMemcpyAsync(w->stream.p, &seg.carry_byte, 1, hipMemcpyHostToDevice, st)); // (the stream was cleared above)
    HIPCHK(hipEventRecord(w->ev[4], st));
    if (df_launch_emit(st, d_in, code, w->bstart.as<u64>(), w->nb.as<u32>(), bcap, w->blocks.as<DfBlock>(), w->lens.as<u8>(),
                       w->hdr.as<u32>(), w->stream.as<u32>()) != 0)
        return BZ_E_UNEXPECTED;
    if (kind != 0 && seg.tail) {
        if (df_launch_sums(st, d_in - seg.prior, ntot, w->asum.as<u64>(), w->bsum.as<u64>(), w->crc.as<u32>(), w->crc.as<u32>() + npieces + 1,
                           df_crc_shifts()) != 0)
            return BZ_E_UNEXPECTED;
    }
    HIPCHK(hipEventRecord(w->ev[5], st));
    if (df_launch_part_tail(st, w->blocks.as<DfBlock>(), w->bstart.as<u64>(), w->nb.as<u32>(), w->total.as<u64>(), w->stream.as<u8>(),
                            w->part_res.as<DfPartRes>()) != 0)
        return BZ_E_UNEXPECTED;
    u64 total_bits = 0;
    u32 nb = 0;
    DfPartRes pres;
    HIPCHK(hipMemcpyAsync(&total_bits, w->total.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&nb, w->nb.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&pres, w->part_res.p, sizeof(pres), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one look at the device per part
    if (seg.more && pres.err) return BZ_E_UNEXPECTED;
    if (nb == 0xFFFFFFFFu || nb > bcap) {
        fprintf(stderr, "bz2_mi355x: deflate parse produced no code start inside a block window (internal error)\n");
        return BZ_E_UNEXPECTED;
    }
    if (seg.more) {
        consumed = pres.consumed;
        next_skip = pres.skip;
    }
    // (a part that is not the last one hands on its last, partly filled byte instead of writing it)
    // ... and the bits of a partly filled byte never leave the BitWriter of a wrapper that ends under Action::Run
    const u64 body = (seg.more || seg.run) ? (total_bits >> 3) : ((total_bits + 7) >> 3);
    if (part_out) {
        part_out->consumed = consumed;
        part_out->skip = next_skip;
        part_out->end_bits = seg.more ? (u32)(total_bits & 7u) : 0u;
        part_out->end_byte = part_out->end_bits ? (u8)pres.end_byte : 0;
    }

    // container (zlib/encoder.rs:63-72,118-156; gzip/encoder.rs:62-75,88-134)
    u8 head[10], tail[8];
    size_t nhead = 0, ntail = 0;
    if (!seg.head) {
        // (a later segment of a stream: the header went out with the first one)
    } else if (kind == 1 && dict_len) { // zlib/encoder.rs:74-93: FDICT + Adler-32 of the whole dictionary
        u32 a = 1, b = 0;
        for (size_t i = 0; i < dict_len; ++i) { a = (a + dict[i]) % 65521; b = (b + a) % 65521; }
        const u32 h = (b << 16) | a;
        head[0] = 0x78; head[1] = 0xF9; head[2] = (u8)(h >> 24); head[3] = (u8)(h >> 16); head[4] = (u8)(h >> 8); head[5] = (u8)h;
        nhead = 6;
    } else if (kind == 1) {
        head[0] = 0x78; head[1] = 0xDA; nhead = 2;
    } else if (kind == 2) {
        const u8 h[10] = {0x1F, 0x8B, 0x08, 0, 0, 0, 0, 0, 0, 0xFF};
        memcpy(head, h, 10); nhead = 10;
    }
    if (kind != 0 && seg.tail) {
        std::vector<u64> a(npieces), b(npieces);
        std::vector<u32> c((size_t)npieces + 1 + 256);
        if (npieces) {
            HIPCHK(hipMemcpy(a.data(), w->asum.p, (size_t)npieces * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(b.data(), w->bsum.p, (size_t)npieces * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(c.data(), w->crc.p, ((size_t)npieces + 1 + 256) * 4, hipMemcpyDeviceToHost));
        }
        if (kind == 1) { // adler32.rs:20-66
            u64 A = 1, B = 0;
            for (u32 t = 0; t < npieces; ++t) {
                const u64 len = (t + 1 == npieces) ? ntot - (u64)t * kSumPiece : kSumPiece;
                B = (B + (len % 65521) * A + b[t]) % 65521;
                A = (A + a[t]) % 65521;
            }
            const u32 h = (u32)((B << 16) | A);
            tail[0] = (u8)(h >> 24); tail[1] = (u8)(h >> 16); tail[2] = (u8)(h >> 8); tail[3] = (u8)h; ntail = 4;
        } else { // CRC-32 (reflected), little endian, then ISIZE
            const u32 xpiece = gf_xpow8_reflected(kSumPiece);
            u32 raw = 0; // register for a zero initial value over the whole input
            for (u32 t = 0; t < npieces; ++t) {
                const u64 len = (t + 1 == npieces) ? ntot - (u64)t * kSumPiece : kSumPiece;
                if (len == kSumPiece) raw = gf_mul_reflected(raw, xpiece) ^ c[t]; // folded on the device
                else
                    for (u32 s = 0; (u64)s * 256 < len; ++s) { // the last, partial piece: its sub-pieces
                        const u64 sl = (len - (u64)s * 256) < 256 ? (len - (u64)s * 256) : 256;
                        raw = gf_mul_reflected(raw, gf_xpow8_reflected(sl)) ^ c[(size_t)npieces + 1 + s];
                    }
            }
            const u32 crc = raw ^ gf_mul_reflected(0xFFFFFFFFu, gf_xpow8_reflected(ntot)) ^ 0xFFFFFFFFu;
            const u32 isz = (u32)ntot;
            for (int i = 0; i < 4; ++i) tail[i] = (u8)(crc >> (8 * i));
            for (int i = 0; i < 4; ++i) tail[4 + i] = (u8)(isz >> (8 * i));
            ntail = 8;
        }
    }
    const size_t need = nhead + body + ntail;
    *out_len = need;
    if (d_out) {
        if (need > cap) return BZ_E_CAPACITY;
        HIPCHK(hipMemcpyAsync(d_out + nhead, w->stream.p, body, hipMemcpyDeviceToDevice, st));
        if (nhead) HIPCHK(hipMemcpyAsync(d_out, head, nhead, hipMemcpyHostToDevice, st)); // (`head` and `tail` live on this stack frame: the wait below)
        if (ntail) HIPCHK(hipMemcpyAsync(d_out + nhead + body, tail, ntail, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipEventRecord(w->ev[6], st));
    HIPCHK(hipStreamSynchronize(st));
    df_stage_times(w, w->t_stage, false);
    // statistics of the last call (tests, bench): counted by k_df_part_tail; the block list itself is fetched when asked for
    w->h_nb = nb;
    w->h_fetched = false;
    const u64 prev_bytes = seg.accumulate_stats ? w->stats[5] : 0;
    if (!seg.accumulate_stats) memset(w->stats, 0, sizeof(w->stats));
    w->stats[0] += nb;
    w->stats[1] += pres.st[0];
    w->stats[2] += pres.st[1];
    w->stats[3] += pres.st[2];
    w->stats[4] += pres.st[3];
    w->stats[6] += pres.st[4];
    w->stats[5] = prev_bytes + need;
    if (dl_out) *dl_out = nb ? (u32)((nb == 1 ? seg.dl0 : 0u) + (n - pres.last_bstart)) : seg.dl0;
    return BZ_OK;
}

// A segment of any length: parts of at most BZ_DF_PART_MIB (default 1024 MiB) positions each, so that
// positions and bit offsets stay inside 32 bits.  A part that is not the last one is handed kPartGuard bytes
// of look-ahead and writes the blocks that cannot change any more; the next part starts at the first block it
// left out (a code start: the lazy parse from a code start does not depend on what came before,
// lzss/encoder.rs:132-184), with the 32 KiB in front of it as history and in the middle of the byte its
// predecessor ended in.  The bytes are those of one pass over the whole segment.
static bool df_trace()
{
    static const bool on = getenv("BZ_DF_TRACE") != nullptr; // (diagnostics: a line per part and per one-shot call)
    return on;
}
static u64 df_part_bytes()
{
    static const u64 v = [] {
        const char *s = getenv("BZ_DF_PART_MIB");
        long mib = s ? atol(s) : 1024;
        if (mib < 1) mib = 1;
        if (mib > 1536) mib = 1536;
        return (u64)mib << 20;
    }();
    return v;
}

// The one-shot call over host buffers runs its parts beside its own copies (df_encode_buffer_dict): a part may start once
// its bytes have been uploaded (need_input: "bytes [0, upto) of the segment must be on the device"), and its bytes of the
// stream leave for the host while the next part is encoded (part_done: "stream bytes [off, off + len) are final").
struct DfPartHooks {
    u64 part_bytes = 0; // 0: BZ_DF_PART_MIB
    u64 first_part_bytes = 0; // (if not 0) the first part's size: short, so that the kernels start behind a short upload
    std::function<int(u64 upto)> need_input;
    std::function<void(size_t off, size_t len)> part_done;
};

static int df_encode_parts(bz_gpu_engine *g, int kind, const u8 *d_in, u64 n, const u8 *dict, size_t dict_len, u8 *d_out,
                           size_t cap, size_t *out_len, const DfSeg &seg0 = DfSeg(), u32 *dl_out = nullptr,
                           const DfPartHooks *hooks = nullptr)
{
    const u64 part_all = hooks && hooks->part_bytes ? hooks->part_bytes : df_part_bytes();
    const u64 part_first = hooks && hooks->first_part_bytes ? std::min<u64>(hooks->first_part_bytes, part_all) : part_all;
    if (n <= part_first + kPartGuard) {
        if (hooks && hooks->need_input) {
            const int irc = hooks->need_input(n);
            if (irc != BZ_OK) return irc;
        }
        const int rc = df_encode_core(g, kind, d_in, n, dict, dict_len, d_out, cap, out_len, seg0, dl_out);
        if (rc == BZ_OK && hooks && hooks->part_done) hooks->part_done(0, *out_len);
        return rc;
    }
    u64 pos = 0;
    size_t written = 0;
    DfSeg seg = seg0;
    *out_len = 0;
    for (u32 k = 0;; ++k) {
        const u64 left = n - pos;
        const u64 part = k == 0 ? part_first : part_all;
        const bool last = left <= part + kPartGuard;
        const u64 len = last ? left : part + kPartGuard;
        seg.prior = seg0.prior + pos;
        seg.dl0 = pos ? 0u : seg0.dl0; // (a part starts at a block start)
        seg.head = seg0.head && pos == 0;
        seg.tail = seg0.tail && last;
        seg.final = seg0.final;
        seg.more = !last;
        seg.run = seg0.run && last;
        seg.accumulate_stats = k > 0;
        size_t got = 0;
        DfPartOut po;
        const double t_part = now_ms();
        if (hooks && hooks->need_input) {
            const int irc = hooks->need_input(std::min<u64>(n, pos + len + 64));
            if (irc != BZ_OK) return irc;
        }
        const double t_in = now_ms();
        const int rc = df_encode_core(g, kind, d_in + pos, len, dict, dict_len, d_out ? d_out + written : nullptr,
                                      d_out ? cap - written : 0, &got, seg, last ? dl_out : nullptr, &po);
        if (rc != BZ_OK) return rc;
        if (hooks && hooks->part_done && d_out) hooks->part_done(written, got);
        if (df_trace())
            fprintf(stderr, "bz2_mi355x: deflate part %u: input [%llu, +%llu) of %llu, kept %llu bytes of it, %zu stream bytes, "
                            "%u bits handed on, %llu blocks; waited for its input %.2f ms, call %.2f ms of which kernels %.2f (at %.1f)\n", k, (unsigned long long)pos, (unsigned long long)len,
                    (unsigned long long)n, (unsigned long long)(last ? len : po.consumed), got, last ? 0u : po.end_bits,
                    (unsigned long long)g->df->h_nb, t_in - t_part, now_ms() - t_in, g->df->t_stage[5] * 1e3, now_ms());
        written += got;
        *out_len = written;
        if (last) return BZ_OK;
        pos += po.consumed;
        seg.skip = po.skip;
        seg.bit0 = po.end_bits;
        seg.carry_byte = po.end_byte;
    }
}

// ---- many inputs in one call ----------------------------------------------------------------------------------
// An input of at most kBlockMax bytes is exactly one block (InflaterInner::next closes a block only when the next code would
// take it past 0xFFFF bytes, deflate/encoder.rs:577-597): it starts at the input's first byte with decompress_len 0 -- with
// a preset dictionary too (InflaterInner::with_dict, :293-308: the dictionary is history, not output) -- and is final.
// Such inputs are encoded together, a sub-batch at a time: gathered into an image with every input at a multiple of kPTile,
// one pass of the chain sort, the match kernel (slot rules: k_df_match2<true>), the parse and one block per input; the
// streams' places come from a scan on the device, the containers are written there too, and the host looks at the device
// once per sub-batch.  Every other input goes through df_encode_parts, in its turn.
// A preset dictionary (df_gpu_encode_batch_device_dict): its last W <= 32768 bytes go to the device once per call and into
// the image in front of EVERY input (DfBatchDict; k_deflate.h "window tiles") -- df_encode_core's history layout, once per slot.
u64 df_batch_image_bytes() // (lzhuf_engine.hip sizes its sub-batches by it too)
{
    const char *s = getenv("BZ_DF_BATCH_MIB"); // slot image per sub-batch (a fraction is taken too), read per call
    double mib = s ? atof(s) : 64.0;
    if (!(mib >= 1.0 / 16)) mib = 1.0 / 16; // (16 tiles; a slot has up to 16, with a dictionary's window up to 24: the first
                                            // input of a sub-batch is admitted whatever the limit)
    if (mib > 1024) mib = 1024;
    return (u64)(mib * 1048576.0);
}
constexpr u32 kBatchSlots = 8192; // inputs per sub-batch at most (k_df_block's scratch is 147 KB per block)
static u32 df_slot_tiles(u64 n) { return n ? (u32)((n + kPTile - 1) / kPTile) : 1u; } // (the input's tiles)

// the dictionary of a batch call as its sub-batches see it; W == 0: none
struct DfBatchDict {
    const u8 *d_win = nullptr; // the window right-aligned in kWin bytes of device memory, zeros in front of it
    u32 W = 0;                 // min(dict_len, 32768)
    u32 wtiles = 0;            // window tiles in front of every slot's input tiles
    u32 dictid = 0;            // Adler-32 of the whole dictionary
};
static int df_batch_window(bz_gpu_engine *g, DfWorkspace *w, const uint8_t *dict, size_t dict_len, DfBatchDict &bd)
{
    bd = DfBatchDict{};
    if (!dict_len) return BZ_OK;
    const u32 W = (u32)std::min<size_t>(dict_len, kWin);
    const int rc = w->b_win.ensure(kWin);
    if (rc != BZ_OK) return rc;
    if (W < kWin) HIPCHK(hipMemsetAsync(w->b_win.p, 0, kWin - W, g->st));
    HIPCHK(hipMemcpyAsync(w->b_win.as<u8>() + (kWin - W), dict + (dict_len - W), W, hipMemcpyHostToDevice, g->st));
    bd.d_win = w->b_win.as<u8>();
    bd.W = W;
    bd.wtiles = (W + kPTile - 1) / kPTile;
    bd.dictid = df_adler32_host(dict, dict_len);
    return BZ_OK;
}

// inputs [first, first + ns) of the call, all of at most kBlockMax bytes, ntiles tiles together (window tiles included); their
// streams go to d_out + cursor .. in input order, *used = bytes taken there (a multiple of 4)
// bgzf (df_gpu_bgzf_encode_device; kind 2, no dictionary): the inputs are cuts of one buffer at any byte offset, the streams are
// BGZF blocks side by side without padding (*used is their bytes, d_out + cursor has any alignment) and no block is a dynamic
// one without a match; the block kinds are counted into bgzf_stats[2..6]
static int df_batch_run(bz_gpu_engine *g, int kind, const u8 *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len, size_t first,
                        u32 ns, u32 ntiles, const DfBatchDict &bd, u8 *d_out, size_t cap, u64 cursor, uint64_t *h_out_off,
                        uint64_t *h_out_len, u64 *used, double t_acc[6], bool bgzf = false)
{
    DfWorkspace *w = g->df;
    hipStream_t st = g->st;
    const u64 nimg = (u64)ntiles * kPTile;
    std::vector<DfSlot> slots(ns);
    std::vector<u32> tile_slot(ntiles);
    std::vector<u64> bse(2 * (size_t)ns);
    size_t bound = 0;
    {
        u32 t = 0;
        for (u32 j = 0; j < ns; ++j) {
            const u64 n = h_in_len[first + j];
            slots[j].src = h_in_off[first + j];
            slots[j].lo = (t + bd.wtiles) * kPTile;
            slots[j].len = (u32)n;
            bse[2 * (size_t)j] = slots[j].lo;
            bse[2 * (size_t)j + 1] = slots[j].lo + n;
            for (u32 k = bd.wtiles + df_slot_tiles(n); k; --k) tile_slot[t++] = j;
            bound += bgzf ? (size_t)n + 31u : (df_encode_bound((size_t)n) + 3u) & ~(size_t)3;
        }
    }
    int rc;
    if ((rc = df_reserve_pipeline(w, nimg, ntiles, ns, bound)) != BZ_OK) return rc;
    if ((rc = w->concat.ensure(nimg + 64)) != BZ_OK) return rc;                            // the image
    if ((rc = w->tabs.ensure((size_t)ntiles * kEntries * 2 + 64)) != BZ_OK) return rc;
    if ((rc = w->ents.ensure(((size_t)ntiles + 8) * 2 + 64)) != BZ_OK) return rc;
    if ((rc = w->b_slots.ensure((size_t)ns * sizeof(DfSlot))) != BZ_OK) return rc;
    if ((rc = w->b_tile_slot.ensure((size_t)ntiles * 4)) != BZ_OK) return rc;
    if ((rc = w->b_bse.ensure((size_t)ns * 16)) != BZ_OK) return rc;
    if ((rc = w->b_outs.ensure((size_t)ns * sizeof(DfBatchOut))) != BZ_OK) return rc;
    if ((rc = w->b_stats.ensure(64)) != BZ_OK) return rc;
    u8 *image = w->concat.as<u8>();
    u32 *M = w->vals_in.as<u32>(), *code = w->vals_out.as<u32>();
    const DfSlot *d_slots = w->b_slots.as<DfSlot>();
    const u32 *d_tile_slot = w->b_tile_slot.as<u32>();
    const u64 *d_bse = w->b_bse.as<u64>();
    const u32 head = bgzf ? 18u : kind == 1 ? (bd.W ? 6u : 2u) : (kind == 2 ? 10u : 0u), tail = kind == 1 ? 4u : (kind == 2 ? 8u : 0u);
    const u32 ns_word = ns;
    // (the host arrays live on this stack frame: the wait below)
    HIPCHK(hipMemcpyAsync(w->b_slots.p, slots.data(), (size_t)ns * sizeof(DfSlot), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->b_tile_slot.p, tile_slot.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->b_bse.p, bse.data(), (size_t)ns * 16, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->nb.p, &ns_word, 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(w->b_stats.p, 0, 64, st));
    HIPCHK(hipEventRecord(w->ev[0], st));
    HIPCHK(hipMemsetAsync(w->stream.p, 0, bound + 64, st));
    if ((bgzf ? df_launch_gather_cut(st, d_in, d_slots, d_tile_slot, ntiles, image)
              : df_launch_gather(st, d_in, d_slots, d_tile_slot, ntiles, image, bd.d_win)) != 0)
        return BZ_E_UNEXPECTED;
    if (df_launch_chains(st, image, nimg, w->vals_in.as<u32>(), w->vals_out.as<u32>(), nullptr, w->sort_tmp.as<u32>(), w->keys_out.as<u32>(),
                         nullptr) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[1], st));
    if (df_launch_match2_batch(st, image, nimg, w->vals_out.as<u32>(), M, d_tile_slot, d_slots, bd.W) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[2], st));
    if (df_launch_parse_batch(st, M, nimg, ntiles, d_slots, ns, bd.wtiles, w->keys_in.as<u16>(), w->tabs.as<u16>(), w->ents.as<u16>(),
                              code, w->bitmap.as<u64>(), w->canon.as<u64>()) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[3], st));
    if ((bgzf ? df_launch_blocks_strict : df_launch_blocks_batch)(st, image, code, d_bse, w->nb.as<u32>(), ns, w->blocks.as<DfBlock>(),
                                                                  w->lens.as<u8>(), w->hdr.as<u32>(), w->lm.as<u32>()) != 0)
        return BZ_E_UNEXPECTED;
    if ((bgzf ? df_launch_exact_offsets : df_launch_batch_offsets)(st, w->blocks.as<DfBlock>(), ns, head, tail, w->b_outs.as<DfBatchOut>(),
                                                                   w->total.as<u64>()) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[4], st));
    if (df_launch_emit_batch(st, image, code, d_bse, w->nb.as<u32>(), ns, w->blocks.as<DfBlock>(), w->lens.as<u8>(), w->hdr.as<u32>(),
                             w->stream.as<u32>()) != 0)
        return BZ_E_UNEXPECTED;
    if ((bgzf ? df_launch_bgzf_wrap(st, image, d_slots, ns, w->blocks.as<DfBlock>(), w->b_outs.as<DfBatchOut>(), df_crc_shifts(),
                                    w->stream.as<u8>(), w->b_stats.as<u32>())
              : df_launch_batch_wrap(st, image, d_slots, ns, w->blocks.as<DfBlock>(), w->b_outs.as<DfBatchOut>(), kind, df_crc_shifts(),
                                     w->stream.as<u8>(), w->b_stats.as<u32>(), bd.W != 0, bd.dictid)) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[5], st));
    std::vector<DfBatchOut> outs(ns);
    u64 total = 0;
    u32 bst[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(outs.data(), w->b_outs.p, (size_t)ns * sizeof(DfBatchOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, w->total.p, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(bst, w->b_stats.p, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one look at the device per sub-batch
    HIPCHK(hipGetLastError());
    if (total > bound) return BZ_E_UNEXPECTED;
    if (cursor + total > cap) return BZ_E_CAPACITY;
    if (total) HIPCHK(hipMemcpyAsync(d_out + cursor, w->stream.p, (size_t)total, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipEventRecord(w->ev[6], st));
    for (u32 j = 0; j < ns; ++j) {
        h_out_off[first + j] = cursor + outs[j].off;
        h_out_len[first + j] = outs[j].len;
    }
    for (int i = 0; i < 5; ++i) (bgzf ? w->bgzf_stats[2 + i] : w->batch_stats[3 + i]) += bst[i];
    HIPCHK(hipStreamSynchronize(st)); // (the workspace is free for the next sub-batch, the events are over)
    df_stage_times(w, t_acc, true);
    *used = total;
    return BZ_OK;
}

extern "C" size_t df_encode_batch_bound(const uint64_t *in_len, size_t count)
{
    size_t s = 0;
    for (size_t i = 0; in_len && i < count; ++i) s += (df_encode_bound((size_t)in_len[i]) + 3u) & ~(size_t)3;
    return s;
}

extern "C" int df_gpu_last_batch_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->batch_stats[i] : 0;
    return BZ_OK;
}

extern "C" int df_gpu_encode_batch_device(bz_gpu_engine *g, int kind, const void *d_in, const uint64_t *h_in_off,
                                          const uint64_t *h_in_len, size_t count, void *d_out, size_t cap, uint64_t *h_out_off,
                                          uint64_t *h_out_len)
{
    return df_gpu_encode_batch_device_dict(g, kind, d_in, h_in_off, h_in_len, count, nullptr, 0, d_out, cap, h_out_off, h_out_len);
}

extern "C" int df_gpu_encode_batch_device_dict(bz_gpu_engine *g, int kind, const void *d_in, const uint64_t *h_in_off,
                                               const uint64_t *h_in_len, size_t count, const uint8_t *dict, size_t dict_len,
                                               void *d_out, size_t cap, uint64_t *h_out_off, uint64_t *h_out_len)
{
    if (!g || kind < 0 || kind > 2) return BZ_E_PARAM;
    if (df_dict_param(kind, dict, dict_len) != BZ_OK) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !d_out) return BZ_E_PARAM;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 3u)) return BZ_E_PARAM;
    u64 in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 15u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i]) return BZ_E_PARAM;
        in_end = h_in_off[i] + h_in_len[i];
    }
    if (in_end && !d_in) return BZ_E_PARAM;
    DfWorkspace *w = nullptr;
    const int wrc = df_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    for (u64 &s : w->batch_stats) s = 0;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    u8 *out8 = static_cast<u8 *>(d_out);
    const u64 image_max = df_batch_image_bytes();
    DfBatchDict bd;
    const int drc = df_batch_window(g, w, dict, dict_len, bd);
    if (drc != BZ_OK) return drc;
    double t_acc[6] = {0, 0, 0, 0, 0, 0};
    u64 cursor = 0;
    bool batched = false;
    for (size_t i = 0; i < count;) {
        if (h_in_len[i] > kBlockMax) { // more than one block: the one-input path, in its place
            size_t got = 0;
            if (cursor > cap) return BZ_E_CAPACITY;
            const int rc = df_encode_parts(g, kind, in8 + h_in_off[i], h_in_len[i], dict, dict_len, out8 + cursor, cap - cursor, &got);
            if (rc != BZ_OK) return rc;
            const u64 slot = ((u64)got + 3u) & ~(u64)3;
            if (cursor + slot > cap) return BZ_E_CAPACITY;
            if (slot > got) HIPCHK(hipMemsetAsync(out8 + cursor + got, 0, (size_t)(slot - got), g->st));
            h_out_off[i] = cursor;
            h_out_len[i] = got;
            cursor += slot;
            w->batch_stats[1] += 1;
            ++i;
            continue;
        }
        size_t j = i;
        u64 tiles = 0;
        while (j < count && h_in_len[j] <= kBlockMax && j - i < kBatchSlots &&
               (j == i || (tiles + bd.wtiles + df_slot_tiles(h_in_len[j])) * kPTile <= image_max)) {
            tiles += bd.wtiles + df_slot_tiles(h_in_len[j]);
            ++j;
        }
        u64 used = 0;
        const int rc = df_batch_run(g, kind, in8, h_in_off, h_in_len, i, (u32)(j - i), (u32)tiles, bd, out8, cap, cursor, h_out_off,
                                    h_out_len, &used, t_acc);
        if (rc != BZ_OK) return rc;
        cursor += used;
        w->batch_stats[0] += j - i;
        w->batch_stats[2] += 1;
        batched = true;
        i = j;
    }
    HIPCHK(hipStreamSynchronize(g->st));
    if (batched) { // df_gpu_last_timings: the stages of the batch path, summed over the sub-batches
        for (int k = 0; k < 6; ++k) w->t_stage[k] = t_acc[k];
        w->h_nb = 0; // (df_gpu_debug_blocks describes one-stream calls)
        w->h_fetched = true;
        w->h_blocks.clear();
        w->h_bstart.assign(1, 0);
    }
    return BZ_OK;
}

// ---- a BGZF file (section 7 of the header): the batch path over cuts of one contiguous input --------------------------
// Block k is the bytes [k * B, min(n, (k + 1) * B)) and a gzip member of its own: the 18-byte BGZF header, one final Deflate
// block, CRC-32 and ISIZE.  The members of a sub-batch come out of df_batch_run side by side, without padding, and are placed
// at the running byte total; the EOF marker follows the last one.
static const u8 kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

static int df_bgzf_params(size_t n, const void *in, uint32_t block_bytes)
{
    return block_bytes > DF_BGZF_BLOCK || (n && !in) ? BZ_E_PARAM : BZ_OK;
}

extern "C" size_t df_bgzf_block_count(size_t n, uint32_t block_bytes)
{
    const size_t B = block_bytes && block_bytes <= DF_BGZF_BLOCK ? block_bytes : DF_BGZF_BLOCK;
    return n / B + (n % B ? 1 : 0);
}

extern "C" size_t df_bgzf_bound(size_t n, uint32_t block_bytes, int eof)
{
    return n + 31 * df_bgzf_block_count(n, block_bytes) + (eof ? sizeof kBgzfEof : 0);
}

extern "C" int df_gpu_last_bgzf_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->bgzf_stats[i] : 0;
    return BZ_OK;
}

extern "C" int df_gpu_bgzf_encode_device(bz_gpu_engine *g, const void *d_in, size_t n, uint32_t block_bytes, int eof, void *d_out,
                                         size_t cap, uint64_t *out_len, uint64_t *h_block_off)
{
    if (!g || !out_len || df_bgzf_params(n, d_in, block_bytes) != BZ_OK || ((uintptr_t)d_in & 15u)) return BZ_E_PARAM;
    const size_t marker = eof ? sizeof kBgzfEof : 0;
    if ((n || marker) && !d_out) return cap ? BZ_E_PARAM : BZ_E_CAPACITY;
    DfWorkspace *w = nullptr;
    const int wrc = df_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    for (u64 &s : w->bgzf_stats) s = 0;
    const u64 B = block_bytes ? block_bytes : DF_BGZF_BLOCK;
    const u64 count = df_bgzf_block_count(n, block_bytes);
    const u8 *in8 = static_cast<const u8 *>(d_in);
    u8 *out8 = static_cast<u8 *>(d_out);
    const u64 image_max = df_batch_image_bytes();
    const u32 slot_tiles = df_slot_tiles(B); // (the last block may take fewer)
    const DfBatchDict bd;
    std::vector<uint64_t> in_off, in_len, o_off, o_len;
    double t_acc[6] = {0, 0, 0, 0, 0, 0};
    u64 cursor = 0;
    for (u64 k = 0; k < count;) {
        u64 ns = std::max<u64>(1, image_max / ((u64)slot_tiles * kPTile));
        ns = std::min<u64>(std::min<u64>(ns, kBatchSlots), count - k);
        in_off.resize(ns); in_len.resize(ns); o_off.resize(ns); o_len.resize(ns);
        u64 tiles = 0;
        for (u64 j = 0; j < ns; ++j) {
            in_off[j] = (k + j) * B;
            in_len[j] = std::min<u64>(B, n - in_off[j]);
            tiles += df_slot_tiles(in_len[j]);
        }
        u64 used = 0;
        const int rc = df_batch_run(g, 2, in8, in_off.data(), in_len.data(), 0, (u32)ns, (u32)tiles, bd, out8, cap, cursor, o_off.data(),
                                    o_len.data(), &used, t_acc, true);
        if (rc != BZ_OK) return rc;
        if (h_block_off)
            for (u64 j = 0; j < ns; ++j) h_block_off[k + j] = o_off[j];
        cursor += used;
        w->bgzf_stats[1] += 1;
        k += ns;
    }
    if (cursor + marker > cap) return BZ_E_CAPACITY;
    if (marker) HIPCHK(hipMemcpyAsync(out8 + cursor, kBgzfEof, marker, hipMemcpyHostToDevice, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    if (h_block_off) h_block_off[count] = cursor;
    w->bgzf_stats[0] = count;
    w->bgzf_stats[7] = cursor + marker;
    *out_len = cursor + marker;
    if (count) { // df_gpu_last_timings: the stages of the batch path, summed over the sub-batches
        for (int i = 0; i < 6; ++i) w->t_stage[i] = t_acc[i];
        w->h_nb = 0; // (df_gpu_debug_blocks describes one-stream calls)
        w->h_fetched = true;
        w->h_blocks.clear();
        w->h_bstart.assign(1, 0);
    }
    return BZ_OK;
}

// ---- the host-to-host forms: an engine of the cache for the length of the call (EngineLease, host_call.h); the forms that
// are one upload, one device call and one download are their own checks and that call inside one_shot() (one_shot.h) ----
// Many inputs: packed at 16-byte-aligned offsets (BatchLayout), one upload, one device call, one download.
extern "C" int df_encode_batch(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t **out,
                               uint64_t *out_off, uint64_t *out_len)
{
    return df_encode_batch_dict(kind, device, ins, lens, count, nullptr, 0, out, out_off, out_len);
}

extern "C" int df_encode_batch_dict(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count, const uint8_t *dict,
                                    size_t dict_len, uint8_t **out, uint64_t *out_off, uint64_t *out_len)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (kind < 0 || kind > 2) return BZ_E_PARAM;
    if (df_dict_param(kind, dict, dict_len) != BZ_OK) return BZ_E_PARAM;
    if (count && (!ins || !lens || !out_off || !out_len)) return BZ_E_PARAM;
    const BatchLayout lay(ins, lens, count, 16);
    if (lay.status != BZ_OK) return lay.status;
    if (count == 0) return one_shot_empty(out);
    const size_t cap = df_encode_batch_bound(lay.in_len.data(), count);
    return one_shot(device, 2, lay, cap, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int rc = df_gpu_encode_batch_device_dict(g, kind, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), count, dict, dict_len,
                                                       g->oneshot_out.p, cap, out_off, out_len);
        if (rc == BZ_OK) *total = (size_t)(out_off[count - 1] + ((out_len[count - 1] + 3u) & ~(u64)3));
        return rc;
    });
}

// A BGZF file from host memory: one upload, df_gpu_bgzf_encode_device on an engine of the cache, one download.
extern "C" int df_bgzf_encode_buffer(int device, const uint8_t *in, size_t n, uint32_t block_bytes, int eof, uint8_t **out, size_t *out_len,
                                     uint64_t *block_off)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (!out_len || df_bgzf_params(n, in, block_bytes) != BZ_OK) return BZ_E_PARAM;
    *out_len = 0;
    if (n == 0) { // the marker alone, or nothing: no device is touched
        const size_t m = eof ? sizeof kBgzfEof : 0;
        uint8_t *h = (uint8_t *)malloc(m ? m : 1);
        if (!h) return BZ_E_NOMEM;
        memcpy(h, kBgzfEof, m);
        if (block_off) block_off[0] = 0;
        *out = h;
        *out_len = m;
        return BZ_OK;
    }
    const size_t cap = df_bgzf_bound(n, block_bytes, eof);
    uint64_t made = 0;
    const int rc = one_shot(device, 2, OneShotIn(in, n), cap, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int drc = df_gpu_bgzf_encode_device(g, g->dec_in.p, n, block_bytes, eof, g->oneshot_out.p, cap, &made, block_off);
        *total = (size_t)made;
        return drc;
    });
    if (rc == BZ_OK) *out_len = (size_t)made;
    return rc;
}

// ---- decode of many streams (section 5 of the header; kernels: k_inflate.hip) -------------------------------
extern "C" int df_gpu_last_decode_batch_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->inf_stats[i] : 0;
    return BZ_OK;
}


// ---- one large entry across many waves (inf_split.h; DESIGN_deflate.md "One large stream across many waves") ----------
// An entry of BZ_DF_INF_SPLIT_KIB or more compressed bytes is cut into pieces of BZ_DF_INF_PIECE_KIB; both are read per call.
static u64 df_env_kib(const char *name, u64 dflt)
{
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    return end == s ? dflt : (u64)v;
}
extern "C" int df_gpu_last_decode_split_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->split_stats[i] : 0;
    return BZ_OK;
}

extern "C" int df_gpu_last_decode_split_timings(bz_gpu_engine *g, double out_seconds[7])
{
    if (!g || !out_seconds) return BZ_E_PARAM;
    for (int i = 0; i < 7; ++i) out_seconds[i] = g->df ? g->df->split_ms[i] * 1e-3 : 0.0;
    return BZ_OK;
}

struct DfSplitEntry {
    size_t index = 0;           // of the entry in the call
    std::vector<DfPiece> chain; // the confirmed pieces in stream order, each with its place in the entry's output and its length
    DfInfRec rec;               // what the one-wave path would have left for the entry
    // its share of df_gpu_last_decode_split_stats and of the phases search, sizes, repair: counted in once the entry is
    // known to stay split
    u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double ms[3] = {0, 0, 0};
};

// the sizes launch over n pieces, and their records
static int df_split_pieces(bz_gpu_engine *g, DfWorkspace *w, int kind, const u8 *ebase, u32 elen, DfWindow win, const DfPiece *pcs, u32 n,
                           DfPieceRec *out, u64 *launches)
{
    int rc = w->s_piece.ensure((size_t)n * sizeof(DfPiece));
    if (rc == BZ_OK) rc = w->s_prec.ensure((size_t)n * sizeof(DfPieceRec));
    if (rc != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->s_piece.p, pcs, (size_t)n * sizeof(DfPiece), hipMemcpyHostToDevice, g->st));
    DfPieceRec *d_rec = w->s_prec.as<DfPieceRec>();
    if (df_launch_inflate_piece(g->st, false, ebase, elen, kind, w->s_piece.as<DfPiece>(), n, d_rec, nullptr, nullptr, win) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipMemcpyAsync(out, w->s_prec.p, (size_t)n * sizeof(DfPieceRec), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    *launches += 1;
    return BZ_OK;
}

// Search, sizes, chain and repair of one entry.  *fallback: the entry takes the one-wave path (an output of 2 GiB or more).
static int df_split_sizes(bz_gpu_engine *g, DfWorkspace *w, int kind, const u8 *ebase, u32 elen, DfWindow win, DfSplitEntry &e, bool *fallback)
{
    using namespace infsplit;
    *fallback = false;
    u64 piece = df_env_kib("BZ_DF_INF_PIECE_KIB", 16);
    piece = (piece < 1 ? 1 : piece > (1u << 20) ? (1u << 20) : piece) * 1024;
    while (elen / piece > (1u << 20)) piece *= 2;
    const u32 npieces = (u32)((elen + piece - 1) / piece);
    double t0 = now_ms();
    std::vector<Cand> cands;
    int rc;
    if (npieces > 1) {
        std::vector<Cand> all(npieces - 1);
        if ((rc = w->s_cand.ensure(all.size() * sizeof(Cand))) != BZ_OK) return rc;
        if (df_launch_split_search(g->st, ebase, elen, (u32)piece, npieces, w->s_cand.p) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(all.data(), w->s_cand.p, all.size() * sizeof(Cand), hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        e.st[7] += 1;
        for (const Cand &c : all)
            if (c.pos != kNoStop) cands.push_back(c);
    }
    e.st[1] += cands.size();
    double t1 = now_ms();
    e.ms[0] += t1 - t0;
    // every piece at once: the entry's first bit and every candidate, each to the next candidate
    std::vector<DfPiece> pcs(1 + cands.size());
    for (size_t k = 0; k < pcs.size(); ++k) {
        DfPiece &q = pcs[k];
        q.start = k ? cands[k - 1].pos : 0;
        q.stop = k < cands.size() ? cands[k].pos : kNoStop;
        q.mode = k ? cands[k - 1].mode : 2u;
        q.base = k ? kBaseUnknown : 0u;
        q.len = q.pad = 0;
    }
    std::vector<DfPieceRec> prs(pcs.size());
    if ((rc = df_split_pieces(g, w, kind, ebase, elen, win, pcs.data(), (u32)pcs.size(), prs.data(), &e.st[7])) != BZ_OK) return rc;
    t0 = now_ms();
    e.ms[1] += t0 - t1;
    // the chain: a candidate's piece counts if and only if the confirmed piece in front of it ended exactly there
    std::vector<DfPieceRec> crec;
    e.chain.clear();
    DfPiece cur = pcs[0];
    DfPieceRec cr = prs[0];
    u64 j = 0;
    u32 repairs = 0;
    for (;;) {
        e.chain.push_back(cur);
        crec.push_back(cr);
        const PieceEnd end{cr.r.end_bit, cr.end_mode, cr.ended != 0};
        u64 stop = kNoStop;
        const Next nx = chain_next(cands.data(), cands.size(), end, repairs, j, stop);
        if (nx == Next::Done) break;
        if (nx == Next::Confirmed) {
            cur = pcs[1 + j];
            cr = prs[1 + j];
            ++j;
            e.st[2] += 1;
            continue;
        }
        cur = DfPiece{end.pos, stop, end.mode, kBaseUnknown, 0, 0};
        if ((rc = df_split_pieces(g, w, kind, ebase, elen, win, &cur, 1, &cr, &e.st[7])) != BZ_OK) return rc;
        if (nx == Next::Repair) {
            ++repairs;
            e.st[3] += 1;
        } else e.st[4] += cr.r.len; // the serial tail
    }
    e.st[2] += 1; // (the first piece)
    // the pieces' places; a piece whose matches reach further back than its place and the window in front of the entry is
    // decoded once more knowing it: the stream ends at the failing code
    u64 sum = 0;
    for (size_t k = 0; k < e.chain.size(); ++k) {
        if (sum >= (1ull << 31)) break;
        e.chain[k].base = (u32)sum;
        if (k > 0 && crec[k].reach > sum + win.W) {
            if ((rc = df_split_pieces(g, w, kind, ebase, elen, win, &e.chain[k], 1, &crec[k], &e.st[7])) != BZ_OK) return rc;
            if (!crec[k].ended || crec[k].r.verdict == BZ_OK) return BZ_E_UNEXPECTED;
            e.chain.resize(k + 1);
            crec.resize(k + 1);
        }
        e.chain[k].len = crec[k].r.len;
        sum += crec[k].r.len;
        if (crec[k].r.flags & 1u) sum = 1ull << 32;
    }
    e.ms[2] += now_ms() - t0;
    if (sum >= (1ull << 31)) {
        *fallback = true;
        return BZ_OK;
    }
    e.rec = crec.back().r;
    e.rec.len = (u32)sum;
    for (int b = 0; b < 3; ++b) {
        e.rec.nblk[b] = 0;
        for (const DfPieceRec &q : crec) e.rec.nblk[b] += q.r.nblk[b];
    }
    e.st[0] = 1;
    return BZ_OK;
}

// The bytes of one split entry at `eout`: the writing launch with its source map, pointer jumping, the gather; for kinds 1 / 2
// the checksum of a clean stream, folded piecewise (k_df_sums) and combined here as df_encode_core combines it.
static int df_split_write(bz_gpu_engine *g, DfWorkspace *w, int kind, const u8 *ebase, u32 elen, DfWindow win, u8 *eout, DfSplitEntry &e)
{
    const u32 n = e.rec.len, np = (u32)e.chain.size();
    u32 *map = w->s_map.as<u32>(), *cnt = w->s_cnt.as<u32>();
    int rc = w->s_piece.ensure((size_t)np * sizeof(DfPiece));
    if (rc != BZ_OK) return rc;
    const double t0 = now_ms();
    HIPCHK(hipMemcpyAsync(w->s_piece.p, e.chain.data(), (size_t)np * sizeof(DfPiece), hipMemcpyHostToDevice, g->st));
    if (df_launch_inflate_piece(g->st, true, ebase, elen, kind, w->s_piece.as<DfPiece>(), np, nullptr, eout, map, win) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipStreamSynchronize(g->st));
    w->split_stats[7] += 1;
    w->split_ms[3] += now_ms() - t0;
    SplitTail t;
    rc = split_jump_gather(g->st, n && np > 1, map, n, cnt, eout, t); // (one piece: every byte is in its place)
    w->split_stats[7] += t.launches;
    w->split_stats[6] += t.rounds;
    w->split_stats[5] += t.left;
    w->split_ms[4] += t.jump_ms;
    w->split_ms[5] += t.gather_ms;
    if (rc != BZ_OK) return rc;
    const double t1 = now_ms();
    if (kind == 0 || e.rec.verdict != BZ_OK) return BZ_OK;
    const u32 npieces = (u32)(((u64)n + kSumPiece - 1) / kSumPiece);
    if ((rc = w->asum.ensure((size_t)(npieces + 1) * 8)) != BZ_OK) return rc;
    if ((rc = w->bsum.ensure((size_t)(npieces + 1) * 8)) != BZ_OK) return rc;
    if ((rc = w->crc.ensure((size_t)(npieces + 1) * 4 + 256 * 4)) != BZ_OK) return rc;
    std::vector<u64> a(npieces), b(npieces);
    std::vector<u32> c((size_t)npieces + 1 + 256);
    if (npieces) {
        if (df_launch_sums(g->st, eout, n, w->asum.as<u64>(), w->bsum.as<u64>(), w->crc.as<u32>(), w->crc.as<u32>() + npieces + 1, df_crc_shifts()) != 0)
            return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(a.data(), w->asum.p, (size_t)npieces * 8, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipMemcpyAsync(b.data(), w->bsum.p, (size_t)npieces * 8, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipMemcpyAsync(c.data(), w->crc.p, c.size() * 4, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        w->split_stats[7] += 1;
    }
    bool ok;
    if (kind == 1) {
        u64 A = 1, B = 0;
        for (u32 t = 0; t < npieces; ++t) {
            const u64 len = (t + 1 == npieces) ? n - (u64)t * kSumPiece : kSumPiece;
            B = (B + (len % 65521) * A + b[t]) % 65521;
            A = (A + a[t]) % 65521;
        }
        ok = (u32)((B << 16) | A) == e.rec.check;
    } else {
        const u32 xpiece = gf_xpow8_reflected(kSumPiece);
        u32 raw = 0;
        for (u32 t = 0; t < npieces; ++t) {
            const u64 len = (t + 1 == npieces) ? n - (u64)t * kSumPiece : kSumPiece;
            if (len == kSumPiece) raw = gf_mul_reflected(raw, xpiece) ^ c[t];
            else
                for (u32 s = 0; (u64)s * 256 < len; ++s) {
                    const u64 sl = (len - (u64)s * 256) < 256 ? (len - (u64)s * 256) : 256;
                    raw = gf_mul_reflected(raw, gf_xpow8_reflected(sl)) ^ c[(size_t)npieces + 1 + s];
                }
        }
        ok = (raw ^ gf_mul_reflected(0xFFFFFFFFu, gf_xpow8_reflected(n)) ^ 0xFFFFFFFFu) == e.rec.check && e.rec.isize == n;
    }
    if (!ok) e.rec.verdict = BZ_E_DATA;
    w->split_ms[6] += now_ms() - t1;
    return BZ_OK;
}

// What the sizes phase of a batch leaves for its writing phase.
struct DfSizes {
    std::vector<DfInfRec> rec;        // every entry's record, the split entries' included
    std::vector<DfSplitEntry> splits; // the entries that go across many waves
    std::vector<u64> len_small;       // the entries' lengths with the split entries as entries of no bytes (empty: none is split)
};

// The sizes phase: the split entries' search, sizes, chain and repair, and the sizes launch over all entries.  will_write:
// a writing phase follows (the split entries' source map is sized here, before any entry is committed to the split path).
// The entries' ranges stay in w->i_in and their records in w->i_rec for a writing phase that follows at once.
static int df_decode_sizes(bz_gpu_engine *g, DfWorkspace *w, int kind, const u8 *in8, const uint64_t *h_in_off, const uint64_t *h_in_len,
                           size_t count, DfWindow win, bool will_write, DfSizes &s)
{
    int rc;
    // the entries that go across many waves; in the launches over all entries they are entries of no bytes
    const u64 split_min = df_env_kib("BZ_DF_INF_SPLIT_KIB", 1024) * 1024;
    std::vector<DfSplitEntry> &splits = s.splits;
    splits.clear();
    for (size_t i = 0; split_min && i < count; ++i) {
        if (h_in_len[i] < split_min) continue;
        DfSplitEntry e;
        bool fallback = false;
        e.index = i;
        rc = df_split_sizes(g, w, kind, in8 + h_in_off[i], (u32)h_in_len[i], win, e, &fallback);
        if (rc != BZ_OK) return rc;
        if (!fallback) splits.push_back(std::move(e));
    }
    (void)split_reserve(splits, will_write, w->s_map, w->s_cnt, h_in_len, count, s.len_small);
    for (const DfSplitEntry &e : splits) {
        for (int k = 0; k < 8; ++k) w->split_stats[k] += e.st[k];
        for (int k = 0; k < 3; ++k) w->split_ms[k] += e.ms[k];
    }
    rc = w->i_in.ensure(2 * count * sizeof(u64));
    if (rc == BZ_OK) rc = w->i_ooff.ensure(count * sizeof(u64));
    if (rc == BZ_OK) rc = w->i_rec.ensure(count * sizeof(DfInfRec));
    if (rc != BZ_OK) return rc;
    u64 *d_off = w->i_in.as<u64>(), *d_len = d_off + count;
    DfInfRec *d_rec = w->i_rec.as<DfInfRec>();
    HIPCHK(hipMemcpyAsync(d_off, h_in_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(d_len, splits.empty() ? h_in_len : s.len_small.data(), count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipEventRecord(w->ev[0], g->st));
    if (df_launch_inflate(g->st, false, in8, d_off, d_len, (u32)count, kind, nullptr, nullptr, d_rec, win) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[1], g->st));
    s.rec.resize(count);
    HIPCHK(hipMemcpyAsync(s.rec.data(), d_rec, count * sizeof(DfInfRec), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    for (const DfSplitEntry &e : splits) s.rec[e.index] = e.rec;
    return BZ_OK;
}

// The writing phase: entry i's bytes at out8 + h_out_off[i] (multiples of 16), at most s.rec[i].len of them; kinds 1 / 2:
// the trailers compared, s.rec[i].verdict turned to BZ_E_DATA where they differ.  upload: the sizes phase that ran last was
// not this batch's, so the ranges and records go to the device first (a split entry's as the entry of no bytes it is there).
static int df_decode_write(bz_gpu_engine *g, DfWorkspace *w, int kind, const u8 *in8, const uint64_t *h_in_off, const uint64_t *h_in_len,
                           size_t count, DfWindow win, u8 *out8, const uint64_t *h_out_off, DfSizes &s, bool upload)
{
    int rc;
    u64 *d_off = w->i_in.as<u64>(), *d_len = d_off + count, *d_ooff = w->i_ooff.as<u64>();
    DfInfRec *d_rec = w->i_rec.as<DfInfRec>();
    std::vector<DfInfRec> small;
    if (upload) {
        rc = w->i_in.ensure(2 * count * sizeof(u64));
        if (rc == BZ_OK) rc = w->i_ooff.ensure(count * sizeof(u64));
        if (rc == BZ_OK) rc = w->i_rec.ensure(count * sizeof(DfInfRec));
        if (rc != BZ_OK) return rc;
        d_off = w->i_in.as<u64>(), d_len = d_off + count, d_ooff = w->i_ooff.as<u64>();
        d_rec = w->i_rec.as<DfInfRec>();
        small = s.rec;
        for (const DfSplitEntry &e : s.splits) {
            small[e.index].len = 0;
            small[e.index].verdict = BZ_E_EOF;
        }
        HIPCHK(hipMemcpyAsync(d_off, h_in_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
        HIPCHK(hipMemcpyAsync(d_len, s.splits.empty() ? h_in_len : s.len_small.data(), count * sizeof(u64), hipMemcpyHostToDevice, g->st));
        HIPCHK(hipMemcpyAsync(d_rec, small.data(), count * sizeof(DfInfRec), hipMemcpyHostToDevice, g->st));
    }
    HIPCHK(hipMemcpyAsync(d_ooff, h_out_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipEventRecord(w->ev[2], g->st));
    if (df_launch_inflate(g->st, true, in8, d_off, d_len, (u32)count, kind, out8, d_ooff, d_rec, win) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipEventRecord(w->ev[3], g->st));
    if (kind != 0) {
        if (df_launch_inflate_check(g->st, out8, d_ooff, (u32)count, d_rec, kind) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(s.rec.data(), d_rec, count * sizeof(DfInfRec), hipMemcpyDeviceToHost, g->st));
    }
    HIPCHK(hipEventRecord(w->ev[4], g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    for (DfSplitEntry &e : s.splits) {
        rc = df_split_write(g, w, kind, in8 + h_in_off[e.index], (u32)h_in_len[e.index], win, out8 + h_out_off[e.index], e);
        if (rc != BZ_OK) return rc;
        s.rec[e.index] = e.rec;
    }
    return BZ_OK;
}

// df_gpu_last_decode_batch_stats [0..6] of one entry
static void df_inf_stats_add(DfWorkspace *w, const DfInfRec &r)
{
    w->inf_stats[r.verdict == BZ_OK ? 0 : 1] += 1;
    for (int k = 0; k < 3; ++k) w->inf_stats[2 + k] += r.nblk[k];
    w->inf_stats[5] += r.len;
    w->inf_stats[6] += (r.end_bit + 7u) >> 3;
}

// The window of a call: the last min(dict_len, 32768) bytes of the dictionary, uploaded into the workspace (once per call, not
// kept: 32 KiB), and the Adler-32 of the WHOLE dictionary (adler32.rs:20-66), which is what a zlib header's DICTID holds.
static int df_decode_window(bz_gpu_engine *g, DfWorkspace *w, const uint8_t *dict, size_t dict_len, DfWindow &win)
{
    win = DfWindow{};
    if (!dict_len) return BZ_OK;
    const u32 W = (u32)std::min<size_t>(dict_len, 32768);
    int rc = w->i_dict.ensure(32768);
    if (rc != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->i_dict.p, dict + (dict_len - W), W, hipMemcpyHostToDevice, g->st));
    win.p = w->i_dict.as<u8>();
    win.W = W;
    win.adler = df_adler32_host(dict, dict_len);
    return BZ_OK;
}

// grow != nullptr: the output is the engine's own buffer, sized between the two launches (the host forms)
static int df_decode_batch_core(bz_gpu_engine *g, int kind, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                                const uint8_t *dict, size_t dict_len, void *d_out, size_t cap, DevBuf *grow, uint64_t *h_out_off,
                                uint64_t *h_out_len, int32_t *h_verdict)
{
    if (!g || kind < 0 || kind > 2) return BZ_E_PARAM;
    if (df_dict_param(kind, dict, dict_len) != BZ_OK) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !h_verdict) return BZ_E_PARAM;
    if (!batch_ranges_ok(d_in, d_out, h_in_off, h_in_len, count)) return BZ_E_PARAM;
    DfWorkspace *w = nullptr;
    int rc = df_workspace(g, &w);
    if (rc != BZ_OK) return rc;
    for (u64 &s : w->inf_stats) s = 0;
    for (u64 &s : w->split_stats) s = 0;
    for (double &t : w->split_ms) t = 0;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    DfWindow win;
    rc = df_decode_window(g, w, dict, dict_len, win);
    if (rc != BZ_OK) return rc;
    DfSizes sz;
    rc = df_decode_sizes(g, w, kind, in8, h_in_off, h_in_len, count, win, d_out != nullptr || grow != nullptr, sz);
    if (rc != BZ_OK) return rc;
    const std::vector<DfInfRec> &rec = sz.rec;
    u64 need = 0;
    u8 *out8 = nullptr;
    if ((rc = batch_place(rec.data(), count, nullptr, h_out_off, h_out_len, h_verdict, &need)) != BZ_OK) return rc;
    if ((rc = batch_output(need, d_out, cap, grow, &out8)) != BZ_OK) return rc;
    float ms[3] = {0, 0, 0};
    if (out8) {
        rc = df_decode_write(g, w, kind, in8, h_in_off, h_in_len, count, win, out8, h_out_off, sz, false);
        if (rc != BZ_OK) return rc;
        for (size_t i = 0; i < count; ++i) h_verdict[i] = rec[i].verdict;
        (void)hipEventElapsedTime(&ms[1], w->ev[2], w->ev[3]);
        (void)hipEventElapsedTime(&ms[2], w->ev[3], w->ev[4]);
        w->inf_stats[7] = kind != 0 ? 3 : 2;
    } else w->inf_stats[7] = 1;
    (void)hipEventElapsedTime(&ms[0], w->ev[0], w->ev[1]);
    for (size_t i = 0; i < count; ++i) df_inf_stats_add(w, rec[i]);
    // df_gpu_last_timings: [0] the sizes launch [1] the writing launch [2] the checksum kernel [5] their sum; the phases of the
    // split entries (host clock around launches that are waited for) go where they belong
    ms[0] += (float)(w->split_ms[0] + w->split_ms[1] + w->split_ms[2]);
    ms[1] += (float)(w->split_ms[3] + w->split_ms[4] + w->split_ms[5]);
    ms[2] += (float)w->split_ms[6];
    if (df_trace() && !sz.splits.empty())
        fprintf(stderr, "bz2_mi355x: inflate split: %zu entries; search %.3f sizes %.3f repair %.3f writing %.3f jump %.3f gather %.3f checksum %.3f ms\n",
                sz.splits.size(), w->split_ms[0], w->split_ms[1], w->split_ms[2], w->split_ms[3], w->split_ms[4], w->split_ms[5], w->split_ms[6]);
    for (double &t : w->t_stage) t = 0;
    for (int k = 0; k < 3; ++k) {
        w->t_stage[k] = ms[k] * 1e-3;
        w->t_stage[5] += ms[k] * 1e-3;
    }
    return BZ_OK;
}

extern "C" int df_gpu_decode_batch_device(bz_gpu_engine *g, int kind, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                                          size_t count, void *d_out, size_t cap, uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict)
{
    return df_decode_batch_core(g, kind, d_in, h_in_off, h_in_len, count, nullptr, 0, d_out, cap, nullptr, h_out_off, h_out_len, h_verdict);
}

extern "C" int df_gpu_decode_batch_device_dict(bz_gpu_engine *g, int kind, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                                               size_t count, const uint8_t *dict, size_t dict_len, void *d_out, size_t cap, uint64_t *h_out_off,
                                               uint64_t *h_out_len, int32_t *h_verdict)
{
    return df_decode_batch_core(g, kind, d_in, h_in_off, h_in_len, count, dict, dict_len, d_out, cap, nullptr, h_out_off, h_out_len, h_verdict);
}

// Many streams: packed at 4-byte-aligned offsets (BatchLayout), one upload, one device call (the engine's output buffer
// sized between its two launches), one download.
extern "C" int df_decode_batch(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t **out,
                               uint64_t *out_off, uint64_t *out_len, int32_t *verdict)
{
    return df_decode_batch_dict(kind, device, ins, lens, count, nullptr, 0, out, out_off, out_len, verdict);
}

extern "C" int df_decode_batch_dict(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count, const uint8_t *dict,
                                    size_t dict_len, uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (kind < 0 || kind > 2) return BZ_E_PARAM;
    if (df_dict_param(kind, dict, dict_len) != BZ_OK) return BZ_E_PARAM;
    if (count && (!ins || !lens || !out_off || !out_len || !verdict)) return BZ_E_PARAM;
    const BatchLayout lay(ins, lens, count, 4);
    if (lay.status != BZ_OK) return lay.status;
    if (count == 0) return one_shot_empty(out);
    // (the entries' verdicts are not the engine's business)
    return one_shot(device, 2, lay, kOutGrown, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int rc = df_decode_batch_core(g, kind, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), count, dict, dict_len, nullptr, 0,
                                            &g->oneshot_out, out_off, out_len, verdict);
        if (rc == BZ_OK) *total = (size_t)(out_off[count - 1] + out_len[count - 1]);
        return rc;
    });
}

// The batch of one: BZ_OK with the bytes, or the entry's verdict with the bytes in front of it (as bz_decode_buffer).
extern "C" int df_decode_buffer(int kind, int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len)
{
    return df_decode_buffer_dict(kind, device, in, in_len, nullptr, 0, out, out_len);
}

extern "C" int df_decode_buffer_dict(int kind, int device, const uint8_t *in, size_t in_len, const uint8_t *dict, size_t dict_len, uint8_t **out,
                                     size_t *out_len)
{
    if (!out || !out_len || (in_len && !in)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    uint64_t off = 0, len = 0;
    int32_t verdict = BZ_OK;
    const uint8_t *ins[1] = {in};
    const size_t lens[1] = {in_len};
    const int rc = df_decode_batch_dict(kind, device, ins, lens, 1, dict, dict_len, out, &off, &len, &verdict);
    if (rc != BZ_OK) return rc;
    *out_len = (size_t)len; // (the one entry lies at offset 0)
    return verdict;
}

// ---- every member of a gzip file (section 6 of the header; gz_members.h, kernels: k_gz_members.hip) ----------------
// DESIGN_deflate.md "Every member of a gzip file".  Pass 1 (the sizes): candidates, a sub-batch of them at a time as one
// batch of spans for the sizes phase above, the walk that keeps the members.  Pass 2 (the bytes, once the capacity is
// known to suffice): the members alone, a sub-batch at a time, through the writing phase into the engine's staging buffer
// and from there side by side into the caller's.
static_assert(gzmem::kOk == BZ_OK && gzmem::kEof == BZ_E_EOF, "gz_members.h names the verdicts by value");

extern "C" int df_gpu_last_decode_members_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->mem_stats[i] : 0;
    return BZ_OK;
}

extern "C" int df_gpu_last_decode_members_timings(bz_gpu_engine *g, double out_seconds[4])
{
    if (!g || !out_seconds) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out_seconds[i] = g->df ? g->df->mem_ms[i] * 1e-3 : 0.0;
    return BZ_OK;
}

// candidates per sizes launch, members per writing launch; read per call
static u64 df_gz_sub_batch()
{
    const u64 v = df_env_kib("BZ_DF_GZ_BATCH", gzmem::kSubBatch);
    return v < 1 ? 1 : v > (1u << 20) ? (1u << 20) : v;
}
constexpr u64 kGzStageMax = (u64)256 << 20; // bytes of spans, and of decoded members, per writing launch (one member may exceed it)

struct GzMember {
    u64 start, span; // the bytes the decoder is shown: from the member's first byte to a candidate behind its end, or the input's end
    DfInfRec rec;
    int split;       // its DfSplitEntry among the call's, -1: one wave
};

// The candidate list, a window at a time: the counts per tile are kept, the positions are listed on demand.
struct GzCands {
    bz_gpu_engine *g = nullptr;
    DfWorkspace *w = nullptr;
    const u8 *in = nullptr;
    u32 len = 0;
    std::vector<u64> tpre; // per tile: the candidates in front of it; [ntiles]: all
    u64 total = 0, sub = 0, first = 0;
    std::vector<u32> win;  // candidates first .. first + win.size()

    int count()
    {
        const u32 ntiles = (u32)(((u64)len + gzmem::kTile - 1) / gzmem::kTile); // (len up to 2^32 - 1: the sum in 64 bits)
        int rc = w->m_cnt.ensure((size_t)ntiles * 4);
        if (rc == BZ_OK) rc = w->m_base.ensure((size_t)ntiles * 4);
        if (rc != BZ_OK) return rc;
        const double t0 = now_ms();
        std::vector<u32> cnt(ntiles), base(ntiles);
        if (df_launch_gz_search_count(g->st, in, len, ntiles, w->m_cnt.as<u32>()) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(cnt.data(), w->m_cnt.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        tpre.assign((size_t)ntiles + 1, 0);
        for (u32 t = 0; t < ntiles; ++t) {
            base[t] = (u32)tpre[t]; // (fewer than len / 3 candidates: 32 bits)
            tpre[t + 1] = tpre[t] + cnt[t];
        }
        total = tpre[ntiles];
        HIPCHK(hipMemcpyAsync(w->m_base.p, base.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        w->mem_ms[0] += now_ms() - t0;
        w->mem_stats[7] += 1;
        return BZ_OK;
    }
    // candidates idx .. idx + n (cut at the list's end) become the window
    int fetch(u64 idx, u64 n)
    {
        if (idx >= total) return BZ_E_UNEXPECTED;
        n = std::min(n, total - idx);
        const u32 t0 = (u32)(std::upper_bound(tpre.begin(), tpre.end(), idx) - tpre.begin() - 1);
        const u32 t1 = (u32)(std::upper_bound(tpre.begin(), tpre.end(), idx + n - 1) - tpre.begin() - 1);
        const int rc = w->m_cand.ensure((size_t)n * 4);
        if (rc != BZ_OK) return rc;
        const double c0 = now_ms();
        if (df_launch_gz_search_list(g->st, in, len, t0, t1 - t0 + 1, w->m_base.as<u32>(), (u32)idx, (u32)n, w->m_cand.as<u32>()) != 0)
            return BZ_E_UNEXPECTED;
        win.resize((size_t)n);
        HIPCHK(hipMemcpyAsync(win.data(), w->m_cand.p, (size_t)n * 4, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        first = idx;
        w->mem_ms[0] += now_ms() - c0;
        w->mem_stats[7] += 1;
        return BZ_OK;
    }
    bool has(u64 idx, u64 n) const { return idx >= first && idx + n <= first + win.size(); }
    int at(u64 idx, u64 *pos)
    {
        if (!has(idx, 1)) {
            const int rc = fetch(idx, sub + 1);
            if (rc != BZ_OK) return rc;
        }
        *pos = win[(size_t)(idx - first)];
        return BZ_OK;
    }
};

// spans of the input (first byte, bytes) -> the batch image in w->m_image, each at a multiple of 4
static int df_gz_gather(bz_gpu_engine *g, DfWorkspace *w, const u8 *in8, const std::vector<std::pair<u64, u64>> &sp, std::vector<u64> &ioff,
                        std::vector<u64> &ilen)
{
    const size_t n = sp.size();
    std::vector<GzSpan> tab(n);
    ioff.resize(n);
    ilen.resize(n);
    u64 cur = 0;
    u32 max_len = 0;
    for (size_t i = 0; i < n; ++i) {
        tab[i] = GzSpan{sp[i].first, cur, (u32)sp[i].second, 0};
        ioff[i] = cur;
        ilen[i] = sp[i].second;
        cur += (sp[i].second + 3u) & ~(u64)3;
        max_len = std::max(max_len, (u32)sp[i].second);
    }
    int rc = w->m_image.ensure((size_t)cur + 64);
    if (rc == BZ_OK) rc = w->m_span.ensure(n * sizeof(GzSpan));
    if (rc != BZ_OK) return rc;
    const double t0 = now_ms();
    HIPCHK(hipMemcpyAsync(w->m_span.p, tab.data(), n * sizeof(GzSpan), hipMemcpyHostToDevice, g->st));
    if (df_launch_gz_gather(g->st, in8, w->m_span.as<GzSpan>(), (u32)n, max_len, w->m_image.as<u8>()) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipStreamSynchronize(g->st));
    w->mem_ms[1] += now_ms() - t0;
    w->mem_stats[7] += 1;
    return BZ_OK;
}

// ... and their sizes phase, each span a one-member entry (kind 2)
static int df_gz_sizes(bz_gpu_engine *g, DfWorkspace *w, const u8 *in8, const std::vector<std::pair<u64, u64>> &sp, bool will_write, DfSizes &s,
                       double *ms_sizes)
{
    std::vector<u64> ioff, ilen;
    int rc = df_gz_gather(g, w, in8, sp, ioff, ilen);
    if (rc != BZ_OK) return rc;
    rc = df_decode_sizes(g, w, DF_KIND_GZIP, w->m_image.as<u8>(), ioff.data(), ilen.data(), sp.size(), DfWindow{}, will_write, s);
    if (rc != BZ_OK) return rc;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, w->ev[0], w->ev[1]);
    *ms_sizes += ms;
    return BZ_OK;
}

// out[j] = the first byte in [from[j], bound[j]) that is not zero, or bound[j]
static int df_gz_zero_skip(bz_gpu_engine *g, DfWorkspace *w, const u8 *in8, const u32 *from, const u32 *bound, u32 n, u32 *out)
{
    const int rc = w->m_zs.ensure((size_t)n * 12);
    if (rc != BZ_OK) return rc;
    u32 *d = w->m_zs.as<u32>();
    const double t0 = now_ms();
    HIPCHK(hipMemcpyAsync(d, from, (size_t)n * 4, hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(d + n, bound, (size_t)n * 4, hipMemcpyHostToDevice, g->st));
    if (df_launch_gz_zero_skip(g->st, in8, d, d + n, n, d + 2 * (size_t)n) != 0) return BZ_E_UNEXPECTED;
    HIPCHK(hipMemcpyAsync(out, d + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    w->mem_ms[2] += now_ms() - t0;
    w->mem_stats[7] += 1;
    return BZ_OK;
}

// grow != nullptr: the output is the engine's own buffer, sized between the passes (the host form)
static int df_members_core(bz_gpu_engine *g, const void *d_in, size_t in_len, void *d_out, size_t cap, DevBuf *grow, uint64_t *out_len,
                           int32_t *verdict)
{
    using gzmem::Step;
    if (!g || !out_len || !verdict) return BZ_E_PARAM;
    *out_len = 0;
    *verdict = BZ_OK;
    if ((in_len && !d_in) || ((uintptr_t)d_in & 15u) || (u64)in_len >= (1ull << 32)) return BZ_E_PARAM;
    DfWorkspace *w = nullptr;
    int rc = df_workspace(g, &w);
    if (rc != BZ_OK) return rc;
    for (u64 &s : w->inf_stats) s = 0;
    for (u64 &s : w->split_stats) s = 0;
    for (double &t : w->split_ms) t = 0;
    for (u64 &s : w->mem_stats) s = 0;
    for (double &t : w->mem_ms) t = 0;
    for (double &t : w->t_stage) t = 0;
    if (in_len == 0) return BZ_OK;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    const u64 len = in_len;
    const bool will_write = d_out != nullptr || grow != nullptr;
    u64 *ms = w->mem_stats;
    double t_sizes = 0, t_write = 0, t_check = 0;
    GzCands cs;
    cs.g = g;
    cs.w = w;
    cs.in = in8;
    cs.len = (u32)len;
    cs.sub = df_gz_sub_batch();
    if ((rc = cs.count()) != BZ_OK) return rc;
    ms[1] = cs.total;

    // ---- pass 1: the members, their lengths and the stream's verdict in front of the trailers
    std::vector<GzMember> mem;
    std::vector<DfSplitEntry> msplits;
    int v = BZ_OK;
    u64 ci = 0; // the first candidate at or behind p
    u64 p = 0;  // where the next member has to start
    {
        u64 b = len;
        if (cs.total && (rc = cs.at(0, &b)) != BZ_OK) return rc;
        const u32 from = 0, bound = (u32)b;
        u32 nz = 0;
        if ((rc = df_gz_zero_skip(g, w, in8, &from, &bound, 1, &nz)) != BZ_OK) return rc;
        p = nz == bound && cs.total == 0 ? len : nz; // (a bound of 2^32 - 1 at most: len < 4 GiB)
        ms[4] += p;
    }
    while (p != len) {
        u64 c0 = len;
        if (ci < cs.total && (rc = cs.at(ci, &c0)) != BZ_OK) return rc;
        if (c0 != p) { // no candidate: the one-member decoder's header rules say what it is
            DfSizes s1;
            if ((rc = df_gz_sizes(g, w, in8, {{p, std::min<u64>(gzmem::kJunkBytes, len - p)}}, false, s1, &t_sizes)) != BZ_OK) return rc;
            v = s1.rec[0].verdict;
            if (v == BZ_OK || s1.rec[0].len != 0) return BZ_E_UNEXPECTED;
            break;
        }
        const u64 n = std::min(cs.sub, cs.total - ci), more = ci + n < cs.total ? 1 : 0;
        if (!cs.has(ci, n + more) && (rc = cs.fetch(ci, n + more)) != BZ_OK) return rc;
        std::vector<u64> c((size_t)n + 1);
        for (u64 j = 0; j < n + more; ++j) c[(size_t)j] = cs.win[(size_t)(ci - cs.first + j)];
        if (!more) c[(size_t)n] = len;
        std::vector<std::pair<u64, u64>> sp((size_t)n);
        for (size_t j = 0; j < n; ++j) sp[j] = {c[j], c[j + 1] - c[j]};
        DfSizes s;
        if ((rc = df_gz_sizes(g, w, in8, sp, will_write, s, &t_sizes)) != BZ_OK) return rc;
        ms[6] += 1;
        std::vector<int> sidx((size_t)n, -1);
        for (size_t k = 0; k < s.splits.size(); ++k) sidx[s.splits[k].index] = (int)k;
        // the zeros behind every span's member, as if each were confirmed
        std::vector<u32> from((size_t)n), bound((size_t)n), nz((size_t)n);
        for (size_t j = 0; j < n; ++j) {
            bound[j] = (u32)c[j + 1];
            from[j] = s.rec[j].verdict == BZ_OK ? (u32)(c[j] + (s.rec[j].end_bit >> 3)) : bound[j];
        }
        if ((rc = df_gz_zero_skip(g, w, in8, from.data(), bound.data(), (u32)n, nz.data())) != BZ_OK) return rc;
        bool over = false;
        for (size_t j = 0; j < n;) {
            DfInfRec r = s.rec[j];
            DfSplitEntry se;
            bool split = sidx[j] >= 0;
            if (split) se = std::move(s.splits[(size_t)sidx[j]]);
            u64 span_end = c[j + 1], bnd = c[j + 1], nonzero = nz[j], next_ci = ci + j + 1;
            u64 e = r.verdict == BZ_OK ? c[j] + (r.end_bit >> 3) : span_end;
            Step st = gzmem::walk_step(r.verdict, span_end, nonzero, bnd, len);
            if (st == Step::Extend) {
                for (u32 round = 1;; ++round) { // over 1, 2, 4, ... candidates more
                    ms[3] += 1;
                    const u64 ei = gzmem::extend_to(ci + j, round);
                    span_end = len;
                    if (ei < cs.total && (rc = cs.at(ei, &span_end)) != BZ_OK) return rc;
                    DfSizes s1;
                    if ((rc = df_gz_sizes(g, w, in8, {{c[j], span_end - c[j]}}, will_write, s1, &t_sizes)) != BZ_OK) return rc;
                    r = s1.rec[0];
                    split = !s1.splits.empty();
                    if (split) se = std::move(s1.splits[0]);
                    if (!(r.verdict == BZ_E_EOF && span_end < len)) break;
                }
                // the candidates that lay inside the member, and what bounds the zeros behind it
                e = r.verdict == BZ_OK ? c[j] + (r.end_bit >> 3) : span_end;
                next_ci = std::max(next_ci, cs.tpre[(size_t)(e / gzmem::kTile)]);
                bnd = len;
                while (next_ci < cs.total) {
                    if ((rc = cs.at(next_ci, &bnd)) != BZ_OK) return rc;
                    if (bnd >= e) break;
                    bnd = len;
                    ++next_ci;
                }
                nonzero = bnd;
                if (r.verdict == BZ_OK) {
                    const u32 f1 = (u32)e, b1 = (u32)bnd;
                    u32 z1 = 0;
                    if ((rc = df_gz_zero_skip(g, w, in8, &f1, &b1, 1, &z1)) != BZ_OK) return rc;
                    nonzero = z1;
                }
                st = gzmem::walk_step(r.verdict, span_end, nonzero, bnd, len);
                if (st == Step::Extend) return BZ_E_UNEXPECTED;
            }
            if (r.flags & 1u) return BZ_E_PARAM; // a member of 4 GiB or more of output
            // an extended span may reach far behind the member: the writing phase is shown the member alone, which decodes
            // alike (unless the long span went across many waves and the member itself would too: its pieces stay as found)
            const u64 split_min = df_env_kib("BZ_DF_INF_SPLIT_KIB", 1024) * 1024;
            if (r.verdict == BZ_OK && e < span_end && !(split && e - c[j] >= split_min)) {
                span_end = e;
                split = false;
            }
            int at = -1;
            if (split) {
                at = (int)msplits.size();
                msplits.push_back(std::move(se));
            }
            mem.push_back(GzMember{c[j], span_end - c[j], r, at});
            if (st == Step::Fault) {
                v = r.verdict;
                over = true;
                break;
            }
            ms[4] += nonzero - e;
            p = st == Step::End ? len : nonzero;
            if (st == Step::Next && next_ci < ci + n) { // (behind an extension too: the spans of the sub-batch stand as decoded)
                j = (size_t)(next_ci - ci);
                continue;
            }
            ci = next_ci; // the next sub-batch starts there, or the byte at p is no candidate, or the input is over
            break;
        }
        if (over) break;
    }
    ms[0] = mem.size();
    ms[2] = cs.total - mem.size();
    u64 need = 0;
    for (const GzMember &m : mem) {
        need += m.rec.len;
        if (m.split >= 0) ms[5] += 1;
    }
    *out_len = need;
    *verdict = v;

    // ---- pass 2: the bytes
    u8 *out8 = static_cast<u8 *>(d_out);
    if (grow) {
        if ((rc = grow->ensure((size_t)need + 64)) != BZ_OK) return rc;
        out8 = grow->as<u8>();
    } else if (d_out && need > cap) return BZ_E_CAPACITY;
    u64 done = 0;
    bool cut = false;
    for (size_t a = 0; out8 && a < mem.size() && !cut;) {
        size_t b = a;
        u64 img = 0, stg = 0;
        while (b < mem.size() && b - a < cs.sub && (b == a || (img + mem[b].span <= kGzStageMax && stg + mem[b].rec.len <= kGzStageMax))) {
            img += mem[b].span;
            stg += ((u64)mem[b].rec.len + 15u) & ~(u64)15;
            ++b;
        }
        const size_t cnt = b - a;
        std::vector<std::pair<u64, u64>> sp(cnt);
        std::vector<u64> ioff, ilen, ooff(cnt);
        DfSizes s;
        s.rec.resize(cnt);
        u64 cur = 0;
        for (size_t i = 0; i < cnt; ++i) {
            const GzMember &m = mem[a + i];
            sp[i] = {m.start, m.span};
            s.rec[i] = m.rec;
            ooff[i] = cur;
            cur += ((u64)m.rec.len + 15u) & ~(u64)15;
            if (m.split >= 0) {
                s.splits.push_back(std::move(msplits[(size_t)m.split]));
                s.splits.back().index = i;
            }
        }
        if ((rc = df_gz_gather(g, w, in8, sp, ioff, ilen)) != BZ_OK) return rc;
        if (!s.splits.empty()) {
            s.len_small = ilen;
            for (const DfSplitEntry &e : s.splits) s.len_small[e.index] = 0;
        }
        if ((rc = w->m_stage.ensure((size_t)cur + 64)) != BZ_OK) return rc;
        rc = df_decode_write(g, w, DF_KIND_GZIP, w->m_image.as<u8>(), ioff.data(), ilen.data(), cnt, DfWindow{}, w->m_stage.as<u8>(), ooff.data(), s, true);
        if (rc != BZ_OK) return rc;
        float e1 = 0, e2 = 0;
        (void)hipEventElapsedTime(&e1, w->ev[2], w->ev[3]);
        (void)hipEventElapsedTime(&e2, w->ev[3], w->ev[4]);
        t_write += e1;
        t_check += e2;
        // the stream ends with the first member that is not clean; its bytes in front of the fault belong to it
        std::vector<GzSpan> tab;
        u32 max_len = 0;
        for (size_t i = 0; i < cnt && !cut; ++i) {
            mem[a + i].rec = s.rec[i];
            tab.push_back(GzSpan{ooff[i], done, s.rec[i].len, 0});
            max_len = std::max(max_len, s.rec[i].len);
            done += s.rec[i].len;
            if (s.rec[i].verdict != BZ_OK) {
                v = s.rec[i].verdict;
                cut = true;
                ms[0] = a + i + 1; // (the members behind it were found by pass 1, and are not decoded)
            }
        }
        if ((rc = w->m_span.ensure(tab.size() * sizeof(GzSpan))) != BZ_OK) return rc;
        const double t0 = now_ms();
        HIPCHK(hipMemcpyAsync(w->m_span.p, tab.data(), tab.size() * sizeof(GzSpan), hipMemcpyHostToDevice, g->st));
        if (df_launch_gz_compact(g->st, w->m_stage.as<u8>(), w->m_span.as<GzSpan>(), (u32)tab.size(), max_len, out8) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipStreamSynchronize(g->st));
        w->mem_ms[3] += now_ms() - t0;
        ms[7] += 1;
        a = b;
    }
    if (out8) {
        *out_len = done;
        *verdict = v;
    }
    for (const GzMember &m : mem) df_inf_stats_add(w, m.rec);
    // df_gpu_last_timings: [0] sizes [1] writing [2] checksums (the split members' phases where they belong) [3] search,
    // gather and zero skip [4] compaction [5] their sum
    w->t_stage[0] = (t_sizes + w->split_ms[0] + w->split_ms[1] + w->split_ms[2]) * 1e-3;
    w->t_stage[1] = (t_write + w->split_ms[3] + w->split_ms[4] + w->split_ms[5]) * 1e-3;
    w->t_stage[2] = (t_check + w->split_ms[6]) * 1e-3;
    w->t_stage[3] = (w->mem_ms[0] + w->mem_ms[1] + w->mem_ms[2]) * 1e-3;
    w->t_stage[4] = w->mem_ms[3] * 1e-3;
    for (int k = 0; k < 5; ++k) w->t_stage[5] += w->t_stage[k];
    return BZ_OK;
}

extern "C" int df_gpu_decode_members_device(bz_gpu_engine *g, const void *d_in, size_t in_len, void *d_out, size_t cap, uint64_t *out_len,
                                            int32_t *verdict)
{
    return df_members_core(g, d_in, in_len, d_out, cap, nullptr, out_len, verdict);
}

// One upload, the device call with the engine's output buffer sized between its passes, one download: BZ_OK with the bytes,
// or the stream's verdict with the bytes in front of it (as df_decode_buffer).
extern "C" int df_decode_members_buffer(int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len || (in_len && !in)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    if ((u64)in_len >= (1ull << 32)) return BZ_E_PARAM;
    if (in_len == 0) return one_shot_empty(out); // (no member: BZ_OK, no bytes, no device)
    uint64_t n = 0;
    int32_t v = BZ_OK;
    // (the stream's verdict is not the engine's business)
    const int rc = one_shot(device, 2, OneShotIn(in, in_len), kOutGrown, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int drc = df_members_core(g, g->dec_in.p, in_len, nullptr, 0, &g->oneshot_out, &n, &v);
        *total = (size_t)n;
        return drc;
    });
    if (rc != BZ_OK) return rc;
    *out_len = (size_t)n;
    return v;
}

// ---- reading BGZF (section 8 of the header; bgzf_index.h; kernels: k_bgzf_read.hip, k_bgzf_inflate / k_bgzf_check) ----------
// The index comes from BSIZE and ISIZE (df_bgzf_index_buffer on the host, df_gpu_bgzf_index_device over a search's list);
// a read decodes the blocks its range touches in ONE pass, each straight to its place, the at most two blocks the range
// cuts through two slots of the workspace.
static_assert(bgzf::kOk == BZ_OK && bgzf::kData == BZ_E_DATA && bgzf::kEof == BZ_E_EOF, "bgzf_index.h names the verdicts by value");

extern "C" int df_gpu_last_bgzf_read_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->bgzf_read_stats[i] : 0;
    return BZ_OK;
}

// candidates per list window, blocks per decode launch; read per call
static u64 df_bgzf_batch()
{
    const u64 v = df_env_kib("BZ_DF_BGZF_BATCH", bgzf::kBatch);
    return v < 1 ? 1 : v > (1u << 20) ? (1u << 20) : v;
}

// the index as the two malloc'ed arrays of the host call
static int df_bgzf_index_out(const std::vector<u64> &c, const std::vector<u64> &u, uint64_t **coff, uint64_t **uoff)
{
    uint64_t *a = (uint64_t *)malloc(c.size() * 8), *b = (uint64_t *)malloc(u.size() * 8);
    if (!a || !b) {
        free(a);
        free(b);
        return BZ_E_NOMEM;
    }
    memcpy(a, c.data(), c.size() * 8);
    memcpy(b, u.data(), u.size() * 8);
    *coff = a;
    *uoff = b;
    return BZ_OK;
}

extern "C" int df_bgzf_index_buffer(const uint8_t *in, size_t in_len, uint64_t **coff, uint64_t **uoff, size_t *count, int32_t *verdict)
{
    if (!coff || !uoff || !count || !verdict || (in_len && !in)) return BZ_E_PARAM;
    *coff = *uoff = nullptr;
    *count = 0;
    *verdict = BZ_OK;
    std::vector<u64> c, u;
    u64 ec = 0, eu = 0;
    int v = BZ_OK;
    (void)bgzf::chain_host(in, in_len, [&](u64 a, u64 b) { c.push_back(a); u.push_back(b); }, &ec, &eu, &v);
    c.push_back(ec);
    u.push_back(eu);
    const int rc = df_bgzf_index_out(c, u, coff, uoff);
    if (rc != BZ_OK) return rc;
    *count = c.size() - 1;
    *verdict = v;
    return BZ_OK;
}

// The candidate list of a file in HBM, a window at a time: the counts per tile are kept, the positions and their blocks'
// sizes are listed on demand (GzCands' way, with 64-bit positions).
struct BgzfCands {
    bz_gpu_engine *g = nullptr;
    DfWorkspace *w = nullptr;
    const u8 *in = nullptr;
    u64 len = 0;
    std::vector<u64> tpre; // per tile: the candidates in front of it; [ntiles]: all
    u64 total = 0, sub = 0, first = 0, launches = 0;
    std::vector<u64> win;  // candidates first .. first + win.size()
    std::vector<BgzfInfo> info;

    int count()
    {
        const u64 nt = (len + bgzf::kTile - 1) / bgzf::kTile;
        if (nt >= (1ull << 31)) return BZ_E_PARAM;
        const u32 ntiles = (u32)nt;
        int rc = w->z_cnt.ensure((size_t)ntiles * 4);
        if (rc == BZ_OK) rc = w->z_base.ensure((size_t)ntiles * 8);
        if (rc != BZ_OK) return rc;
        std::vector<u32> cnt(ntiles);
        if (df_launch_bgzf_search_count(g->st, in, len, ntiles, w->z_cnt.as<u32>()) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(cnt.data(), w->z_cnt.p, (size_t)ntiles * 4, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        tpre.assign((size_t)ntiles + 1, 0);
        for (u32 t = 0; t < ntiles; ++t) tpre[t + 1] = tpre[t] + cnt[t];
        total = tpre[ntiles];
        HIPCHK(hipMemcpyAsync(w->z_base.p, tpre.data(), (size_t)ntiles * 8, hipMemcpyHostToDevice, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        launches += 1;
        return BZ_OK;
    }
    // candidates idx .. idx + n (cut at the list's end) become the window
    int fetch(u64 idx, u64 n)
    {
        if (idx >= total) return BZ_E_UNEXPECTED;
        n = std::min(n, total - idx);
        const u32 t0 = (u32)(std::upper_bound(tpre.begin(), tpre.end(), idx) - tpre.begin() - 1);
        const u32 t1 = (u32)(std::upper_bound(tpre.begin(), tpre.end(), idx + n - 1) - tpre.begin() - 1);
        int rc = w->z_cand.ensure((size_t)n * 8);
        if (rc == BZ_OK) rc = w->z_info.ensure((size_t)n * sizeof(BgzfInfo));
        if (rc != BZ_OK) return rc;
        if (df_launch_bgzf_search_list(g->st, in, len, t0, t1 - t0 + 1, w->z_base.as<u64>(), idx, (u32)n, w->z_cand.as<u64>()) != 0)
            return BZ_E_UNEXPECTED;
        if (df_launch_bgzf_block_info(g->st, in, len, w->z_cand.as<u64>(), (u32)n, w->z_info.as<BgzfInfo>()) != 0) return BZ_E_UNEXPECTED;
        win.resize((size_t)n);
        info.resize((size_t)n);
        HIPCHK(hipMemcpyAsync(win.data(), w->z_cand.p, (size_t)n * 8, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipMemcpyAsync(info.data(), w->z_info.p, (size_t)n * sizeof(BgzfInfo), hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        first = idx;
        launches += 2;
        return BZ_OK;
    }
    bool has(u64 idx) const { return idx >= first && idx < first + win.size(); }
};

extern "C" int df_gpu_bgzf_index_device(bz_gpu_engine *g, const void *d_in, size_t in_len, uint64_t *h_coff, uint64_t *h_uoff, size_t cap_blocks,
                                        size_t *count, int32_t *verdict)
{
    if (!g || !count || !verdict || (in_len && !d_in) || ((uintptr_t)d_in & 15u)) return BZ_E_PARAM;
    if (cap_blocks && (!h_coff || !h_uoff)) return BZ_E_PARAM;
    *count = 0;
    *verdict = BZ_OK;
    DfWorkspace *w = nullptr;
    const int wrc = df_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    w->bgzf_read_stats[3] = w->bgzf_read_stats[4] = 0;
    w->bgzf_index_s = 0;
    const double t0 = now_ms();
    BgzfCands cs;
    cs.g = g;
    cs.w = w;
    cs.in = static_cast<const u8 *>(d_in);
    cs.len = in_len;
    cs.sub = df_bgzf_batch();
    if (in_len) {
        const int rc = cs.count();
        if (rc != BZ_OK) return rc;
    }
    // the chain over the list: a position that is not in it is a header-rule failure; the candidates the chain steps over
    // (a stored block whose payload is a BGZF file) are never looked at
    u64 idx = 0, landed = 0, nblocks = 0, ec = 0, eu = 0;
    int v = BZ_OK;
    const int rc = bgzf::chain(
        in_len,
        [&](u64 pos, bool *ok, u32 *bsize1, u32 *isize) {
            idx = std::max(idx, cs.tpre[(size_t)(pos / bgzf::kTile)]);
            for (; idx < cs.total; ++idx) {
                if (!cs.has(idx)) {
                    const int frc = cs.fetch(idx, cs.sub);
                    if (frc != BZ_OK) return frc;
                }
                const u64 c = cs.win[(size_t)(idx - cs.first)];
                if (c < pos) continue;
                if (c == pos) {
                    const BgzfInfo bi = cs.info[(size_t)(idx - cs.first)];
                    *ok = true;
                    *bsize1 = bi.bsize1;
                    *isize = bi.isize;
                    ++landed;
                    ++idx;
                }
                break;
            }
            return (int)BZ_OK;
        },
        [&](u64 a, u64 b) {
            if (nblocks < cap_blocks) {
                h_coff[nblocks] = a;
                h_uoff[nblocks] = b;
            }
            ++nblocks;
        },
        &ec, &eu, &v);
    if (rc != BZ_OK) return rc;
    *count = (size_t)nblocks;
    w->bgzf_read_stats[3] = cs.total;
    w->bgzf_read_stats[4] = cs.total - landed;
    w->bgzf_index_s = (now_ms() - t0) * 1e-3;
    for (int i = 0; i < 6; ++i) w->t_stage[i] = 0;
    w->t_stage[0] = w->t_stage[5] = w->bgzf_index_s;
    if (nblocks > cap_blocks) return BZ_E_CAPACITY;
    if (h_coff && h_uoff) { // (cap_blocks + 1 pairs of room: the last one is the end of the last complete block)
        h_coff[nblocks] = ec;
        h_uoff[nblocks] = eu;
    }
    *verdict = v;
    return BZ_OK;
}

extern "C" int df_gpu_bgzf_read_device(bz_gpu_engine *g, const void *d_in, size_t in_len, const uint64_t *h_coff, const uint64_t *h_uoff, size_t count,
                                       uint64_t ustart, uint64_t ulen, void *d_out, size_t cap, uint64_t *out_len, int32_t *verdict)
{
    if (!g || !out_len || !verdict || !h_coff || !h_uoff || (in_len && !d_in) || ((uintptr_t)d_in & 15u)) return BZ_E_PARAM;
    *out_len = 0;
    *verdict = BZ_OK;
    if (g->df)
        for (int i : {0, 1, 2, 5, 6, 7}) g->df->bgzf_read_stats[i] = 0; // (a call that launches nothing decodes nothing)
    if (h_coff[count] > in_len || ustart < h_uoff[0]) return BZ_E_PARAM;
    for (size_t k = 0; k < count; ++k)
        if (h_coff[k + 1] <= h_coff[k] || h_uoff[k + 1] < h_uoff[k] || h_coff[k + 1] - h_coff[k] > bgzf::kMaxBlock ||
            h_uoff[k + 1] - h_uoff[k] > bgzf::kMaxBlock)
            return BZ_E_PARAM;
    const u64 total = h_uoff[count];
    if (ulen == 0 || ustart >= total) return BZ_OK;
    const u64 uend = ulen < total - ustart ? ustart + ulen : total, rlen = uend - ustart;
    if (!d_out) { // sizes only: the index says it all
        *out_len = rlen;
        return BZ_OK;
    }
    if (cap < rlen) {
        *out_len = rlen;
        return BZ_E_CAPACITY;
    }
    DfWorkspace *w = nullptr;
    const int wrc = df_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    u64 *rs = w->bgzf_read_stats;
    rs[0] = rs[1] = rs[2] = rs[5] = rs[6] = rs[7] = 0;
    u64 first = 0, last = 0;
    bgzf::touched(h_uoff, count, ustart, uend, &first, &last);
    const u64 batch = df_bgzf_batch();
    const u8 *in8 = static_cast<const u8 *>(d_in);
    u8 *out8 = static_cast<u8 *>(d_out);
    int rc = w->z_slots.ensure(2 * (size_t)bgzf::kMaxBlock + 16);
    if (rc != BZ_OK) return rc;
    double t_dec = 0, t_chk = 0, t_copy = 0;
    std::vector<BgzfDesc> desc;
    std::vector<BgzfRec> rec;
    u64 fault = ~0ull;
    for (u64 a = first; a <= last && fault == ~0ull; a += batch) {
        const u64 n = std::min<u64>(batch, last + 1 - a);
        desc.clear();
        std::vector<BgzfDesc> edges;
        for (u64 k = a; k < a + n; ++k) {
            BgzfDesc q = {};
            q.coff = h_coff[k];
            q.csize = (u32)(h_coff[k + 1] - h_coff[k]);
            q.usize = (u32)(h_uoff[k + 1] - h_uoff[k]);
            const u64 lo = std::max<u64>(ustart, h_uoff[k]), hi = std::min<u64>(uend, h_uoff[k + 1]);
            q.dst = lo - ustart;
            if (h_uoff[k] < ustart || h_uoff[k + 1] > uend) { // the range cuts it: through a slot
                q.slot = k == first ? 1u : 2u;
                q.lo = (u32)(lo - h_uoff[k]);
                q.n = (u32)(hi - lo);
                edges.push_back(q);
            }
            desc.push_back(q);
        }
        desc.insert(desc.end(), edges.begin(), edges.end()); // (the edge copy's table: behind the group's)
        if ((rc = w->z_desc.ensure(desc.size() * sizeof(BgzfDesc))) != BZ_OK) return rc;
        if ((rc = w->z_rec.ensure((size_t)n * sizeof(BgzfRec))) != BZ_OK) return rc;
        const BgzfDesc *d_desc = w->z_desc.as<BgzfDesc>();
        HIPCHK(hipMemcpyAsync(w->z_desc.p, desc.data(), desc.size() * sizeof(BgzfDesc), hipMemcpyHostToDevice, g->st));
        HIPCHK(hipEventRecord(w->ev[0], g->st));
        if (df_launch_bgzf_inflate(g->st, in8, d_desc, (u32)n, out8, w->z_slots.as<u8>(), w->z_rec.as<BgzfRec>()) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipEventRecord(w->ev[1], g->st));
        if (df_launch_bgzf_check(g->st, d_desc, (u32)n, out8, w->z_slots.as<u8>(), w->z_rec.as<BgzfRec>()) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipEventRecord(w->ev[2], g->st));
        if (!edges.empty() && df_launch_bgzf_edge_copy(g->st, d_desc + n, (u32)edges.size(), w->z_slots.as<u8>(), out8) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipEventRecord(w->ev[3], g->st));
        rec.resize((size_t)n);
        HIPCHK(hipMemcpyAsync(rec.data(), w->z_rec.p, (size_t)n * sizeof(BgzfRec), hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, w->ev[0], w->ev[1]);
        t_dec += ms;
        (void)hipEventElapsedTime(&ms, w->ev[1], w->ev[2]);
        t_chk += ms;
        (void)hipEventElapsedTime(&ms, w->ev[2], w->ev[3]);
        t_copy += ms;
        rs[0] += n;
        rs[1] += n - edges.size();
        rs[2] += edges.size();
        rs[7] += edges.empty() ? 2 : 3;
        for (u64 i = 0; i < n; ++i) {
            rs[5] += rec[(size_t)i].len;
            if (rec[(size_t)i].verdict != BZ_OK && fault == ~0ull) fault = a + i; // the lowest k decides
        }
    }
    if (fault != ~0ull) {
        *verdict = BZ_E_DATA;
        *out_len = h_uoff[fault] > ustart ? h_uoff[fault] - ustart : 0;
    } else *out_len = rlen;
    rs[6] = *out_len;
    // df_gpu_last_timings: [0] search and chain of the last index call [1] decode [2] checksums [3] edge copy [5] their sum
    w->t_stage[0] = w->bgzf_index_s;
    w->t_stage[1] = t_dec * 1e-3;
    w->t_stage[2] = t_chk * 1e-3;
    w->t_stage[3] = t_copy * 1e-3;
    w->t_stage[4] = 0;
    w->t_stage[5] = w->t_stage[0] + w->t_stage[1] + w->t_stage[2] + w->t_stage[3];
    return BZ_OK;
}

// Host to host: the index on the host, the compressed bytes of the blocks touched up, one device call, the range down.
extern "C" int df_bgzf_read_buffer(int device, const uint8_t *in, size_t in_len, uint64_t ustart, uint64_t ulen, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len || (in_len && !in)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    std::vector<u64> c, u;
    u64 ec = 0, eu = 0;
    int vi = BZ_OK;
    (void)bgzf::chain_host(in, in_len, [&](u64 a, u64 b) { c.push_back(a); u.push_back(b); }, &ec, &eu, &vi);
    c.push_back(ec);
    u.push_back(eu);
    const u64 count = c.size() - 1, total = eu;
    // the index's fault lies at uncompressed position `total`: inside or in front of a range that reaches behind it
    const bool reaches = ulen != 0 && (ustart >= total || ulen > total - ustart);
    const int v_index = reaches ? vi : BZ_OK;
    if (ulen == 0 || ustart >= total) return one_shot_empty(out) == BZ_OK ? v_index : BZ_E_NOMEM; // no bytes: no device
    const u64 uend = ulen < total - ustart ? ustart + ulen : total, rlen = uend - ustart;
    u64 first = 0, last = 0;
    bgzf::touched(u.data(), count, ustart, uend, &first, &last);
    const u64 cbase = c[(size_t)first] & ~(u64)15, clen = c[(size_t)last + 1] - cbase; // (the device call wants 16-byte alignment)
    std::vector<u64> rc_off((size_t)(last - first + 2));
    for (size_t k = 0; k < rc_off.size(); ++k) rc_off[k] = c[(size_t)first + k] - cbase;
    uint64_t n = 0;
    int32_t v = BZ_OK;
    // (the file's verdict is not the engine's business)
    const int rc = one_shot(device, 2, OneShotIn(in + cbase, (size_t)clen), (size_t)rlen, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int drc = df_gpu_bgzf_read_device(g, g->dec_in.p, (size_t)clen, rc_off.data(), u.data() + first, (size_t)(last - first + 1), ustart,
                                                rlen, g->oneshot_out.p, (size_t)rlen, &n, &v);
        *total = (size_t)n;
        return drc;
    });
    if (rc != BZ_OK) return rc;
    *out_len = (size_t)n;
    return v != BZ_OK ? v : v_index;
}

// ---- C ABI ------------------------------------------------------------------------------------------------
extern "C" int df_gpu_encode_device(bz_gpu_engine *g, int kind, const void *d_in, size_t n, void *d_out, size_t cap,
                                    size_t *out_len)
{
    if (!g || !out_len || (!d_in && n) || kind < 0 || kind > 2) return BZ_E_PARAM;
    if (n && ((uintptr_t)d_in & 3u)) return BZ_E_PARAM;
    *out_len = 0;
    return df_encode_parts(g, kind, static_cast<const u8 *>(d_in), n, nullptr, 0, static_cast<u8 *>(d_out), cap, out_len);
}

extern "C" int df_gpu_encode_device_dict(bz_gpu_engine *g, int kind, const void *d_in, size_t n, const uint8_t *dict,
                                         size_t dict_len, void *d_out, size_t cap, size_t *out_len)
{
    if (!g || !out_len || (!d_in && n) || kind < 0 || kind > 2 || (!dict && dict_len)) return BZ_E_PARAM;
    if (n && ((uintptr_t)d_in & 3u)) return BZ_E_PARAM;
    *out_len = 0;
    return df_encode_parts(g, kind, static_cast<const u8 *>(d_in), n, dict, dict_len, static_cast<u8 *>(d_out), cap, out_len);
}

extern "C" int df_gpu_last_timings(bz_gpu_engine *g, double out_seconds[6])
{
    if (!g || !out_seconds) return BZ_E_PARAM;
    for (int i = 0; i < 6; ++i) out_seconds[i] = g->df ? g->df->t_stage[i] : 0.0;
    return BZ_OK;
}

extern "C" int df_gpu_last_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->df ? g->df->stats[i] : 0;
    return BZ_OK;
}

// test hook: the LZSS codes of the last call in stream order as (len, pos) pairs, len 0 = literal `pos`
// (what LzssEncoder::next yields, lzss/encoder.rs:203-234).  Returns the code count through *count.
extern "C" int df_gpu_debug_codes(bz_gpu_engine *g, const void *d_in, size_t n, uint32_t *out_pairs, size_t cap, size_t *count)
{
    if (!g || !g->df || !count) return BZ_E_PARAM;
    DfWorkspace *w = g->df;
    std::vector<u32> code(n);
    std::vector<u8> in(n);
    if (n) {
        HIPCHK(hipMemcpy(code.data(), w->vals_out.p, n * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(in.data(), d_in, n, hipMemcpyDeviceToHost));
    }
    size_t k = 0;
    for (size_t q = 0; q < n; ++q) {
        const u32 c = code[q];
        if (!(c & F_CODE)) continue;
        if (k < cap) {
            if (c & F_REF) { out_pairs[2 * k] = c & 511u; out_pairs[2 * k + 1] = (c >> 9) & 32767u; }
            else { out_pairs[2 * k] = 0; out_pairs[2 * k + 1] = in[q]; }
        }
        ++k;
    }
    *count = k;
    return BZ_OK;
}

// test hook: (tokens are not counted here) per block: start offset, bytes, btype, bits
extern "C" int df_gpu_debug_blocks(bz_gpu_engine *g, uint64_t *out4, size_t cap, size_t *count)
{
    if (!g || !g->df || !count) return BZ_E_PARAM;
    DfWorkspace *w = g->df;
    if (!w->h_fetched) { // (the last call's blocks are still on the device)
        HIPCHK(hipSetDevice(g->device));
        w->h_blocks.resize(w->h_nb);
        w->h_bstart.resize((size_t)w->h_nb + 1);
        if (w->h_nb) HIPCHK(hipMemcpy(w->h_blocks.data(), w->blocks.p, (size_t)w->h_nb * sizeof(DfBlock), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(w->h_bstart.data(), w->bstart.p, ((size_t)w->h_nb + 1) * 8, hipMemcpyDeviceToHost));
        w->h_fetched = true;
    }
    *count = w->h_blocks.size();
    for (size_t k = 0; k < w->h_blocks.size() && k < cap; ++k) {
        const DfBlock &b = w->h_blocks[k];
        out4[4 * k] = w->h_bstart[k];
        out4[4 * k + 1] = b.bytes;
        out4[4 * k + 2] = b.btype;
        out4[4 * k + 3] = b.btype == 0 ? (((b.bit_off + 3 + 7) & ~7ull) + 32 + 8ull * b.bytes - b.bit_off) : b.bits;
    }
    return BZ_OK;
}

extern "C" int df_encode_buffer_dict(int kind, int device, const uint8_t *in, size_t in_len, const uint8_t *dict,
                                     size_t dict_len, uint8_t **out, size_t *out_len);

extern "C" int df_encode_buffer(int kind, int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len)
{
    return df_encode_buffer_dict(kind, device, in, in_len, nullptr, 0, out, out_len);
}

extern "C" int df_encode_buffer_dict(int kind, int device, const uint8_t *in, size_t in_len, const uint8_t *dict,
                                     size_t dict_len, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len || (!in && in_len) || kind < 0 || kind > 2 || (!dict && dict_len)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    if (df_trace()) fprintf(stderr, "bz2_mi355x: df_encode_buffer entered at %.1f\n", now_ms());
    // (an engine per device is kept between one-shot calls, with its workspace and the two buffers below:
    // bz_release_cached_resources frees it)
    EngineLease lease(device, 2, 1);
    if (lease.status() != BZ_OK) return lease.status();
    bz_gpu_engine *g = lease.engine();
    const size_t cap = df_encode_bound(in_len) + 8;
    uint8_t *h = nullptr;
    size_t n_out = 0;
    int rc = g->dec_in.ensure(in_len + 64);
    if (rc == BZ_OK) rc = g->oneshot_out.ensure(cap);
    // Large inputs: the call's two copies run beside its kernels (copy_pool.h).  The input goes up in 32 MiB slices from one
    // thread, in order; the encode runs in parts (the bytes do not depend
    // on the parts, tests/test_gpu_deflate.py::test_many_part_seams_equal_oracle_golden), each as soon as its bytes have
    // arrived, and a part's bytes of the stream leave for the caller's buffer while the next part is encoded.  Rounds 1-4
    // uploaded everything, encoded, downloaded: 110 ms per GiB for 66 ms of kernels.
    if (rc == BZ_OK && in_len >= ((size_t)64 << 20)) {
        // Parts: a short first one (64 MiB: the kernels start 1.5 ms into the upload), then 256 MiB each -- a part's kernels cost
        // 1.4 ms more than its share of one pass (the block chain of a part stands behind its marking, every launch has its tail),
        // and the upload (50 GB/s) is 300 MiB ahead when the first part is over.  Eight parts of 128 MiB: 77 ms of kernels per
        // GiB instead of 66 (profiles/r05_host_copies.md).
        const u64 part_bytes = (u64)256 << 20, first_bytes = (u64)64 << 20;
        // the caller's buffer: 2 MiB-aligned memory that asks for huge pages (its pages are touched where stream bytes land, on
        // several threads, in front of each copy: 44 MB of 4 KiB pages took 5 ms, the last part's stood behind the call)
        {
            void *q = nullptr;
            const size_t want = (cap + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
            if (posix_memalign(&q, (size_t)2 << 20, want) != 0) q = nullptr;
            if (q) (void)madvise(q, want, MADV_HUGEPAGE);
            h = static_cast<uint8_t *>(q);
        }
        if (!h) rc = BZ_E_NOMEM;
        if (rc == BZ_OK) {
            CopyPool pool(device);
            const size_t S = CopyPool::slice_bytes();
            std::vector<size_t> up;
            for (size_t off = 0; off < in_len; off += S)
                up.push_back(pool.submit(static_cast<u8 *>(g->dec_in.p) + off, in + off, std::min(S, in_len - off), hipMemcpyHostToDevice));
            size_t waited = 0;
            DfPartHooks hooks;
            hooks.part_bytes = std::min<u64>(part_bytes, df_part_bytes());
            hooks.first_part_bytes = first_bytes;
            hooks.need_input = [&](u64 upto) {
                const size_t want = (size_t)std::min<u64>((upto + S - 1) / S, up.size());
                for (; waited < want; ++waited) pool.wait(up[waited]);
                return pool.failed() ? BZ_E_UNEXPECTED : BZ_OK;
            };
            hooks.part_done = [&](size_t off, size_t len) {
                if (len) pool.submit(h + off, static_cast<const u8 *>(g->oneshot_out.p) + off, len, hipMemcpyDeviceToHost, true);
            };
            rc = df_encode_parts(g, kind, static_cast<const u8 *>(g->dec_in.p), in_len, dict, dict_len, static_cast<u8 *>(g->oneshot_out.p), cap,
                                 &n_out, DfSeg(), nullptr, &hooks);
            const double t_parts = now_ms();
            pool.wait_all();
            if (df_trace()) fprintf(stderr, "bz2_mi355x: df_encode_buffer: parts over at %.1f, copies over at %.1f\n", t_parts, now_ms());
            if (rc == BZ_OK && pool.failed()) rc = BZ_E_UNEXPECTED;
        }
        if (rc != BZ_OK) { // (the buffer is not shrunk to the stream: the pages behind it were never touched)
            free(h);
            h = nullptr;
        }
    } else {
        if (rc == BZ_OK && in_len && hipMemcpy(g->dec_in.p, in, in_len, hipMemcpyHostToDevice) != hipSuccess) rc = BZ_E_UNEXPECTED;
        if (rc == BZ_OK) rc = df_gpu_encode_device_dict(g, kind, g->dec_in.p, in_len, dict, dict_len, g->oneshot_out.p, cap, &n_out);
        if (rc == BZ_OK) rc = one_shot_download(&h, g->oneshot_out.p, n_out);
    }
    lease.settle(rc);
    if (rc != BZ_OK) return rc;
    *out = h;
    *out_len = n_out;
    return BZ_OK;
}

// ---- streaming context: the Encoder::next contract of Inflater / ZlibEncoder / GZipEncoder ----------------
// Action::Run accumulates, Action::Finish encodes everything written so far (the stream of these encoders
// depends on all of the input: one 32 KiB window, one bit string).  Action::Flush is refused.
struct df_enc {
    int kind = 0, device = 0;
    std::vector<uint8_t> in, out, dict; // in: bytes written since the last segment went to the device
    size_t out_head = 0;
    bool finished = false;
    // the stream so far lives on the device: a segment needs the 32 KiB in front of it as history, a stored
    // block behind a flush up to 0xFFFF bytes, the container's checksums all of it
    bz_gpu_engine *g = nullptr;
    DevBuf d_data, d_out;
    size_t total = 0;   // stream bytes on the device
    size_t encoded = 0; // ... of which segments have been written for
    uint32_t dl = 0;    // InflaterInner.decompress_len behind the last segment (deflate/encoder.rs:267)
    bool wrote_head = false;
    int last_status = BZ_OK; // of the last df_enc_end: an engine that met an infrastructure error is not parked for others
};

extern "C" int df_enc_create(df_enc **out, int kind, int device)
{
    if (!out || kind < 0 || kind > 2) return BZ_E_PARAM;
    if (device_in_range(device) != BZ_OK) return BZ_E_NOGPU;
    df_enc *e = new df_enc();
    e->kind = kind;
    e->device = device;
    *out = e;
    return BZ_OK;
}

extern "C" int df_enc_create_dict(df_enc **out, int kind, int device, const uint8_t *dict, size_t dict_len)
{
    if ((!dict && dict_len) || (dict_len && kind == 2)) return BZ_E_PARAM;
    const int rc = df_enc_create(out, kind, device);
    if (rc == BZ_OK && dict_len) (*out)->dict.assign(dict, dict + dict_len);
    return rc;
}

extern "C" void df_enc_destroy(df_enc *e)
{
    if (!e) return;
    // (the engine is kept, with its workspace, for the next context or one-shot call on the device -- unless the context's
    // last df_enc_end met an infrastructure error: the lease's rule, host_call.h)
    if (e->g) EngineLease(e->device, e->g).settle(e->last_status);
    delete e;
}

extern "C" int df_enc_write(df_enc *e, const uint8_t *in, size_t n)
{
    if (!e || (!in && n)) return BZ_E_PARAM;
    if (e->finished) return BZ_OK; // Inflater ignores input behind the final block (deflate/encoder.rs:638-660)
    e->in.insert(e->in.end(), in, in + n);
    return BZ_OK;
}

// Action::Run (Inflater): everything stays pending (the LZSS stage holds 261 bytes of look-ahead, the block stage up
// to 0xFFFF bytes; the blocks the reference would hand out early come with the next Flush / Finish: same bytes,
// coarser moments).
// Action::Flush (Inflater only): the bytes written since the last segment are encoded as one SEGMENT -- the LZSS
// stage drained (lzss/encoder.rs:196-200, :224-226), the block closed without the final bit
// (deflate/encoder.rs:177-184, :638-647), the bit string padded to a byte (:227-235); the 32 KiB window and
// decompress_len carry over.  Action::Finish: the last segment, final bit set, container trailer.
// The zlib / gzip wrappers end their container at the first None they see, whatever the action
// (zlib/encoder.rs:131-151): see `ends_container` below.
static int df_enc_end_impl(df_enc *e, int action);
extern "C" int df_enc_end(df_enc *e, int action)
{
    if (!e || action < 0 || action > 2) return BZ_E_PARAM;
    // flush() / finish() behind the final block do nothing (:636-660), nor does Run on a bare Inflater
    if ((action == 0 && e->kind == 0) || e->finished) return e->last_status = BZ_OK;
    // the context's engine: the one it holds, a parked one or a new one; it stays with the context (df_enc_destroy ends it)
    EngineLease lease = e->g ? EngineLease(e->device, e->g) : EngineLease(e->device, 2, 0);
    e->g = lease.release();
    return e->last_status = lease.status() == BZ_OK ? df_enc_end_impl(e, action) : lease.status();
}
static int df_enc_end_impl(df_enc *e, int action)
{
    // zlib / gzip: the container ends at the first None of the inner Inflater whatever the Action
    // (zlib/encoder.rs:146-150, gzip/encoder.rs:129-133): header + what the Inflater yields under this Action
    // (Run: the whole bytes of the blocks it has closed; Flush: the flushed segment) + the trailer over everything
    // the iterator handed over; afterwards the encoder yields None and leaves its caller's iterator alone.
    const bool ends_container = e->kind != 0;
    int rc;
    const size_t add = e->in.size();
    if (e->total + add + 64 > e->d_data.cap) { // grow, keeping the stream so far
        DevBuf bigger;
        if ((rc = bigger.ensure((e->total + add) * 2 + 4096)) != BZ_OK) return rc;
        if (e->total) { // (on the engine's stream and waited for: a device-to-device copy need not be over when it returns)
            HIPCHK(hipMemcpyAsync(bigger.p, e->d_data.p, e->total, hipMemcpyDeviceToDevice, e->g->st));
            HIPCHK(hipStreamSynchronize(e->g->st));
        }
        e->d_data = std::move(bigger); // (frees the old block)
    }
    if (add) HIPCHK(hipMemcpy(e->d_data.as<u8>() + e->total, e->in.data(), add, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(e->d_data.as<u8>() + e->total + add, 0, 64, e->g->st)); // (ordered in front of the engine's kernels)
    e->total += add;
    e->in.clear();
    DfSeg seg;
    seg.prior = e->encoded;
    seg.dl0 = e->dl;
    seg.final = (action == 2);
    seg.run = (action == 0);
    seg.head = !e->wrote_head;
    seg.tail = (action == 2) || ends_container;
    const size_t n = e->total - e->encoded;
    const size_t cap = df_encode_bound(n) + 64;
    if ((rc = e->d_out.ensure(cap)) != BZ_OK) return rc;
    size_t k = 0;
    uint32_t dl = 0;
    rc = df_encode_parts(e->g, e->kind, e->d_data.as<u8>() + e->encoded, n, e->dict.data(), e->dict.size(), e->d_out.as<u8>(), cap,
                        &k, seg, &dl);
    if (rc != BZ_OK) return rc;
    if (e->out_head && e->out_head == e->out.size()) {
        e->out.clear();
        e->out_head = 0;
    }
    const size_t old = e->out.size();
    e->out.resize(old + k);
    if (k) HIPCHK(hipMemcpy(e->out.data() + old, e->d_out.p, k, hipMemcpyDeviceToHost));
    e->wrote_head = true;
    e->encoded = e->total;
    e->dl = dl;
    if (action == 2 || ends_container) {
        e->finished = true;
        e->d_data.release();
    }
    return BZ_OK;
}

extern "C" int df_enc_finished(const df_enc *e) { return e && e->finished ? 1 : 0; }

extern "C" size_t df_enc_pending(const df_enc *e) { return e ? e->out.size() - e->out_head : 0; }

extern "C" long df_enc_read(df_enc *e, uint8_t *out, size_t cap)
{
    if (!e || (!out && cap)) return BZ_E_PARAM;
    const size_t avail = e->out.size() - e->out_head;
    const size_t k = avail < cap ? avail : cap;
    if (k) memcpy(out, e->out.data() + e->out_head, k);
    e->out_head += k;
    return (long)k;
}
