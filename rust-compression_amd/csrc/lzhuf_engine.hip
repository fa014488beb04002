// lzhuf_engine.hip -- the drivers of the LZHUF decoder (include/bz2_mi355x.h section 9; kernel: k_lzhuf.hip) and encoder
// (section 10; kernels: k_deflate.hip, the batch front end and "LZHUF encode"): the device calls, their figures, and the
// host-to-host forms on an engine of the per-process cache (host_call.h).
#include "engine_state.h"
#include "batch_decode.h"
#include "k_lzhuf.h"
#include "k_deflate.h"
#include "lzh_split.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace lzhgpu;
using namespace dfgpu;

struct LzhWorkspace {
    DevBuf in, olen, ooff, rec; // the entries' ranges, their known lengths, their outputs' places, their records
    u64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    // an entry across many waves: the search waves' counts and firsts, the candidates, pieces, their records, the source map
    // and the jump rounds' counters
    DevBuf s_cnt, s_cand, s_piece, s_prec, s_map, s_jump;
    u64 split_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    double split_ms[6] = {0, 0, 0, 0, 0, 0}; // search, sizes, pieces decoded again, writing, jump, gather
    // the encoder: a sub-batch's image, the sort's two arrays (later match and code words), step words, digit counts and bases,
    // canonical orbits, the code-start bitmap, exit tables, tile entries, slot tables, blocks, their lengths, headers and
    // scratch, the streams' places, and what the debug entries move
    DevBuf e_image, e_v0, e_s, e_step, e_hist, e_tbase, e_canon, e_bm, e_tabs, e_ents, e_slots, e_tile_slot, e_bbase, e_blks, e_lens, e_hdr,
        e_lm, e_outs, e_total, e_dbg;
    u64 enc_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
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

// ---- one large entry across many waves (lzh_split.h; DESIGN_lzhuf.md section 11) --------------------------------------
// An entry of BZ_LZH_SPLIT_KIB KiB or more of compressed bytes is split (0: none is; a fraction is allowed); an entry with more
// than max(64, in_len / BZ_LZH_SPLIT_CAND_BYTES) candidates is not.  Both are read per call.
static double lzh_env_num(const char *name, double dflt)
{
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const double v = strtod(s, &end);
    return end == s || !(v >= 0) ? dflt : v;
}

extern "C" int bz_gpu_last_lzh_decode_split_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->lzh ? g->lzh->split_stats[i] : 0;
    return BZ_OK;
}
extern "C" int bz_gpu_last_lzh_decode_split_timings(bz_gpu_engine *g, double out_seconds[6])
{
    if (!g || !out_seconds) return BZ_E_PARAM;
    for (int i = 0; i < 6; ++i) out_seconds[i] = g->lzh ? g->lzh->split_ms[i] * 1e-3 : 0.0;
    return BZ_OK;
}

struct LzhSplitEntry {
    size_t index = 0;            // of the entry in the call
    std::vector<LzhPiece> chain; // the confirmed pieces in stream order, each with its place in the entry's output and its length
    LzhRec rec;                  // what the one-wave path would have left for the entry
    // its share of bz_gpu_last_lzh_decode_split_stats, of the launches and of the phases search, sizes, pieces decoded again:
    // counted in once the entry is known to stay split
    u64 st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u64 launches = 0;
    double ms[3] = {0, 0, 0};
};
struct LzhMethod {
    u32 dbits, pbits;
    int prefill;
};

// the sizes launch over n pieces, and their records
static int lzh_split_pieces(bz_gpu_engine *g, LzhWorkspace *w, LzhMethod m, const u8 *ebase, u32 elen, const LzhPiece *pcs, u32 n, LzhPieceRec *out,
                            u64 *launches)
{
    int rc = w->s_piece.ensure((size_t)n * sizeof(LzhPiece));
    if (rc == BZ_OK) rc = w->s_prec.ensure((size_t)n * sizeof(LzhPieceRec));
    if (rc != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->s_piece.p, pcs, (size_t)n * sizeof(LzhPiece), hipMemcpyHostToDevice, g->st));
    if (lzh_launch_decode_piece(g->st, false, ebase, elen, m.dbits, m.pbits, m.prefill, w->s_piece.as<LzhPiece>(), n, w->s_prec.as<LzhPieceRec>(),
                                nullptr, nullptr) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipMemcpyAsync(out, w->s_prec.p, (size_t)n * sizeof(LzhPieceRec), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    *launches += 1;
    return BZ_OK;
}

// Search, sizes and chain of one entry.  ol: its known length or kNoLen.  *fallback: the entry takes the one-wave path.
static int lzh_split_sizes(bz_gpu_engine *g, LzhWorkspace *w, LzhMethod m, const u8 *ebase, u32 elen, u64 ol, LzhSplitEntry &e, bool *fallback)
{
    using namespace lzhsplit;
    *fallback = true;
    int rc;
    double t0 = now_ms();
    // ---- every candidate, ascending: the search waves' counts, their sums, the list
    const u32 waves = lzh_split_search_waves(elen);
    if ((rc = w->s_cnt.ensure((size_t)waves * 8)) != BZ_OK) return rc;
    u32 *d_cnt = w->s_cnt.as<u32>(), *d_first = d_cnt + waves;
    if (lzh_launch_split_search(g->st, false, ebase, elen, m.dbits, m.pbits, d_cnt, nullptr, nullptr, 0) != 0) return BZ_E_UNEXPECTED;
    std::vector<u32> first(waves);
    HIPCHK(hipMemcpyAsync(first.data(), d_cnt, (size_t)waves * 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    e.launches += 1;
    u64 ncand = 0;
    for (u32 &c : first) {
        const u32 n = c;
        c = (u32)ncand;
        ncand += n;
    }
    const double per = std::max(1.0, lzh_env_num("BZ_LZH_SPLIT_CAND_BYTES", 1024.0));
    if (ncand > std::max<u64>(64, (u64)(elen / per))) return BZ_OK; // every candidate is a wave that may decode 65 535 codes
    std::vector<u64> cands((size_t)ncand);
    if (ncand) {
        if ((rc = w->s_cand.ensure((size_t)ncand * 8)) != BZ_OK) return rc;
        HIPCHK(hipMemcpyAsync(d_first, first.data(), (size_t)waves * 4, hipMemcpyHostToDevice, g->st));
        if (lzh_launch_split_search(g->st, true, ebase, elen, m.dbits, m.pbits, d_cnt, d_first, w->s_cand.as<u64>(), (u32)ncand) != 0)
            return BZ_E_UNEXPECTED;
        HIPCHK(hipMemcpyAsync(cands.data(), w->s_cand.p, (size_t)ncand * 8, hipMemcpyDeviceToHost, g->st));
        HIPCHK(hipStreamSynchronize(g->st));
        e.launches += 1;
    }
    if (!cands.empty() && cands[0] == 0) cands.erase(cands.begin()); // (piece 0 starts there whatever the header says)
    e.st[1] = cands.size();
    double t1 = now_ms();
    e.ms[0] += t1 - t0;
    // ---- every piece at once: the entry's first bit and every candidate, each to the next candidate.  Piece 0 knows its place
    // and the entry's length; the others believe their distances.
    const bool has_len = ol != kNoLen;
    const auto limit_of = [&](u64 sum) { return !has_len || ol - sum > 0xFFFFFFFEull ? kNoLimit : (u32)(ol - sum); };
    std::vector<LzhPiece> pcs(1 + cands.size());
    for (size_t k = 0; k < pcs.size(); ++k) {
        LzhPiece &q = pcs[k];
        q.start = k ? cands[k - 1] : 0;
        q.stop = k < cands.size() ? cands[k] : kNoStop;
        q.base = k ? kBaseUnknown : 0u;
        q.limit = k ? kNoLimit : limit_of(0);
        q.has_len = k ? 0u : (u32)has_len;
        q.pad = 0;
    }
    std::vector<LzhPieceRec> prs(pcs.size());
    if ((rc = lzh_split_pieces(g, w, m, ebase, elen, pcs.data(), (u32)pcs.size(), prs.data(), &e.launches)) != BZ_OK) return rc;
    t0 = now_ms();
    e.ms[1] += t0 - t1;
    // ---- the chain: a candidate's piece counts if and only if the confirmed piece in front of it stopped exactly there.  A
    // piece is decoded again, alone, with its place and what is left of the known length, where the strict distance rule, the
    // known length or the 4 GiB guard may end the stream inside it.
    e.chain.clear();
    LzhRec total{};
    u64 sum = 0, j = 0;
    size_t cur = 0;
    for (;;) {
        LzhPiece pc = pcs[cur];
        LzhPieceRec pr = prs[cur];
        pc.base = (u32)sum;
        if (cur != 0) {
            const u64 left = has_len ? ol - sum : ~0ull; // (sum < ol here: the chain ends where the length is reached)
            const bool again = (m.prefill < 0 && pr.reach > sum) || pr.r.len > left || (pr.r.len == left && pr.ended) ||
                               sum + pr.r.len > 0xFFFFFFFFull - 0x200u;
            if (again) {
                pc.limit = limit_of(sum);
                pc.has_len = (u32)has_len;
                if ((rc = lzh_split_pieces(g, w, m, ebase, elen, &pc, 1, &pr, &e.launches)) != BZ_OK) return rc;
                e.st[4] += 1;
            } else if (has_len && pr.ended && pr.r.verdict == BZ_OK && pr.r.len < left) pr.r.verdict = BZ_E_EOF; // the end (a) in front of it
        }
        pc.limit = pr.r.len; // (the writing launch)
        pc.has_len = 0;
        e.chain.push_back(pc);
        sum += pr.r.len;
        total.nblk += pr.r.nblk;
        total.nlit += pr.r.nlit;
        total.nmatch += pr.r.nmatch;
        total.flags |= pr.r.flags;
        total.end_bit = pr.r.end_bit;
        total.verdict = pr.r.verdict;
        if (pr.ended || (has_len && sum >= ol)) break;
        if (chain_next(cands.data(), cands.size(), PieceEnd{pr.r.end_bit, false}, j) != Next::Confirmed) return BZ_OK; // (the rule is broken)
        cur = 1 + (size_t)j++;
    }
    e.ms[2] += now_ms() - t0;
    if (e.chain.size() < 2 || (sum > 0xFFFFFFFFull && !(total.flags & 1u))) return BZ_OK;
    total.len = (u32)sum;
    e.rec = total;
    e.st[0] = 1;
    e.st[2] = e.chain.size();
    e.st[3] = pcs.size() - e.chain.size();
    *fallback = false;
    return BZ_OK;
}

// The bytes of one split entry at `eout`: the writing launch over the chain's pieces with its source map, pointer jumping
// until nothing moves, the gather.
static int lzh_split_write(bz_gpu_engine *g, LzhWorkspace *w, LzhMethod m, const u8 *ebase, u32 elen, u8 *eout, const LzhSplitEntry &e)
{
    const u32 n = e.rec.len, np = (u32)e.chain.size();
    if (n == 0) return BZ_OK;
    u32 *map = w->s_map.as<u32>(), *cnt = w->s_jump.as<u32>();
    int rc = w->s_piece.ensure((size_t)np * sizeof(LzhPiece));
    if (rc != BZ_OK) return rc;
    const double t0 = now_ms();
    HIPCHK(hipMemcpyAsync(w->s_piece.p, e.chain.data(), (size_t)np * sizeof(LzhPiece), hipMemcpyHostToDevice, g->st));
    if (lzh_launch_decode_piece(g->st, true, ebase, elen, m.dbits, m.pbits, m.prefill, w->s_piece.as<LzhPiece>(), np, nullptr, eout, map) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipStreamSynchronize(g->st));
    w->stats[7] += 1;
    w->split_ms[3] += now_ms() - t0;
    SplitTail t;
    rc = split_jump_gather(g->st, true, map, n, cnt, eout, t);
    w->stats[7] += t.launches;
    w->split_stats[5] += t.rounds;
    w->split_stats[6] += t.left;
    w->split_ms[4] += t.jump_ms;
    w->split_ms[5] += t.gather_ms;
    return rc;
}

// grow != nullptr: the output is the engine's own buffer, sized between the two launches (the host forms).
// h_place != nullptr: the caller has places for the outputs (multiples of 16, disjoint, entry i with room for h_orig_len[i]
// bytes, which it then must have): the archive reader's members lie in its own order among those of other calls.
static int lzh_decode_batch_core(bz_gpu_engine *g, int method, int prefill, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                                 const uint64_t *h_orig_len, size_t count, void *d_out, size_t cap, DevBuf *grow, const uint64_t *h_place,
                                 uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict)
{
    u32 dbits = 0, pbits = 0;
    if (!g || !lzh_method(method, dbits, pbits) || prefill < -1 || prefill > 255) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !h_verdict) return BZ_E_PARAM;
    if (!batch_ranges_ok(d_in, d_out, h_in_off, h_in_len, count)) return BZ_E_PARAM;
    for (size_t i = 0; h_place && i < count; ++i)
        if (!h_orig_len || h_orig_len[i] == kNoLen || (h_place[i] & 15u)) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    if (!g->lzh) g->lzh = new LzhWorkspace();
    LzhWorkspace *w = g->lzh;
    for (u64 &s : w->stats) s = 0;
    for (u64 &s : w->split_stats) s = 0;
    for (double &s : w->split_ms) s = 0;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    const LzhMethod m{dbits, pbits, prefill};
    // the entries that go across many waves, one after the other; in the launches over all entries they are entries of no bytes
    const u64 split_min = (u64)(lzh_env_num("BZ_LZH_SPLIT_KIB", 1024.0) * 1024.0);
    std::vector<LzhSplitEntry> splits;
    u64 fallbacks = 0;
    for (size_t i = 0; split_min && i < count; ++i) {
        if (h_in_len[i] < split_min) continue;
        LzhSplitEntry e;
        bool fallback = false;
        e.index = i;
        const int src = lzh_split_sizes(g, w, m, in8 + h_in_off[i], (u32)h_in_len[i], h_orig_len ? h_orig_len[i] : kNoLen, e, &fallback);
        if (src != BZ_OK) return src;
        if (!fallback && (e.rec.flags & 1u)) return BZ_E_PARAM; // an entry of 4 GiB or more of output
        w->stats[7] += e.launches;
        if (fallback) ++fallbacks;
        else splits.push_back(std::move(e));
    }
    std::vector<u64> len_small;
    fallbacks += split_reserve(splits, d_out || grow, w->s_map, w->s_jump, h_in_len, count, len_small);
    w->split_stats[7] = fallbacks;
    for (const LzhSplitEntry &e : splits) {
        for (int k = 0; k < 7; ++k) w->split_stats[k] += e.st[k];
        for (int k = 0; k < 3; ++k) w->split_ms[k] += e.ms[k];
    }
    int rc = w->in.ensure(2 * count * sizeof(u64));
    if (rc == BZ_OK) rc = w->olen.ensure(count * sizeof(u64));
    if (rc == BZ_OK) rc = w->ooff.ensure(count * sizeof(u64));
    if (rc == BZ_OK) rc = w->rec.ensure(count * sizeof(LzhRec));
    if (rc != BZ_OK) return rc;
    u64 *d_off = w->in.as<u64>(), *d_len = d_off + count, *d_ooff = w->ooff.as<u64>();
    u64 *d_olen = h_orig_len ? w->olen.as<u64>() : nullptr;
    LzhRec *d_rec = w->rec.as<LzhRec>();
    HIPCHK(hipMemcpyAsync(d_off, h_in_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(d_len, splits.empty() ? h_in_len : len_small.data(), count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    if (d_olen) HIPCHK(hipMemcpyAsync(d_olen, h_orig_len, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
    // ---- the sizes
    if (lzh_launch_decode(g->st, false, in8, d_off, d_len, d_olen, (u32)count, dbits, pbits, prefill, nullptr, nullptr, d_rec) != 0)
        return BZ_E_UNEXPECTED;
    std::vector<LzhRec> rec(count);
    HIPCHK(hipMemcpyAsync(rec.data(), d_rec, count * sizeof(LzhRec), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    for (const LzhSplitEntry &e : splits) rec[e.index] = e.rec;
    u64 need = 0;
    u8 *out8 = nullptr;
    if ((rc = batch_place(rec.data(), count, h_place, h_out_off, h_out_len, h_verdict, &need)) != BZ_OK) return rc;
    if ((rc = batch_output(need, d_out, cap, grow, &out8)) != BZ_OK) return rc;
    // ---- the bytes
    if (out8) {
        HIPCHK(hipMemcpyAsync(d_ooff, h_out_off, count * sizeof(u64), hipMemcpyHostToDevice, g->st));
        if (lzh_launch_decode(g->st, true, in8, d_off, d_len, d_olen, (u32)count, dbits, pbits, prefill, out8, d_ooff, d_rec) != 0)
            return BZ_E_UNEXPECTED;
        HIPCHK(hipStreamSynchronize(g->st));
        w->stats[7] += 2;
        for (const LzhSplitEntry &e : splits)
            if ((rc = lzh_split_write(g, w, m, in8 + h_in_off[e.index], (u32)h_in_len[e.index], out8 + h_out_off[e.index], e)) != BZ_OK) return rc;
    } else w->stats[7] += 1;
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
    return lzh_decode_batch_core(g, method, prefill, d_in, h_in_off, h_in_len, h_orig_len, count, d_out, cap, nullptr, nullptr, h_out_off, h_out_len,
                                 h_verdict);
}

// The same call with the outputs' places given (lha_engine.hip: one call per method of an archive's members).
int lzh_decode_batch_placed(bz_gpu_engine *g, int method, int prefill, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                            const uint64_t *h_orig_len, size_t count, void *d_out, size_t cap, const uint64_t *h_place, uint64_t *h_out_len,
                            int32_t *h_verdict)
{
    std::vector<uint64_t> off(count);
    return lzh_decode_batch_core(g, method, prefill, d_in, h_in_off, h_in_len, h_orig_len, count, d_out, cap, nullptr, h_place, off.data(), h_out_len,
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
    if (count == 0) return one_shot_empty(out);
    // a call the sizes launch refused (an entry of 4 GiB of output) leaves a sound engine; so do the entries' verdicts
    return one_shot(device, 0, lay, kOutGrown, kSettleParamSound, out, [&](bz_gpu_engine *g, size_t *total) {
        const int rc = lzh_decode_batch_core(g, method, prefill, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), orig_lens, count, nullptr, 0,
                                             &g->oneshot_out, nullptr, out_off, out_len, verdict);
        if (rc == BZ_OK) *total = (size_t)(out_off[count - 1] + out_len[count - 1]);
        return rc;
    });
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

// ---- the encoder (section 10 of the header; DESIGN_lzhuf.md sections 7 to 9) ------------------------------------------
constexpr u32 kLzhBatchSlots = 4096;     // inputs per sub-batch at most (a block's scratch is 134 KB)
constexpr u64 kLzhMaxInput = 1ull << 30; // positions are 32-bit
static u32 lzh_slot_tiles(u64 n) { return n ? (u32)((n + kPTile - 1) / kPTile) : 1u; }
static u32 lzh_max_blocks(u64 n) { return (u32)((n + kLzhBlockCodes - 1) / kLzhBlockCodes); } // (codes <= bytes)

// DESIGN_lzhuf.md section 8: 16 bits per input byte, 1 084 bytes of header per block, blocks <= ceil(n / 65535)
static size_t lzh_bound_one(u64 n) { return n ? (size_t)((2 * n + 1084ull * lzh_max_blocks(n) + 3u) & ~(u64)3) : 0; }

extern "C" size_t bz_lzh_encode_batch_bound(const uint64_t *in_len, size_t count)
{
    size_t s = 0;
    for (size_t i = 0; in_len && i < count; ++i) s += lzh_bound_one(in_len[i]);
    return s;
}

extern "C" int bz_gpu_last_lzh_encode_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->lzh ? g->lzh->enc_stats[i] : 0;
    return BZ_OK;
}

static int lzh_enc_workspace(bz_gpu_engine *g, LzhWorkspace **out)
{
    HIPCHK(hipSetDevice(g->device));
    if (!g->lzh) g->lzh = new LzhWorkspace();
    *out = g->lzh;
    return BZ_OK;
}

// the image of the slots and its parse: afterwards e_s holds the code words, e_bm the code starts, e_image the bytes
// (the host arrays must outlive the stream's work: the callers wait before they let go of them)
static int lzh_front(bz_gpu_engine *g, LzhWorkspace *w, u32 dbits, const u8 *d_in, const std::vector<DfSlot> &slots,
                     const std::vector<u32> &tile_slot)
{
    hipStream_t st = g->st;
    const u32 ns = (u32)slots.size(), ntiles = (u32)tile_slot.size();
    const u64 nimg = (u64)ntiles * kPTile, npad = nimg + 16;
    const u64 nchunks = df_chunks(nimg), nsort = nchunks * kLzhStride + 16;
    const u64 words = nsort > npad ? nsort : npad;
    int rc;
    if ((rc = w->e_image.ensure(nimg + 64)) != BZ_OK) return rc;
    if ((rc = w->e_v0.ensure(words * 4)) != BZ_OK) return rc;
    if ((rc = w->e_s.ensure(words * 4)) != BZ_OK) return rc;
    if ((rc = w->e_step.ensure(npad * 2)) != BZ_OK) return rc;
    if ((rc = w->e_hist.ensure((nchunks * (kLzhStride / kSortTile) + 1) * 256 * 4)) != BZ_OK) return rc;
    if ((rc = w->e_tbase.ensure(2 * (nchunks + 1) * 256 * 4)) != BZ_OK) return rc;
    if ((rc = w->e_canon.ensure((size_t)ntiles * 64 * 8 + 64)) != BZ_OK) return rc;
    if ((rc = w->e_bm.ensure((nimg / 64 + 8) * 8)) != BZ_OK) return rc;
    if ((rc = w->e_tabs.ensure(lzh_tab_entries(ntiles) * 2)) != BZ_OK) return rc;
    if ((rc = w->e_ents.ensure(lzh_ent_entries(ntiles) * 2)) != BZ_OK) return rc;
    if ((rc = w->e_slots.ensure((size_t)ns * sizeof(DfSlot))) != BZ_OK) return rc;
    if ((rc = w->e_tile_slot.ensure((size_t)ntiles * 4)) != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->e_slots.p, slots.data(), (size_t)ns * sizeof(DfSlot), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(w->e_tile_slot.p, tile_slot.data(), (size_t)ntiles * 4, hipMemcpyHostToDevice, st));
    if (df_launch_gather(st, d_in, w->e_slots.as<DfSlot>(), w->e_tile_slot.as<u32>(), ntiles, w->e_image.as<u8>(), nullptr) != 0)
        return BZ_E_UNEXPECTED;
    if (lzh_launch_front(st, dbits, w->e_image.as<u8>(), nimg, ntiles, w->e_slots.as<DfSlot>(), ns, w->e_tile_slot.as<u32>(), w->e_v0.as<u32>(),
                         w->e_s.as<u32>(), w->e_hist.as<u32>(), w->e_tbase.as<u32>(), w->e_step.as<u16>(), w->e_tabs.as<u16>(), w->e_ents.as<u16>(),
                         w->e_bm.as<u64>(), w->e_canon.as<u64>()) != 0)
        return BZ_E_UNEXPECTED;
    return BZ_OK;
}

// inputs [first, first + ns) of the call in ntiles tiles; their streams go to d_out + cursor .. in input order, *used = the
// bytes taken there (a multiple of 4)
static int lzh_batch_run(bz_gpu_engine *g, LzhWorkspace *w, u32 dbits, u32 pbits, const u8 *d_in, const uint64_t *h_in_off,
                         const uint64_t *h_in_len, size_t first, u32 ns, u32 ntiles, u8 *d_out, size_t cap, u64 cursor, uint64_t *h_out_off,
                         uint64_t *h_out_len, u64 *used)
{
    hipStream_t st = g->st;
    std::vector<DfSlot> slots(ns);
    std::vector<u32> tile_slot(ntiles), bbase((size_t)ns + 1);
    {
        u32 t = 0, b = 0;
        for (u32 j = 0; j < ns; ++j) {
            const u64 n = h_in_len[first + j];
            slots[j].src = h_in_off[first + j];
            slots[j].lo = t * kPTile;
            slots[j].len = (u32)n;
            for (u32 k = lzh_slot_tiles(n); k; --k) tile_slot[t++] = j;
            bbase[j] = b;
            b += lzh_max_blocks(n);
        }
        bbase[ns] = b;
    }
    const u32 nblks = bbase[ns];
    int rc;
    if ((rc = lzh_front(g, w, dbits, d_in, slots, tile_slot)) != BZ_OK) return rc;
    if ((rc = w->e_bbase.ensure(((size_t)ns + 1) * 4)) != BZ_OK) return rc;
    if ((rc = w->e_blks.ensure(((size_t)nblks + 1) * sizeof(LzhBlk))) != BZ_OK) return rc;
    if ((rc = w->e_lens.ensure(((size_t)nblks + 1) * kLzhLensBytes)) != BZ_OK) return rc;
    if ((rc = w->e_hdr.ensure(((size_t)nblks + 1) * kLzhHdrWords * 4)) != BZ_OK) return rc;
    if ((rc = w->e_lm.ensure(((size_t)nblks + 1) * kLzhLmWords * 4)) != BZ_OK) return rc;
    if ((rc = w->e_outs.ensure((size_t)ns * sizeof(LzhOut))) != BZ_OK) return rc;
    if ((rc = w->e_total.ensure(64)) != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->e_bbase.p, bbase.data(), ((size_t)ns + 1) * 4, hipMemcpyHostToDevice, st));
    LzhBlk *d_blks = w->e_blks.as<LzhBlk>();
    if (lzh_launch_cuts(st, w->e_slots.as<DfSlot>(), ns, w->e_bbase.as<u32>(), w->e_bm.as<u64>(), d_blks) != 0) return BZ_E_UNEXPECTED;
    if (lzh_launch_blocks(st, w->e_image.as<u8>(), w->e_s.as<u32>(), d_blks, nblks, pbits, w->e_lens.as<u8>(), w->e_hdr.as<u32>(),
                          w->e_lm.as<u32>()) != 0)
        return BZ_E_UNEXPECTED;
    if (lzh_launch_offsets(st, d_blks, w->e_bbase.as<u32>(), ns, w->e_outs.as<LzhOut>(), w->e_total.as<u64>()) != 0) return BZ_E_UNEXPECTED;
    std::vector<LzhOut> outs(ns);
    std::vector<LzhBlk> blks(nblks);
    u64 total = 0;
    HIPCHK(hipMemcpyAsync(outs.data(), w->e_outs.p, (size_t)ns * sizeof(LzhOut), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&total, w->e_total.p, 8, hipMemcpyDeviceToHost, st));
    if (nblks) HIPCHK(hipMemcpyAsync(blks.data(), d_blks, (size_t)nblks * sizeof(LzhBlk), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st)); // the one look at the device per sub-batch: the streams' sizes decide about `cap`
    HIPCHK(hipGetLastError());
    if (total > cap || cursor > cap - total) return BZ_E_CAPACITY;
    if (total) {
        HIPCHK(hipMemsetAsync(d_out + cursor, 0, (size_t)total, st)); // (emission ORs its bits into zeroed words)
        if (lzh_launch_emit(st, w->e_image.as<u8>(), w->e_s.as<u32>(), d_blks, nblks, w->e_lens.as<u8>(), w->e_hdr.as<u32>(),
                            reinterpret_cast<u32 *>(d_out + cursor)) != 0)
            return BZ_E_UNEXPECTED;
    }
    for (u32 j = 0; j < ns; ++j) {
        h_out_off[first + j] = cursor + outs[j].off;
        h_out_len[first + j] = outs[j].len;
        w->enc_stats[5] += h_in_len[first + j];
        w->enc_stats[6] += outs[j].len;
    }
    for (const LzhBlk &b : blks) {
        if (!b.ncodes) continue;
        w->enc_stats[2] += 1;
        w->enc_stats[3] += b.nlit;
        w->enc_stats[4] += b.nmatch;
        w->enc_stats[7] += b.lm;
    }
    HIPCHK(hipStreamSynchronize(st)); // (the workspace is free for the next sub-batch)
    HIPCHK(hipGetLastError());
    *used = total;
    return BZ_OK;
}

extern "C" int bz_gpu_lzh_encode_batch_device(bz_gpu_engine *g, int method, const void *d_in, const uint64_t *h_in_off,
                                              const uint64_t *h_in_len, size_t count, void *d_out, size_t cap, uint64_t *h_out_off,
                                              uint64_t *h_out_len)
{
    u32 dbits = 0, pbits = 0;
    if (!g || !lzh_method(method, dbits, pbits)) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !d_out) return BZ_E_PARAM;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 3u)) return BZ_E_PARAM;
    u64 in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 15u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i] || h_in_len[i] > kLzhMaxInput) return BZ_E_PARAM;
        in_end = h_in_off[i] + h_in_len[i];
    }
    if (in_end && !d_in) return BZ_E_PARAM;
    LzhWorkspace *w = nullptr;
    const int wrc = lzh_enc_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    for (u64 &s : w->enc_stats) s = 0;
    const u64 image_max = df_batch_image_bytes(); // (the Deflate batch path's switch, BZ_DF_BATCH_MIB)
    u64 cursor = 0;
    for (size_t i = 0; i < count;) {
        size_t j = i;
        u64 tiles = 0;
        while (j < count && j - i < kLzhBatchSlots && (j == i || (tiles + lzh_slot_tiles(h_in_len[j])) * kPTile <= image_max)) {
            tiles += lzh_slot_tiles(h_in_len[j]);
            ++j;
        }
        u64 used = 0;
        const int rc = lzh_batch_run(g, w, dbits, pbits, static_cast<const u8 *>(d_in), h_in_off, h_in_len, i, (u32)(j - i), (u32)tiles,
                                     static_cast<u8 *>(d_out), cap, cursor, h_out_off, h_out_len, &used);
        if (rc != BZ_OK) return rc;
        cursor += used;
        w->enc_stats[0] += j - i;
        w->enc_stats[1] += 1;
        i = j;
    }
    return BZ_OK;
}

extern "C" int bz_gpu_lzh_debug_codes(bz_gpu_engine *g, int method, const void *d_in, size_t n, uint32_t *out_pairs, size_t cap, size_t *count)
{
    u32 dbits = 0, pbits = 0;
    if (!g || !lzh_method(method, dbits, pbits) || !count || (cap && !out_pairs) || (n && !d_in) || n > kLzhMaxInput) return BZ_E_PARAM;
    if ((uintptr_t)d_in & 15u) return BZ_E_PARAM;
    *count = 0;
    if (!n) return BZ_OK;
    LzhWorkspace *w = nullptr;
    const int wrc = lzh_enc_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    std::vector<DfSlot> slots(1);
    slots[0].src = 0; slots[0].lo = 0; slots[0].len = (u32)n;
    std::vector<u32> tile_slot(lzh_slot_tiles(n), 0u);
    const int rc = lzh_front(g, w, dbits, static_cast<const u8 *>(d_in), slots, tile_slot);
    if (rc != BZ_OK) return rc;
    std::vector<u32> code(n);
    std::vector<u8> in(n);
    HIPCHK(hipMemcpyAsync(code.data(), w->e_s.p, n * 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(in.data(), w->e_image.p, n, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    size_t k = 0;
    for (size_t q = 0; q < n; ++q) {
        const u32 c = code[q];
        if (!(c & F_CODE)) continue;
        if (k < cap) {
            if (c & F_REF) { out_pairs[2 * k] = c & 511u; out_pairs[2 * k + 1] = (c >> 9) & 0xFFFFu; }
            else { out_pairs[2 * k] = 0; out_pairs[2 * k + 1] = in[q]; }
        }
        ++k;
    }
    *count = k;
    return BZ_OK;
}

extern "C" int bz_gpu_lzh_debug_tables(bz_gpu_engine *g, int method, const uint32_t *c_freq, const uint32_t *p_freq, uint8_t *c_len,
                                       uint8_t *p_len, uint8_t *t_len, uint32_t res[3])
{
    u32 dbits = 0, pbits = 0;
    if (!g || !lzh_method(method, dbits, pbits) || !c_freq || !p_freq || !c_len || !p_len || !t_len || !res) return BZ_E_PARAM;
    LzhWorkspace *w = nullptr;
    const int wrc = lzh_enc_workspace(g, &w);
    if (wrc != BZ_OK) return wrc;
    // [c counts 512][p counts 32][res 16][header words][lengths][scratch]
    const size_t o_p = 512, o_res = o_p + 32, o_hdr = o_res + 16, o_lens = o_hdr + kLzhHdrWords, o_lm = o_lens + kLzhLensBytes / 4;
    const int rc = w->e_dbg.ensure((o_lm + kLzhLmWords) * 4);
    if (rc != BZ_OK) return rc;
    u32 *d = w->e_dbg.as<u32>();
    HIPCHK(hipMemcpyAsync(d, c_freq, kLzhNC * 4, hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(d + o_p, p_freq, kLzhNP * 4, hipMemcpyHostToDevice, g->st));
    if (lzh_launch_tables_debug(g->st, d, d + o_p, pbits, reinterpret_cast<u8 *>(d + o_lens), d + o_hdr, d + o_lm, d + o_res) != 0)
        return BZ_E_UNEXPECTED;
    u8 lens[kLzhLensBytes];
    HIPCHK(hipMemcpyAsync(lens, d + o_lens, kLzhLensBytes, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(res, d + o_res, 12, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    memcpy(c_len, lens, kLzhNC);
    memcpy(p_len, lens + 512, kLzhNP);
    memcpy(t_len, lens + 544, kLzhNT);
    return BZ_OK;
}

// Many inputs: packed at 16-byte-aligned offsets (BatchLayout), one upload, one device call, one download.
extern "C" int bz_lzh_encode_batch(int method, int device, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t **out,
                                   uint64_t *out_off, uint64_t *out_len)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    u32 dbits = 0, pbits = 0;
    if (!lzh_method(method, dbits, pbits)) return BZ_E_PARAM;
    if (count && (!ins || !lens || !out_off || !out_len)) return BZ_E_PARAM;
    const BatchLayout lay(ins, lens, count, 16);
    if (lay.status != BZ_OK) return lay.status;
    for (size_t i = 0; i < count; ++i)
        if (lens[i] > kLzhMaxInput) return BZ_E_PARAM;
    if (count == 0) return one_shot_empty(out);
    const size_t cap = bz_lzh_encode_batch_bound(lay.in_len.data(), count);
    return one_shot(device, 0, lay, cap, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int rc = bz_gpu_lzh_encode_batch_device(g, method, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), count, g->oneshot_out.p, cap,
                                                      out_off, out_len);
        if (rc == BZ_OK) *total = (size_t)(out_off[count - 1] + out_len[count - 1]);
        return rc;
    });
}

extern "C" int bz_lzh_encode_buffer(int method, int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len || (in_len && !in)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    uint64_t off = 0, len = 0;
    const uint8_t *ins[1] = {in};
    const size_t lens[1] = {in_len};
    const int rc = bz_lzh_encode_batch(method, device, ins, lens, 1, out, &off, &len);
    if (rc != BZ_OK) return rc;
    *out_len = (size_t)len; // (the one stream lies at offset 0)
    return BZ_OK;
}
