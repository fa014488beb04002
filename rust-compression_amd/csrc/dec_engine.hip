// dec_engine.hip -- host orchestration of the BZip2 DECODE path and its C ABI
// (include/bz2_mi355x.h, section 3).  Kernels: k_dec.hip.
//
// Reference being replaced: `bytes.decode(&mut BZip2Decoder::new())` --
// BZip2DecoderBase::init_block / next (src/bzip2/decoder.rs:163-581).
//
// The record chain of a .bz2 file (stream header, blocks, end-of-stream record, next stream ...)
// is walked on the host from the per-candidate results of kernel D1; everything that touches
// payload bytes runs on the GPU.  Error behaviour follows the reference's iterator: the bytes of
// all blocks in front of the failing record are produced, then the error (a block CRC mismatch
// is only noticed after that block's bytes were handed out, decoder.rs:189-201).
#include "engine_state.h"
#include "copy_pool.h"
#include "dec_chain.h"

#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <sys/mman.h>
#include <thread>
#include <utility>

#include <algorithm>
#include <cstdlib>
#include <cstring>

static constexpr u32 kForcedSlots = 16; // blocks per batch that start without a full 48-bit magic

static bool dec_trace()
{
    static const bool on = getenv("BZ_DEC_TRACE") != nullptr;
    return on;
}

struct DecWorkspace {
    size_t slots = 0;
    DevBuf win_base, win_bytes; // the chain's windows behind the blocks' ends (see DevBits)
    DevBuf cands, count, info, sym, sel, slot, nbmax, perm, chunk_emit, tt_len, err, L, T, X, samp_next, samp_len,
        samp_off, cycle_len, sub_trans, sub_off, sub_state, work_ctr, walk_meta, seg_buf, seg_cont, long_list, out_len, thist, tbase, crc, out_base, staging, staging2, cand_all;
    hipEvent_t ev_a = nullptr, ev_b = nullptr; // fork / join of the second walk
    DevBuf ents, chain;                        // batched decode: the entry table, a group's chain results
    double t_stage[5] = {0, 0, 0, 0, 0};
    u64 stats[4] = {0, 0, 0, 0}; // candidates, blocks, streams, forced blocks
    u64 bstats[4] = {0, 0, 0, 0}; // last batch call: entries on the batch path, on the one-stream path, blocks, groups
};

void dec_workspace_free(DecWorkspace *w)
{
    if (!w) return;
    if (w->ev_a) (void)hipEventDestroy(w->ev_a);
    if (w->ev_b) (void)hipEventDestroy(w->ev_b);
    delete w;
}

static int dec_ensure(DecWorkspace *w, size_t slots)
{
    if (slots <= w->slots) return BZ_OK;
    int rc = BZ_OK;
    const size_t s = slots;
    if ((rc = w->cands.ensure(s * sizeof(DecCand))) || (rc = w->info.ensure(s * sizeof(DecBlockInfo))) ||
        (rc = w->sym.ensure(s * (size_t)kMtfStride * 2 + 64)) || (rc = w->sel.ensure(s * 32768)) ||
        (rc = w->slot.ensure(s * 4)) || (rc = w->nbmax.ensure(s * 4)) ||
        (rc = w->perm.ensure(s * (size_t)kMaxMtfChunks * 256)) || (rc = w->chunk_emit.ensure(s * (size_t)kMaxMtfChunks * 4)) ||
        (rc = w->tt_len.ensure(s * 4)) || (rc = w->err.ensure(s * 4)) || (rc = w->L.ensure(s * (size_t)kSlot + 64)) ||
        (rc = w->T.ensure(s * (size_t)kSlot * 4)) || (rc = w->X.ensure(s * (size_t)kSlot + 64)) ||
        (rc = w->samp_next.ensure(s * (size_t)kDecSamples * 4)) || (rc = w->samp_len.ensure(s * (size_t)kDecSamples * 4)) ||
        (rc = w->samp_off.ensure(s * (size_t)kDecSamples * 4)) || (rc = w->cycle_len.ensure(s * 4)) ||
        (rc = w->sub_trans.ensure(s * (size_t)kDecSubs * 16)) || (rc = w->sub_off.ensure(s * (size_t)(kDecSubs + 1) * 4)) ||
        (rc = w->sub_state.ensure(s * (size_t)kDecSubs)) || (rc = w->work_ctr.ensure(2048)) || (rc = w->walk_meta.ensure(s * 16)) || (rc = w->seg_buf.ensure(s * (size_t)kDecSamples * kSegCap + 64)) ||
        (rc = w->seg_cont.ensure(s * (size_t)kDecSamples * 4)) || (rc = w->long_list.ensure(s * (size_t)kDecSamples * 4)) ||
        (rc = w->out_len.ensure(s * 4)) || (rc = w->thist.ensure(s * (size_t)kTilesPerBlock * 256 * 4)) ||
        (rc = w->tbase.ensure(s * 256 * 4)) || (rc = w->crc.ensure(s * 4)) || (rc = w->out_base.ensure(s * 8)))
        return rc;
    w->slots = slots;
    return BZ_OK;
}

namespace {

// BitReader<Left> over the input in HBM, for the few header bytes the host looks at.  A read at
// the end of the input returns the bits that are left as a shorter number (bitio/reader.rs:70-186).
struct DevBits {
    const u8 *d = nullptr;
    u64 nbytes = 0;
    u8 buf[64];
    u64 base = ~0ull; // byte offset of buf[0]
    u64 len = 0;
    bool failed = false;
    // 64-byte windows fetched ahead in ONE copy (the bytes behind every block of a batch: a stream's trailer and the
    // next stream's header lie there; a file of many short streams -- pbzip2, lbzip2 -- otherwise costs a synchronous
    // 64-byte copy per stream, 14 us each): sorted window bases and the windows' bytes
    std::vector<u64> pre_base;
    std::vector<u8> pre_bytes;
    u32 byte_at(u64 i)
    {
        if (i >= nbytes) return 0;
        if (!(base != ~0ull && i >= base && i < base + len) && !pre_base.empty()) {
            // the last window that starts at or in front of byte i
            size_t lo = 0, hi = pre_base.size();
            while (lo < hi) {
                const size_t mid = (lo + hi) >> 1;
                if (pre_base[mid] <= i) lo = mid + 1; else hi = mid;
            }
            if (lo > 0 && i < pre_base[lo - 1] + 64u) return pre_bytes[(lo - 1) * 64u + (size_t)(i - pre_base[lo - 1])];
        }
        if (base == ~0ull || i < base || i >= base + len) {
            base = i & ~(u64)15;
            len = (nbytes - base < sizeof(buf)) ? nbytes - base : sizeof(buf);
            if (hipMemcpy(buf, d + base, len, hipMemcpyDeviceToHost) != hipSuccess) {
                failed = true;
                memset(buf, 0, sizeof(buf));
            }
        }
        return buf[i - base];
    }
    u32 read(u64 &pos, u32 nbits)
    {
        const u64 total = nbytes * 8;
        const u64 avail = total > pos ? total - pos : 0;
        const u32 k = avail < nbits ? (u32)avail : nbits;
        u32 v = 0;
        for (u32 i = 0; i < k; ++i) {
            const u64 b = pos + i;
            v = (v << 1) | ((byte_at(b >> 3) >> (7u - (u32)(b & 7u))) & 1u);
        }
        pos += k;
        return v;
    }
};

// where decoded bytes go
// Decoded bytes on the host: a plain growable buffer (no value initialisation -- a std::vector's resize() writes every
// byte before the copy from the device does), in 2 MiB-aligned memory that asks for huge pages: the first touch of a
// GiB of fresh 4 KiB pages costs 0.2 s, more than its decode.  free() takes it (bz_free).
struct HostBuf {
    u8 *p = nullptr;
    size_t len = 0, cap = 0;
    int reserve(size_t need)
    {
        if (need <= cap) return BZ_OK;
        size_t want = std::max(need, cap + cap / 2 + 4096);
        void *q = nullptr;
        if (want >= ((size_t)4 << 20)) {
            want = (want + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
            if (posix_memalign(&q, (size_t)2 << 20, want) != 0) q = nullptr;
            if (q) (void)madvise(q, want, MADV_HUGEPAGE);
        } else {
            q = malloc(want);
        }
        if (!q) return BZ_E_NOMEM;
        if (len) memcpy(q, p, len);
        free(p);
        p = static_cast<u8 *>(q);
        cap = want;
        return BZ_OK;
    }
    void drop_front(size_t k)
    {
        if (k >= len) {
            len = 0;
            return;
        }
        memmove(p, p + k, len - k);
        len -= k;
    }
    u8 *release() // the caller owns the bytes now
    {
        u8 *q = p;
        p = nullptr;
        len = cap = 0;
        return q;
    }
    ~HostBuf() { free(p); }
};

// Incremental decode (the streaming context): the chain's state between two calls, and whether
// more input may follow.  A call that is not the last one stops in front of the first record it
// cannot be sure about (not wholly inside the bytes it has, or failing -- which near the end of a
// buffer may just mean "cut off"); the caller keeps the input from `pos` on and calls again.
struct Resume : ChainState { // pos: bit position of the next record (in: inside the buffer handed in; out: likewise)
    bool final = true;    // no more input will come
    bool stopped = false; // out: stopped in front of an unsure record, nothing wrong so far
};

struct Sink {
    u8 *d_out = nullptr; // device destination (device API) or nullptr
    u64 cap = 0;
    bool dry = false;    // sizes only
    HostBuf *host = nullptr; // host destination, one growing buffer (the one-shot call over host buffers)
    // host destination, a buffer of its own for every sub-batch (the streaming context: its reader takes the bytes of a
    // sub-batch while the next one is rebuilt): seg_alloc(n) -> n bytes of fresh memory or nullptr, seg_done(p, n, ok) when
    // the bytes have landed there -- on the copying thread -- or the copy failed
    std::function<u8 *(size_t)> seg_alloc;
    std::function<bool(u8 *)> seg_fresh; // (optional) are the pages of this buffer untouched?  (default: yes)
    std::function<void(u8 *, size_t, bool)> seg_done;
    DevBuf *staging[2] = {nullptr, nullptr}; // ... through these, sub-batch by sub-batch in turn
    CopyPool *pool = nullptr; // ... copied by its thread while the next sub-batch's kernels run (nullptr: one hipMemcpy per batch)
    u64 produced = 0;
    bool to_host() const { return host != nullptr || (bool)seg_alloc; }
    // (the streaming context's two lanes, see bz_dec) chain_final(state): the record chain of this call has been walked to
    // its end -- `state` is what the next call starts from -- and only the rebuilding of its blocks is left: the next chunk's
    // scan and Huffman stage may begin beside it.  before_output(): called once in front of the first block that is rebuilt;
    // waits until the chunk in front has handed out all its bytes; false = give up (an error in front, or the context ends).
    std::function<void(const Resume &)> chain_final;
    std::function<bool()> before_output;
    bool aborted = false;
};

} // namespace

#define HIPDEC(x)                                                                                     \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "bz2_mi355x: HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__,   \
                    __LINE__);                                                                        \
            return BZ_E_UNEXPECTED;                                                                   \
        }                                                                                             \
    } while (0)

// Multi-GPU decode: every rank holds the whole compressed file, scans it, and runs D1 on its own
// contiguous range of block candidates.  What the record chain needs from every candidate is
// exchanged with one all-gather; each rank then links the chain (the same, cheap host loop) and
// rebuilds the true blocks of its own range into its own output slice.  A second all-gather
// settles where the stream failed, if it did, and where each slice sits in the decoded file.
namespace {
struct ShardRec { // what the chain needs to know about one candidate
    u64 end_bit;
    u32 status, stored_crc, next_head, next_bits;
};
struct ShardSum { // one rank's result
    u64 bytes;      // bytes of its blocks up to (CRC failure: including) its first failing block
    u64 fail_ord;   // ordinal (in stream order) of its first failing block, ~0 if none
    u64 first_ord;  // ordinal of its first block (~0: it owns none)
    u64 pad;
};
struct Shard {
    int rank = 0, world = 1;
    bz_allgather_fn allgather = nullptr;
    void *ctx = nullptr;
    u64 out_offset = 0, total_len = 0; // results
    int phase = 0; // exchanges this rank has been through: 0 none, 1 the candidate records, 2 all (or the transport failed)
};
} // namespace

// The D1 workspace for `nc` candidates: blocks in flight per D1 launch -- BZ_DEC_BATCH (read on every call), default 4096,
// about 13 MB of workspace each; or exactly `want` of them: a rank's share of a sharded decode has to fit one batch
// (BZ_E_NOMEM otherwise, reported to the peers by the caller) -- and kForcedSlots on top.  Never more of them than about
// half of the free HBM holds (the decoded bytes need room too).
static int dec_plan_slots(DecWorkspace *w, size_t nc, u32 want, u32 *slots)
{
    u32 B = want ? want : 4096;
    if (const char *e = want ? nullptr : getenv("BZ_DEC_BATCH")) {
        const long v = atol(e);
        if (v >= 1 && v <= 65536) B = (u32)v;
    }
    if (nc < B) B = (u32)(nc ? nc : 1);
    const size_t per_slot = sizeof(DecCand) + sizeof(DecBlockInfo) + (size_t)kMtfStride * 2 + 32768 + 8 +
                            (size_t)kMaxMtfChunks * 260 + (size_t)kSlot * 6 + (size_t)kDecSamples * (16 + kSegCap) +
                            (size_t)kDecSubs * 21 + (size_t)kTilesPerBlock * 1024 + 2048;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && w->slots < (size_t)B + kForcedSlots) {
        const size_t have = w->slots * per_slot; // what the workspace already holds is free to reuse
        const size_t fit = (free_b / 2 + have) / per_slot;
        if (fit < (size_t)B + kForcedSlots) {
            const u32 fits = fit > kForcedSlots + 1 ? (u32)(fit - kForcedSlots) : 1u;
            if (want && fits < B) return BZ_E_NOMEM;
            B = fits;
        }
    }
    *slots = B;
    return dec_ensure(w, (size_t)B + kForcedSlots);
}
// the workspace behind a DecArgs (the caller sets nb, slot and nblock_max), and the launch shapes that follow the
// largest block of the blocks at hand
static void dec_args_bind(const DecWorkspace *w, DecArgs &a)
{
    a.info = w->info.as<DecBlockInfo>();
    a.sym = w->sym.as<u16>();
    a.perm = w->perm.as<u8>();
    a.chunk_emit = w->chunk_emit.as<u32>();
    a.tt_len = w->tt_len.as<u32>();
    a.err = w->err.as<u32>();
    a.L = w->L.as<u8>();
    a.T = w->T.as<u32>();
    a.X = w->X.as<u8>();
    a.samp_next = w->samp_next.as<u32>();
    a.samp_len = w->samp_len.as<u32>();
    a.samp_off = w->samp_off.as<u32>();
    a.cycle_len = w->cycle_len.as<u32>();
    a.sub_trans = w->sub_trans.as<uint4>();
    a.sub_off = w->sub_off.as<u32>();
    a.sub_state = w->sub_state.as<u8>();
    a.work_ctr = w->work_ctr.as<u32>();
    a.walk_meta = w->walk_meta.as<uint4>();
    a.seg_buf = w->seg_buf.as<u8>();
    a.seg_cont = w->seg_cont.as<u32>();
    a.long_list = w->long_list.as<u32>();
    a.out_len = w->out_len.as<u32>();
    a.thist = w->thist.as<u32>();
    a.tbase = w->tbase.as<u32>();
    a.crc = w->crc.as<u32>();
}
static void dec_args_shape(DecArgs &a, u32 max_bytes, u32 max_nsym)
{
    // The chunk kernels: the workgroups the largest block's chunks need, made ODD.  Workgroups go round the eight
    // XCDs and, inside an XCD, round its four shader engines: with FEW filled workgroups per block at a stride
    // that shares a factor with 4 (level 1: one filled workgroup per block, the other 13 of a full slot's 14
    // idle) the filled ones met on half or a quarter of the shader engines -- MTF stage of 1 GiB at level 1:
    // 15.3 ms with 1 workgroup per block, 30 with 2, 59 with 4, 17 with 3 or 7, 32 with 14, 123 with 56.
    const u32 cw_full = (kMaxMtfChunks + 255) / 256, chunks = (max_nsym + kMtfChunk - 1) / kMtfChunk;
    a.cw = std::min<u32>(cw_full, std::max<u32>(1u, (chunks + 255) / 256)) | 1u;
    a.tiles = std::min<u32>(kTilesPerBlock, (max_bytes + kSortTile - 1) / kSortTile);
    a.sub_wgs = std::min<u32>((kDecSubs + 255) / 256, ((max_bytes + 63) / 64 + 255) / 256);
}

// ---- what the two drivers share: the frame of a call, and the stages D0, D2 + D3, D4 ---------------------------
namespace {

constexpr u32 kWalkWgs = 256; // persistent walker workgroups (bounds the window of blocks being walked; 128 ... 1024 measured: profiles/r04_decode_walk_schedule.md)

// the true blocks of a batch or group in stream order: device slot, 100000 * level, stored CRC, symbols
struct TrueBlock {
    u32 slot, max_len, crc, nsym;
};
typedef std::vector<TrueBlock> TrueBlocks;

// D2 + D3 of `nb` blocks: their launch arguments, and what came back
struct Rebuilt {
    DecArgs a;
    std::vector<u32> err, len;
};

// The frame of one decode call: device, workspace, the fork / join events of the second walk, and two timing events
// around every stage (destroyed whatever way the call is left).
struct DecCall {
    bz_gpu_engine *g = nullptr;
    DecWorkspace *w = nullptr;
    hipStream_t st = nullptr;
    KernelProf *prof = nullptr; // per-kernel records (the one-stream driver sets it when the engine's profiler is on)
    double *t_acc = nullptr;    // where stage times add up: the workspace's t_stage, or the sums of a batch call
    hipEvent_t ev[2] = {nullptr, nullptr};
    int open(bz_gpu_engine *g_, double *sums = nullptr)
    {
        g = g_;
        HIPDEC(hipSetDevice(g->device));
        if (!g->dec) g->dec = new DecWorkspace();
        w = g->dec;
        if (!w->ev_a) {
            HIPDEC(hipEventCreateWithFlags(&w->ev_a, hipEventDisableTiming));
            HIPDEC(hipEventCreateWithFlags(&w->ev_b, hipEventDisableTiming));
        }
        st = g->st;
        for (double &t : w->t_stage) t = 0;
        for (u64 &s : w->stats) s = 0;
        t_acc = sums ? sums : w->t_stage;
        HIPDEC(hipEventCreate(&ev[0]));
        HIPDEC(hipEventCreate(&ev[1]));
        return BZ_OK;
    }
    ~DecCall()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void stage_time(int stage)
    {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) t_acc[stage] += ms * 1e-3;
    }

    // ---- D0: every bit position that carries the 48-bit block magic, in the order `less`.  launch(cands, cap, count)
    // scans; a first attempt that finds more than `cap` is repeated once with the count it reported.
    template <class Launch, class Less>
    int dec_scan_candidates(u32 cap, Launch launch, Less less, std::vector<DecCand> &cands)
    {
        int rc;
        if ((rc = w->count.ensure(16))) return rc;
        for (int attempt = 0; attempt < 2; ++attempt) {
            if ((rc = w->cand_all.ensure((size_t)cap * sizeof(DecCand)))) return rc;
            HIPDEC(hipEventRecord(ev[0], st));
            launch(w->cand_all.as<DecCand>(), cap, w->count.as<u32>());
            HIPDEC(hipEventRecord(ev[1], st));
            u32 cnt = 0;
            HIPDEC(hipMemcpyAsync(&cnt, w->count.p, 4, hipMemcpyDeviceToHost, st));
            HIPDEC(hipStreamSynchronize(st));
            stage_time(0);
            if (cnt <= cap) {
                cands.resize(cnt);
                if (cnt) HIPDEC(hipMemcpy(cands.data(), w->cand_all.p, (size_t)cnt * sizeof(DecCand), hipMemcpyDeviceToHost));
                break;
            }
            cap = cnt;
        }
        cands.erase(std::remove_if(cands.begin(), cands.end(), [](const DecCand &x) { return x.type != 1u; }), cands.end());
        std::sort(cands.begin(), cands.end(), less);
        return BZ_OK;
    }

    // ---- D2, D3: the blocks tb[s0, s0 + nb) from Huffman symbols to the RLE1 image.  (s0 == 0 uploads the whole list.)
    int dec_rebuild(const TrueBlocks &tb, u32 s0, u32 nb, Rebuilt &r)
    {
        r.err.assign(nb, 0);
        r.len.assign(nb, 0);
        DecArgs &a = r.a;
        a.nb = nb;
        // The launches of the T-vector sort and of the RLE1 undo follow the largest block at hand (bytes from the
        // stream's level); small gain, low levels only (level 1: 64.3 -> 63 ms per GiB).
        u32 max_bytes = 1, max_nsym = 1;
        for (u32 i = s0; i < s0 + nb; ++i) {
            max_bytes = std::max(max_bytes, tb[i].max_len);
            max_nsym = std::max(max_nsym, tb[i].nsym);
        }
        dec_args_shape(a, max_bytes, max_nsym);
        dec_args_bind(w, a);
        a.slot = w->slot.as<u32>() + s0;
        a.nblock_max = w->nbmax.as<u32>() + s0;
        if (!nb) return BZ_OK;
        std::vector<u32> up; // (lives until the stream has been waited for)
        if (s0 == 0) {
            up.resize(2 * tb.size()); // slots, then lengths
            for (size_t i = 0; i < tb.size(); ++i) up[i] = tb[i].slot, up[tb.size() + i] = tb[i].max_len;
            HIPDEC(hipMemcpyAsync(w->slot.p, up.data(), tb.size() * 4, hipMemcpyHostToDevice, st));
            HIPDEC(hipMemcpyAsync(w->nbmax.p, up.data() + tb.size(), tb.size() * 4, hipMemcpyHostToDevice, st));
        }
        HIPDEC(hipMemsetAsync(w->err.p, 0, (size_t)nb * 4, st));
        HIPDEC(hipMemsetAsync(w->out_len.p, 0, (size_t)nb * 4, st));
        HIPDEC(hipEventRecord(ev[0], st));
        int mtf_rec = -1, wrec[4] = {-1, -1, -1, -1};
        launch_dec_mtf(st, a, prof, &mtf_rec);
        HIPDEC(hipEventRecord(ev[1], st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(1);
        HIPDEC(hipEventRecord(ev[0], st));
        launch_dec_walks(st, a, kWalkWgs, g->st2, w->ev_a, w->ev_b, prof, wrec);
        HIPDEC(hipEventRecord(ev[1], st));
        std::vector<u32> h_tt(prof ? nb : 0);
        if (prof) HIPDEC(hipMemcpyAsync(h_tt.data(), w->tt_len.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipMemcpyAsync(r.err.data(), w->err.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipMemcpyAsync(r.len.data(), w->out_len.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(2);
        if (prof) { // algorithmic bytes per stage, now that symbol counts and block lengths are known
            u64 nsym = 0, ntt = 0;
            for (u32 i = 0; i < nb; ++i) {
                nsym += tb[s0 + i].nsym;
                ntt += r.err[i] ? 0 : h_tt[i];
            }
            prof->set_bytes(mtf_rec, nsym * 4 + ntt);    // symbols read twice (2 B), column written
            prof->set_bytes(wrec[0], ntt * (1 + 1 + 4)); // column read twice, T written
            prof->set_bytes(wrec[1], ntt * (4 + 1));     // one T entry read, one byte kept per step
            prof->set_bytes(wrec[2], ntt * 2);           // rows read, image written
            prof->set_bytes(wrec[3], ntt * (1 + 16.0 / 64 + 1)); // image read twice + tables
        }
        return BZ_OK;
    }

    // ---- D4: the bytes of the rebuilt blocks at dst + base[i], and their CRCs.  r.err[first_mark ...] goes up first:
    // a block marked there writes nothing.
    int dec_emit(const Rebuilt &r, u32 first_mark, const std::vector<u64> &base, u64 bytes, u32 max_len, u8 *dst, std::vector<u32> &h_crc)
    {
        const u32 nb = r.a.nb;
        if (first_mark < nb)
            HIPDEC(hipMemcpyAsync(w->err.as<u32>() + first_mark, r.err.data() + first_mark, (size_t)(nb - first_mark) * 4, hipMemcpyHostToDevice, st));
        HIPDEC(hipMemcpyAsync(w->out_base.p, base.data(), (size_t)nb * 8, hipMemcpyHostToDevice, st));
        HIPDEC(hipEventRecord(ev[0], st));
        int xrec = prof ? prof->begin(st, KID_DEC_RLE, bytes) : -1;
        launch_dec_expand(st, r.a, w->out_base.as<u64>(), dst);
        if (prof) prof->end(st, xrec);
        xrec = prof ? prof->begin(st, KID_DEC_CRC, bytes) : -1;
        launch_dec_crc(st, r.a, w->out_base.as<u64>(), dst, max_len, g->crc_tab.as<u32>(), g->xp2.as<u32>(), g->xp16.as<u32>());
        if (prof) prof->end(st, xrec);
        HIPDEC(hipEventRecord(ev[1], st));
        h_crc.resize(nb);
        HIPDEC(hipMemcpyAsync(h_crc.data(), w->crc.p, (size_t)nb * 4, hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(3);
        return BZ_OK;
    }
};

} // namespace

// ---- one stream (or a file of concatenated streams) ------------------------------------------------------------
namespace {

// The state of one decode_core call.  run() reads as the stages of a batch: D1, (sharded) the exchange of candidate
// records, the record chain, D2..D4 with delivery, (sharded) the exchange of results.
struct DecRun : DecCall {
    const u8 *d_in;
    u64 n;
    Sink &sink;
    int *verdict;
    Shard *sh;
    Resume *rs;
    const u64 nbits = n * 8ull;
    std::vector<DecCand> cands;
    size_t nc = 0, c0 = 0, c1 = 0; // candidates; [c0, c1) are this rank's
    size_t ci = 0;                 // first candidate of the batch at hand
    u32 B = 0, Bphys = 0;          // blocks per batch as the chain sees them, and device slots
    int inject_rank = -1, inject_phase = -1; // (tests) BZ_DEC_SHARD_FAIL=<rank>:<phase>: that rank fails on its own there
    DevBits rd;
    std::vector<DecBlockInfo> hinfo, hphys; // D1's results by chain slot, and (sharded) by device slot
    ChainState cs, rec; // the chain, and its state at the start of the record being looked at (what a partial call falls back to)
    bool partial = false; // more input may follow: do not judge what is near the end
    // host destination: sub-batches leave through the two staging buffers in turn (see Sink)
    u32 batch_no = 0;
    size_t stage_ticket[2] = {0, 0};
    bool stage_busy[2] = {false, false};
    // whatever way the call is left, the copies in flight are over when it returns (the staging buffers and the caller's
    // buffer outlive them)
    ~DecRun()
    {
        if (sink.to_host() && sink.pool) sink.pool->wait_all();
    }

    // ---- D1 over the batch's candidates (sharded: over this rank's share of all of them)
    int d1_batch(u32 nb1)
    {
        const size_t d1_first = sh ? c0 : ci;
        const u32 d1_count = sh ? (u32)(c1 - c0) : nb1;
        DecBlockInfo *d1_host = sh ? hphys.data() : hinfo.data();
        if (!d1_count) return BZ_OK;
        HIPDEC(hipMemcpyAsync(w->cands.p, cands.data() + d1_first, (size_t)d1_count * sizeof(DecCand), hipMemcpyHostToDevice, st));
        HIPDEC(hipEventRecord(ev[0], st));
        const int prec = prof ? prof->begin(st, KID_DEC_BLOCK, 0) : -1;
        launch_dec_blocks(st, d_in, n, w->cands.as<DecCand>(), d1_count, w->info.as<DecBlockInfo>(), w->sym.as<u16>(), w->sel.as<u8>());
        if (prof) prof->end(st, prec);
        HIPDEC(hipEventRecord(ev[1], st));
        HIPDEC(hipMemcpyAsync(d1_host, w->info.p, (size_t)d1_count * sizeof(DecBlockInfo), hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(0);
        const int rc = prefetch_windows(d1_host, d1_count);
        if (rc) return rc;
        if (prec >= 0) { // algorithmic bytes of D1: the compressed bits of its candidates + 2 B per symbol
            u64 by = 0;
            for (u32 i = 0; i < d1_count; ++i)
                by += (d1_host[i].end_bit > cands[d1_first + i].bitpos ? (d1_host[i].end_bit - cands[d1_first + i].bitpos) / 8 : 0) +
                      2ull * d1_host[i].nsym;
            prof->set_bytes(prec, by);
        }
        return BZ_OK;
    }

    // the 64 bytes behind every candidate's end, in one copy: what the chain reads at stream ends (see DevBits)
    int prefetch_windows(const DecBlockInfo *info, u32 count)
    {
        std::vector<u64> bases;
        bases.reserve(count);
        for (u32 i = 0; i < count; ++i) {
            const u64 b = (info[i].end_bit >> 3) & ~(u64)15;
            if (b < n && (bases.empty() || bases.back() != b)) bases.push_back(b);
        }
        std::sort(bases.begin(), bases.end());
        bases.erase(std::unique(bases.begin(), bases.end()), bases.end());
        rd.pre_base.clear();
        rd.pre_bytes.clear();
        if (bases.size() < 4) return BZ_OK; // (a handful of streams: the copies on demand are as cheap)
        int rc;
        if ((rc = w->win_base.ensure(bases.size() * 8)) || (rc = w->win_bytes.ensure(bases.size() * 64))) return rc;
        HIPDEC(hipMemcpyAsync(w->win_base.p, bases.data(), bases.size() * 8, hipMemcpyHostToDevice, st));
        launch_dec_gather_windows(st, d_in, n, w->win_base.as<u64>(), (u32)bases.size(), w->win_bytes.as<u8>());
        rd.pre_bytes.resize(bases.size() * 64);
        HIPDEC(hipMemcpyAsync(rd.pre_bytes.data(), w->win_bytes.p, bases.size() * 64, hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        rd.pre_base.swap(bases);
        return BZ_OK;
    }

    // (sharded) the status round, then every rank learns what the chain needs about every candidate
    int exchange_records()
    {
        // Before the exchange whose size depends on the scan: 8 bytes of status per rank.  A rank that
        // failed on its own before this point (memory, a HIP error) reports it here (the caller of
        // decode_core does, bz_gpu_decode_device_sharded) and every rank returns that error instead of
        // waiting in a collective its peer never enters.
        int64_t st0 = 0;
        std::vector<int64_t> sts((size_t)sh->world, 0);
        if (sh->allgather(sh->ctx, &st0, 8, sts.data()) != 0) {
            sh->phase = 2;
            return BZ_E_UNEXPECTED;
        }
        for (int r = 0; r < sh->world; ++r)
            if (sts[(size_t)r] != 0) {
                sh->phase = 2;
                return (int)sts[(size_t)r];
            }
        const size_t maxc = (nc + (size_t)sh->world - 1) / (size_t)sh->world;
        std::vector<ShardRec> mine(maxc ? maxc : 1), all((maxc ? maxc : 1) * (size_t)sh->world);
        memset(mine.data(), 0, mine.size() * sizeof(ShardRec));
        for (size_t i = 0; i < c1 - c0; ++i)
            mine[i] = ShardRec{hphys[i].end_bit, hphys[i].status, hphys[i].stored_crc, hphys[i].next_head, hphys[i].next_bits};
        if (sh->allgather(sh->ctx, mine.data(), mine.size() * sizeof(ShardRec), all.data()) != 0) {
            sh->phase = 2;
            return BZ_E_UNEXPECTED;
        }
        sh->phase = 1; // from here on a rank-local error travels in the second exchange (ShardSum.pad)
        if (inject_rank == sh->rank && inject_phase == 1) return BZ_E_UNEXPECTED;
        for (int r = 0; r < sh->world; ++r) {
            const size_t r0 = nc * (size_t)r / (size_t)sh->world, r1 = nc * (size_t)(r + 1) / (size_t)sh->world;
            for (size_t i = r0; i < r1; ++i) {
                const ShardRec &s = all[(size_t)r * mine.size() + (i - r0)];
                DecBlockInfo &bi = hinfo[i];
                bi.end_bit = s.end_bit;
                bi.status = s.status;
                bi.stored_crc = s.stored_crc;
                bi.next_head = s.next_head;
                bi.next_bits = s.next_bits;
                bi.nsym = (i >= c0 && i < c1) ? hphys[i - c0].nsym : 0;
            }
        }
        return BZ_OK;
    }

    // a block that starts without its full 48-bit magic has no candidate: D1 for it alone, into a forced slot
    int decode_forced(u32 slot)
    {
        const DecCand fc = {cs.pos, 1, 0};
        HIPDEC(hipMemcpyAsync(w->cands.as<DecCand>() + slot, &fc, sizeof(fc), hipMemcpyHostToDevice, st));
        HIPDEC(hipEventRecord(ev[0], st));
        launch_dec_blocks(st, d_in, n, w->cands.as<DecCand>() + slot, 1, w->info.as<DecBlockInfo>() + slot,
                          w->sym.as<u16>() + (size_t)slot * kMtfStride, w->sel.as<u8>() + (size_t)slot * 32768u);
        HIPDEC(hipEventRecord(ev[1], st));
        HIPDEC(hipMemcpyAsync(&hinfo[slot], w->info.as<DecBlockInfo>() + slot, sizeof(DecBlockInfo), hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(0);
        w->stats[3] += 1;
        return BZ_OK;
    }

    // ---- the record chain through this batch (the rules: dec_chain.h; the policy of batches, forced slots and partial
    // input: here).  term 0: the batch ended, more to come; 1: the end of the input, cleanly; 2: (partial) stopped in
    // front of the record at `rec`; < 0: the decoder's verdict
    int walk_chain(u32 nb1, TrueBlocks &tb, int &term)
    {
        u32 nforced = 0;
        size_t cj = ci;
        for (;;) {
            rec = cs;
            if (partial && nbits - cs.pos < 256) { // a header, a trailer or a block start may be cut off here
                term = 2;
                break;
            }
            const ChainEvent ev = chain_open_record(cs, rd, nbits);
            if (ev == ChainEvent::StreamEnd) continue;
            if (ev != ChainEvent::Block) {
                term = ev == ChainEvent::End ? 1 : ev == ChainEvent::Data ? BZ_E_DATA : ev == ChainEvent::MagicFirst ? BZ_E_MAGIC_FIRST : BZ_E_MAGIC;
                break;
            }
            while (cj < nc && cands[cj].bitpos < cs.pos) ++cj;
            u32 slot;
            if (cj < nc && cands[cj].bitpos == cs.pos) {
                if (cj >= ci + nb1) break; // decoded by the next batch
                slot = (u32)(cj - ci);
            } else {
                if (sh) return BZ_E_UNEXPECTED; // (a sharded decode needs every block to carry its full magic)
                if (nforced == kForcedSlots) break;
                slot = B + nforced++;
                const int rc = decode_forced(slot);
                if (rc) return rc;
            }
            const DecBlockInfo &bi = hinfo[slot];
            // (partial) a block that ends at the edge of what has arrived, or fails and starts within one
            // maximal block of that edge, may just be cut off: look again with more input.  A block that
            // fails further in front cannot be repaired by more input (a record is at most a header of
            // < 2^16 bits and 900001 codes of <= 20 bits): its verdict is final now, and the context does
            // not keep -- and re-scan -- everything behind it until the input ends.
            // (header: magic 48 + CRC 32 + randomised 1 + origPtr 24 + in-use maps 16 + 256 + tables 3 + selectors 15,
            // 18002 selectors of <= 6 bits, six tables of 5 + 258 * (up to 39 delta bits) -- about 170 Kbit)
            constexpr u64 kMaxRecordBits = (48 + 32 + 1 + 24 + 16 + 256 + 3 + 15) + 18002ull * 6ull + 6ull * (5ull + 258ull * 39ull) +
                                           900001ull * 20ull;
            if (partial && (bi.end_bit + 64 > nbits || (bi.status && nbits - rec.pos <= kMaxRecordBits))) {
                term = 2;
                break;
            }
            if (bi.status) {
                term = BZ_E_DATA;
                break;
            }
            tb.push_back({slot, 100000u * cs.level, bi.stored_crc, bi.nsym});
            chain_take_block(cs, bi.end_bit, bi.stored_crc, bi.next_head, bi.next_bits);
            if (!sh && tb.size() >= B) break; // (sharded: the chain is not batched)
        }
        if (rd.failed) return BZ_E_UNEXPECTED;
        ci = cj;
        return BZ_OK;
    }

    // (sharded) of all true blocks, the ones this rank rebuilds, by device slot
    void keep_own_blocks(TrueBlocks &tb, u64 &my_first_ord) const
    {
        TrueBlocks own;
        for (size_t i = 0; i < tb.size(); ++i)
            if (tb[i].slot >= c0 && tb[i].slot < c1) {
                if (my_first_ord == ~0ull) my_first_ord = i;
                own.push_back(tb[i]);
                own.back().slot -= (u32)c0;
            }
        tb.swap(own);
    }

    // ---- D2..D4 for the true blocks of the batch
    // Host destination: the blocks are rebuilt in SUB-BATCHES, so that the copy of sub-batch k to the caller's memory
    // (sink.pool's thread) runs beside the kernels of sub-batch k + 1 -- with everything in one go the download stood
    // behind the whole decode (118 ms per GiB host to host against 48 ms of kernels).  D1 stays one
    // launch over the whole batch: it takes the time of ONE block's Huffman decode however many blocks there are
    // (11 ms; four batches of 300 blocks paid it four times: measured, profiles/r05_host_copies.md).
    // local_fail: index (in this rank's list) of its first failing block; shard_rc: an infrastructure error of this rank,
    // told to the others.
    int rebuild_batch(const TrueBlocks &tb, int term, u64 &local_fail, int &shard_rc, bool &finished)
    {
        const u32 nb_all = (u32)tb.size();
        u32 sub_max = nb_all;
        if (sink.to_host() && sink.pool && !sh && nb_all) {
            const u32 hb = 320;
            const u32 nbat = (nb_all + hb - 1) / hb; // (equal sub-batches: 1189 blocks are 4 x 298, not 3 x 320 + 229)
            sub_max = (nb_all + nbat - 1) / nbat;
        }
        w->stats[1] += nb_all;
        for (u32 s0 = 0; s0 < nb_all && !finished && local_fail == ~0ull && shard_rc == BZ_OK; s0 += sub_max) {
            const u32 nb = std::min(sub_max, nb_all - s0);
            Rebuilt r;
            int rc = dec_rebuild(tb, s0, nb, r);
            if (rc) return rc;
            // blocks in front of the first one that failed to rebuild
            u32 good = nb;
            for (u32 i = 0; i < nb; ++i)
                if (r.err[i]) {
                    good = i;
                    break;
                }
            std::vector<u64> h_base(nb, 0);
            u64 bytes = 0;
            u32 max_len = 0;
            for (u32 i = 0; i < good; ++i) {
                h_base[i] = bytes;
                bytes += r.len[i];
                max_len = std::max(max_len, r.len[i]);
            }
            u32 keep = good; // blocks whose bytes are handed out
            bool crc_bad = false;
            u8 *dst = nullptr;
            const bool emit = !sink.dry && good;
            if (sink.dry) sink.produced += bytes;
            if (emit && (rc = emit_dst(bytes, dst, shard_rc))) return rc;
            if (emit && shard_rc == BZ_OK) {
                for (u32 i = good; i < nb; ++i) r.err[i] = 1u; // blocks behind `good` write nothing
                std::vector<u32> h_crc;
                if ((rc = dec_emit(r, good, h_base, bytes, max_len, dst, h_crc))) return rc;
                u64 valid = bytes;
                for (u32 i = 0; i < good; ++i) {
                    if (~h_crc[i] != tb[s0 + i].crc) { // decoder.rs:189-198: noticed after the block's bytes went out
                        crc_bad = true;
                        keep = i + 1;
                        valid = h_base[i] + r.len[i];
                        break;
                    }
                }
                if (sink.seg_alloc) rc = deliver_segment(dst, valid, nb);
                else if (sink.host) rc = deliver_host(dst, valid, nb, keep, (size_t)(nb_all - s0 - nb), term);
                if (rc) return rc;
                sink.produced += valid;
            }
            if (crc_bad) local_fail = s0 + keep - 1;
            else if (good < nb) local_fail = s0 + good;
            if (!sh && (crc_bad || good < nb)) {
                *verdict = BZ_E_DATA;
                finished = true;
            }
        }
        return BZ_OK;
    }

    // where D4 writes `bytes` bytes: a staging buffer (host destination) or the caller's device memory
    int emit_dst(u64 bytes, u8 *&dst, int &shard_rc)
    {
        if (sink.to_host()) {
            const u32 sb = batch_no & 1u;
            if (stage_busy[sb]) { // the copy of the batch before the last one reads this buffer
                sink.pool->wait(stage_ticket[sb]);
                stage_busy[sb] = false;
            }
            const int rc = sink.staging[sb]->ensure(bytes + 64);
            if (rc) return rc;
            dst = sink.staging[sb]->as<u8>();
            return BZ_OK;
        }
        if (sink.produced + bytes > sink.cap) {
            if (!sh) return BZ_E_CAPACITY;
            shard_rc = BZ_E_CAPACITY; // reported after the exchange: peers are waiting in it
        }
        dst = sink.d_out + sink.produced;
        return BZ_OK;
    }

    void trace_batch(const char *what, u32 nb, u64 valid) const
    {
        if (dec_trace())
            fprintf(stderr, "bz decode %s %u: %u blocks, %llu bytes; stages so far D0+D1 %.2f, MTF %.2f, walks %.2f, expand+CRC %.2f ms (at %.1f)\n",
                    what, batch_no, nb, (unsigned long long)valid, w->t_stage[0] * 1e3, w->t_stage[1] * 1e3, w->t_stage[2] * 1e3,
                    w->t_stage[3] * 1e3, now_ms());
    }

    // host destination, a buffer of its own for every sub-batch (the streaming context)
    int deliver_segment(const u8 *dst, u64 valid, u32 nb)
    {
        if (valid) {
            u8 *hp = sink.seg_alloc((size_t)valid);
            if (!hp) return BZ_E_NOMEM;
            if (sink.pool) {
                const u32 sb = batch_no & 1u;
                auto done_cb = sink.seg_done;
                const size_t vb = (size_t)valid;
                const bool fresh = sink.seg_fresh ? sink.seg_fresh(hp) : true;
                stage_ticket[sb] = sink.pool->submit(hp, dst, vb, hipMemcpyDeviceToHost, fresh, [done_cb, hp, vb](bool ok) { done_cb(hp, vb, ok); });
                stage_busy[sb] = true;
            } else {
                const bool ok = hipMemcpy(hp, dst, valid, hipMemcpyDeviceToHost) == hipSuccess;
                sink.seg_done(hp, (size_t)valid, ok);
                if (!ok) return BZ_E_UNEXPECTED;
            }
        }
        trace_batch("sub-batch", nb, valid);
        batch_no += 1;
        return BZ_OK;
    }

    // host destination, one growing buffer (the one-shot call over host buffers)
    int deliver_host(const u8 *dst, u64 valid, u32 nb, u32 keep, size_t blocks_behind, int term)
    {
        const size_t old = sink.host->len;
        if (old + valid > sink.host->cap) {
            // room for the rest of the file too, going by this batch's bytes per block (growing moves the
            // buffer: copies in flight are waited for, and every growth copies what is there)
            if (sink.pool) sink.pool->wait_all();
            stage_busy[0] = stage_busy[1] = false;
            size_t want = old + valid;
            // blocks behind this sub-batch, and -- while the chain has not ended -- the candidates behind the batch,
            // but no more of them than the input left can hold (a block record is 80 bits and more; junk behind
            // a stream may hold magic patterns by the million, and a chain that has ended takes none of them)
            size_t rest = blocks_behind;
            if (term == 0 && nc > ci) {
                const u64 bits_left = nbits > cs.pos ? nbits - cs.pos : 0ull;
                rest += std::min<size_t>(nc - ci, (size_t)(bits_left / 80ull));
            }
            if (rest && keep) {
                const double per_block = std::min((double)valid / (double)keep, 900000.0 * 1.25 + 64.0);
                want += (size_t)(per_block * (double)rest * 1.02) + ((size_t)1 << 20);
            }
            int hrc = sink.host->reserve(want);
            if (hrc != BZ_OK && want > old + valid) hrc = sink.host->reserve(old + valid); // (the guess was too much: what is needed now)
            if (hrc != BZ_OK) return hrc;
        }
        if (valid) {
            if (sink.pool) {
                const u32 sb = batch_no & 1u;
                stage_ticket[sb] = sink.pool->submit(sink.host->p + old, dst, valid, hipMemcpyDeviceToHost, true); // (fresh pages: touched first, on several threads)
                stage_busy[sb] = true;
            } else {
                HIPDEC(hipMemcpy(sink.host->p + old, dst, valid, hipMemcpyDeviceToHost));
            }
        }
        sink.host->len = old + valid; // (bytes whose copies may still be in flight: settled before decode_core returns)
        trace_batch("batch", nb, valid);
        batch_no += 1;
        return BZ_OK;
    }

    // (sharded) settle the verdict and the place of every slice
    int settle_shards(u64 my_first_ord, u64 local_fail, int shard_rc, u64 n_true, int term)
    {
        std::vector<ShardSum> sums((size_t)sh->world);
        const ShardSum mine = {sink.produced, (local_fail == ~0ull) ? ~0ull : my_first_ord + local_fail, my_first_ord, (u64)(u32)(-shard_rc)};
        sh->phase = 2;
        if (sh->allgather(sh->ctx, &mine, sizeof(mine), sums.data()) != 0) return BZ_E_UNEXPECTED;
        for (const ShardSum &s : sums)
            if (s.pad) return -(int)s.pad; // some rank could not hold its slice (BZ_E_CAPACITY ...)
        u64 fail = ~0ull;
        for (const ShardSum &s : sums) fail = std::min(fail, s.fail_ord);
        u64 off = 0, tot = 0;
        for (int r = 0; r < sh->world; ++r) {
            // a rank whose blocks all lie behind the failing one contributes nothing
            const u64 by = (sums[r].first_ord == ~0ull || sums[r].first_ord > fail) ? 0 : sums[r].bytes;
            if (r < sh->rank) off += by;
            if (r == sh->rank) sink.produced = by;
            tot += by;
        }
        sh->out_offset = off;
        sh->total_len = tot;
        w->stats[1] = n_true;
        w->stats[2] = cs.stream_no;
        if (fail != ~0ull) *verdict = BZ_E_DATA;
        else if (term < 0) *verdict = term;
        return BZ_OK;
    }

    int run(bz_gpu_engine *g_)
    {
        int rc;
        if ((rc = open(g_))) return rc;
        prof = g->prof.on ? &g->prof : nullptr;
        if ((rc = dec_scan_candidates(
                 (u32)std::min<u64>(n / 2048 + 1024, 0x7FFFFFFFu),
                 [&](DecCand *out, u32 cap, u32 *count) { launch_dec_scan(st, d_in, n, out, cap, count); },
                 [](const DecCand &a, const DecCand &b) { return a.bitpos < b.bitpos; }, cands)))
            return rc;
        nc = c1 = cands.size();
        w->stats[0] = nc;
        u32 want = 0;
        if (sh) { // every rank runs D1 on its own contiguous range of candidates, in one batch
            c0 = nc * (size_t)sh->rank / (size_t)sh->world;
            c1 = nc * (size_t)(sh->rank + 1) / (size_t)sh->world;
            want = (u32)std::max<size_t>(c1 - c0, 1);
            if (const char *e = getenv("BZ_DEC_SHARD_FAIL")) (void)sscanf(e, "%d:%d", &inject_rank, &inject_phase);
        }
        if (sh && inject_rank == sh->rank && inject_phase == 0) return BZ_E_NOMEM;
        if ((rc = dec_plan_slots(w, nc, want, &B))) return rc;
        Bphys = B;
        if (sh) B = (u32)(nc ? nc : 1); // the chain sees all candidates as one batch
        rd.d = d_in;
        rd.nbytes = n;
        hinfo.resize((size_t)B + kForcedSlots);
        hphys.resize(sh ? (size_t)Bphys : 0);
        if (rs) {
            cs = *rs;
            cs.have_next = false; // (the head byte of the next record is read from the bytes handed in)
            partial = !rs->final;
            rs->stopped = false;
        }
        rec = cs;
        bool chain_told = false, out_open = false, finished = false;
        while (!finished) {
            while (ci < nc && cands[ci].bitpos < cs.pos) ++ci;
            const u32 nb1 = (u32)std::min<size_t>(B, nc - ci);
            if ((rc = d1_batch(nb1))) return rc;
            if (sh && (rc = exchange_records())) return rc;
            TrueBlocks tb;
            int term = 0;
            if ((rc = walk_chain(nb1, tb, term))) return rc;
            if (term != 0 && sink.chain_final && !chain_told) {
                chain_told = true;
                Resume fin;
                static_cast<ChainState &>(fin) = term == 2 ? rec : cs;
                fin.stopped = term == 2;
                sink.chain_final(fin);
            }
            if (sink.before_output && !out_open) {
                out_open = true;
                if (!sink.before_output()) {
                    sink.aborted = true;
                    return BZ_OK;
                }
            }
            u64 my_first_ord = ~0ull; // stream ordinal of this rank's first block
            const u64 n_true = tb.size();
            if (sh) keep_own_blocks(tb, my_first_ord);
            u64 local_fail = ~0ull;
            int shard_rc = BZ_OK;
            if ((rc = rebuild_batch(tb, term, local_fail, shard_rc, finished))) return rc;
            if (finished) continue;
            if (sh) {
                if ((rc = settle_shards(my_first_ord, local_fail, shard_rc, n_true, term))) return rc;
                finished = true;
            } else if (term == 2) { // (partial) stopped in front of a record: everything before it is decoded
                rs->stopped = true;
                cs = rec;
                finished = true;
            } else if (term != 0) {
                if (term < 0) *verdict = term;
                w->stats[2] = cs.stream_no;
                finished = true;
            }
        }
        if (sink.to_host() && sink.pool) {
            sink.pool->wait_all();
            if (sink.pool->failed()) return BZ_E_UNEXPECTED;
        }
        if (prof) prof->collect();
        if (rs) static_cast<ChainState &>(*rs) = cs;
        return BZ_OK;
    }
};

} // namespace

// Decodes d_in[n].  Returns an infrastructure status (BZ_OK, BZ_E_NOMEM, BZ_E_UNEXPECTED,
// BZ_E_CAPACITY); the decoder's own verdict goes to *verdict (BZ_OK, BZ_E_DATA, BZ_E_MAGIC_FIRST,
// BZ_E_MAGIC) and the bytes produced in front of it to sink.produced.
static int decode_core(bz_gpu_engine *g, const u8 *d_in, u64 n, Sink &sink, int *verdict, Shard *sh = nullptr,
                       Resume *rs = nullptr)
{
    *verdict = BZ_OK;
    sink.produced = 0;
    DecRun run{{}, d_in, n, sink, verdict, sh, rs};
    return run.run(g);
}

// ---- many independent streams in one call ------------------------------------------------------------------
// Entry i is in_len[i] bytes at d_in + in_off[i]; its result is that of decode_core on those bytes alone.  What reaches
// across entries in decode_core -- one (in, nbytes) for the scan and for D1, one serial record chain on the host -- is
// replaced by a front end that knows about entries (k_dec_scan_batch, k_dec_block<true>, k_dec_chain_batch: k_dec.hip);
// D2..D4 (dec_rebuild, dec_emit) run on the true blocks of all entries of a GROUP together: a maximal run of consecutive
// entries whose candidates fit the D1 workspace.  Where decode_core stops at the first failing block, this driver stops
// only that block's ENTRY.  An entry with more candidates than a group holds, and one whose chain meets a block without
// its full magic (no candidate: `irregular`), is decoded by decode_core on its own range behind the batch path's output.
// Of the Sink `o` the driver takes d_out / cap, dry, or host: one buffer that grows group by group (offsets are relative to it).
namespace {
inline u64 up16(u64 x) { return (x + 15ull) & ~15ull; }

// The state of one decode_batch_core call.
struct DecBatchRun : DecCall {
    const u8 *d_in;
    const u64 *in_len;
    size_t count;
    Sink &o;
    u64 *out_off, *out_len;
    int32_t *verdict;
    // timings and stats of the call: sums over its groups and its one-stream decodes (decode_core clears the workspace's)
    double t_sum[4] = {0, 0, 0, 0};
    u64 s_sum[4] = {0, 0, 0, 0}, b_sum[4] = {0, 0, 0, 0};
    std::vector<DecEntry> ents; // the entries that hold bytes (an empty one is BZ_E_MAGIC_FIRST without a look at the device)
    std::vector<size_t> orig;   // their indices in the call
    std::vector<DecCand> cands; // sorted by (entry, bit position)
    std::vector<u32> one;       // entries (indices into ents) of the one-stream path
    u32 B = 0;
    u64 run_end = 0;   // end of the output so far
    size_t next_i = 0; // entries of the call in front of this one have their offsets (or wait for the one-stream path)

    ~DecBatchRun()
    {
        if (w)
            for (int i = 0; i < 4; ++i) w->t_stage[i] = t_sum[i], w->stats[i] = s_sum[i], w->bstats[i] = b_sum[i];
    }
    void place_empties(size_t upto)
    {
        for (; next_i < upto; ++next_i)
            if (!in_len[next_i]) {
                out_off[next_i] = up16(run_end);
                b_sum[0] += 1;
            }
    }

    // ---- D0: one scan over the span of all entries; every entry learns its range of the candidate list
    int scan()
    {
        const u32 nent = (u32)ents.size();
        int rc;
        if ((rc = w->ents.ensure((size_t)nent * sizeof(DecEntry)))) return rc;
        const u64 span0 = ents.front().off, span_end = ents.back().off + ents.back().len;
        if ((span_end - span0 + 1023u) / 1024u > 0x7FFFFFFFull) return BZ_E_PARAM;
        HIPDEC(hipMemcpyAsync(w->ents.p, ents.data(), (size_t)nent * sizeof(DecEntry), hipMemcpyHostToDevice, st));
        // (a tiny stream holds two magics in a few dozen bytes: room for those of every entry on top of decode_core's guess)
        if ((rc = dec_scan_candidates(
                 (u32)std::min<u64>((span_end - span0) / 2048 + 2ull * nent + 1024, 0x7FFFFFFFu),
                 [&](DecCand *out, u32 cap, u32 *cnt) { launch_dec_scan_batch(st, d_in, span0, span_end, w->ents.as<DecEntry>(), nent, out, cap, cnt); },
                 [](const DecCand &a, const DecCand &b) { return a.pad != b.pad ? a.pad < b.pad : a.bitpos < b.bitpos; }, cands)))
            return rc;
        if (cands.size() > 0xFFFFFFF0ull) return BZ_E_NOMEM;
        for (size_t k = 0; k < cands.size(); ++k) {
            if (cands[k].pad >= nent) return BZ_E_UNEXPECTED;
            DecEntry &e = ents[cands[k].pad];
            if (e.ncand++ == 0) e.first_cand = (u32)k;
        }
        return BZ_OK;
    }

    // ---- the group of entries [k0, k1) with n candidates: D1 inside each entry, every entry's record chain, D2..D4
    int group(u32 k0, u32 k1, u32 n)
    {
        const u32 ne = k1 - k0;
        u32 cand0 = 0; // the group's first candidate in the sorted list
        for (u32 k = k0; k < k1; ++k)
            if (ents[k].ncand) {
                cand0 = ents[k].first_cand;
                break;
            }
        b_sum[3] += 1;

        std::vector<u8> hchain((size_t)ne * sizeof(DecChainEntry) + (size_t)n * sizeof(DecChainCand));
        int rc;
        if ((rc = w->chain.ensure(hchain.size()))) return rc;
        DecChainEntry *d_ce = w->chain.as<DecChainEntry>();
        DecChainCand *d_cc = reinterpret_cast<DecChainCand *>(d_ce + ne);
        if (n) HIPDEC(hipMemcpyAsync(w->cands.p, cands.data() + cand0, (size_t)n * sizeof(DecCand), hipMemcpyHostToDevice, st));
        HIPDEC(hipMemsetAsync(w->chain.p, 0, hchain.size(), st));
        HIPDEC(hipEventRecord(ev[0], st));
        launch_dec_blocks_batch(st, d_in, w->ents.as<DecEntry>(), w->cands.as<DecCand>(), n, w->info.as<DecBlockInfo>(), w->sym.as<u16>(),
                                w->sel.as<u8>());
        launch_dec_chain_batch(st, d_in, w->ents.as<DecEntry>(), k0, ne, w->cands.as<DecCand>(), cand0, w->info.as<DecBlockInfo>(), d_ce, d_cc);
        HIPDEC(hipEventRecord(ev[1], st));
        HIPDEC(hipMemcpyAsync(hchain.data(), w->chain.p, hchain.size(), hipMemcpyDeviceToHost, st));
        HIPDEC(hipStreamSynchronize(st));
        stage_time(0);
        const DecChainEntry *ce = reinterpret_cast<const DecChainEntry *>(hchain.data());
        const DecChainCand *cc = reinterpret_cast<const DecChainCand *>(hchain.data() + (size_t)ne * sizeof(DecChainEntry));

        // the true blocks of the group in entry order, and where each entry's begin
        TrueBlocks tb;
        std::vector<u32> bfirst((size_t)ne + 1, 0);
        for (u32 k = k0; k < k1; ++k) {
            bfirst[k - k0] = (u32)tb.size();
            if (ce[k - k0].irregular) {
                one.push_back(k);
                continue;
            }
            s_sum[2] += ce[k - k0].streams;
            for (u32 q = ents[k].first_cand - cand0, q_end = q + ents[k].ncand; ents[k].ncand && q < q_end; ++q)
                if (cc[q].is_true) tb.push_back({q, cc[q].max_len, cc[q].stored_crc, cc[q].nsym});
        }
        const u32 nb = bfirst[ne] = (u32)tb.size();
        b_sum[2] += nb;
        s_sum[1] += nb;
        Rebuilt r;
        if ((rc = dec_rebuild(tb, 0, nb, r))) return rc;

        // ---- every entry's place, from the lengths of the blocks in front of its first failing one (before any CRC is
        // looked at: a sizes-only call assigns the same offsets)
        const u64 grp_start = up16(run_end);
        std::vector<u64> h_base(nb, 0);
        std::vector<u32> good((size_t)ne, 0); // blocks of the entry that were rebuilt
        u32 max_len = 0;
        u64 bytes = 0;
        for (u32 k = k0; k < k1; ++k) {
            const size_t i = orig[k];
            place_empties(i);
            next_i = i + 1;
            if (ce[k - k0].irregular) continue;
            b_sum[0] += 1;
            const u32 b0 = bfirst[k - k0], b1 = bfirst[k - k0 + 1];
            u32 gd = b1 - b0;
            for (u32 b = b0; b < b1; ++b)
                if (r.err[b]) {
                    gd = b - b0;
                    break;
                }
            good[k - k0] = gd;
            const u64 off = up16(run_end);
            u64 len = 0;
            for (u32 b = b0; b < b0 + gd; ++b) {
                h_base[b] = off + len - (o.host ? grp_start : 0ull);
                len += r.len[b];
                max_len = std::max(max_len, r.len[b]);
            }
            for (u32 b = b0 + gd; b < b1; ++b) r.err[b] = 1u; // the blocks behind a failing one are not the entry's any more
            out_off[i] = off;
            out_len[i] = len;
            static const int kVerdict[4] = {BZ_OK, BZ_E_DATA, BZ_E_MAGIC_FIRST, BZ_E_MAGIC};
            verdict[i] = gd < b1 - b0 ? BZ_E_DATA : kVerdict[ce[k - k0].verdict & 3u];
            run_end = off + len;
            bytes += len;
        }
        if (o.dry || !bytes) return BZ_OK;
        u8 *dst = o.d_out;
        if (o.host) {
            if ((rc = w->staging.ensure((size_t)(run_end - grp_start) + 64)) || (rc = o.host->reserve((size_t)run_end))) return rc;
            dst = w->staging.as<u8>();
        } else if (run_end > o.cap) {
            return BZ_E_CAPACITY;
        }

        std::vector<u32> h_crc;
        if ((rc = dec_emit(r, 0, h_base, bytes, max_len, dst, h_crc))) return rc;
        for (u32 k = k0; k < k1; ++k) {
            const u32 e = k - k0;
            if (ce[e].irregular) continue;
            const size_t i = orig[k];
            u64 len = 0;
            for (u32 b = bfirst[e]; b < bfirst[e] + good[e]; ++b) {
                len += r.len[b];
                if (~h_crc[b] != tb[b].crc) { // decoder.rs:189-198: noticed after the block's bytes went out
                    out_len[i] = len;
                    verdict[i] = BZ_E_DATA;
                    break;
                }
            }
        }
        if (o.host) {
            HIPDEC(hipMemcpy(o.host->p + grp_start, dst, (size_t)(run_end - grp_start), hipMemcpyDeviceToHost));
            o.host->len = (size_t)run_end;
        }
        return BZ_OK;
    }

    // ---- the one-stream path: decode_core on the entry's range, behind everything the batch path wrote
    int one_stream(u32 k)
    {
        const size_t i = orig[k];
        const u64 off = up16(run_end);
        Sink sink;
        if (o.host) {
            const int rc = o.host->reserve((size_t)off);
            if (rc) return rc;
            o.host->len = (size_t)off; // (decode_core appends)
            sink.host = o.host;
            sink.staging[0] = &w->staging;
            sink.staging[1] = &w->staging2;
        } else {
            sink.dry = o.dry;
            sink.d_out = o.dry ? nullptr : o.d_out + std::min(off, o.cap);
            sink.cap = o.cap > off ? o.cap - off : 0;
        }
        int v = BZ_OK;
        int rc = decode_core(g, d_in + ents[k].off, ents[k].len, sink, &v);
        for (int q = 0; q < 4; ++q) t_sum[q] += w->t_stage[q], s_sum[q] += w->stats[q];
        if (rc) return rc;
        u64 adv = sink.produced;
        if (!o.host && !o.dry && v == BZ_E_DATA) {
            // a CRC verdict cuts the entry short of what a sizes-only call counts: the entries behind keep its offsets
            Sink sizes;
            sizes.dry = true;
            int v2 = BZ_OK;
            rc = decode_core(g, d_in + ents[k].off, ents[k].len, sizes, &v2);
            for (int q = 0; q < 4; ++q) t_sum[q] += w->t_stage[q];
            if (rc) return rc;
            adv = std::max(adv, sizes.produced);
        }
        out_off[i] = off;
        out_len[i] = sink.produced;
        verdict[i] = v;
        run_end = off + adv;
        if (o.host) o.host->len = (size_t)(off + sink.produced);
        b_sum[1] += 1;
        return BZ_OK;
    }

    int run(bz_gpu_engine *g_, const u64 *in_off)
    {
        int rc;
        if ((rc = open(g_, t_sum))) return rc;
        for (size_t i = 0; i < count; ++i) {
            out_off[i] = out_len[i] = 0;
            verdict[i] = BZ_E_MAGIC_FIRST;
            if (in_len[i]) {
                ents.push_back(DecEntry{in_off[i], in_len[i], 0, 0});
                orig.push_back(i);
            }
        }
        const u32 nent = (u32)ents.size();
        if (nent && (rc = scan())) return rc;
        s_sum[0] = cands.size();
        if ((rc = dec_plan_slots(w, cands.size(), 0, &B))) return rc;
        for (u32 k = 0; k < nent; ++k)
            if (ents[k].ncand > B) {
                one.push_back(k);
                ents[k].ncand = kDecEntrySkip;
            }
        if (nent) HIPDEC(hipMemcpyAsync(w->ents.p, ents.data(), (size_t)nent * sizeof(DecEntry), hipMemcpyHostToDevice, st));

        for (u32 k0 = 0; k0 < nent;) {
            if (ents[k0].ncand == kDecEntrySkip) { // (no group reaches across it: a group's candidates are one range of the list)
                place_empties(orig[k0]);
                next_i = orig[k0] + 1;
                ++k0;
                continue;
            }
            u32 k1 = k0, n = 0;
            while (k1 < nent && ents[k1].ncand != kDecEntrySkip && n + ents[k1].ncand <= B) n += ents[k1++].ncand;
            if ((rc = group(k0, k1, n))) return rc;
            k0 = k1;
        }
        std::sort(one.begin(), one.end());
        for (const u32 k : one)
            if ((rc = one_stream(k))) return rc;
        place_empties(count);
        return BZ_OK;
    }
};
} // namespace

static int decode_batch_core(bz_gpu_engine *g, const u8 *d_in, const u64 *in_off, const u64 *in_len, size_t count,
                             Sink &o, u64 *out_off, u64 *out_len, int32_t *verdict)
{
    DecBatchRun run{{}, d_in, in_len, count, o, out_off, out_len, verdict};
    return run.run(g, in_off);
}

int dec_decode_for_verify(bz_gpu_engine *g, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap,
                          uint64_t *produced, int *verdict)
{
    Sink sink;
    sink.d_out = d_out;
    sink.cap = cap;
    const int rc = decode_core(g, d_in, n, sink, verdict);
    *produced = sink.produced;
    return rc;
}

// ---- C ABI ------------------------------------------------------------------------------------------------
extern "C" int bz_gpu_decode_device(bz_gpu_engine *g, const void *d_in, size_t n, void *d_out, size_t cap,
                                    size_t *out_len)
{
    if (!g || !out_len || (!d_in && n)) return BZ_E_PARAM;
    if (n && ((uintptr_t)d_in & 3u)) return BZ_E_PARAM;
    *out_len = 0;
    Sink sink;
    sink.d_out = static_cast<u8 *>(d_out);
    sink.cap = cap;
    sink.dry = (d_out == nullptr);
    int verdict = BZ_OK;
    const int rc = decode_core(g, static_cast<const u8 *>(d_in), n, sink, &verdict);
    *out_len = (size_t)sink.produced;
    return rc != BZ_OK ? rc : verdict;
}

extern "C" int bz_gpu_decode_device_sharded(bz_gpu_engine *g, const void *d_in, size_t n, void *d_out, size_t cap,
                                            int rank, int world, bz_allgather_fn allgather, void *ctx, size_t *out_len,
                                            size_t *out_offset, size_t *total_len)
{
    if (!g || !out_len || !out_offset || !total_len || (!d_in && n) || !d_out || !allgather) return BZ_E_PARAM;
    if (world < 1 || rank < 0 || rank >= world) return BZ_E_PARAM;
    if (n && ((uintptr_t)d_in & 3u)) return BZ_E_PARAM;
    *out_len = *out_offset = *total_len = 0;
    Sink sink;
    sink.d_out = static_cast<u8 *>(d_out);
    sink.cap = cap;
    Shard sh;
    sh.rank = rank;
    sh.world = world;
    sh.allgather = allgather;
    sh.ctx = ctx;
    int verdict = BZ_OK;
    const int rc = decode_core(g, static_cast<const u8 *>(d_in), n, sink, &verdict, &sh);
    if (rc != BZ_OK && sh.phase < 2) {
        // this rank failed on its own in front of an exchange its peers are about to enter: go through
        // that exchange with the error in the status word (they return it too)
        if (sh.phase == 0) {
            int64_t st0 = rc;
            std::vector<int64_t> sts((size_t)world, 0);
            (void)allgather(ctx, &st0, 8, sts.data());
        } else {
            ShardSum mine;
            mine.bytes = 0;
            mine.fail_ord = ~0ull;
            mine.first_ord = ~0ull;
            mine.pad = (u64)(u32)(-rc);
            std::vector<ShardSum> sums((size_t)world);
            (void)allgather(ctx, &mine, sizeof(mine), sums.data());
        }
    }
    *out_len = (size_t)sink.produced;
    *out_offset = (size_t)sh.out_offset;
    *total_len = (size_t)sh.total_len;
    return rc != BZ_OK ? rc : verdict;
}

extern "C" int bz_gpu_last_decode_timings(bz_gpu_engine *g, double out_seconds[5])
{
    if (!g || !out_seconds) return BZ_E_PARAM;
    for (int i = 0; i < 5; ++i) out_seconds[i] = 0;
    if (!g->dec) return BZ_OK;
    double tot = 0;
    for (int i = 0; i < 4; ++i) {
        out_seconds[i] = g->dec->t_stage[i];
        tot += g->dec->t_stage[i];
    }
    out_seconds[4] = tot;
    return BZ_OK;
}

extern "C" int bz_gpu_last_decode_stats(bz_gpu_engine *g, uint64_t out[4])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out[i] = g->dec ? g->dec->stats[i] : 0;
    return BZ_OK;
}

extern "C" int bz_gpu_decode_batch_device(bz_gpu_engine *g, const void *d_in, const uint64_t *h_in_off,
                                          const uint64_t *h_in_len, size_t count, void *d_out, size_t cap,
                                          uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict)
{
    if (!g) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !h_verdict) return BZ_E_PARAM;
    if (count > 0xFFFFFFF0ull || ((uintptr_t)d_in & 3u)) return BZ_E_PARAM;
    u64 end = 0;
    bool bytes = false;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 3u) || h_in_off[i] < end || h_in_off[i] + h_in_len[i] < h_in_off[i]) return BZ_E_PARAM;
        end = h_in_off[i] + h_in_len[i];
        bytes = bytes || h_in_len[i];
    }
    if (bytes && !d_in) return BZ_E_PARAM;
    Sink o;
    o.d_out = static_cast<u8 *>(d_out);
    o.cap = cap;
    o.dry = (d_out == nullptr);
    return decode_batch_core(g, static_cast<const u8 *>(d_in), h_in_off, h_in_len, count, o, h_out_off, h_out_len, h_verdict);
}

extern "C" int bz_gpu_last_decode_batch_stats(bz_gpu_engine *g, uint64_t out[4])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out[i] = g->dec ? g->dec->bstats[i] : 0;
    return BZ_OK;
}

extern "C" int bz_decode_buffer(int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len || (!in && in_len)) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    const double t_enter = now_ms();
    EngineLease lease(device, 1, 0); // (a parked engine that has decoded before, or a new one; host_call.h)
    if (lease.status() != BZ_OK) return lease.status();
    bz_gpu_engine *g = lease.engine();
    HostBuf host;
    int verdict = BZ_OK;
    int rc = g->dec_in.ensure(in_len + 64);
    if (rc == BZ_OK) {
        // The decoded bytes leave batch by batch beside the kernels of the next batch (copy_pool.h: one copying thread, the
        // fresh pages of the caller's buffer touched on several threads in front of it); the compressed bytes go up in one
        // hipMemcpy as before (50 GB/s from pageable memory: 226 MB in 6 ms).  (Rounds 1-4: one batch, one hipMemcpy behind it.)
        CopyPool pool(device);
        rc = BZ_E_UNEXPECTED;
        // (the 64 bytes behind the stream are read as zeros by the bit readers)
        if (hipMemsetAsync(static_cast<u8 *>(g->dec_in.p) + in_len, 0, 64, g->st) == hipSuccess &&
            (!in_len || hipMemcpyAsync(g->dec_in.p, in, in_len, hipMemcpyHostToDevice, g->st) == hipSuccess) &&
            hipStreamSynchronize(g->st) == hipSuccess) {
            if (!g->dec) g->dec = new DecWorkspace();
            Sink sink;
            sink.host = &host;
            sink.staging[0] = &g->dec->staging;
            sink.staging[1] = &g->dec->staging2;
            sink.pool = &pool;
            rc = decode_core(g, static_cast<const u8 *>(g->dec_in.p), in_len, sink, &verdict);
        }
    }
    if (dec_trace()) fprintf(stderr, "bz_decode_buffer: %zu -> %zu bytes, rc %d, done at %.1f (entered at %.1f)\n", in_len, host.len, rc, now_ms(), t_enter);
    lease.settle(rc); // (`verdict`, the stream's, is not the engine's business)
    if (rc != BZ_OK) return rc;
    // the bytes in front of an error are handed over too, as the reference's iterator yields them
    *out_len = host.len;
    uint8_t *h = host.len ? host.release() : (uint8_t *)malloc(1);
    if (!h) return BZ_E_NOMEM;
    *out = h;
    return verdict;
}

// The same for many independent streams: the entries packed at 4-byte-aligned offsets (BatchLayout, host_call.h), one
// upload, decode_batch_core on a cached engine, the bytes down group by group into ONE buffer.
extern "C" int bz_decode_batch(int device, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t **out,
                               uint64_t *out_off, uint64_t *out_len, int32_t *verdict)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (count == 0) {
        *out = (uint8_t *)malloc(1);
        return *out ? BZ_OK : BZ_E_NOMEM;
    }
    if (!ins || !lens || !out_off || !out_len || !verdict || count > 0xFFFFFFF0ull) return BZ_E_PARAM;
    const BatchLayout lay(ins, lens, count, 4);
    if (lay.status != BZ_OK) return lay.status;
    EngineLease lease(device, 1, 0);
    if (lease.status() != BZ_OK) return lease.status();
    bz_gpu_engine *g = lease.engine();
    HostBuf host;
    int rc = g->dec_in.ensure((size_t)lay.total + 64);
    if (rc == BZ_OK) {
        // packed on the host first: one upload, whatever the number of entries
        std::vector<u8> packed((size_t)lay.total, 0);
        lay.pack_into(packed.data());
        rc = BZ_E_UNEXPECTED;
        if ((!lay.total || hipMemcpyAsync(g->dec_in.p, packed.data(), (size_t)lay.total, hipMemcpyHostToDevice, g->st) == hipSuccess) &&
            hipStreamSynchronize(g->st) == hipSuccess) {
            Sink o;
            o.host = &host;
            rc = decode_batch_core(g, static_cast<const u8 *>(g->dec_in.p), lay.in_off.data(), lay.in_len.data(), count, o, out_off, out_len,
                                   verdict);
        }
    }
    lease.settle(rc); // (the entries' verdicts are not the engine's business)
    if (rc != BZ_OK) return rc;
    uint8_t *h = host.len ? host.release() : (uint8_t *)malloc(1);
    if (!h) return BZ_E_NOMEM;
    *out = h;
    return BZ_OK;
}

// ---- streaming mirror of BZip2Decoder (decoder.rs:583-612) ------------------------------------------------
// The reference pulls input bytes on demand and yields output bytes one by one.  Here compressed bytes are collected
// (bz_dec_write); whenever BZ_DEC_CHUNK bytes (default 64 MiB; the first chunk of a stream 16 MiB, so that the GPU has work
// early) have come in, and when the input ends (bz_dec_end), they go to the context's WORKER thread, which decodes the
// records that are wholly there and queues their bytes (bz_dec_read), sub-batch by sub-batch as they land in host memory
// -- while the caller goes on writing and reading: the caller's copies (compressed bytes in, decoded bytes out: a GiB of
// them is 0.1 s of one core) run beside the upload, the kernels and the download instead of in a row with them (rounds
// 1-4 decoded inside bz_dec_write: 4.2 GB/s for what the kernels do at 22).  The chain's state (bit position, stream
// number, level, combined CRC) is carried from chunk to chunk, the bytes from the first undecided record on are kept.
// An error, if any, is reported after the bytes in front of it -- the same sequence of items the reference's iterator
// produces; memory is bounded by the chunks in flight (two at most wait for the worker), not by the file.
// bz_dec_end says "the input iterator has ended" and returns at once (with the verdict if it is already final);
// behind it bz_dec_read WAITS for the next bytes or the final verdict instead of answering "nothing yet" -- a consumer
// reads the head of the file while its tail is still being decoded.
namespace {
// Compressed bytes on their way to a lane: plain memory without value initialisation, 2 MiB-aligned and asking for huge
// pages from 4 MiB on (a chunk is written once and uploaded once: what its buffer costs is the first touch of its pages
// -- a malloc'ed std::vector that doubled its way to 64 MiB took the writer 25 ms per chunk, a third of a second per GiB).
struct ByteBuf {
    u8 *p = nullptr;
    size_t len = 0, cap = 0;
    ByteBuf() = default;
    ByteBuf(const ByteBuf &) = delete;
    ByteBuf &operator=(const ByteBuf &) = delete;
    ByteBuf(ByteBuf &&o) noexcept : p(o.p), len(o.len), cap(o.cap) { o.p = nullptr, o.len = o.cap = 0; }
    ByteBuf &operator=(ByteBuf &&o) noexcept
    {
        if (this != &o) {
            free(p);
            p = o.p, len = o.len, cap = o.cap;
            o.p = nullptr, o.len = o.cap = 0;
        }
        return *this;
    }
    ~ByteBuf() { free(p); }
    size_t size() const { return len; }
    bool empty() const { return len == 0; }
    size_t capacity() const { return cap; }
    const u8 *data() const { return p; }
    void clear() { len = 0; }
    void swap(ByteBuf &o)
    {
        std::swap(p, o.p);
        std::swap(len, o.len);
        std::swap(cap, o.cap);
    }
    bool reserve(size_t want)
    {
        if (want <= cap) return true;
        void *q = nullptr;
        if (want >= ((size_t)4 << 20)) {
            want = (want + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
            if (posix_memalign(&q, (size_t)2 << 20, want) != 0) q = nullptr;
            if (q) (void)madvise(q, want, MADV_HUGEPAGE);
        } else {
            q = malloc(want);
        }
        if (!q) return false;
        if (len) memcpy(q, p, len);
        free(p);
        p = static_cast<u8 *>(q);
        cap = want;
        return true;
    }
    bool append(const u8 *src, size_t k)
    {
        if (len + k > cap && !reserve(len + k)) return false;
        memcpy(p + len, src, k);
        len += k;
        return true;
    }
};
struct DecJob {
    ByteBuf bytes;
    bool final = false;
};
struct DecSeg { // decoded bytes of one sub-batch, handed out from `pos` on
    u8 *p = nullptr;
    size_t len = 0, pos = 0, cap = 0;
    bool landed = false; // the copy from the device is over (segments are queued in order when they are allocated)
    bool fresh = true;   // its pages have not been touched yet
    ~DecSeg() { free(p); }
};
} // namespace
// Chunk buffers of contexts that have ended, kept for the next context (up to four, 64 MiB each by default: their pages
// are touched already); bz_release_cached_resources frees them with the engines.
static std::mutex g_dec_spare_mu;
static std::vector<ByteBuf> g_dec_spare_bufs;
void dec_spare_bufs_clear()
{
    std::vector<ByteBuf> all;
    {
        std::lock_guard<std::mutex> lk(g_dec_spare_mu);
        all.swap(g_dec_spare_bufs);
    }
}
static void dec_spare_buf_take(ByteBuf &into, size_t want)
{
    std::lock_guard<std::mutex> lk(g_dec_spare_mu);
    for (size_t i = 0; i < g_dec_spare_bufs.size(); ++i)
        if (g_dec_spare_bufs[i].capacity() >= want) {
            into.swap(g_dec_spare_bufs[i]);
            into.clear();
            g_dec_spare_bufs.erase(g_dec_spare_bufs.begin() + (ptrdiff_t)i);
            return;
        }
}
static void dec_spare_buf_put(ByteBuf &b)
{
    if (b.capacity() < ((size_t)4 << 20) || b.capacity() > ((size_t)256 << 20)) return;
    std::lock_guard<std::mutex> lk(g_dec_spare_mu);
    if (g_dec_spare_bufs.size() >= 4) return;
    b.clear();
    g_dec_spare_bufs.push_back(std::move(b));
}
struct bz_dec {
    int device = 0;
    size_t chunk = (size_t)64 << 20, first_chunk = (size_t)16 << 20;
    // the caller's side
    ByteBuf in; // compressed bytes not yet handed to the worker
    bool ended = false;
    u64 chunks_sent = 0;
    // shared (mu)
    std::mutex mu;
    std::condition_variable cv;
    std::deque<DecJob> jobs;
    std::deque<DecSeg *> outq;
    // Buffers that have been read (decoded bytes) or uploaded (compressed bytes) are kept for the sub-batches and chunks
    // to come instead of being freed: memory the runtime has had registered for a copy is expensive to give back while
    // kernels run (the unmapping invalidates the registration and stalls the process' queues -- chunks took 50-60 ms
    // instead of 30 when every segment was freed behind its reader, profiles/r05_host_copies.md), and a buffer that
    // comes back has its pages touched already.  At most four of each are kept.
    std::vector<DecSeg *> spare_segs;
    std::vector<ByteBuf> spare_bytes;
    size_t out_bytes = 0;                // landed and not yet read
    u64 submitted = 0, processed = 0;    // jobs
    bool stop = false;
    bool done = false;                   // the verdict is final (error, or clean end): later input is ignored
    int verdict = BZ_OK;
    // the workers' side.  TWO lanes (an engine, an input buffer and a thread each) take the chunks in turn: a chunk's
    // record chain is known once its Huffman stage (D1: 11 ms whatever the chunk holds) is over, and from there on the
    // next chunk's upload, scan and D1 run on the other lane beside the rebuilding (D2..D4) of this one's blocks.  The
    // chain -- carry, rs -- belongs to the lane whose job number is `chain_turn`; decoded bytes are handed out by the lane
    // whose job number is `out_turn` (a lane whose chain is walked waits there for the chunk in front to finish, and
    // gives up if that one ended with an error).  BZ_DEC_LANES=1: one lane (round 5's first form: D1 of a chunk behind
    // D4 of the one in front).
    struct Lane {
        bz_gpu_engine *g = nullptr;
        DevBuf d_in;
        std::thread th;
    } lane[2];
    int n_lanes = 2;
    u64 taken = 0, chain_turn = 0, out_turn = 0; // job numbers (mu)
    std::vector<u8> carry; // compressed bytes from the next record on (what the last chunk left undecided)
    Resume rs;
    CopyPool *pool = nullptr;
};

// a lane: one chunk (everything not yet decided + the new bytes); `no` is the chunk's job number
static void dec_process(bz_dec *d, bz_dec::Lane &ln, DecJob &j, u64 no)
{
    bool chain_mine = true; // (this lane holds the chain until the hook below or the end of this function passes it on)
    auto pass_chain = [&] {
        if (!chain_mine) return;
        chain_mine = false;
        {
            std::lock_guard<std::mutex> lk(d->mu);
            d->chain_turn = no + 1;
        }
        d->cv.notify_all();
    };
    auto finish = [&](int v) {
        std::lock_guard<std::mutex> lk(d->mu);
        if (d->done) return;
        d->done = true;
        d->verdict = v;
    };
    auto wait_out_turn = [&]() -> bool { // false: the chunk in front ended the context (an error), or the context is being destroyed
        std::unique_lock<std::mutex> lk(d->mu);
        d->cv.wait(lk, [&] { return d->out_turn == no || d->stop; });
        return d->out_turn == no && !d->done;
    };
    if (!ln.g) { // (an engine kept by an earlier one-shot call or context, with its workspace, or a new one)
        EngineLease lease(d->device, 1, 0);
        if (lease.status() != BZ_OK) {
            pass_chain();
            if (wait_out_turn()) finish(lease.status());
            return;
        }
        ln.g = lease.release(); // (the lane holds it until bz_dec_destroy ends it through a lease that adopts it)
    }
    const double t0 = now_ms();
    // the device holds [carry | new bytes]: two uploads, no copy of the chunk on the host; room for a whole chunk and a
    // block's worth of carry from the start, so that the buffer is made once
    const size_t nc = d->carry.size(), nn = j.bytes.size(), n = nc + nn;
    int rc = hipSetDevice(d->device) == hipSuccess ? ln.d_in.ensure(std::max(n, d->chunk + ((size_t)4 << 20)) + 64) : BZ_E_UNEXPECTED;
    // (the 64 bytes behind the input are read as zeros by the bit readers)
    if (rc == BZ_OK && hipMemsetAsync(static_cast<u8 *>(ln.d_in.p) + n, 0, 64, ln.g->st) != hipSuccess) rc = BZ_E_UNEXPECTED;
    if (rc == BZ_OK && nc && hipMemcpyAsync(ln.d_in.p, d->carry.data(), nc, hipMemcpyHostToDevice, ln.g->st) != hipSuccess) rc = BZ_E_UNEXPECTED;
    if (rc == BZ_OK && nn && hipMemcpyAsync(static_cast<u8 *>(ln.d_in.p) + nc, j.bytes.data(), nn, hipMemcpyHostToDevice, ln.g->st) != hipSuccess)
        rc = BZ_E_UNEXPECTED;
    if (rc == BZ_OK && hipStreamSynchronize(ln.g->st) != hipSuccess) rc = BZ_E_UNEXPECTED;
    const double t1 = now_ms();
    int verdict = BZ_OK;
    size_t produced = 0;
    bool stopped = false, aborted = false;
    double t_chain = 0, t_out = 0;
    if (rc == BZ_OK) {
        if (!ln.g->dec) ln.g->dec = new DecWorkspace();
        Sink sink;
        // a buffer of its own for every sub-batch, queued at once (the order of the queue is the order of the file) and
        // handed to the reader when its bytes have landed
        sink.seg_alloc = [d](size_t k) -> u8 * {
            DecSeg *sg = nullptr;
            {
                std::lock_guard<std::mutex> lk(d->mu);
                size_t best = ~(size_t)0;
                for (size_t i = 0; i < d->spare_segs.size(); ++i)
                    if (d->spare_segs[i]->cap >= k && (best == ~(size_t)0 || d->spare_segs[i]->cap < d->spare_segs[best]->cap)) best = i;
                if (best != ~(size_t)0) {
                    sg = d->spare_segs[best];
                    d->spare_segs.erase(d->spare_segs.begin() + (ptrdiff_t)best);
                }
            }
            if (!sg) {
                void *q = nullptr;
                const size_t want = (k + k / 16 + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1); // (sub-batches of a file differ by a per cent or two)
                if (posix_memalign(&q, (size_t)2 << 20, want) != 0) return nullptr;
                (void)madvise(q, want, MADV_HUGEPAGE);
                sg = new DecSeg();
                sg->p = static_cast<u8 *>(q);
                sg->cap = want;
            }
            sg->len = k;
            sg->pos = 0;
            sg->landed = false;
            std::lock_guard<std::mutex> lk(d->mu);
            d->outq.push_back(sg);
            return sg->p;
        };
        sink.seg_fresh = [d](u8 *p8) {
            std::lock_guard<std::mutex> lk(d->mu);
            for (DecSeg *sg : d->outq)
                if (sg->p == p8) {
                    const bool f = sg->fresh;
                    sg->fresh = false;
                    return f;
                }
            return true;
        };
        sink.seg_done = [d](u8 *p8, size_t k, bool ok) {
            {
                std::lock_guard<std::mutex> lk(d->mu);
                for (DecSeg *sg : d->outq)
                    if (sg->p == p8) {
                        sg->landed = true; // (a failed copy ends the context with an error: its bytes are never read as data)
                        if (ok) d->out_bytes += k;
                        else sg->len = sg->pos;
                    }
            }
            d->cv.notify_all();
        };
        // the chain is walked: the state and the bytes the next chunk starts from, and the chain goes to the other lane
        sink.chain_final = [&](const Resume &fin) {
            stopped = fin.stopped;
            if (fin.stopped) { // keep the input from the undecided record on
                const size_t used = (size_t)(fin.pos >> 3);
                std::vector<u8> keep;
                if (used < nc) {
                    keep.assign(d->carry.begin() + (ptrdiff_t)used, d->carry.end());
                    keep.insert(keep.end(), j.bytes.data(), j.bytes.data() + nn);
                } else {
                    keep.assign(j.bytes.data() + (used - nc), j.bytes.data() + nn);
                }
                d->carry.swap(keep);
            } else {
                d->carry.clear();
            }
            d->rs = fin;
            d->rs.pos &= 7u;
            t_chain = now_ms();
            pass_chain();
        };
        sink.before_output = [&]() -> bool {
            const bool go = wait_out_turn();
            t_out = now_ms();
            return go;
        };
        sink.staging[0] = &ln.g->dec->staging;
        sink.staging[1] = &ln.g->dec->staging2;
        sink.pool = d->pool;
        Resume rs = d->rs; // (a copy: d->rs is the next chunk's from chain_final on)
        rs.final = j.final;
        rc = decode_core(ln.g, ln.d_in.as<u8>(), n, sink, &verdict, nullptr, &rs);
        produced = (size_t)sink.produced;
        aborted = sink.aborted;
        if (chain_mine) stopped = rs.stopped; // (left before the chain's end: an error of the library's own)
    }
    pass_chain();
    if (dec_trace())
        fprintf(stderr, "bz_dec chunk %llu: %zu + %zu compressed bytes (final %d): upload %.2f ms, chain known after %.2f, waited for its turn %.2f, decode %.2f ms -> %zu bytes, rc %d verdict %d%s (at %.1f)\n",
                (unsigned long long)no, nc, nn, (int)j.final, t1 - t0, t_chain ? t_chain - t1 : 0.0, t_out && t_chain ? t_out - t_chain : 0.0, now_ms() - t1,
                produced, rc, verdict, aborted ? " GIVEN UP" : "", now_ms());
    if (aborted) return;
    // (the bytes in front of an error have been handed over too, as the reference's iterator yields them)
    if (rc != BZ_OK || verdict != BZ_OK) {
        if (wait_out_turn()) finish(rc != BZ_OK ? rc : verdict); // (an error in front of the first block: its turn has not been waited for yet)
        return;
    }
    if (!stopped) finish(BZ_OK); // the file ended cleanly
}

static void dec_worker(bz_dec *d, int li)
{
    bz_dec::Lane &ln = d->lane[li];
    for (;;) {
        DecJob j;
        bool skip;
        u64 no;
        {
            std::unique_lock<std::mutex> lk(d->mu);
            d->cv.wait(lk, [&] { return d->stop || (!d->jobs.empty() && d->chain_turn == d->taken); });
            if (d->jobs.empty() || d->chain_turn != d->taken) return; // (stop)
            j = std::move(d->jobs.front());
            d->jobs.pop_front();
            no = d->taken++;
            skip = d->done; // (an error is waiting behind the queued bytes; further input is ignored)
        }
        d->cv.notify_all(); // (a writer may be waiting for room in the queue)
        if (!skip) dec_process(d, ln, j, no);
        {
            std::unique_lock<std::mutex> lk(d->mu);
            if (d->chain_turn == no) d->chain_turn = no + 1; // (a skipped chunk)
            d->cv.notify_all();
            d->cv.wait(lk, [&] { return d->out_turn == no || d->stop; }); // chunks are done in their order
            if (d->out_turn == no) d->out_turn = no + 1;
            d->processed += 1;
            if (j.bytes.capacity() >= ((size_t)4 << 20) && d->spare_bytes.size() < 4) { // (kept for the writer, see spare_segs)
                j.bytes.clear();
                d->spare_bytes.push_back(std::move(j.bytes));
            }
        }
        d->cv.notify_all();
    }
}

extern "C" int bz_dec_create(bz_dec **out, int device)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BZ_E_NOGPU;
    if (device < 0 || device >= ndev) return BZ_E_PARAM;
    bz_dec *d = new bz_dec();
    d->device = device;
    if (const char *e = getenv("BZ_DEC_CHUNK")) {
        const long long v = atoll(e);
        if (v >= 1) d->chunk = d->first_chunk = (size_t)v;
    }
    if (const char *e = getenv("BZ_DEC_FIRST_CHUNK")) {
        const long long v = atoll(e);
        if (v >= 1) d->first_chunk = (size_t)v;
    }
    d->pool = new CopyPool(device);
    if (const char *e = getenv("BZ_DEC_LANES")) d->n_lanes = atoi(e) == 1 ? 1 : 2;
    *out = d;
    return BZ_OK;
}

// hands what has been written to the worker (final: the input iterator has ended)
static void dec_submit(bz_dec *d, bool final)
{
    DecJob j;
    j.bytes.swap(d->in);
    j.final = final;
    d->chunks_sent += 1;
    // A small chunk (less than 4 MiB: short files, and every test that sets a small BZ_DEC_CHUNK to look at the moments
    // bytes and errors come out) is decoded before this call returns, as in rounds 1-4: handing it over would only delay
    // its bytes by a thread switch.  A large one is decoded beside the caller.
    const bool wait = j.bytes.size() < ((size_t)4 << 20);
    u64 ticket;
    {
        std::unique_lock<std::mutex> lk(d->mu);
        for (int i = 0; i < d->n_lanes; ++i)
            if (!d->lane[i].th.joinable() && (i == 0 || d->chunks_sent > 1)) d->lane[i].th = std::thread(dec_worker, d, i); // (the second lane with the second chunk)
        d->cv.wait(lk, [&] { return d->jobs.size() < 2; }); // (two chunks wait at most: memory is bounded by the chunk)
        d->jobs.push_back(std::move(j));
        ticket = ++d->submitted;
    }
    d->cv.notify_all();
    if (wait) {
        std::unique_lock<std::mutex> lk(d->mu);
        d->cv.wait(lk, [&] { return d->processed >= ticket; });
    }
}

extern "C" int bz_dec_write(bz_dec *d, const uint8_t *data, size_t n)
{
    if (!d || (!data && n)) return BZ_E_PARAM;
    if (d->ended) return BZ_E_UNEXPECTED;
    {
        std::lock_guard<std::mutex> lk(d->mu);
        if (d->done) { // (an error is waiting behind the queued bytes; further input is ignored -- unless it is the library's own)
            const int v = d->verdict;
            return (v == BZ_OK || v == BZ_E_DATA || v == BZ_E_MAGIC_FIRST || v == BZ_E_MAGIC || v == BZ_E_EOF) ? BZ_OK : v;
        }
    }
    // A chunk goes to the worker once BZ_DEC_CHUNK bytes are there; a large write is cut at that size, but never into
    // pieces of less than 1 MiB (a tiny BZ_DEC_CHUNK -- the tests' way to stop the decoder in mid-record -- hands over what
    // a call brought, as rounds 1-4 did, not thousands of jobs).
    while (n) {
        // (measured on 1 GiB of text, 226 MB compressed: chunks of 16 + 64 + 64 + ... MiB 142 ms, of 16 + 48 + 128 + ... 150-156 ms,
        // of 16 + 128 + ... 169-197 ms -- a chunk must have arrived whole before its Huffman stage can begin, and that stage
        // is 11 ms per chunk whatever the chunk holds)
        const size_t chunk = d->chunks_sent == 0 ? d->first_chunk : d->chunk;
        const size_t gran = std::max(chunk, (size_t)1 << 20);
        const size_t room = d->in.size() < gran ? gran - d->in.size() : 0;
        const size_t k = room ? std::min(n, room) : n;
        if (d->in.empty() && d->in.capacity() < gran && gran >= ((size_t)4 << 20)) { // (a buffer an earlier chunk went up from, if one has come back)
            {
                std::lock_guard<std::mutex> lk(d->mu);
                if (!d->spare_bytes.empty()) {
                    d->in.swap(d->spare_bytes.back());
                    d->spare_bytes.pop_back();
                }
            }
            if (d->in.capacity() < gran) dec_spare_buf_take(d->in, gran); // (or one an earlier context left behind)
        }
        // room for the whole chunk as soon as the file is not a tiny one (untouched pages cost nothing)
        if (d->in.size() + k > d->in.capacity()) {
            const size_t need = d->in.size() + k;
            const size_t want = need >= ((size_t)1 << 20) ? std::max(need, gran) : std::max(need, std::max((size_t)65536, 2 * d->in.capacity()));
            if (!d->in.reserve(want)) return BZ_E_NOMEM;
        }
        (void)d->in.append(data, k);
        data += k;
        n -= k;
        if (d->in.size() >= chunk && (d->in.size() >= gran || n == 0)) dec_submit(d, false);
    }
    return BZ_OK;
}

extern "C" int bz_dec_end(bz_dec *d)
{
    if (!d) return BZ_E_PARAM;
    if (!d->ended) {
        d->ended = true;
        dec_submit(d, true);
    }
    std::lock_guard<std::mutex> lk(d->mu);
    return d->done ? d->verdict : BZ_OK; // (not final yet: the verdict follows the last byte out of bz_dec_read, which waits for it now)
}

extern "C" long bz_dec_read(bz_dec *d, uint8_t *out, size_t cap)
{
    if (!d || (!out && cap)) return BZ_E_PARAM;
    DecSeg *seg = nullptr;
    {
        std::unique_lock<std::mutex> lk(d->mu);
        for (;;) {
            while (!d->outq.empty() && d->outq.front()->landed && d->outq.front()->pos == d->outq.front()->len) { // (read, or lost)
                if (d->spare_segs.size() < 4) d->spare_segs.push_back(d->outq.front());
                else delete d->outq.front();
                d->outq.pop_front();
            }
            if (!d->outq.empty() && d->outq.front()->landed) break;
            const bool idle = d->processed >= d->submitted; // (a chunk that has been looked at has all its segments landed)
            // the verdict (0 = clean end) once it is final and every chunk handed over has been looked at
            if (d->outq.empty() && d->done && idle) return (long)d->verdict;
            // "nothing yet" while more input may come; behind the end of the input the next bytes or the verdict are waited for
            if (!d->ended || (d->outq.empty() && idle)) return 0;
            d->cv.wait(lk);
        }
        seg = d->outq.front(); // (only this thread takes segments off the queue; the worker appends behind it)
    }
    const size_t left = seg->len - seg->pos;
    const size_t k = left < cap ? left : cap;
    memcpy(out, seg->p + seg->pos, k);
    {
        std::lock_guard<std::mutex> lk(d->mu);
        seg->pos += k;
        d->out_bytes -= k;
    }
    return (long)k;
}

extern "C" size_t bz_dec_pending(const bz_dec *d)
{
    if (!d) return 0;
    bz_dec *m = const_cast<bz_dec *>(d);
    std::lock_guard<std::mutex> lk(m->mu);
    return d->out_bytes;
}

extern "C" void bz_dec_destroy(bz_dec *d)
{
    if (!d) return;
    {
        std::lock_guard<std::mutex> lk(d->mu);
        d->stop = true;
        d->jobs.clear(); // (chunks that wait are dropped; the one being decoded is finished)
    }
    d->cv.notify_all();
    for (auto &ln : d->lane)
        if (ln.th.joinable()) ln.th.join();
    for (ByteBuf &b : d->spare_bytes) dec_spare_buf_put(b);
    dec_spare_buf_put(d->in);
    delete d->pool;
    for (DecSeg *sg : d->outq) delete sg;
    for (DecSeg *sg : d->spare_segs) delete sg;
    for (auto &ln : d->lane) {
        if (!ln.g) continue;
        EngineLease lease(d->device, ln.g);
        ln.d_in.release();
        // (kept for the next context or one-shot call unless the context met an infrastructure error)
        const bool data_verdict = d->verdict == BZ_OK || d->verdict == BZ_E_DATA || d->verdict == BZ_E_MAGIC_FIRST || d->verdict == BZ_E_MAGIC ||
                                  d->verdict == BZ_E_EOF;
        lease.settle(data_verdict ? BZ_OK : d->verdict);
    }
    delete d;
}
