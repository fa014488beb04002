// engine.hip -- host orchestration of the device-resident BZip2 block-encode engine and the
// device half of the C ABI (include/bz2_mi355x.h, section 2).
//
// One engine == one GPU == one HIP stream.  Multi-GPU jobs run one process (one engine) per
// GPU and exchange block bit strings with RCCL outside this library (bench.py,
// rust-compression_amd/__init__.py); nothing here needs a collective.
#include "engine_state.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// a few bytes for the host and the stream's earlier work done (mail_fetch, k_emit.hip)
#define MAILCHK(st, ...)                                                             \
    do {                                                                             \
        const MailSeg mail_segs_[] = {__VA_ARGS__};                                  \
        if (mail_fetch((st), mail_segs_, (int)(sizeof(mail_segs_) / sizeof(mail_segs_[0]))) != 0) return BZ_E_UNEXPECTED; \
    } while (0)

static int span_begin(bz_gpu_engine *g, int stage, hipStream_t st = nullptr)
{
    bz_gpu_engine::Span s;
    s.stage = stage;
    s.st = st ? st : g->st;
    if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) return -1;
    (void)hipEventRecord(s.a, s.st);
    g->spans.push_back(s);
    return (int)g->spans.size() - 1;
}
static void span_end(bz_gpu_engine *g, int idx)
{
    if (idx >= 0) (void)hipEventRecord(g->spans[idx].b, g->spans[idx].st);
}
static void spans_collect(bz_gpu_engine *g)
{
    (void)hipStreamSynchronize(g->st);
    (void)hipStreamSynchronize(g->st2);
    g->prof.collect();
    for (auto &s : g->spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) g->t_stage[s.stage] += ms * 1e-3;
        (void)hipEventDestroy(s.a);
        (void)hipEventDestroy(s.b);
    }
    g->spans.clear();
    g->t_stage[5] = g->t_stage[0] + g->t_stage[1] + g->t_stage[2] + g->t_stage[3] + g->t_stage[4];
}

// BZ_PAIR_KEYS=0: every block sorts by keys of single symbols, as before round 7 (tests/test_gpu_pair_keys.py)
static bool pair_keys_wanted()
{
    static const bool on = !(getenv("BZ_PAIR_KEYS") && atoi(getenv("BZ_PAIR_KEYS")) == 0);
    return on;
}

// BZ_ONESWEEP=0: the three-kernel radix passes from the start (tests/test_gpu_parity.py::test_radix_pass_flavours_agree)
static bool fused_wanted()
{
    static const bool on = !(getenv("BZ_ONESWEEP") && atoi(getenv("BZ_ONESWEEP")) == 0);
    return on;
}

// The batch workspace, buffer by buffer in the order of allocation: `per_block` bytes for every block in flight plus
// `fixed` bytes.  This table is the one place on the host that states what a block takes of each buffer; the argument
// blocks below (make_*_args) hand out base pointers, and the kernels stride by the same constants.
struct WsBuf {
    DevBuf bz_gpu_engine::*buf;
    size_t per_block, fixed;
    bool fused_only; // exists only with the fused radix passes (fused_wanted())
};
static constexpr WsBuf kWorkspace[] = {
    {&bz_gpu_engine::lblocks, sizeof(BlockDesc), 0, false},
    {&bz_gpu_engine::lcrc, 4, 0, false},
    {&bz_gpu_engine::SA, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::R, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::KA, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::VA, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::KB, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::VB, (size_t)kSlot * 4, 0, false},
    {&bz_gpu_engine::tile_hist, (size_t)kTilesPerBlock * kMaxBins * 4, 0, false},
    {&bz_gpu_engine::count, 4, 0, false},
    {&bz_gpu_engine::bin_base, (size_t)kMaxBins * 4, 0, false},
    {&bz_gpu_engine::sym_code, 256, 0, false},
    {&bz_gpu_engine::count2, 4, 0, false},
    {&bz_gpu_engine::tile_nf, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::keyinfo, 4, 0, false},
    {&bz_gpu_engine::flags, kSlot, 0, false},
    {&bz_gpu_engine::newbits, kSlot / 8, 256, false},
    {&bz_gpu_engine::tlo, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::tln, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::nonfinal, 4, 0, false},
    {&bz_gpu_engine::active, 0, 64 * 8 + 64 * 4, false},
    {&bz_gpu_engine::per_k, 4, 0, false},
    {&bz_gpu_engine::per_shift, 4, 0, false},
    {&bz_gpu_engine::lin_p, (size_t)4 * kPerK, 0, false},
    {&bz_gpu_engine::lin_sig, (size_t)4 * kPerK, 0, false},
    {&bz_gpu_engine::bin_cursor, (size_t)1024 * 4, 0, false},
    {&bz_gpu_engine::pb_gate, 4, 1024, false}, // (+ loc_stats behind the gates: 256 words)
    {&bz_gpu_engine::L, kSlot, 64, false},
    {&bz_gpu_engine::orig_ptr, 4, 0, false},
    {&bz_gpu_engine::inuse_bits, 32, 0, false},
    {&bz_gpu_engine::summ, (size_t)kMaxMtfChunks * 256, 0, false},
    {&bz_gpu_engine::summ_len, (size_t)kMaxMtfChunks * 2, 0, false},
    {&bz_gpu_engine::init_state, (size_t)kMaxMtfChunks * 256, 0, false},
    {&bz_gpu_engine::rank8, kSlot, 64, false},
    // the last column without its repeats (k_mtf.hip "M0"): buffers of their own -- the sort's `flags` and `ptext` are
    // idle during the tail stages of encode_batch, but bz_gpu_debug_mtf and a redo on the main stream would each need
    // the same argument, and 1.0 MB beside 35 is not worth one
    {&bz_gpu_engine::mtf_heads_buf, kSlot, 64, false},
    {&bz_gpu_engine::headbits, kSlot / 8, 64, false},
    {&bz_gpu_engine::hcount, 4, 0, false},
    {&bz_gpu_engine::tile_hcnt, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::tile_hbase, (size_t)kTilesPerBlock * 4, 0, false},
    // the packed text has its own buffer: in the pair form it takes up to 10 bits per position, more than rank8's bytes
    // (which it borrowed until round 7); `impure` of the period and link rounds still fits, its stride is kSlot
    {&bz_gpu_engine::ptext, kPtSlot, 64, false},
    {&bz_gpu_engine::pair_bits, (size_t)kPairWords * 4, 0, false},
    {&bz_gpu_engine::ztile_last, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::ztile_cnt, (size_t)kTilesPerBlock * 4, 0, false},
    {&bz_gpu_engine::zstate, (size_t)kTilesPerBlock * 16, 0, false},
    {&bz_gpu_engine::ztick, 0, 64, false},
    {&bz_gpu_engine::mtf, (size_t)kMtfStride * 2, 0, false},
    {&bz_gpu_engine::mtf_freq, (size_t)kMaxAlpha * 4, 0, false},
    {&bz_gpu_engine::bout, sizeof(BlockOut), 0, false},
    {&bz_gpu_engine::selector, kSelStride, 0, false},
    {&bz_gpu_engine::code_len, (size_t)6 * kMaxAlpha * 4, 0, false},
    {&bz_gpu_engine::group_bitoff, (size_t)kGboStride * 4, 0, false},
    {&bz_gpu_engine::lm_scratch, (size_t)6 * kLmWords * 4, 0, false},
    {&bz_gpu_engine::hglen, (size_t)6 * (kMaxAlpha + 6), 0, false},
    {&bz_gpu_engine::hpack, (size_t)kMaxAlpha * 8, 0, false},
    {&bz_gpu_engine::hrfreq, (size_t)6 * kMaxAlpha * 4, 0, false},
    {&bz_gpu_engine::hlm, 4, 0, false},
    {&bz_gpu_engine::hpass, (size_t)32 * 4, 0, false},
    {&bz_gpu_engine::stream, (size_t)kStreamWords * 4, 0, false},
    {&bz_gpu_engine::error_flag, 0, 4, false},
    {&bz_gpu_engine::packlist, sizeof(PackBlock), 0, false},
    {&bz_gpu_engine::gh_tiles, (size_t)kTilesPerBlock * 3 * kMaxBins * 4, 0, true},
    {&bz_gpu_engine::gbase, (size_t)3 * kMaxBins * 4, 0, true},
    // the key boundaries of the init's order, a bit per position (k_radix_scatter_lb<SRC_WALKA> -> k_group_refine<true, true>).
    // Not `newbits`: the refinement reads the bit behind a wave's span when another tile may have written that word of newbits.
    {&bz_gpu_engine::abits, kSlot / 8, 256, true},
    {&bz_gpu_engine::tile_state, (size_t)kTilesPerBlock * kMaxBins * 4, 0, true},
    {&bz_gpu_engine::tickets, 0, (size_t)kSortEpochs * 8 * 4 + 64, true},
};
// Per block in flight, before DevBuf's slack of one eighth: 36 441 696 bytes (32 700 000 without the fused radix passes).
// The batch workspace holds `ws_blocks` blocks in flight: as many as the call at hand needs (up to max_blocks, the batch
// size), grown when a later call needs more -- a context that only ever sees small inputs does not take 36.4 MB x max_blocks.
static int ensure_workspace(bz_gpu_engine *g, size_t need_blocks)
{
    if (need_blocks > g->max_blocks) need_blocks = g->max_blocks;
    if (need_blocks < 8) need_blocks = 8;
    if (g->ws_blocks >= need_blocks) return BZ_OK;
    // (grow in steps: a stream of growing chunks does not reallocate for every one)
    size_t nb = need_blocks + need_blocks / 4;
    if (nb > g->max_blocks) nb = g->max_blocks;
    g->ws_blocks = 0; // (a growth that fails half way leaves some buffers NULL: the next call must ensure them all again)
    const bool fused = fused_wanted();
    for (const WsBuf &w : kWorkspace) {
        if (w.fused_only && !fused) continue;
        if (const int rc = (g->*w.buf).ensure(nb * w.per_block + w.fixed)) return rc;
    }
    // (cleared ON THE ENGINE'S STREAM: a memset on the null stream is not ordered against work on a non-blocking stream,
    // and it need not be over when the call returns)
    if (hipMemsetAsync(g->pb_gate.p, 0, g->pb_gate.cap, g->st) != hipSuccess) return BZ_E_UNEXPECTED;
    if (fused && (hipMemsetAsync(g->tile_state.p, 0, g->tile_state.cap, g->st) != hipSuccess ||
                  hipMemsetAsync(g->tickets.p, 0, g->tickets.cap, g->st) != hipSuccess))
        return BZ_E_UNEXPECTED;
    if (fused) g->sort_epoch = 0;
    g->ws_blocks = nb;
    return BZ_OK;
}

extern "C" int bz_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" size_t bz_encode_bound(size_t n)
{
    // RLE1 expands by at most 5/4; a Huffman code over <= 258 symbols averages < 10 bits;
    // per block: header + selectors + tables < 24 KiB.
    return n + n / 2 + (n / 700000 + 2) * 24576 + 64;
}

extern "C" int bz_gpu_engine_create(bz_gpu_engine **out, int device, size_t max_blocks_in_flight)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return BZ_E_NOGPU;
    if (device < 0 || device >= ndev) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(device));
    bz_gpu_engine *g = new bz_gpu_engine();
    g->device = device;
    g->max_blocks = max_blocks_in_flight ? max_blocks_in_flight : 64;
    g->verify = bzgpu::env_verify();
    HIPCHK(hipStreamCreateWithFlags(&g->st, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&g->st2, hipStreamNonBlocking));
    HIPCHK(hipHostMalloc((void **)&g->h_active, 64, hipHostMallocDefault));

    // CRC byte table (src/crc32.rs:58-72) and powers of x
    u32 tab[256], xp16[256], xp2[48];
    for (u32 i = 0; i < 256; ++i) {
        u32 v = i << 24;
        for (int k = 0; k < 8; ++k) v = (v & 0x80000000u) ? ((v << 1) ^ kCrcPoly) : (v << 1);
        tab[i] = v;
    }
    xp2[0] = 0x100u; // x^8
    for (int k = 1; k < 48; ++k) xp2[k] = gf_mulmod(xp2[k - 1], xp2[k - 1]);
    xp16[0] = 1u;
    for (int k = 1; k < 256; ++k) xp16[k] = gf_mulmod(xp16[k - 1], xp2[4]); // * x^(8*16)
    int rc;
    if ((rc = g->crc_tab.ensure(sizeof(tab))) || (rc = g->xp16.ensure(sizeof(xp16))) ||
        (rc = g->xp2.ensure(sizeof(xp2)))) {
        delete g;
        return rc;
    }
    HIPCHK(hipMemcpy(g->crc_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g->xp16.p, xp16, sizeof(xp16), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(g->xp2.p, xp2, sizeof(xp2), hipMemcpyHostToDevice));
    *out = g;
    return BZ_OK;
}

// Sizes the batch workspace for `blocks` blocks in flight now (clamped to the engine's maximum), so that a caller who
// knows what is coming -- a one-shot call that will hand this engine jobs of a known size -- pays ONE allocation
// instead of a small one for its first job and a larger one (after freeing the first) for its second: fresh device
// memory costs about 40 ms per GiB on this platform.
extern "C" int bz_gpu_engine_reserve(bz_gpu_engine *g, size_t blocks)
{
    if (!g) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    return ensure_workspace(g, blocks);
}

extern "C" void bz_gpu_engine_destroy(bz_gpu_engine *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->st);
    (void)hipStreamSynchronize(g->st2);
    dec_workspace_free(g->dec);
    df_workspace_free(g->df);
    lzh_workspace_free(g->lzh);
    lha_workspace_free(g->lha);
    if (g->h_active) (void)hipHostFree(g->h_active);
    mail_release(g->st);
    mail_release(g->st2);
    if (g->st) (void)hipStreamDestroy(g->st);
    if (g->ev_aux) (void)hipEventDestroy(g->ev_aux);
    if (g->st2) (void)hipStreamDestroy(g->st2);
    delete g; // (the device buffers go with it: dev_buf.h)
}

static RleBuffers rle_buffers(bz_gpu_engine *g)
{
    RleBuffers rb;
    rb.tile_last = g->tile_last.as<i64>();
    rb.carry_in = g->carry_in.as<i64>();
    rb.tile_crc = g->tile_crc.as<u32>();
    rb.tile_count = g->tile_count.as<u32>();
    rb.tile_off = g->tile_off.as<u64>();
    rb.sub_off = g->sub_off.as<u16>();
    rb.sub_rs = g->sub_rs.as<i64>();
    rb.total = g->scal.as<u64>();
    rb.cut_result = g->scal.as<u64>() + 2;
    rb.scan_part = g->scan_part.as<u64>();
    rb.lb_ctl = g->rle_lb.as<u32>();
    rb.lb_rs = g->rle_lb.p ? reinterpret_cast<u64 *>(g->rle_lb.as<u8>() + 64) : nullptr;
    rb.lb_off = g->rle_lb.p ? rb.lb_rs + g->rle_lb_spans : nullptr;
    return rb;
}

// BZ_RLE_ONEPASS=0: the three-kernel front end from the start; BZ_RLE_ONEPASS_FAILTEST=1: the host treats the first
// one-pass split of every engine as failed and redoes it (tests/test_gpu_rle_onepass.py)
static bool onepass_wanted()
{
    static const bool on = !(getenv("BZ_RLE_ONEPASS") && atoi(getenv("BZ_RLE_ONEPASS")) == 0);
    return on;
}
static bool onepass_failtest()
{
    static const bool on = getenv("BZ_RLE_ONEPASS_FAILTEST") && atoi(getenv("BZ_RLE_ONEPASS_FAILTEST")) != 0;
    return on;
}
// the image by the three-kernel path (the profile tells the two forms of the front end apart)
static void image_launch(bz_gpu_engine *g, hipStream_t st, u64 tb, u64 t1, u64 in_begin, const RleBuffers &rb, u8 *d_rle)
{
    if (t1 <= tb) return;
    const int pi = g->prof.begin(st, KID_RLE_SCATTER, std::min<u64>(g->n_in, t1 * (u64)kRleTile) - tb * (u64)kRleTile);
    launch_rle_image(st, g->d_in, g->n_in, tb, t1, in_begin, rb, d_rle);
    g->prof.end(st, pi);
}
// The front end in one pass over the whole input: tables, image (g->rle, sized by RLE1's bound: the image is written
// before its length reaches the host) and *last.  false in *done: not taken, or it failed and the engine is off it.
static int onepass_split(bz_gpu_engine *g, u64 ntiles, i64 *d_last, i64 *last, bool *done)
{
    *done = false;
    const u64 n = g->n_in, spans = rle_onepass_spans(ntiles);
    if (g->rle_lb.ensure(64 + spans * 16) || g->rle.ensure(n + n / 4 + 256)) {
        (void)hipGetLastError(); // (the three kernels need neither)
        return BZ_OK;
    }
    // (a fresh or regrown buffer holds anything, and so may a tag of 65 535 launches ago: clear, and count from 1)
    if (g->rle_lb_spans < spans || g->rle_epoch == 0 || g->rle_epoch >= rle_onepass_epochs()) {
        g->rle_lb_spans = (g->rle_lb.cap - 64) / 16;
        HIPCHK(hipMemsetAsync(g->rle_lb.p, 0, g->rle_lb.cap, g->st));
        g->rle_epoch = 0;
    }
    ++g->rle_epoch;
    const RleBuffers rb = rle_buffers(g);
    const int pi = g->prof.begin(g->st, KID_RLE_ONEPASS, n);
    launch_rle_onepass(g->st, g->d_in, n, ntiles, g->rle_epoch, g->crc_tab.as<u32>(), g->xp16.as<u32>(), rb, g->rle.as<u8>(), d_last);
    g->prof.end(g->st, pi);
    u32 ctl[2] = {0, 0};
    u64 total = 0;
    MAILCHK(g->st, {last, d_last, 8}, {&total, rb.total, 8}, {ctl, rb.lb_ctl, 8});
    HIPCHK(hipGetLastError());
    if (ctl[0] != (u32)spans || ctl[1] != 0 || onepass_failtest()) {
        fprintf(stderr, "bz2_mi355x: the one-pass RLE1 front end did not complete (%u of %llu spans, error word %u); the three kernels take over\n",
                ctl[0], (unsigned long long)spans, ctl[1]);
        g->rle_onepass_broken = true;
        g->rle_epoch = 0; // (words of a launch that stopped half way: cleared before anybody reads them again)
        *last = -1;
        return BZ_OK;
    }
    g->onepass_total = total;
    *done = true;
    return BZ_OK;
}

// ---- the split, in three steps (a slab of tiles per rank; one rank = the whole input) ------------
extern "C" int bz_gpu_partition_slab_begin(bz_gpu_engine *g, int level, const void *d_in, size_t n,
                                           uint64_t tile0, uint64_t tile1, int64_t *slab_last_start)
{
    if (!g || level < 1 || level > 9) return BZ_E_PARAM;
    if (n && ((uintptr_t)d_in & 15u)) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    const u64 ntiles = (n + kRleTile - 1) / kRleTile;
    if (tile1 > ntiles) tile1 = ntiles;
    if (tile0 > tile1) tile0 = tile1;
    g->level = level;
    g->d_in = (const u8 *)d_in;
    g->n_in = n;
    g->slab_t0 = tile0;
    g->slab_t1 = tile1;
    g->h_blocks.clear();
    g->h_crc.clear();
    for (double &t : g->t_stage) t = 0;
    for (u64 &s : g->bwt_stats) s = 0;
    for (u64 &s : g->round_active) s = 0;
    if (slab_last_start) *slab_last_start = -1;
    if (ntiles == 0) return BZ_OK;
    int rc;
    if ((rc = g->tile_last.ensure(ntiles * 8)) || (rc = g->carry_in.ensure(ntiles * 8)) ||
        (rc = g->tile_crc.ensure(ntiles * 4)) || (rc = g->tile_count.ensure(ntiles * 4)) ||
        (rc = g->tile_off.ensure((ntiles + 1) * 8)) || (rc = g->sub_off.ensure(ntiles * 32)) ||
        (rc = g->sub_rs.ensure(ntiles * 128)) || (rc = g->scal.ensure(128)) ||
        (rc = g->scan_part.ensure((ntiles / 1024 + 2) * 8)))
        return rc;
    const int sp = span_begin(g, 0);
    i64 *d_last = reinterpret_cast<i64 *>(g->scal.as<u64>() + 8);
    // one engine codes the whole input: scan, carries, counts, offsets and the image in one pass over it
    g->onepass_done = false;
    if (tile0 == 0 && tile1 == ntiles && onepass_wanted() && !g->rle_onepass_broken) {
        i64 last = -1;
        bool done = false;
        if ((rc = onepass_split(g, ntiles, d_last, &last, &done)) != BZ_OK) {
            span_end(g, sp);
            return rc;
        }
        if (done) {
            g->onepass_done = true;
            span_end(g, sp);
            if (slab_last_start) *slab_last_start = last;
            return BZ_OK;
        }
    }
    const RleBuffers rb = rle_buffers(g);
    launch_rle_scan(g->st, g->d_in, n, tile0, tile1, 0, g->crc_tab.as<u32>(), g->xp16.as<u32>(), rb);
    // the range's last run start falls out of the carry scan (its carries are redone in _count)
    if (tile1 > tile0) {
        launch_slab_last(g->st, rb, tile0, tile1, d_last);
        i64 last = -1;
        span_end(g, sp);
        MAILCHK(g->st, {&last, d_last, 8});
        if (slab_last_start) *slab_last_start = last;
    } else {
        span_end(g, sp);
    }
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

extern "C" int bz_gpu_partition_slab_count(bz_gpu_engine *g, int64_t carry_run)
{
    if (!g) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    if (g->slab_t1 <= g->slab_t0) return BZ_OK;
    if (g->onepass_done && carry_run == -1) return BZ_OK; // (k_rle_onepass wrote the carries and the counts)
    g->onepass_done = false;
    const RleBuffers rb = rle_buffers(g);
    const int sp = span_begin(g, 0);
    // (the run start live at the first byte BEHIND the slab goes to carry_in[slab_t1]: the cut tables look at that tile)
    const u64 ntiles = (g->n_in + kRleTile - 1) / kRleTile;
    launch_rle_count(g->st, g->d_in, g->n_in, g->slab_t0, g->slab_t1, 0, carry_run, rb,
                     g->slab_t1 < ntiles ? rb.carry_in + g->slab_t1 : nullptr);
    span_end(g, sp);
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

// The last step of the split in two halves, so that a rank of a sharded job can hand the cut on before it writes
// its image: only the chain of cuts depends on the rank before (and the next rank's on this one's).
//   slab_cuts : left halo, tile offsets, the cut chain from start_in -> blocks, next_in, tail
//   slab_image: the RLE1 image of [tb, t1), block CRCs, the host copies of the block records
struct SlabCuts {
    u64 tb = 0, start_in = 0;
    size_t nb = 0;
    int span = -1;
    bool pending = false, image_done = false;
};
static bool cut_tables_enabled()
{
    static const bool on = [] {
        const char *e = getenv("BZ_CUT_TABLES");
        return !(e && atoi(e) == 0);
    }();
    return on;
}
static CutBuffers cut_buffers(bz_gpu_engine *g)
{
    CutBuffers cb;
    cb.step_t0 = g->cut_step_t0.as<u64>();
    cb.step_nt = g->cut_step_nt.as<u32>();
    cb.step_w0 = g->cut_step_w0.as<u64>();
    cb.tab = g->cut_tab.as<u32>();
    cb.comp = g->cut_comp.as<u16>();
    return cb;
}
// Fills the cut tables for the targets inside the range [tb, t1) whose image is `total` bytes and begins at offset
// g_base of the whole input's image (tile_off relative to tb must be there).  g->cut_ready says whether they will
// answer: not when the switch is off or the range is beyond what the tables are sized for (the chain kernel then).
// One host synchronisation (the number of workgroups of the table kernel).
static int cut_tables_prepare(bz_gpu_engine *g, u64 g_base, u64 total, u64 tb, u64 t1)
{
    g->cut_ready = false;
    if (!cut_tables_enabled()) return BZ_OK;
    const u64 ntiles = (g->n_in + kRleTile - 1) / kRleTile;
    CutPlan pl;
    pl.L = (u64)g->level * 100000u - 19u; // encoder.rs:186
    pl.g_base = g_base;
    pl.own_hi = g_base + total;
    pl.tb = tb;
    pl.t1 = t1;
    pl.t_last = t1 < ntiles ? t1 : (t1 > tb ? t1 - 1 : tb);
    pl.t_eval = t1 > tb ? t1 - 1 : tb;
    pl.w_min = g_base >= 4u ? g_base - 3u : 1u;
    pl.j_lo = pl.w_min - 1u < pl.L ? 0 : (pl.w_min - 1u - pl.L) / (pl.L + 4u) + 1u; // smallest j with (j + 1) L + 4 j >= w_min
    const bool none = t1 <= tb || pl.own_hi < pl.L || pl.own_hi / pl.L - 1u < pl.j_lo;
    if (none) {
        pl.j_lo = 1;
        pl.j_hi = 0;
    } else {
        pl.j_hi = pl.own_hi / pl.L - 1u; // largest j with (j + 1) L <= own_hi
    }
    const u64 nsteps = none ? 0 : pl.j_hi - pl.j_lo + 1u;
    const u64 entries = cut_table_entries(pl);
    // The tables grow with the SQUARE of the number of blocks behind one start (2 N^2 entries): beyond 2^26 entries
    // (256 MB; 5 800 blocks = 5 GiB at level 9, 0.55 GiB at level 1) the chain kernel's ~4 ms per GiB are cheaper than
    // the room and the clearing, and so they are when the room cannot be had.
    if (nsteps / 16u + 64u >= cut_seg_cap() || entries > (1ull << 26)) return BZ_OK;
    u64 g_lo, g_hi, centries;
    cut_groups(pl, &g_lo, &g_hi, &centries);
    if (g->cut_step_t0.ensure((nsteps + 1) * 8) || g->cut_step_nt.ensure((nsteps + 1) * 4) || g->cut_step_w0.ensure((nsteps + 2 + nsteps / 1024 + 4) * 8) ||
        g->cut_tab.ensure((entries + 1) * 4) || g->cut_comp.ensure((centries + 1) * 2)) {
        (void)hipGetLastError(); // (an allocation that failed is not an error of the encode: the chain kernel needs none of it)
        return BZ_OK;
    }
    g->cut_plan = pl;
    if (nsteps) {
        const RleBuffers rb = rle_buffers(g);
        const CutBuffers cb = cut_buffers(g);
        launch_cut_steps(g->st, pl, rb, cb);
        u64 work = 0;
        MAILCHK(g->st, {&work, cb.step_w0 + nsteps, 8});
        if (work >= (1ull << 31)) return BZ_OK;
        const u64 n_lim = std::min<u64>(g->n_in, (pl.t_last + 1u) * (u64)kRleTile);
        launch_cut_tables(g->st, pl, g->d_in, n_lim, rb, cb, work);
    }
    g->cut_ready = true;
    return BZ_OK;
}
// The chain from block j0 at image offset s0 / input byte start_in; the image of the range begins at g->rle + rle_at.
// res: blocks, consumed, tail flag, image offset and number of the block behind the last one cut here.
static int cut_tables_select(bz_gpu_engine *g, u64 j0, u64 s0, u64 start_in, u64 rle_at, int emit_tail, u32 max_blocks,
                             u64 res[5])
{
    const RleBuffers rb = rle_buffers(g);
    launch_cut_select(g->st, g->cut_plan, j0, s0, start_in, g->n_in, (long long)rle_at - (long long)g->cut_plan.g_base, emit_tail, rb,
                      cut_buffers(g), g->blocks_all.as<BlockDesc>(), max_blocks);
    MAILCHK(g->st, {res, rb.cut_result, 5 * sizeof(u64)});
    return BZ_OK;
}

// image_beside: the image is written on g->st while the cut chain runs on g->st2 (nobody waits for the cut)
static int slab_cuts(bz_gpu_engine *g, uint64_t start_in, int is_last, bool image_beside, SlabCuts &sc, size_t *n_blocks,
                     uint64_t *next_in, int *tail_block)
{
    sc = SlabCuts();
    HIPCHK(hipSetDevice(g->device));
    if (n_blocks) *n_blocks = 0;
    if (next_in) *next_in = start_in;
    if (tail_block) *tail_block = 0;
    const u64 n = g->n_in;
    if (n == 0) return BZ_OK;
    const u64 t0 = g->slab_t0, t1 = g->slab_t1;
    u64 tb = start_in / kRleTile; // tile holding the first byte of this rank's first block
    if (tb > t0) tb = t0;         // (start_in never lies beyond the slab's first byte)
    if (start_in > t0 * (u64)kRleTile) return BZ_E_PARAM;
    const RleBuffers rb = rle_buffers(g);
    const u32 block_max_len = (u32)g->level * 100000u - 19u; // encoder.rs:186
    sc.span = span_begin(g, 0);
    if (tb < t0) {
        // left halo: the tail of the previous slab(s) that belongs to this rank's first block, coded
        // afresh from the cut (RLE1 restarted at a cut is RLE1 continued)
        launch_rle_scan(g->st, g->d_in, n, tb, t0, start_in, g->crc_tab.as<u32>(), g->xp16.as<u32>(), rb);
        launch_rle_count(g->st, g->d_in, n, tb, t0, start_in, -1, rb, nullptr);
    }
    // (the one pass has written the offsets and the image, and its total came with its tickets)
    const bool onepass = g->onepass_done && start_in == 0 && t0 == 0;
    u64 total = g->onepass_total;
    if (!onepass) {
        g->onepass_done = false;
        launch_rle_prefix(g->st, tb, t1, rb);
        MAILCHK(g->st, {&total, rb.total, 8});
    }
    const size_t max_blocks = (size_t)(total / block_max_len + 2);
    int rc;
    if ((rc = g->rle.ensure(total + 256)) || (rc = g->blocks_all.ensure(max_blocks * sizeof(BlockDesc))) ||
        (rc = g->crc_all.ensure(max_blocks * 4)))
        return rc;
    // The cut chain (one workgroup, latency-bound) stays on g->st, which is busy and starts it at once; the image
    // (262 144 workgroups per GiB) goes to g->st2, whose first launch after a pause comes ~100 us later -- the order
    // that lets the chain's workgroup in first (the other way round it took 3.2 ms instead of 1.8 in two runs of
    // three).  g->st waits for the image before it goes on.
    // From the first byte of the input every cut is one of 4 j + 1 known candidates: the tables (k_rle1.hip, "kernels
    // H") answer them all at once; the chain kernel is what a caller with a start_in of its own gets, and the fallback.
    const bool tables = start_in == 0 && t0 == 0 && cut_tables_enabled();
    if (onepass) {
        sc.image_done = true;
        image_beside = false;
    }
    if (image_beside) {
        if (!g->ev_aux) HIPCHK(hipEventCreateWithFlags(&g->ev_aux, hipEventDisableTiming));
        if (tables) { // (the table kernels are small launches: the image goes first and they run beside it)
            image_launch(g, g->st2, tb, t1, start_in, rb, g->rle.as<u8>());
            HIPCHK(hipEventRecord(g->ev_aux, g->st2));
            sc.image_done = true;
        }
    }
    u64 res[5] = {~0ull, 0, 0, 0, 0};
    if (tables) {
        if ((rc = cut_tables_prepare(g, 0, total, tb, t1)) != BZ_OK) return rc;
        if (g->cut_ready && (rc = cut_tables_select(g, 0, 0, 0, 0, is_last ? 1 : 0, (u32)max_blocks, res)) != BZ_OK) return rc;
        if (res[0] == ~0ull) {
            if (g->cut_ready) fprintf(stderr, "bz2_mi355x: the cut tables did not answer a target; the chain kernel takes over\n");
            ++g->cut_stats[1];
        } else {
            ++g->cut_stats[0];
        }
    }
    if (res[0] == ~0ull) {
        launch_rle_cuts(g->st, g->d_in, n, tb, t1, start_in, rb, block_max_len, is_last ? 1 : 0,
                        g->blocks_all.as<BlockDesc>(), (u32)max_blocks);
        if (image_beside && !sc.image_done) {
            image_launch(g, g->st2, tb, t1, start_in, rb, g->rle.as<u8>());
            HIPCHK(hipEventRecord(g->ev_aux, g->st2));
            sc.image_done = true;
        }
        MAILCHK(g->st, {res, rb.cut_result, 3 * sizeof(u64)});
    }
    if (image_beside) HIPCHK(hipStreamWaitEvent(g->st, g->ev_aux, 0));
    const size_t nb = (size_t)res[0];
    if (nb > max_blocks) return BZ_E_UNEXPECTED;
    sc.tb = tb;
    sc.start_in = start_in;
    sc.nb = nb;
    sc.pending = true;
    if (n_blocks) *n_blocks = nb;
    if (next_in) *next_in = nb || is_last ? res[1] : start_in;
    if (tail_block) *tail_block = (int)res[2];
    return BZ_OK;
}
static int slab_image(bz_gpu_engine *g, SlabCuts &sc)
{
    if (!sc.pending) return BZ_OK;
    sc.pending = false;
    const RleBuffers rb = rle_buffers(g);
    if (!sc.image_done) image_launch(g, g->st, sc.tb, g->slab_t1, sc.start_in, rb, g->rle.as<u8>());
    const size_t nb = sc.nb;
    g->h_blocks.resize(nb);
    g->h_crc.resize(nb);
    if (nb) {
        launch_block_crc(g->st, g->d_in, g->blocks_all.as<BlockDesc>(), (u32)nb, g->crc_tab.as<u32>(),
                         g->xp2.as<u32>(), g->tile_crc.as<u32>(), g->crc_all.as<u32>());
    }
    span_end(g, sc.span);
    if (nb) MAILCHK(g->st, {g->h_blocks.data(), g->blocks_all.p, nb * sizeof(BlockDesc)}, {g->h_crc.data(), g->crc_all.p, nb * 4});
    spans_collect(g);
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

// ---- a rank of a sharded job: what does not depend on the rank in front of it happens before that rank's cut arrives --
// The slab's image offsets and its image do not depend on where the first block begins (RLE1 is a function of the input
// alone: the run start live at the slab's first byte came with the all-gather), and with the slab's offset in the image
// of the WHOLE input (an all-gather of the slabs' totals) neither do the cuts: the tables answer every target inside the
// slab.  What is left for the link of the serial chain is k_cut_select.  The bytes of the first block that lie in front
// of the slab (the halo) are coded after the cut has been handed on, into the room in front of the slab's image.
struct SlabSpec {
    u64 total = 0;    // bytes of the slab's image
    u64 g_base = 0;   // its offset in the image of the whole input
    u64 halo_cap = 0; // room in front of it in g->rle
    bool image_done = false;
    u64 want_halo_total = 0; // (what was found: g->h_halo_total)
};
static int slab_spec_total(bz_gpu_engine *g, SlabSpec &sp)
{
    sp = SlabSpec();
    if (g->n_in == 0) return BZ_OK;
    HIPCHK(hipSetDevice(g->device));
    g->onepass_done = false; // (a rank of a sharded job lays its image out behind a halo: the slab's own offsets and image)
    const RleBuffers rb = rle_buffers(g);
    const int span = span_begin(g, 0);
    launch_rle_prefix(g->st, g->slab_t0, g->slab_t1, rb);
    span_end(g, span);
    MAILCHK(g->st, {&sp.total, rb.total, 8});
    return BZ_OK;
}
static int slab_spec_tables(bz_gpu_engine *g, SlabSpec &sp, u64 g_base)
{
    sp.g_base = g_base;
    g->cut_ready = false;
    if (g->n_in == 0) return BZ_OK;
    const u64 L = (u64)g->level * 100000u - 19u;
    sp.halo_cap = g_base ? (L + 8u + 255u) / 256u * 256u : 0u;
    const size_t max_blocks = (size_t)((sp.total + L + 4u) / L + 2u);
    int rc;
    if ((rc = g->rle.ensure(sp.halo_cap + sp.total + 256)) || (rc = g->blocks_all.ensure(max_blocks * sizeof(BlockDesc))) ||
        (rc = g->crc_all.ensure(max_blocks * 4)))
        return rc;
    const RleBuffers rb = rle_buffers(g);
    const int span = span_begin(g, 0);
    if (!g->ev_aux) HIPCHK(hipEventCreateWithFlags(&g->ev_aux, hipEventDisableTiming));
    image_launch(g, g->st2, g->slab_t0, g->slab_t1, 0, rb, g->rle.as<u8>() + sp.halo_cap);
    HIPCHK(hipEventRecord(g->ev_aux, g->st2));
    sp.image_done = true;
    rc = cut_tables_prepare(g, g_base, sp.total, g->slab_t0, g->slab_t1);
    span_end(g, span);
    return rc;
}
// start_in / s0 / j0: first input byte, image offset and number (in the whole input) of this rank's first block
static int slab_spec_select(bz_gpu_engine *g, SlabSpec &sp, u64 start_in, u64 s0, u64 j0, int is_last, SlabCuts &sc,
                            size_t *n_blocks, u64 *next_in, u64 *s_next, u64 *j_next)
{
    sc = SlabCuts();
    *n_blocks = 0;
    *next_in = start_in;
    *s_next = s0;
    *j_next = j0;
    if (g->n_in == 0) return BZ_OK;
    const u64 t0 = g->slab_t0;
    if (start_in > t0 * (u64)kRleTile || s0 > sp.g_base) return BZ_E_PARAM;
    const u64 L = (u64)g->level * 100000u - 19u;
    const u64 D = sp.g_base - s0; // bytes of the first block's image in front of the slab
    if (D > sp.halo_cap) return BZ_E_UNEXPECTED;
    const size_t max_blocks = (size_t)((sp.total + L + 4u) / L + 2u);
    u64 res[5] = {~0ull, 0, 0, 0, 0};
    int rc;
    if (g->cut_ready) {
        if ((rc = cut_tables_select(g, j0, s0, start_in, sp.halo_cap, is_last, (u32)max_blocks, res)) != BZ_OK) return rc;
        if (res[0] == ~0ull) fprintf(stderr, "bz2_mi355x: the cut tables did not answer a target; the chain kernel takes over\n");
    }
    if (res[0] == ~0ull) {
        // the chain kernel: offsets relative to the first block's first tile, the image written again from there
        if (cut_tables_enabled()) ++g->cut_stats[1];
        HIPCHK(hipStreamWaitEvent(g->st, g->ev_aux, 0));
        sp.image_done = false;
        int tail = 0;
        if ((rc = slab_cuts(g, start_in, is_last, false, sc, n_blocks, next_in, &tail)) != BZ_OK) return rc;
        std::vector<BlockDesc> hb(*n_blocks);
        if (*n_blocks) HIPCHK(hipMemcpy(hb.data(), g->blocks_all.p, *n_blocks * sizeof(BlockDesc), hipMemcpyDeviceToHost));
        const size_t closed = *n_blocks - (tail ? 1 : 0);
        for (size_t k = 0; k < closed; ++k) *s_next += hb[k].n;
        *j_next = j0 + closed;
        return BZ_OK;
    }
    ++g->cut_stats[0];
    if (res[0] > max_blocks) return BZ_E_UNEXPECTED;
    sc.tb = std::min<u64>(start_in / kRleTile, t0);
    sc.start_in = start_in;
    sc.nb = (size_t)res[0];
    sc.pending = true;
    sc.image_done = true;
    sc.span = -1;
    *n_blocks = sc.nb;
    *next_in = sc.nb || is_last ? res[1] : start_in;
    *s_next = res[3];
    *j_next = res[4];
    sp.want_halo_total = D;
    return BZ_OK;
}
// the halo's image, then block CRCs and the host copies of the records (slab_image)
static int slab_spec_finish(bz_gpu_engine *g, SlabSpec &sp, SlabCuts &sc)
{
    if (!sc.pending) return BZ_OK;
    if (!sp.image_done) return slab_image(g, sc); // (the chain kernel's layout)
    const RleBuffers rb = rle_buffers(g);
    const u64 t0 = g->slab_t0;
    sc.span = span_begin(g, 0);
    g->h_halo_total = sp.want_halo_total;
    if (sc.tb < t0) {
        // left halo: the tail of the previous slab(s) that belongs to this rank's first block, coded afresh from the
        // cut (RLE1 restarted at a cut is RLE1 continued); it ends where the slab's image begins
        launch_rle_scan(g->st, g->d_in, g->n_in, sc.tb, t0, sc.start_in, g->crc_tab.as<u32>(), g->xp16.as<u32>(), rb);
        launch_rle_count(g->st, g->d_in, g->n_in, sc.tb, t0, sc.start_in, -1, rb, nullptr);
        launch_rle_prefix(g->st, sc.tb, t0, rb, false);
        HIPCHK(hipMemcpyAsync(&g->h_halo_total, rb.total, 8, hipMemcpyDeviceToHost, g->st)); // (checked by the caller once the stream has been waited for)
        image_launch(g, g->st, sc.tb, t0, sc.start_in, rb, g->rle.as<u8>() + sp.halo_cap - sp.want_halo_total);
    }
    HIPCHK(hipStreamWaitEvent(g->st, g->ev_aux, 0)); // the slab's image (st2)
    return slab_image(g, sc);
}

extern "C" int bz_gpu_partition_slab_finish(bz_gpu_engine *g, uint64_t start_in, int is_last, size_t *n_blocks,
                                            uint64_t *next_in, int *tail_block)
{
    if (!g) return BZ_E_PARAM;
    SlabCuts sc;
    // (one GPU, or a caller that drives the steps itself: the image is written beside the cut chain)
    const int rc = slab_cuts(g, start_in, is_last, true, sc, n_blocks, next_in, tail_block);
    if (rc != BZ_OK) {
        if (sc.span >= 0) { span_end(g, sc.span); spans_collect(g); }
        return rc;
    }
    return slab_image(g, sc);
}

extern "C" int bz_gpu_partition(bz_gpu_engine *g, int level, const void *d_in, size_t n, int mode,
                                size_t *n_blocks, size_t *consumed, int *tail_block)
{
    if (!g || level < 1 || level > 9) return BZ_E_PARAM;
    if (n_blocks) *n_blocks = 0;
    if (consumed) *consumed = 0;
    if (tail_block) *tail_block = 0;
    const u64 ntiles = (n + kRleTile - 1) / kRleTile;
    int64_t last = -1;
    int rc = bz_gpu_partition_slab_begin(g, level, d_in, n, 0, ntiles, &last);
    if (rc != BZ_OK || n == 0) return rc;
    if ((rc = bz_gpu_partition_slab_count(g, -1)) != BZ_OK) return rc;
    uint64_t next = 0;
    rc = bz_gpu_partition_slab_finish(g, 0, mode == BZ_ACTION_RUN ? 0 : 1, n_blocks, &next, tail_block);
    if (consumed) *consumed = (size_t)next;
    return rc;
}

// Argument blocks for a batch of `nb` blocks: the base of every buffer (the kernels stride by block; what a block takes
// of each buffer is stated once, in kWorkspace).
static BwtArgs make_bwt_args(bz_gpu_engine *g, u32 nb)
{
    BwtArgs x;
    x.rle = g->rle.as<u8>();
    x.blocks = g->lblocks.as<BlockDesc>();
    x.nb = nb;
    x.tiles = kTilesPerBlock;
    x.SA = g->SA.as<u32>();
    x.R = g->R.as<u32>();
    x.KA = g->KA.as<u32>();
    x.VA = g->VA.as<u32>();
    x.KB = g->KB.as<u32>();
    x.VB = g->VB.as<u32>();
    x.tile_hist = g->tile_hist.as<u32>();
    x.count = g->count.as<u32>();
    x.count2 = g->count2.as<u32>();
    x.tile_nf = g->tile_nf.as<u32>();
    x.bin_base = g->bin_base.as<u32>();
    x.flags = g->flags.as<u8>();
    x.newbits = g->newbits.as<u64>();
    x.tile_last_old = g->tlo.as<int>();
    x.tile_last_new = g->tln.as<int>();
    x.nonfinal = g->nonfinal.as<u32>();
    x.active = g->active.as<unsigned long long>();
    x.maxnf = reinterpret_cast<u32 *>(g->active.as<unsigned long long>() + 64);
    x.per_k = g->per_k.as<u32>();
    x.per_shift = g->per_shift.as<u32>();
    x.lin_p = g->lin_p.as<u32>();
    x.lin_sig = g->lin_sig.as<u32>();
    x.bin_cursor = g->bin_cursor.as<u32>();
    x.pb_gate = g->pb_gate.as<u32>();
    x.loc_stats = g->pb_gate.as<u32>() + g->ws_blocks; // (behind the gates)
    x.L = g->L.as<u8>();
    x.orig_ptr = g->orig_ptr.as<u32>();
    x.ptext = g->ptext.as<u8>();
    x.pair_bits = pair_keys_wanted() ? g->pair_bits.as<u32>() : nullptr;
    x.sym_code = g->sym_code.as<u8>();
    x.keyinfo = g->keyinfo.as<u8>();
    x.gh_tiles = g->gh_tiles.as<u32>();
    x.gbase = g->gbase.as<u32>();
    x.abits = g->abits.as<u64>();
    x.pack_blocks = 0;
    x.tile_state = g->tile_state.as<u32>();
    x.tickets = g->tickets.as<u32>();
    x.sort_err = g->tickets.p ? g->tickets.as<u32>() + (size_t)kSortEpochs * 8 : nullptr; // (no fused passes: not allocated)
    x.epoch = &g->sort_epoch;
    x.fused_state = g->fused_state;
    x.tile_state_all = g->tile_state.as<u32>();
    x.tile_state_bytes = g->tile_state.cap;
    x.fused = fused_wanted() ? 1u : 0u;
    static const u32 want_links = (getenv("BZ_LINK_ROUND") && atoi(getenv("BZ_LINK_ROUND")) == 0) ? 0u : 1u;
    x.per_links = want_links;
    x.per_keyshift = 0;
    x.per_wide = 0;
    x.per_aux = g->mtf.as<u8>();
    return x;
}

static MtfArgs make_mtf_args(bz_gpu_engine *g, u32 nb)
{
    MtfArgs ma;
    ma.blocks = g->lblocks.as<BlockDesc>();
    ma.nb = nb;
    ma.tiles = kTilesPerBlock; // (encode_batch: what the batch's largest block needs)
    ma.L = g->L.as<u8>();
    ma.inuse_bits = g->inuse_bits.as<u32>();
    ma.summ = g->summ.as<u8>();
    ma.summ_len = g->summ_len.as<u16>();
    ma.init_state = g->init_state.as<u8>();
    ma.rank8 = g->rank8.as<u8>();
    static const bool want_heads = !(getenv("BZ_MTF_HEADS") && atoi(getenv("BZ_MTF_HEADS")) == 0);
    ma.heads = want_heads ? 1u : 0u;
    // (measurements and tests: 1000 collapses every block, 0 none; the default's evidence is in profiles/r16_mtf_heads.md)
    static const u32 dense_permille = getenv("BZ_MTF_DENSE_PERMILLE") ? (u32)std::min(1000, std::max(0, atoi(getenv("BZ_MTF_DENSE_PERMILLE")))) : 750u;
    ma.dense_permille = dense_permille;
    ma.H = g->mtf_heads_buf.as<u8>();
    ma.headbits = g->headbits.as<u16>();
    ma.hcount = g->hcount.as<u32>();
    ma.tile_hcnt = g->tile_hcnt.as<u32>();
    ma.tile_hbase = g->tile_hbase.as<u32>();
    ma.ztile_last = g->ztile_last.as<int>();
    ma.ztile_cnt = g->ztile_cnt.as<u32>();
    ma.zstate = g->zstate.as<u32>();
    ma.ztick = g->ztick.as<u32>();
    static const bool want_fused_zle = !(getenv("BZ_FUSED_ZLE") && atoi(getenv("BZ_FUSED_ZLE")) == 0);
    ma.fused_zle = (want_fused_zle && !g->zle_fused_broken) ? 1u : 0u;
    ma.mtf = g->mtf.as<u16>();
    ma.mtf_freq = g->mtf_freq.as<u32>();
    ma.out = g->bout.as<BlockOut>();
    return ma;
}

static HuffArgs make_huff_args(bz_gpu_engine *g, u32 nb)
{
    HuffArgs ha;
    ha.blocks = g->lblocks.as<BlockDesc>();
    ha.nb = nb;
    ha.mtf = g->mtf.as<u16>();
    ha.mtf_stride = kMtfStride;
    ha.mtf_freq = g->mtf_freq.as<u32>();
    ha.inuse_bits = g->inuse_bits.as<u32>();
    ha.crc = g->lcrc.as<u32>();
    ha.orig_ptr = g->orig_ptr.as<u32>();
    ha.selector = g->selector.as<u8>();
    ha.code_len = g->code_len.as<u32>();
    ha.group_bitoff = g->group_bitoff.as<u32>();
    ha.lm_scratch = g->lm_scratch.as<u32>();
    ha.glen = g->hglen.as<u8>();
    ha.pack = g->hpack.as<unsigned long long>();
    ha.rfreq = g->hrfreq.as<u32>();
    ha.hlm = g->hlm.as<u32>();
    ha.pass_stats = g->debug_figures ? g->hpass.as<u32>() : nullptr; // (armed by bz_gpu_profile_enable(g, 2))
    ha.stream = g->stream.as<u32>();
    ha.out = g->bout.as<BlockOut>();
    ha.error_flag = g->error_flag.as<u32>();
    return ha;
}

__global__ void k_test_bump(u32 *p, u32 n) { *p = (*p + 1u) % n; } // (fault injections for the self-check's tests)
__global__ void k_test_swap(u8 *L, u32 n)
{
    for (u32 i = n / 2; i + 1 < n; ++i)
        if (L[i] != L[i + 1]) {
            const u8 t = L[i];
            L[i] = L[i + 1];
            L[i + 1] = t;
            return;
        }
}

// symbols in use -> key geometry -> rotation sort.  Returns rounds (<0: error).
static int sort_batch(bz_gpu_engine *g, const BwtArgs &ba, u32 max_n, u64 total_n, u64 *sorted, KernelProf *prof, u64 *round_active)
{
    launch_block_symbols(g->st, ba, g->inuse_bits.as<u32>(), const_cast<u8 *>(ba.sym_code), const_cast<u8 *>(ba.keyinfo));
    std::vector<u8> ki((size_t)ba.nb * 4);
    {
        const MailSeg sg = {ki.data(), ba.keyinfo, ki.size()};
        if (mail_fetch(g->st, &sg, 1) != 0) return -1;
    }
    bool wide = false;
    u32 min_chars = 8;
    u32 pack_blocks = 0; // (KeyInfo {bits, chars, form}: the pair form with 10-bit codes, counts_from_pack in k_bwt.hip)
    for (u32 i = 0; i < ba.nb; ++i) {
        if (ki[(size_t)i * 4 + 2] == 0 && ki[(size_t)i * 4] >= 8) wide = true; // (a pair-form key is never wider than 30 bits)
        if (ki[(size_t)i * 4 + 1] < min_chars) min_chars = ki[(size_t)i * 4 + 1];
        if (ki[(size_t)i * 4 + 2] != 0 && ki[(size_t)i * 4] == 10) pack_blocks += 1;
    }
    BwtArgs bs = ba;
    bs.pack_blocks = pack_blocks;
    return run_bwt(g->st, bs, max_n, total_n, g->h_active, sorted, prof, round_active, wide, min_chars);
}

// Encode one batch of local blocks (descriptors already in g->lblocks / g->lcrc; `descs` is the host copy).  The whole
// batch is sorted on the main stream; MTF / Huffman / emission follow on the second stream behind an event, and the main
// stream waits for them.  (Sub-batches -- the sort of one beside the tail stages of the one before -- were measured in
// rounds 1-2 and dropped: a batch fills the chip better whole.)  Whatever happens, both streams are idle and both events
// are gone when this returns.
static int encode_batch(bz_gpu_engine *g, u32 nb, const std::vector<BlockDesc> &descs)
{
    hipEvent_t ev_fork = nullptr, ev_join = nullptr; // st -> st2 behind the sort, st2 -> st behind the tail stages
    const bool have_events = hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming) == hipSuccess &&
                             hipEventCreateWithFlags(&ev_join, hipEventDisableTiming) == hipSuccess;
    u32 max_n = 0;
    u64 total_n = 0;
    for (u32 i = 0; i < nb; ++i) {
        max_n = std::max(max_n, descs[i].n);
        total_n += descs[i].n;
    }
    MtfArgs ma = make_mtf_args(g, nb);
    ma.tiles = std::min<u32>(kTilesPerBlock, std::max<u32>(1u, (max_n + kSortTile - 1u) / kSortTile));
    int sp = have_events ? span_begin(g, 1) : -1;
    u64 sorted = 0;
    const int rounds = have_events ? sort_batch(g, make_bwt_args(g, nb), max_n, total_n, &sorted, &g->prof, g->round_active) : -1;
    int rc = rounds < 0 ? BZ_E_UNEXPECTED : BZ_OK;
    if (rc == BZ_OK) {
        // (tests) BZ_TEST_CORRUPT=1: a wrong origPtr for the batch's first block while the engine is on its fused passes --
        // a stream that is well formed and decodes to other bytes; nothing but a check of the result can notice
        static const bool corrupt_test = getenv("BZ_TEST_CORRUPT") && atoi(getenv("BZ_TEST_CORRUPT")) != 0;
        if (corrupt_test && g->fused_state[0] == 0 && descs[0].n > 1)
            hipLaunchKernelGGL(k_test_bump, dim3(1), dim3(1), 0, g->st, g->orig_ptr.as<u32>(), descs[0].n);
        // (tests) BZ_TEST_LATE_CLEAR=1: the OUTCOME of round 3's fault -- a sorted order that is not the block's -- as two
        // unequal neighbours of the last column swapped.  (The fault itself, stale look-back words under the first
        // pass's epoch tag, was tried as an injection and is not replayed: tiles scattered to wrong offsets break the
        // digit-count invariants the later passes index with, and the run ends in a GPU memory fault rather than in a
        // wrong stream -- on the test box in two attempts of two.)
        static const bool late_clear_test = getenv("BZ_TEST_LATE_CLEAR") && atoi(getenv("BZ_TEST_LATE_CLEAR")) != 0;
        if (late_clear_test && g->fused_state[0] == 0 && descs[0].n > 1)
            hipLaunchKernelGGL(k_test_swap, dim3(1), dim3(1), 0, g->st, g->L.as<u8>(), descs[0].n);
        span_end(g, sp);
        g->bwt_stats[0] = std::max<u64>(g->bwt_stats[0], (u64)rounds);
        g->bwt_stats[1] += sorted;
        g->bwt_stats[2] += 1;
        (void)hipEventRecord(ev_fork, g->st);
        (void)hipStreamWaitEvent(g->st2, ev_fork, 0);
        sp = span_begin(g, 2, g->st2);
        launch_mtf(g->st2, ma, &g->prof, total_n);
        span_end(g, sp);
        sp = span_begin(g, 3, g->st2);
        launch_huffman(g->st2, make_huff_args(g, nb));
        span_end(g, sp);
        (void)hipEventRecord(ev_join, g->st2); // the main stream continues only after the tail stages are done
        (void)hipStreamWaitEvent(g->st, ev_join, 0);
    }
    if (rc == BZ_OK && ma.fused_zle) {
        // Did the one-launch ZLE stage hand out every tile on every XCD, and did no look-back give up?  (Its tickets come
        // with the wait for the batch.)  If not (it never has), the MTF / ZLE and Huffman stages run again with the three
        // ZLE kernels, and the engine stays on them.
        u32 tk[9] = {};
        const MailSeg sg = {tk, g->ztick.p, sizeof(tk)};
        if (mail_fetch(g->st, &sg, 1) != 0) {
            rc = BZ_E_UNEXPECTED; // (no tickets to look at)
        } else {
            static const bool fail_test = getenv("BZ_FUSED_ZLE_FAILTEST") != nullptr; // (tests: exercise the redo)
            bool bad = tk[8] != 0 || fail_test;
            for (u32 x = 0; x < 8; ++x) // (exactly its share of the launch's workgroups: fewer = tiles left out, more = tiles run twice)
                if (tk[x] != ma.tiles * (xcd_grid_y(nb) / 8u)) bad = true;
            if (bad) {
                fprintf(stderr, "bz2_mi355x: the one-launch ZLE stage misbehaved (tile tickets / look-back); stage redone with three kernels\n");
                g->zle_fused_broken = true;
                launch_mtf(g->st, make_mtf_args(g, nb));
                launch_huffman(g->st, make_huff_args(g, nb));
            }
        }
    }
    // the one way out: nothing of this batch is queued or running on either stream behind this point
    const bool idle = hipStreamSynchronize(g->st2) == hipSuccess;
    if ((hipStreamSynchronize(g->st) != hipSuccess || !idle) && rc == BZ_OK) rc = BZ_E_UNEXPECTED;
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    return rc;
}

extern "C" size_t bz_gpu_block_count(const bz_gpu_engine *g) { return g ? g->h_blocks.size() : 0; }

static int encode_blocks_once(bz_gpu_engine *g, const std::vector<size_t> &mine, void *d_packed, size_t cap_words,
                              uint64_t *h_word_off, uint64_t *h_bit_len, uint32_t *h_crc, size_t *words_used)
{
    if (words_used) *words_used = 0;
    g->h_out.clear();
    g->h_out_nblock.clear();
    g->h_out_pass.clear();
    int rc = ensure_workspace(g, mine.size());
    if (rc != BZ_OK) return rc;
    HIPCHK(hipMemsetAsync(g->error_flag.p, 0, 4, g->st));

    u64 word_cursor = 0;
    std::vector<BlockDesc> descs;
    std::vector<u32> crcs;
    std::vector<BlockOut> outs;
    std::vector<PackBlock> pbs;
    for (size_t k0 = 0; k0 < mine.size(); k0 += g->ws_blocks) {
        const u32 nb = (u32)std::min(g->ws_blocks, mine.size() - k0);
        descs.resize(nb);
        crcs.resize(nb);
        for (u32 i = 0; i < nb; ++i) {
            descs[i] = g->h_blocks[mine[k0 + i]];
            crcs[i] = g->h_crc[mine[k0 + i]];
            if (descs[i].n > kMaxBlockLen) return BZ_E_UNEXPECTED;
        }
        if (mail_poke(g->st, g->lblocks.p, descs.data(), nb * sizeof(BlockDesc)) || mail_poke(g->st, g->lcrc.p, crcs.data(), nb * 4)) return BZ_E_UNEXPECTED;
        const bool last_batch = k0 + nb == mine.size();
        if (!last_batch) HIPCHK(hipStreamSynchronize(g->st)); // descs/crcs are reused by the next batch (the last one's live until the call's final wait)
        rc = encode_batch(g, nb, descs);
        if (rc != BZ_OK) return rc;
        outs.resize(nb);
        u32 err = 0;
        const size_t pass0 = g->h_out_pass.size();
        g->h_out_pass.resize(pass0 + (size_t)nb * 32);
        if (g->debug_figures) HIPCHK(hipMemcpyAsync(g->h_out_pass.data() + pass0, g->hpass.p, (size_t)nb * 32 * 4, hipMemcpyDeviceToHost, g->st));
        MAILCHK(g->st, {outs.data(), g->bout.p, nb * sizeof(BlockOut)}, {&err, g->error_flag.p, 4});
        HIPCHK(hipGetLastError());
        if (err) return BZ_E_UNEXPECTED;
        pbs.resize(nb);
        for (u32 i = 0; i < nb; ++i) {
            const u64 nwords = (outs[i].total_bits + 31) / 32;
            pbs[i].src_word = (u64)i * kStreamWords;
            pbs[i].dst_word = word_cursor;
            pbs[i].nwords = nwords;
            h_word_off[k0 + i] = word_cursor;
            h_bit_len[k0 + i] = outs[i].total_bits;
            h_crc[k0 + i] = crcs[i];
            word_cursor += nwords;
            g->h_out.push_back(outs[i]);
            g->h_out_nblock.push_back(descs[i].n);
        }
        if (word_cursor > cap_words) return BZ_E_CAPACITY;
        const int sp = span_begin(g, 4);
        if (mail_poke(g->st, g->packlist.p, pbs.data(), nb * sizeof(PackBlock))) return BZ_E_UNEXPECTED;
        launch_pack(g->st, g->stream.as<u32>(), g->packlist.as<PackBlock>(), nb, (u32 *)d_packed);
        span_end(g, sp);
        if (!last_batch) HIPCHK(hipStreamSynchronize(g->st)); // pbs reused
    }
    spans_collect(g);
    HIPCHK(hipGetLastError());
    if (words_used) *words_used = (size_t)word_cursor;
    return BZ_OK;
}

// ---- self-check: decode what was just encoded, on the same device, and compare it with the input ------------------
// The reference encoder cannot write a stream that does not decode to its input; a GPU pipeline with look-back words,
// tickets and stream-ordered clears can (round 3 saw one wrong stream in six from a clear on the wrong stream).  With
// verify on, the bit strings of a call's blocks are framed as a stream of their own (header, blocks, trailer), decoded
// by the decode path of this library (k_dec*.hip: header parse, Huffman, inverse MTF, inverse BWT, RLE1 undo, block
// CRCs) and the bytes are compared with the input bytes the blocks cover.  A call whose check fails is encoded again
// with the three-kernel radix passes and the three-kernel ZLE stage (no look-back anywhere) and checked again; if that
// fails too the call returns BZ_E_UNEXPECTED: no byte of a stream that does not decode leaves the library.
struct VerifySeg {
    u64 in_off, out_off, len;
};
__global__ __launch_bounds__(256) void k_verify_compare(const u8 *__restrict__ in, const u8 *__restrict__ out,
                                                        const VerifySeg *__restrict__ segs, u32 *__restrict__ mismatches)
{
    const VerifySeg sg = segs[blockIdx.y];
    bool bad = false;
    for (u64 i = ((u64)blockIdx.x * 256u + threadIdx.x) * 16u; i < sg.len; i += (u64)gridDim.x * 256u * 16u) {
        const u64 k = sg.len - i < 16u ? sg.len - i : 16u;
        if (k == 16u) {
            uint4 a, b;
            __builtin_memcpy(&a, in + sg.in_off + i, 16);
            __builtin_memcpy(&b, out + sg.out_off + i, 16);
            bad = bad || a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
        } else {
            for (u64 j = 0; j < k; ++j) bad = bad || in[sg.in_off + i + j] != out[sg.out_off + i + j];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0u) atomicAdd(mismatches, 1u);
}

// 0: the blocks decode to their input; 1: they do not; < 0: the check itself could not run (status)
static int verify_blocks(bz_gpu_engine *g, const std::vector<size_t> &mine, const void *d_packed, const uint64_t *h_word_off,
                         const uint64_t *h_bit_len, const uint32_t *h_crc)
{
    const size_t nb = mine.size();
    u64 bits = 32 + 80 + 64, in_bytes = 0;
    std::vector<VerifySeg> segs(nb);
    for (size_t k = 0; k < nb; ++k) {
        const BlockDesc &d = g->h_blocks[mine[k]];
        bits += h_bit_len[k];
        segs[k].in_off = d.in_off;
        segs[k].out_off = in_bytes;
        segs[k].len = d.in_end - d.in_off;
        in_bytes += segs[k].len;
    }
    int rc;
    const size_t zcap = (size_t)(bits / 8 + 64) & ~(size_t)3;
    if ((rc = g->vstream.ensure(zcap + 64)) || (rc = g->vout.ensure((size_t)in_bytes + 64)) ||
        (rc = g->vseg.ensure(nb * sizeof(VerifySeg))) || (rc = g->vmis.ensure(4)))
        return rc;
    size_t zlen = 0;
    const double t4 = g->t_stage[4], t5 = g->t_stage[5]; // (the check's framing is not part of the call's stage times)
    rc = bz_gpu_assemble(g, g->level, nb, d_packed, h_word_off, h_bit_len, h_crc, 1, 1, 1, 0, 0, 0, nullptr, g->vstream.p,
                         zcap, &zlen, nullptr, nullptr);
    g->t_stage[4] = t4;
    g->t_stage[5] = t5;
    if (rc != BZ_OK) return rc;
    HIPCHK(hipMemsetAsync((u8 *)g->vstream.p + zlen, 0, 64, g->st)); // (the decoder's bit reader looks a few bytes ahead)
    HIPCHK(hipStreamSynchronize(g->st));
    uint64_t produced = 0;
    int verdict = BZ_OK;
    const bool prof_on = g->prof.on;
    g->prof.on = false; // (the decode kernels of the check do not belong in the encode profile)
    rc = dec_decode_for_verify(g, g->vstream.as<u8>(), zlen, g->vout.as<u8>(), in_bytes, &produced, &verdict);
    g->prof.on = prof_on;
    if (rc == BZ_E_CAPACITY) return 1; // (decodes to MORE than the input)
    if (rc != BZ_OK) return rc;
    if (verdict != BZ_OK || produced != in_bytes) return 1;
    u32 max_len = 1;
    for (const VerifySeg &sg : segs) max_len = std::max<u32>(max_len, (u32)std::min<u64>(sg.len, 0xFFFFFFFFu));
    HIPCHK(hipMemcpyAsync(g->vseg.p, segs.data(), nb * sizeof(VerifySeg), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemsetAsync(g->vmis.p, 0, 4, g->st));
    const u32 gx = std::min<u32>((max_len + 4095u) / 4096u, 4096u);
    for (size_t k0 = 0; k0 < nb; k0 += 65535) { // (grid.y is a 16-bit number)
        const u32 ny = (u32)std::min<size_t>(nb - k0, 65535);
        hipLaunchKernelGGL(k_verify_compare, dim3(gx, ny), dim3(256), 0, g->st, g->d_in, g->vout.as<u8>(),
                           g->vseg.as<VerifySeg>() + k0, g->vmis.as<u32>());
    }
    u32 mis = 0;
    HIPCHK(hipMemcpyAsync(&mis, g->vmis.p, 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    return mis ? 1 : 0;
}

extern "C" int bz_gpu_encode_blocks(bz_gpu_engine *g, size_t first, size_t stride, void *d_packed,
                                    size_t cap_words, uint64_t *h_word_off, uint64_t *h_bit_len,
                                    uint32_t *h_crc, size_t *words_used)
{
    if (!g || stride == 0) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    if (words_used) *words_used = 0;
    const size_t total = g->h_blocks.size();
    std::vector<size_t> mine;
    for (size_t b = first; b < total; b += stride) mine.push_back(b);
    if (mine.empty()) {
        g->h_out.clear();
        g->h_out_nblock.clear();
        g->h_out_pass.clear();
        return BZ_OK;
    }
    int rc = encode_blocks_once(g, mine, d_packed, cap_words, h_word_off, h_bit_len, h_crc, words_used);
    if (rc != BZ_OK || !g->verify) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    int v = verify_blocks(g, mine, d_packed, h_word_off, h_bit_len, h_crc);
    g->verify_stats[0] += mine.size();
    if (v == 1) {
        g->verify_stats[1] += 1;
        fprintf(stderr, "bz2_mi355x: self-check: %zu blocks did not decode to their input; encoded again without look-back passes\n",
                mine.size());
        g->fused_state[0] = 1;      // the three-kernel radix passes ...
        g->fused_state[1] += 1;
        g->zle_fused_broken = true; // ... and the three-kernel ZLE stage, for the rest of this engine's life
        rc = encode_blocks_once(g, mine, d_packed, cap_words, h_word_off, h_bit_len, h_crc, words_used);
        if (rc == BZ_OK) v = verify_blocks(g, mine, d_packed, h_word_off, h_bit_len, h_crc);
        if (rc == BZ_OK && v == 1) {
            g->verify_stats[2] += 1;
            fprintf(stderr, "bz2_mi355x: self-check failed again: the call returns an error, no stream is produced\n");
            rc = BZ_E_UNEXPECTED;
        }
    }
    if (rc == BZ_OK && v < 0) rc = v;
    g->verify_stats[3] += (u64)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

extern "C" int bz_gpu_engine_set_verify(bz_gpu_engine *g, int on)
{
    if (!g) return BZ_E_PARAM;
    g->verify = on != 0;
    return BZ_OK;
}

extern "C" int bz_gpu_verify_stats(bz_gpu_engine *g, uint64_t out[4])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out[i] = g->verify_stats[i];
    return BZ_OK;
}

extern "C" int bz_gpu_assemble(bz_gpu_engine *g, int level, size_t n_blocks, const void *d_packed,
                               const uint64_t *h_word_off, const uint64_t *h_bit_len, const uint32_t *h_crc,
                               int write_header, int write_trailer, int pad_to_byte, unsigned carry_bits,
                               unsigned carry_byte, uint32_t combined_crc_in, uint32_t *combined_crc_out,
                               void *d_out, size_t cap, size_t *out_len, unsigned *out_carry_bits,
                               unsigned *out_carry_byte)
{
    if (!g || level < 1 || level > 9 || carry_bits > 7) return BZ_E_PARAM;
    if ((uintptr_t)d_out & 3u) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    std::vector<AsmBlock> ab(n_blocks);
    u64 pos = carry_bits + (write_header ? 32u : 0u);
    u32 comb = combined_crc_in;
    u64 max_words = 0;
    for (size_t k = 0; k < n_blocks; ++k) {
        ab[k].src_word = h_word_off[k];
        ab[k].bit_len = h_bit_len[k];
        ab[k].dst_bit = pos;
        pos += h_bit_len[k];
        comb = ((comb << 1) | (comb >> 31)) ^ h_crc[k]; // encoder.rs:237-238
        max_words = std::max<u64>(max_words, (h_bit_len[k] + 31) / 32 + 1);
    }
    const u64 trailer_bit = pos;
    if (write_trailer) pos += 80;
    const u64 total_bits = pos;
    const u64 nwords = (total_bits + 31) / 32;
    if (nwords * 4 > cap) return BZ_E_CAPACITY;
    const int sp = span_begin(g, 4);
    if (nwords) HIPCHK(hipMemsetAsync(d_out, 0, nwords * 4, g->st));
    if (n_blocks) {
        int rc = g->asmlist.ensure(n_blocks * sizeof(AsmBlock));
        if (rc != BZ_OK) return rc;
        if (mail_poke(g->st, g->asmlist.p, ab.data(), n_blocks * sizeof(AsmBlock))) return BZ_E_UNEXPECTED;
        launch_assemble(g->st, (const u32 *)d_packed, g->asmlist.as<AsmBlock>(), (u32)n_blocks, max_words,
                        (u32 *)d_out);
    }
    if (nwords)
        launch_frame(g->st, (u32 *)d_out, write_header, (u32)level, carry_bits, carry_byte, write_trailer,
                     trailer_bit, comb);
    span_end(g, sp);
    size_t bytes;
    unsigned ocb = 0, ocy = 0;
    if (pad_to_byte) {
        bytes = (size_t)((total_bits + 7) / 8);
    } else {
        bytes = (size_t)(total_bits / 8);
        ocb = (unsigned)(total_bits & 7u);
        if (ocb) {
            u8 last = 0;
            MAILCHK(g->st, {&last, (const u8 *)d_out + bytes, 1});
            ocy = last & (0xFFu << (8 - ocb));
        }
    }
    spans_collect(g);
    HIPCHK(hipGetLastError());
    if (combined_crc_out) *combined_crc_out = comb;
    if (out_len) *out_len = bytes;
    if (out_carry_bits) *out_carry_bits = ocb;
    if (out_carry_byte) *out_carry_byte = ocy;
    return BZ_OK;
}

extern "C" int bz_gpu_encode_device(bz_gpu_engine *g, int level, const void *d_in, size_t n, void *d_out,
                                    size_t cap, size_t *out_len)
{
    if (!g) return BZ_E_PARAM;
    size_t nblocks = 0, consumed = 0;
    int rc = bz_gpu_partition(g, level, d_in, n, BZ_ACTION_FINISH, &nblocks, &consumed, nullptr);
    if (rc != BZ_OK) return rc;
    std::vector<uint64_t> woff(nblocks + 1), blen(nblocks + 1);
    std::vector<uint32_t> crc(nblocks + 1);
    size_t used = 0;
    if (nblocks) {
        const size_t cap_words = bz_encode_bound(n) / 4 + 2 * nblocks + 16;
        rc = g->packed.ensure(cap_words * 4);
        if (rc != BZ_OK) return rc;
        rc = bz_gpu_encode_blocks(g, 0, 1, g->packed.p, cap_words, woff.data(), blen.data(), crc.data(), &used);
        if (rc != BZ_OK) return rc;
    }
    return bz_gpu_assemble(g, level, nblocks, g->packed.p, woff.data(), blen.data(), crc.data(), 1, 1, 1, 0, 0, 0,
                           nullptr, d_out, cap, out_len, nullptr, nullptr);
}

// ---- many inputs, one stream each -------------------------------------------------------------------------------------
// The pipeline behind the split takes `nb` independent blocks per launch and does not ask where they come from: the
// one-block inputs of a batch are split by ONE launch (k_rle_batch, a workgroup per input), become the blocks of ONE
// bz_gpu_encode_blocks call (sub-batches of ws_blocks, the fused-pass fallbacks, the block statistics and the self-check
// as for any other call) and are framed by one k_assemble and one k_frame_batch launch over all their streams.
//
// One block for certain: RLE1 turns n bytes into at most 5 * (n / 4) + n % 4 (runs of exactly four), and the cut of
// encoder.rs:692 fires only behind a run that is not the last one, so an image of at most 100000 * level - 19 bytes is
// never cut.  Image slots: the exclusive sum of those bounds, each rounded up to 16, and 256 bytes of slack behind the
// last (the single-input path sizes its image the same way).
//
// Inputs that may take several blocks go through bz_gpu_encode_device one at a time.  That path overwrites the image,
// g->h_blocks and g->packed, and the place of a stream in d_out depends on the lengths of ALL streams in front of it.
// Order chosen: the whole small batch FIRST, up to its bit strings -- they go to a buffer of their own (batch_packed),
// and their lengths are on the host -- then the inputs in order: a large one is encoded straight into its final slot
// of d_out (every length in front of it is known by then), a small one only gets its place.  The small streams are
// written last.  The other order would have to park every large stream somewhere and copy it once the small lengths
// are known.  (After a batch with large inputs bz_gpu_debug_block_stats describes the last of them, as after any
// bz_gpu_encode_device call; after a batch of one-block inputs, all its blocks in input order.)
static bool batch_one_block(u64 n, int level) { return 5u * (n / 4u) + n % 4u <= 100000ull * (u64)level - 19u; }

extern "C" size_t bz_encode_batch_bound(const uint64_t *in_len, size_t count)
{
    size_t s = 0;
    for (size_t i = 0; in_len && i < count; ++i) s += (bz_encode_bound((size_t)in_len[i]) + 3u) & ~(size_t)3;
    return s;
}

extern "C" int bz_gpu_last_batch_stats(bz_gpu_engine *g, uint64_t out[4])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out[i] = g->batch_stats[i];
    return BZ_OK;
}

extern "C" int bz_gpu_encode_batch_device(bz_gpu_engine *g, int level, const void *d_in, const uint64_t *h_in_off,
                                          const uint64_t *h_in_len, size_t count, void *d_out, size_t cap,
                                          uint64_t *h_out_off, uint64_t *h_out_len)
{
    if (!g || level < 1 || level > 9) return BZ_E_PARAM;
    if (count == 0) return BZ_OK;
    if (!h_in_off || !h_in_len || !h_out_off || !h_out_len || !d_out) return BZ_E_PARAM;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 3u)) return BZ_E_PARAM;
    u64 in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 15u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i]) return BZ_E_PARAM;
        in_end = h_in_off[i] + h_in_len[i];
    }
    if (in_end && !d_in) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    for (u64 &s : g->batch_stats) s = 0;

    // ---- the one-block inputs: split, encode -------------------------------------------------------------
    std::vector<RleBatchItem> items;
    std::vector<size_t> small; // their input numbers
    u64 image = 0, packed_words = 16;
    for (size_t i = 0; i < count; ++i) {
        if (!batch_one_block(h_in_len[i], level)) continue;
        const u64 n = h_in_len[i];
        items.push_back({h_in_off[i], n, image});
        small.push_back(i);
        image += (5u * (n / 4u) + n % 4u + 15u) & ~(u64)15;
        if (n) packed_words += bz_encode_bound((size_t)n) / 4 + 2;
    }
    const size_t ns = small.size();
    g->batch_stats[0] = ns;
    g->batch_stats[1] = count - ns;
    // as bz_gpu_partition_slab_begin leaves the engine, with the batch as "the input" (the self-check compares the
    // decoded blocks with g->d_in + in_off)
    g->level = level;
    g->d_in = (const u8 *)d_in;
    g->n_in = in_end;
    g->onepass_done = false; // (the image buffer no longer holds what the last partition wrote)
    g->h_blocks.clear();
    g->h_crc.clear();
    g->h_out.clear();
    g->h_out_nblock.clear();
    g->h_out_pass.clear();
    for (double &t : g->t_stage) t = 0;
    for (u64 &s : g->bwt_stats) s = 0;
    for (u64 &s : g->round_active) s = 0;
    std::vector<long long> block_of(count, -1); // input -> its block among the batch's blocks
    std::vector<BlockDesc> bd(ns);
    std::vector<u32> bc(ns);
    int rc;
    if (ns) {
        if ((rc = g->rle.ensure(image + 256)) || (rc = g->batch_items.ensure(ns * sizeof(RleBatchItem))) ||
            (rc = g->blocks_all.ensure(ns * sizeof(BlockDesc))) || (rc = g->crc_all.ensure(ns * 4)))
            return rc;
        HIPCHK(hipMemcpyAsync(g->batch_items.p, items.data(), ns * sizeof(RleBatchItem), hipMemcpyHostToDevice, g->st));
        const int sp = span_begin(g, 0);
        launch_rle_batch(g->st, g->d_in, g->batch_items.as<RleBatchItem>(), (u32)ns, g->crc_tab.as<u32>(), g->xp2.as<u32>(),
                         g->rle.as<u8>(), g->blocks_all.as<BlockDesc>(), g->crc_all.as<u32>());
        span_end(g, sp);
        MAILCHK(g->st, {bd.data(), g->blocks_all.p, ns * sizeof(BlockDesc)}, {bc.data(), g->crc_all.p, ns * 4});
        HIPCHK(hipGetLastError());
        for (size_t j = 0; j < ns; ++j) {
            if (bd[j].n == 0) continue; // an empty input: no block, a stream of header and trailer
            block_of[small[j]] = (long long)g->h_blocks.size();
            g->h_blocks.push_back(bd[j]);
            g->h_crc.push_back(bc[j]);
        }
    }
    const size_t nb = g->h_blocks.size();
    std::vector<uint64_t> woff(nb + 1), blen(nb + 1);
    std::vector<uint32_t> crc(nb + 1);
    if (nb) {
        size_t used = 0;
        if ((rc = g->batch_packed.ensure(packed_words * 4)) != BZ_OK) return rc;
        rc = bz_gpu_encode_blocks(g, 0, 1, g->batch_packed.p, packed_words, woff.data(), blen.data(), crc.data(), &used);
        if (rc != BZ_OK) return rc;
        g->batch_stats[2] = nb;
        g->batch_stats[3] = (nb + g->ws_blocks - 1) / g->ws_blocks;
    } else {
        spans_collect(g);
    }

    // ---- the streams' places, the large inputs on the way ---------------------------------------------------------
    std::vector<AsmBlock> ab;
    std::vector<FrameItem> fr;
    std::vector<std::pair<u64, u64>> zero; // byte ranges of d_out that hold small streams (runs of neighbours as one)
    ab.reserve(nb);
    fr.reserve(ns);
    u64 cursor = 0, max_words = 0;
    for (size_t i = 0; i < count; ++i) {
        h_out_off[i] = cursor;
        if (batch_one_block(h_in_len[i], level)) {
            const long long k = block_of[i];
            const u64 bits = 32u + (k >= 0 ? blen[(size_t)k] : 0u) + 80u, len = (bits + 7u) / 8u, slot = (len + 3u) & ~(u64)3;
            if (cursor + slot > cap) return BZ_E_CAPACITY;
            if (k >= 0) {
                ab.push_back({woff[(size_t)k], blen[(size_t)k], cursor * 8u + 32u});
                max_words = std::max<u64>(max_words, (blen[(size_t)k] + 31) / 32 + 1);
            }
            // the combined CRC of one block: rotl(0, 1) ^ crc (encoder.rs:237-238); of none: 0
            fr.push_back({cursor / 4u, cursor * 8u + bits - 80u, k >= 0 ? crc[(size_t)k] : 0u, 0u});
            if (!zero.empty() && zero.back().second == cursor) zero.back().second = cursor + slot;
            else zero.push_back({cursor, cursor + slot});
            h_out_len[i] = len;
            cursor += slot;
        } else {
            size_t len = 0;
            if (cursor >= cap) return BZ_E_CAPACITY;
            rc = bz_gpu_encode_device(g, level, (const u8 *)d_in + h_in_off[i], (size_t)h_in_len[i], (u8 *)d_out + cursor,
                                      (size_t)(cap - cursor), &len);
            if (rc != BZ_OK) return rc;
            h_out_len[i] = len;
            cursor += ((u64)len + 3u) & ~(u64)3; // (bz_gpu_assemble has cleared the slot to its last word)
        }
    }

    // ---- the small streams: zeros, blocks, frames ------------------------------------------------------------------
    if (!fr.empty()) {
        if ((rc = g->batch_frames.ensure(fr.size() * sizeof(FrameItem))) || (rc = g->asmlist.ensure((ab.size() + 1) * sizeof(AsmBlock))))
            return rc;
        const int sp = span_begin(g, 4);
        for (const auto &z : zero) HIPCHK(hipMemsetAsync((u8 *)d_out + z.first, 0, z.second - z.first, g->st)); // (one range unless large inputs lie between)
        if (!ab.empty()) {
            HIPCHK(hipMemcpyAsync(g->asmlist.p, ab.data(), ab.size() * sizeof(AsmBlock), hipMemcpyHostToDevice, g->st));
            for (size_t k0 = 0; k0 < ab.size(); k0 += 65535) // (grid.y is a 16-bit number)
                launch_assemble(g->st, g->batch_packed.as<u32>(), g->asmlist.as<AsmBlock>() + k0,
                                (u32)std::min<size_t>(ab.size() - k0, 65535), max_words, (u32 *)d_out);
        }
        HIPCHK(hipMemcpyAsync(g->batch_frames.p, fr.data(), fr.size() * sizeof(FrameItem), hipMemcpyHostToDevice, g->st));
        launch_frame_batch(g->st, (u32 *)d_out, g->batch_frames.as<FrameItem>(), (u32)fr.size(), (u32)level);
        span_end(g, sp);
    }
    spans_collect(g); // (waits for both streams: the host arrays above are free, the streams are in d_out)
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

// ---- the whole stream over several GPUs: one process (one engine) per GPU --------------------------
// Rank r splits its SLAB of the input (an equal share of the 4 KiB tiles), encodes the blocks that
// end in it and hands their bit strings to rank 0, which assembles the serial stream.  What crosses
// ranks (all through the caller's bz_shard_comm; RCCL, MPI or torch.distributed sit behind it):
//   1. all-gather of 8 bytes per rank: the last run start inside each slab (the RLE1 phase at
//      every slab's left edge);
//   2. the cut chain: rank r-1 tells rank r where r's first block starts (16 bytes per hop: the
//      position and the sender's status, so that an error runs down the chain instead of leaving
//      the later ranks waiting);
//   3. all-gather of 24 bytes per rank (block count, words, status), then of 24 bytes per block
//      (word offset, bit length, CRC), padded to the largest count;
//   4. ONE variable-length gather of the packed bit strings (device memory) to rank 0.
// Every rank takes part in every exchange whatever happened to it locally: a rank-local error is
// carried in the status words and returned by ALL ranks after the exchange that reveals it.
struct ShardHead {
    u64 blocks, words;
    i64 status;
};
struct ShardBlock {
    u64 word_off, bit_len;
    u32 crc, pad;
};

// Which tiles a rank owns.  The cut chain makes rank r start its blocks r links later than rank 0 (a link: ~2 ms per GiB
// of slab against ~85 ms for the slab's blocks), and the step ends with the LAST rank: slabs that shrink a little from
// rank to rank -- weights 1 + skew ((world - 1) / 2 - r), which sum to world -- let all ranks finish together instead
// (at N = 8 and skew = link / slab time = 0.02: the last rank's 14 ms of waiting become 7 ms for everybody).  The bytes
// of the stream do not depend on the split.  BZ_SHARD_SKEW in the environment (0 = equal slabs; default 0.004 -- with the
// cut tables a link is 0.1-0.3 ms, not the 2 ms of the chain kernel the 0.02 above was worked out for; every rank of a job
// must see the same value).
static double shard_skew()
{
    static const double v = [] {
        const char *e = getenv("BZ_SHARD_SKEW");
        double s = e ? atof(e) : 0.004; // (a link is 0.1-0.3 ms of look-ups + the transport's hop against ~85 ms per GiB slab)
        if (!(s >= 0.0)) s = 0.0;
        if (s > 0.2) s = 0.2;
        return s;
    }();
    return v;
}
static u64 shard_tile_begin(u64 ntiles, int rank, int world)
{
    if (rank <= 0) return 0;
    if (rank >= world) return ntiles;
    const double r = rank, w = world, s = shard_skew();
    const double share = (r + s * (r * (w - 1.0) / 2.0 - r * (r - 1.0) / 2.0)) / w; // sum of the weights of ranks < r, over world
    u64 t = (u64)((double)ntiles * share + 0.5);
    return t > ntiles ? ntiles : t;
}
extern "C" int bz_shard_slab_tiles(size_t n, int rank, int world, uint64_t *tile0, uint64_t *tile1)
{
    if (world < 1 || rank < 0 || rank >= world || !tile0 || !tile1) return BZ_E_PARAM;
    const u64 ntiles = ((u64)n + kRleTile - 1) / kRleTile;
    *tile0 = shard_tile_begin(ntiles, rank, world);
    *tile1 = shard_tile_begin(ntiles, rank + 1, world);
    if (*tile1 < *tile0) *tile1 = *tile0;
    return BZ_OK;
}

// A level-`level` block covers at most (100000 level - 19) * 255 / 5 input bytes (a run of 255 equal bytes is five
// RLE1 bytes, encoder.rs:676-690): what a rank may have to re-read in front of its slab, rounded up to whole tiles.
extern "C" size_t bz_shard_halo_bytes(int level)
{
    if (level < 1 || level > 9) return 0;
    const u64 most = ((u64)level * 100000u - 19u) * 51u;
    return (size_t)((most + 2 * kRleTile - 1) / kRleTile * kRleTile);
}

extern "C" int bz_shard_window(int level, size_t n, int rank, int world, uint64_t *window_off, size_t *window_bytes)
{
    if (level < 1 || level > 9 || world < 1 || rank < 0 || rank >= world || !window_off || !window_bytes) return BZ_E_PARAM;
    const u64 ntiles = ((u64)n + kRleTile - 1) / kRleTile;
    const u64 t0 = shard_tile_begin(ntiles, rank, world), t1 = std::max(t0, shard_tile_begin(ntiles, rank + 1, world));
    const u64 begin = t0 * kRleTile, end = std::min<u64>((u64)n, t1 * kRleTile);
    const u64 halo = bz_shard_halo_bytes(level);
    const u64 lo = begin > halo ? begin - halo : 0;
    const u64 hi = std::min<u64>((u64)n, end + kRleTile); // (the split looks one byte past a slab's end)
    *window_off = lo;
    *window_bytes = (size_t)(hi > lo ? hi - lo : 0);
    return BZ_OK;
}

// win_lo / win_hi: the input bytes that really lie behind d_in (the whole input: 0, n).
static int encode_sharded_impl2(bz_gpu_engine *g, int level, const void *d_in, size_t n, u64 win_lo, u64 win_hi,
                               const bz_shard_comm *comm, void *d_packed, size_t packed_cap_words,
                               void *d_gather, size_t gather_cap_words, void *d_out, size_t cap,
                               size_t *out_len)
{
    if (!g || !comm || comm->world < 1 || comm->rank < 0 || comm->rank >= comm->world) return BZ_E_PARAM;
    if (level < 1 || level > 9) return BZ_E_PARAM;
    if (out_len) *out_len = 0;
    const int rank = comm->rank, world = comm->world;
    if (world > 1 && (!comm->allgather || !comm->send || !comm->recv || !comm->gatherv)) return BZ_E_PARAM;
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
    const clk::time_point t_entry = clk::now();
    for (double &t : g->shard_ms) t = 0;
    const u64 ntiles = (n + kRleTile - 1) / kRleTile;
    const u64 t0 = shard_tile_begin(ntiles, rank, world), t1 = std::max(t0, shard_tile_begin(ntiles, rank + 1, world));
    int rc = BZ_OK; // this rank's status; collectives go on regardless
    {
        // the window must hold the slab, a tile in front of it (the split looks at the byte before a slab) and the
        // tile behind it (a chunk that begins in the slab ends there); how far the first block reaches back is only
        // known when the cut arrives (checked there)
        const u64 begin = t0 * kRleTile, end = std::min<u64>((u64)n, t1 * kRleTile);
        const u64 need_lo = begin >= kRleTile ? begin - kRleTile : 0, need_hi = std::min<u64>((u64)n, end + kRleTile);
        if (t1 > t0 && (win_lo > need_lo || win_hi < need_hi)) rc = BZ_E_PARAM;
    }

    // 1. slab scan + the RLE1 phase at the left edge
    int64_t last = -1;
    if (rc == BZ_OK) rc = bz_gpu_partition_slab_begin(g, level, d_in, n, t0, t1, &last);
    std::vector<int64_t> lasts((size_t)world, -1);
    if (world > 1) {
        if (comm->allgather(comm->ctx, &last, 8, lasts.data()) != 0) return BZ_E_UNEXPECTED; // (the transport itself failed: nothing to wait for)
    } else {
        lasts[0] = last;
    }
    int64_t carry = -1;
    for (int r = 0; r < rank; ++r) carry = std::max(carry, lasts[(size_t)r]);
    if (rc == BZ_OK) rc = bz_gpu_partition_slab_count(g, carry);

    // 2. where the slab's image lies in the image of the whole input; then its own image and the tables of its cuts
    SlabSpec sp;
    std::vector<uint64_t> totals((size_t)world, 0);
    if (world > 1) {
        if (rc == BZ_OK) rc = slab_spec_total(g, sp);
        uint64_t mine_total = rc == BZ_OK ? sp.total : 0;
        if (comm->allgather(comm->ctx, &mine_total, 8, totals.data()) != 0) return BZ_E_UNEXPECTED;
        u64 g_base = 0;
        for (int r = 0; r < rank; ++r) g_base += totals[(size_t)r];
        if (rc == BZ_OK) rc = slab_spec_tables(g, sp, g_base);
    }

    // 3. the cut chain
    g->shard_ms[4] = ms_since(t_entry);
    const clk::time_point t_wait = clk::now();
    // {first input byte of the receiver's first block, sender's status, the block's offset in the image of the whole
    // input, its number}
    uint64_t hop[4] = {0, 0, 0, 0};
    if (rank > 0 && comm->recv(comm->ctx, rank - 1, hop, sizeof(hop)) != 0) return BZ_E_UNEXPECTED;
    g->shard_ms[0] = ms_since(t_wait);
    const clk::time_point t_link = clk::now(); // this rank's link of the serial chain: from the hop's arrival to the hand-on
    if (rc == BZ_OK && hop[1] != 0) rc = -(int)hop[1];
    // (a window: the first block's bytes in front of the slab must lie inside it, from the start of their tile on)
    if (rc == BZ_OK && t1 > t0 && hop[0] / kRleTile * kRleTile < win_lo) {
        fprintf(stderr, "bz2_mi355x: rank %d: its first block starts at input byte %llu, in front of the window it was given (%llu); "
                        "bz_shard_window sizes one that always holds it\n", rank, (unsigned long long)hop[0], (unsigned long long)win_lo);
        rc = BZ_E_CAPACITY;
    }
    size_t nb = 0;
    uint64_t next = hop[0];
    // (the cut goes to the next rank before this rank writes its image: the chain over the ranks is serial, and
    // only the cuts are part of it)
    SlabCuts sc;
    uint64_t s_next = hop[2], j_next = hop[3];
    if (rc == BZ_OK) {
        const clk::time_point t_sel = clk::now();
        if (world == 1) rc = slab_cuts(g, hop[0], 1, true, sc, &nb, &next, nullptr);
        else rc = slab_spec_select(g, sp, hop[0], hop[2], hop[3], rank == world - 1, sc, &nb, &next, &s_next, &j_next);
        g->shard_ms[5] = ms_since(t_sel);
    }
    if (rank < world - 1) {
        uint64_t out_hop[4] = {next, (uint64_t)(rc == BZ_OK ? 0 : -rc), s_next, j_next};
        if (comm->send(comm->ctx, rank + 1, out_hop, sizeof(out_hop)) != 0) return BZ_E_UNEXPECTED;
    }
    g->shard_ms[1] = ms_since(t_link);
    if (rc == BZ_OK) rc = world == 1 ? slab_image(g, sc) : slab_spec_finish(g, sp, sc);
    else if (sc.span >= 0) { span_end(g, sc.span); spans_collect(g); }

    // this rank's blocks (the sort starts as soon as its own cuts are known)
    std::vector<uint64_t> woff(nb + 1), blen(nb + 1);
    std::vector<uint32_t> crc(nb + 1);
    size_t used = 0;
    if (rc == BZ_OK && nb) {
        if (!d_packed) {
            packed_cap_words = bz_encode_bound(n / (size_t)world + ((size_t)48 << 20)) / 4 + 2 * nb + 16;
            rc = g->packed.ensure(packed_cap_words * 4);
            d_packed = g->packed.p;
        }
        if (rc == BZ_OK)
            rc = bz_gpu_encode_blocks(g, 0, 1, d_packed, packed_cap_words, woff.data(), blen.data(), crc.data(), &used);
    }
    if (rc == BZ_OK && world > 1 && g->h_halo_total != sp.want_halo_total) {
        if (hipStreamSynchronize(g->st) != hipSuccess || g->h_halo_total != sp.want_halo_total) {
            fprintf(stderr, "bz2_mi355x: rank %d: the image of its first block's bytes in front of the slab has %llu bytes, the "
                            "offsets of the whole input's image say %llu\n", rank, (unsigned long long)g->h_halo_total,
                    (unsigned long long)sp.want_halo_total);
            rc = BZ_E_UNEXPECTED;
        }
    }
    if (world == 1) {
        if (rc != BZ_OK) return rc;
        return bz_gpu_assemble(g, level, nb, d_packed, woff.data(), blen.data(), crc.data(), 1, 1, 1, 0, 0, 0, nullptr,
                               d_out, cap, out_len, nullptr, nullptr);
    }

    // 3. who has how much, and the first error if there is one
    ShardHead mine = {(u64)nb, (u64)used, (i64)rc};
    std::vector<ShardHead> heads((size_t)world);
    if (comm->allgather(comm->ctx, &mine, sizeof(mine), heads.data()) != 0) return BZ_E_UNEXPECTED;
    u64 kmax = 1, total_words = 0, total_blocks = 0;
    for (int r = 0; r < world; ++r) {
        if (heads[(size_t)r].status != 0) return (int)heads[(size_t)r].status; // the same verdict on every rank
        kmax = std::max(kmax, heads[(size_t)r].blocks);
        total_words += heads[(size_t)r].words;
        total_blocks += heads[(size_t)r].blocks;
    }
    std::vector<ShardBlock> meta((size_t)kmax), metas((size_t)kmax * (size_t)world);
    for (size_t k = 0; k < (size_t)kmax; ++k) {
        meta[k].word_off = k < nb ? woff[k] : 0;
        meta[k].bit_len = k < nb ? blen[k] : 0;
        meta[k].crc = k < nb ? crc[k] : 0;
        meta[k].pad = 0;
    }
    if (comm->allgather(comm->ctx, meta.data(), (size_t)kmax * sizeof(ShardBlock), metas.data()) != 0) return BZ_E_UNEXPECTED;

    // 4. the bit strings -> rank 0 (room is settled first so that a rank that cannot receive says so before the gather)
    // (the packed words must be complete before the transport reads them; a HIP failure here travels with the
    // same status word, so that no rank is left waiting in the gather)
    int grc = BZ_OK;
    if (hipStreamSynchronize(g->st) != hipSuccess) {
        fprintf(stderr, "bz2_mi355x: rank %d: HIP error while finishing its blocks\n", rank);
        grc = BZ_E_UNEXPECTED;
    }
    if (rank == 0 && grc == BZ_OK) {
        if (!d_gather) {
            grc = g->gathered.ensure((size_t)(total_words + 16) * 4);
            d_gather = g->gathered.p;
        } else if (gather_cap_words < total_words) {
            grc = BZ_E_CAPACITY;
        }
    }
    std::vector<int64_t> grcs((size_t)world, 0);
    int64_t g64 = grc;
    if (comm->allgather(comm->ctx, &g64, 8, grcs.data()) != 0) return BZ_E_UNEXPECTED;
    for (int r = 0; r < world; ++r)
        if (grcs[(size_t)r] != 0) return (int)grcs[(size_t)r]; // the same verdict on every rank
    std::vector<uint64_t> roff((size_t)world), rlen((size_t)world);
    u64 cursor = 0;
    for (int r = 0; r < world; ++r) {
        roff[(size_t)r] = cursor * 4;
        rlen[(size_t)r] = heads[(size_t)r].words * 4;
        cursor += heads[(size_t)r].words;
    }
    const clk::time_point t_gather = clk::now();
    if (comm->gatherv(comm->ctx, d_packed, (size_t)used * 4, rank == 0 ? d_gather : nullptr, roff.data(), rlen.data()) != 0)
        return BZ_E_UNEXPECTED;
    g->shard_ms[2] = ms_since(t_gather);
    if (rank != 0) return BZ_OK;
    const clk::time_point t_asm = clk::now();

    std::vector<uint64_t> awoff((size_t)total_blocks + 1), ablen((size_t)total_blocks + 1);
    std::vector<uint32_t> acrc((size_t)total_blocks + 1);
    size_t q = 0;
    for (int r = 0; r < world; ++r)
        for (u64 k = 0; k < heads[(size_t)r].blocks; ++k, ++q) {
            const ShardBlock &m = metas[(size_t)r * (size_t)kmax + (size_t)k];
            awoff[q] = m.word_off + roff[(size_t)r] / 4;
            ablen[q] = m.bit_len;
            acrc[q] = m.crc;
        }
    const int arc = bz_gpu_assemble(g, level, (size_t)total_blocks, d_gather, awoff.data(), ablen.data(), acrc.data(), 1, 1, 1, 0, 0,
                                    0, nullptr, d_out, cap, out_len, nullptr, nullptr);
    g->shard_ms[3] = ms_since(t_asm);
    return arc;
}

static int encode_sharded_impl(bz_gpu_engine *g, int level, const void *d_in, size_t n, u64 win_lo, u64 win_hi,
                               const bz_shard_comm *comm, void *d_packed, size_t packed_cap_words,
                               void *d_gather, size_t gather_cap_words, void *d_out, size_t cap,
                               size_t *out_len)
{
    const std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    const int rc = encode_sharded_impl2(g, level, d_in, n, win_lo, win_hi, comm, d_packed, packed_cap_words, d_gather,
                                        gather_cap_words, d_out, cap, out_len);
    if (g) g->shard_ms[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    return rc;
}

extern "C" int bz_gpu_last_shard_timings(bz_gpu_engine *g, double out_ms[4])
{
    if (!g || !out_ms) return BZ_E_PARAM;
    for (int i = 0; i < 4; ++i) out_ms[i] = g->shard_ms[i];
    return BZ_OK;
}
extern "C" int bz_gpu_last_shard_phases(bz_gpu_engine *g, double out_ms[8])
{
    if (!g || !out_ms) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out_ms[i] = g->shard_ms[i];
    return BZ_OK;
}

extern "C" int bz_gpu_encode_sharded(bz_gpu_engine *g, int level, const void *d_in, size_t n,
                                     const bz_shard_comm *comm, void *d_packed, size_t packed_cap_words,
                                     void *d_gather, size_t gather_cap_words, void *d_out, size_t cap,
                                     size_t *out_len)
{
    return encode_sharded_impl(g, level, d_in, n, 0, n, comm, d_packed, packed_cap_words, d_gather, gather_cap_words, d_out,
                               cap, out_len);
}

// The same call for a rank that holds only a WINDOW of the input: d_window[0 .. window_bytes) are the input bytes
// [window_off, window_off + window_bytes).  The kernels address the input by absolute position, so the window is
// handed on as the base it would have inside the whole input (never dereferenced outside the window).
extern "C" int bz_gpu_encode_sharded_window(bz_gpu_engine *g, int level, const void *d_window, uint64_t window_off,
                                            size_t window_bytes, size_t n, const bz_shard_comm *comm, void *d_packed,
                                            size_t packed_cap_words, void *d_gather, size_t gather_cap_words,
                                            void *d_out, size_t cap, size_t *out_len)
{
    if ((window_off & 15u) || window_off > n || window_bytes > n - window_off) return BZ_E_PARAM;
    const void *base = reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(d_window) - (uintptr_t)window_off);
    return encode_sharded_impl(g, level, base, n, window_off, window_off + window_bytes, comm, d_packed, packed_cap_words,
                               d_gather, gather_cap_words, d_out, cap, out_len);
}

// Exercises a transport (the four callbacks of a bz_shard_comm) with known patterns, shaped like the
// exchanges of bz_gpu_encode_sharded; every rank calls it.  host_memory != 0: the "device" buffers of
// gatherv are plain host memory (a CPU transport under test), else hipMalloc'ed on the current device.
extern "C" int bz_shard_comm_selftest(const bz_shard_comm *comm, int host_memory)
{
    if (!comm || comm->world < 1 || comm->rank < 0 || comm->rank >= comm->world) return BZ_E_PARAM;
    if (!comm->allgather || !comm->send || !comm->recv || !comm->gatherv) return BZ_E_PARAM;
    const int rank = comm->rank, world = comm->world;
    int bad = 0;
    // all-gather of 24 bytes per rank
    uint64_t mine[3] = {0x1111111111111111ull * (uint64_t)(rank + 1), (uint64_t)rank, ~(uint64_t)rank};
    std::vector<uint64_t> all((size_t)world * 3, 0);
    if (comm->allgather(comm->ctx, mine, sizeof(mine), all.data()) != 0) return BZ_E_UNEXPECTED;
    for (int r = 0; r < world; ++r)
        if (all[(size_t)r * 3] != 0x1111111111111111ull * (uint64_t)(r + 1) || all[(size_t)r * 3 + 1] != (uint64_t)r ||
            all[(size_t)r * 3 + 2] != ~(uint64_t)r)
            bad |= 1;
    // the chain: every rank adds its number + 1 to what it is handed
    uint64_t hop[2] = {0, 0};
    if (rank > 0 && comm->recv(comm->ctx, rank - 1, hop, sizeof(hop)) != 0) return BZ_E_UNEXPECTED;
    if (hop[0] != (uint64_t)rank * (uint64_t)(rank + 1) / 2 || hop[1] != (uint64_t)rank) bad |= 2;
    hop[0] += (uint64_t)rank + 1;
    hop[1] += 1;
    if (rank < world - 1 && comm->send(comm->ctx, rank + 1, hop, sizeof(hop)) != 0) return BZ_E_UNEXPECTED;
    // variable-length gather: rank r contributes 1000 * (r + 1) + 7 bytes (rank 1 of a world > 2: nothing)
    std::vector<uint64_t> off((size_t)world), len((size_t)world);
    uint64_t total = 0;
    for (int r = 0; r < world; ++r) {
        len[(size_t)r] = (world > 2 && r == 1) ? 0 : 1000ull * (uint64_t)(r + 1) + 7;
        off[(size_t)r] = total;
        total += len[(size_t)r];
    }
    const size_t my_len = (size_t)len[(size_t)rank];
    std::vector<uint8_t> h_send(my_len + 1), h_recv((size_t)total + 1, 0);
    for (size_t i = 0; i < my_len; ++i) h_send[i] = (uint8_t)(i * 7 + (size_t)rank * 13 + 1);
    void *d_send = nullptr, *d_recv = nullptr;
    if (host_memory) {
        d_send = h_send.data();
        d_recv = h_recv.data();
    } else {
        HIPCHK(hipMalloc(&d_send, my_len + 16));
        HIPCHK(hipMalloc(&d_recv, (size_t)total + 16));
        HIPCHK(hipMemcpy(d_send, h_send.data(), my_len, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_recv, 0, (size_t)total + 16));
    }
    const int grc = comm->gatherv(comm->ctx, d_send, my_len, rank == 0 ? d_recv : nullptr, off.data(), len.data());
    if (!host_memory) {
        if (rank == 0 && grc == 0) (void)hipMemcpy(h_recv.data(), d_recv, (size_t)total, hipMemcpyDeviceToHost);
        (void)hipFree(d_send);
        (void)hipFree(d_recv);
    }
    if (grc != 0) return BZ_E_UNEXPECTED;
    if (rank == 0)
        for (int r = 0; r < world; ++r)
            for (size_t i = 0; i < (size_t)len[(size_t)r]; ++i)
                if (h_recv[(size_t)off[(size_t)r] + i] != (uint8_t)(i * 7 + (size_t)r * 13 + 1)) bad |= 4;
    // the verdict is shared, like the status words of the real path
    int64_t v = bad;
    std::vector<int64_t> vs((size_t)world, 0);
    if (comm->allgather(comm->ctx, &v, 8, vs.data()) != 0) return BZ_E_UNEXPECTED;
    for (int r = 0; r < world; ++r)
        if (vs[(size_t)r] != 0) return BZ_E_DATA;
    return BZ_OK;
}

extern "C" int bz_gpu_last_timings(bz_gpu_engine *g, double out_seconds[6])
{
    if (!g) return BZ_E_PARAM;
    for (int i = 0; i < 6; ++i) out_seconds[i] = g->t_stage[i];
    return BZ_OK;
}

extern "C" int bz_gpu_last_bwt_stats(bz_gpu_engine *g, uint64_t out[4])
{
    if (!g) return BZ_E_PARAM;
    for (int i = 0; i < 3; ++i) out[i] = g->bwt_stats[i];
    out[3] = g->fused_state[1]; // sorts of this engine (since its creation) that fell back to the three-kernel passes
    return BZ_OK;
}

extern "C" int bz_gpu_cut_stats(bz_gpu_engine *g, uint64_t out[2])
{
    if (!g || !out) return BZ_E_PARAM;
    out[0] = g->cut_stats[0];
    out[1] = g->cut_stats[1];
    return BZ_OK;
}

extern "C" int bz_gpu_last_bwt_rounds(bz_gpu_engine *g, uint64_t out[64])
{
    if (!g) return BZ_E_PARAM;
    for (int i = 0; i < 64; ++i) out[i] = g->round_active[i];
    return BZ_OK;
}

extern "C" int bz_gpu_debug_block_stats(bz_gpu_engine *g, uint32_t *h_stats, size_t cap_blocks, size_t *n_blocks)
{
    if (!g) return BZ_E_PARAM;
    const size_t nb = g->h_out.size();
    if (n_blocks) *n_blocks = nb;
    for (size_t i = 0; i < nb && i < cap_blocks; ++i) {
        const BlockOut &o = g->h_out[i];
        uint32_t *s = h_stats + i * 8;
        s[0] = g->h_out_nblock[i];
        s[1] = o.crc;
        s[2] = o.orig_ptr;
        s[3] = o.mtf_count;
        s[4] = o.in_use_count;
        s[5] = o.group_num;
        s[6] = o.n_selectors;
        s[7] = o.max_len | (o.lm_tables << 16);
    }
    return BZ_OK;
}

// The figures behind the reference's other two log::debug! lines of write_blockdata (src/bzip2/encoder.rs:483-498 "pass k: size
// is .., grp uses are ..", :556-636 "bits: mapping .., selectors .., code lengths .., codes ..") for every block of the last
// encode: 32 words per block -- [0..3] totc / 8 of the four refinement passes, [4 + 6 k + t] groups that chose table t in
// pass k (fave), [28] bits of the mapping table, [29] of the selectors (3 + 15 + their unary codes), [30] of the code
// lengths, [31] of the block's symbols.  The per-pass figures are collected only while bz_gpu_profile_enable(g, 2) is in force
// (0.1 ms per GiB in k_huff_sweep and a copy per batch; off: they read 0) and not by the BZ_HUFF_SPLIT=0 flavour.
extern "C" int bz_gpu_debug_block_sections(bz_gpu_engine *g, uint32_t *h_sections, size_t cap_blocks, size_t *n_blocks)
{
    if (!g) return BZ_E_PARAM;
    const size_t nb = g->h_out.size();
    if (n_blocks) *n_blocks = nb;
    if (g->h_out_pass.size() < nb * 32) return nb ? BZ_E_UNEXPECTED : BZ_OK;
    for (size_t i = 0; i < nb && i < cap_blocks; ++i) {
        const BlockOut &o = g->h_out[i];
        const uint32_t *ps = g->h_out_pass.data() + i * 32;
        uint32_t *s = h_sections + i * 32;
        for (int k = 0; k < 4; ++k) {
            s[k] = ps[k * 8] / 8u;
            for (int t = 0; t < 6; ++t) s[4 + 6 * k + t] = ps[k * 8 + 1 + t];
        }
        const uint32_t used_ranges = o.pad & 31u, sel_total = o.pad >> 5;
        const uint32_t mapping = 16u + 16u * used_ranges, selectors = 3u + 15u + sel_total;
        s[28] = mapping;
        s[29] = selectors;
        s[30] = o.header_bits - (48u + 32u + 1u + 24u) - mapping - selectors;
        s[31] = (uint32_t)(o.total_bits - o.header_bits);
    }
    return BZ_OK;
}

extern "C" int bz_gpu_debug_bwt(bz_gpu_engine *g, const uint8_t *h_block, size_t n, uint32_t *h_sa)
{
    if (!g || n == 0 || n > kMaxBlockLen) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    int rc = ensure_workspace(g, 1);
    if (rc != BZ_OK) return rc;
    if ((rc = g->rle.ensure(n + 256)) != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(g->rle.p, h_block, n, hipMemcpyHostToDevice, g->st));
    BlockDesc d;
    d.rle_off = 0;
    d.in_off = 0;
    d.in_end = n;
    d.n = (u32)n;
    d.pad = 0;
    HIPCHK(hipMemcpyAsync(g->lblocks.p, &d, sizeof(d), hipMemcpyHostToDevice, g->st));
    u64 sorted = 0;
    const int rounds = sort_batch(g, make_bwt_args(g, 1), (u32)n, (u64)n, &sorted, nullptr, nullptr);
    if (rounds < 0) return BZ_E_UNEXPECTED;
    g->bwt_stats[0] = (u64)rounds;
    g->bwt_stats[1] = sorted;
    HIPCHK(hipMemcpyAsync(h_sa, g->SA.p, n * 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

// The MTF / ZLE stage alone, as encode_batch runs it, on `nb` last columns given by the host (column i: h_cols + h_off[i],
// h_len[i] bytes).  The bytes in use are taken from the columns (a column is a permutation of its block).
extern "C" int bz_gpu_debug_mtf(bz_gpu_engine *g, size_t nb, const uint8_t *h_cols, const uint64_t *h_off, const uint32_t *h_len,
                                int heads, uint16_t *h_sym, size_t sym_stride, uint32_t *h_mtf_count, uint32_t *h_in_use,
                                uint32_t *h_freq)
{
    if (!g || nb == 0 || !h_cols || !h_off || !h_len || !h_sym || !h_mtf_count || !h_in_use || !h_freq) return BZ_E_PARAM;
    u32 max_n = 0;
    u64 total_n = 0;
    for (size_t i = 0; i < nb; ++i) {
        if (h_len[i] == 0 || h_len[i] > kMaxBlockLen || sym_stride < (size_t)h_len[i] + 1u) return BZ_E_PARAM;
        max_n = std::max(max_n, h_len[i]);
        total_n += h_len[i];
    }
    HIPCHK(hipSetDevice(g->device));
    int rc = ensure_workspace(g, nb);
    if (rc != BZ_OK) return rc;
    if (nb > g->ws_blocks) return BZ_E_PARAM;
    std::vector<BlockDesc> descs(nb);
    for (size_t i = 0; i < nb; ++i) {
        descs[i].rle_off = (u64)i * kSlot; // (the column's slot: k_block_symbols reads it as the block's image)
        descs[i].in_off = 0;
        descs[i].in_end = h_len[i];
        descs[i].n = h_len[i];
        descs[i].pad = 0;
        HIPCHK(hipMemcpyAsync(g->L.as<u8>() + i * kSlot, h_cols + h_off[i], h_len[i], hipMemcpyHostToDevice, g->st));
    }
    HIPCHK(hipMemcpyAsync(g->lblocks.p, descs.data(), nb * sizeof(BlockDesc), hipMemcpyHostToDevice, g->st));
    BwtArgs ba = make_bwt_args(g, (u32)nb);
    ba.rle = g->L.as<u8>();
    launch_block_symbols(g->st, ba, g->inuse_bits.as<u32>(), const_cast<u8 *>(ba.sym_code), const_cast<u8 *>(ba.keyinfo));
    MtfArgs ma = make_mtf_args(g, (u32)nb);
    if (heads >= 0) ma.heads = heads != 0 ? 1u : 0u;
    ma.tiles = std::min<u32>(kTilesPerBlock, std::max<u32>(1u, (max_n + kSortTile - 1u) / kSortTile));
    launch_mtf(g->st, ma, nullptr, total_n);
    if (ma.fused_zle) { // the ticket check of encode_batch: a one-launch ZLE stage that misbehaved is redone with the three kernels
        u32 tk[9] = {};
        const MailSeg sg = {tk, g->ztick.p, sizeof(tk)};
        if (mail_fetch(g->st, &sg, 1) != 0) return BZ_E_UNEXPECTED;
        bool bad = tk[8] != 0;
        for (u32 x = 0; x < 8; ++x)
            if (tk[x] != ma.tiles * (xcd_grid_y((u32)nb) / 8u)) bad = true;
        if (bad) {
            fprintf(stderr, "bz2_mi355x: the one-launch ZLE stage misbehaved (tile tickets / look-back); stage redone with three kernels\n");
            g->zle_fused_broken = true;
            ma.fused_zle = 0;
            launch_mtf(g->st, ma, nullptr, total_n);
        }
    }
    std::vector<BlockOut> outs(nb);
    HIPCHK(hipMemcpyAsync(outs.data(), g->bout.p, nb * sizeof(BlockOut), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(h_freq, g->mtf_freq.p, nb * kMaxAlpha * 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    for (size_t i = 0; i < nb; ++i) {
        if (outs[i].mtf_count == 0 || outs[i].mtf_count > h_len[i] + 1u) return BZ_E_UNEXPECTED;
        h_mtf_count[i] = outs[i].mtf_count;
        h_in_use[i] = outs[i].in_use_count;
        HIPCHK(hipMemcpyAsync(h_sym + i * sym_stride, g->mtf.as<u16>() + i * kMtfStride, (size_t)outs[i].mtf_count * 2,
                              hipMemcpyDeviceToHost, g->st));
    }
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    return BZ_OK;
}

extern "C" int bz_gpu_debug_code_lengths(bz_gpu_engine *g, const uint32_t *h_freq, size_t alpha, uint8_t *h_len,
                                         int *took_length_limited_path)
{
    if (!g || alpha == 0 || alpha > kMaxAlpha) return BZ_E_PARAM;
    {   // the domain of the device's 32-bit weights (k_huff.hip "DOMAIN"): what a block can hold, with room to spare
        uint64_t total = 0;
        for (size_t i = 0; i < alpha; ++i) total += h_freq[i] ? h_freq[i] : 1u;
        if (total >= (1u << 20)) return BZ_E_PARAM;
    }
    HIPCHK(hipSetDevice(g->device));
    DevBuf f, o, s, fl;
    int rc;
    if ((rc = f.ensure(alpha * 4)) || (rc = o.ensure(alpha + 8)) || (rc = s.ensure((size_t)kLmWords * 4)) ||
        (rc = fl.ensure(4)))
        return rc;
    HIPCHK(hipMemcpyAsync(f.p, h_freq, alpha * 4, hipMemcpyHostToDevice, g->st));
    launch_probe_code_lengths(g->st, f.as<u32>(), (u32)alpha, o.as<u8>(), s.as<u32>(), fl.as<int>());
    int flag = 0;
    HIPCHK(hipMemcpyAsync(h_len, o.p, alpha, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipMemcpyAsync(&flag, fl.p, 4, hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    if (took_length_limited_path) *took_length_limited_path = flag;
    return BZ_OK;
}

static const char *kKernelNames[KID_COUNT] = {"k_radix_hist", "k_radix_scan", "k_radix_scatter",
                                              "k_group_flags", "k_group_apply", "k_last_column",
                                              "k_radix_scatter_lb", "k_ghist_text", "k_ghist_scan", "k_rank_place", "k_phase_b_local", "k_group_refine",
                                              "k_dec_block", "k_dec_mtf", "k_dec_tsort", "k_dec_walk_lengths",
                                              "k_dec_place", "k_dec_rle", "k_dec_crc", "k_rle_onepass", "k_rle_scatter", "k_mtf_heads"};

extern "C" int bz_gpu_profile_enable(bz_gpu_engine *g, int on)
{
    if (!g) return BZ_E_PARAM;
    g->prof.reset();
    g->prof.on = (on & 1) != 0;
    g->debug_figures = (on & 2) != 0; // (the per-pass figures of bz_gpu_debug_block_sections: a few ballots per group in k_huff_sweep)
    return BZ_OK;
}

extern "C" int bz_gpu_profile_kernels(bz_gpu_engine *g)
{
    (void)g;
    return KID_COUNT;
}

extern "C" int bz_gpu_profile_get(bz_gpu_engine *g, int idx, const char **name, uint64_t *launches,
                                  double *seconds, uint64_t *algorithmic_bytes)
{
    if (!g || idx < 0 || idx >= KID_COUNT) return BZ_E_PARAM;
    if (name) *name = kKernelNames[idx];
    if (launches) *launches = g->prof.launches[idx];
    if (seconds) *seconds = g->prof.seconds[idx];
    if (algorithmic_bytes) *algorithmic_bytes = g->prof.bytes[idx];
    return BZ_OK;
}
