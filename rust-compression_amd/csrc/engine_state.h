// engine_state.h -- the engine object behind `bz_gpu_engine*` (include/bz2_mi355x.h, section 2),
// shared by the encode orchestration (engine.hip) and the decode orchestration (dec_engine.hip).
#pragma once
#include "../../include/bz2_mi355x.h"
#include "bzgpu.h"
#include "dev_buf.h"
#include "host_call.h"

#include <cstdio>
#include <vector>

using namespace bzgpu;

struct DecWorkspace;
void dec_workspace_free(DecWorkspace *w);
// the decode path as the encoder's self-check uses it (dec_engine.hip): d_in[n] -> d_out (device memory, cap bytes);
// returns an infrastructure status, the decoder's verdict in *verdict and the bytes it produced in *produced
int dec_decode_for_verify(struct bz_gpu_engine *g, const uint8_t *d_in, uint64_t n, uint8_t *d_out, uint64_t cap,
                          uint64_t *produced, int *verdict);
// (the engines that calls and contexts of both codecs park between uses: dec_cache_take / dec_cache_put /
// dec_release_cached, declared in host_call.h with the lease that is their one user, defined in engine_cache.hip)
void dec_spare_bufs_clear(); // dec_engine.hip: the byte buffers finished bz_dec contexts leave for the next one
struct DfWorkspace;
void df_workspace_free(DfWorkspace *w);
uint64_t df_batch_image_bytes(); // deflate_engine.hip: BZ_DF_BATCH_MIB, the slot image of a sub-batch of either encoder
struct LzhWorkspace;
void lzh_workspace_free(LzhWorkspace *w);
// bz_gpu_lzh_decode_batch_device with the outputs' places given by the caller (lzhuf_engine.hip; every entry has a known
// original length, and h_place[i], a multiple of 16, has room for it)
int lzh_decode_batch_placed(struct bz_gpu_engine *g, int method, int prefill, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                            const uint64_t *h_orig_len, size_t count, void *d_out, size_t cap, const uint64_t *h_place, uint64_t *h_out_len,
                            int32_t *h_verdict);
struct LhaWorkspace;
void lha_workspace_free(LhaWorkspace *w);

struct bz_gpu_engine {
    int device = 0;
    hipStream_t st = nullptr;   // rotation sort (and everything serial)
    hipStream_t st2 = nullptr;  // MTF / Huffman of a batch behind its sort (encode_batch); the RLE1 image beside the cut chain
    size_t max_blocks = 0;

    // constant tables
    DevBuf crc_tab, xp16, xp2;
    // partition state (sized by the input)
    DevBuf tile_last, carry_in, tile_crc, tile_count, tile_off, sub_off, sub_rs, scal, scan_part, rle, blocks_all, crc_all;
    // the cuts from tables (k_rle1.hip "kernels H")
    DevBuf cut_step_t0, cut_step_nt, cut_step_w0, cut_tab, cut_comp;
    CutPlan cut_plan = {};
    bool cut_ready = false;       // the tables of the current range are filled (or being filled on st)
    u64 h_halo_total = 0;         // sharded job: the image bytes a rank found in front of its slab (a D2H copy queued on st lands here:
                                  // the engine outlives every return path of the call, a stack frame does not)
    u64 cut_stats[2] = {0, 0};    // since creation: partitions cut from tables, partitions that fell back to the chain kernel
    // the front end in one pass (k_rle_onepass): its look-back words, their epoch, and what the current split has of it
    DevBuf rle_lb;                // [64 bytes: tickets, error word][spans] run starts [spans] image offsets
    u64 rle_lb_spans = 0;         // spans the words are laid out for
    u32 rle_epoch = 0;            // tag of the last launch (1 .. rle_onepass_epochs(); the words are cleared when it wraps)
    bool rle_onepass_broken = false; // it misbehaved on this engine once: the engine stays on the three kernels
    bool onepass_done = false;    // the tables and the image of the current input came from it
    u64 onepass_total = 0;        // ... and the image has this many bytes
    std::vector<BlockDesc> h_blocks;
    std::vector<u32> h_crc;
    const u8 *d_in = nullptr;
    u64 n_in = 0;
    u64 slab_t0 = 0, slab_t1 = 0; // tiles this engine splits (the whole input on one GPU)
    int level = 9;
    // batch workspace (sized by max_blocks)
    DevBuf lblocks, lcrc, SA, R, KA, VA, KB, VB, tile_hist, count, flags, tlo, tln, nonfinal, active, per_k,
        per_shift, lin_p, lin_sig, bin_cursor, pb_gate, bin_base, newbits, sym_code, keyinfo, count2, tile_nf, L, orig_ptr, inuse_bits, summ, summ_len, init_state, rank8, mtf_heads_buf, headbits, hcount, tile_hcnt, tile_hbase, ptext, pair_bits, ztile_last, ztile_cnt, zstate, ztick, mtf,
        mtf_freq, bout, selector, code_len, group_bitoff, lm_scratch, hglen, hpack, hrfreq, hlm, hpass, stream, error_flag, packlist, gh_tiles, gbase, abits,
        tile_state, tickets;
    u32 sort_epoch = 0; // fused radix passes: tag of the current pass in tile_state / tickets
    bool zle_fused_broken = false; // the one-launch ZLE stage misbehaved on this engine once: it stays on the three kernels
    u32 fused_state[2] = {0, 0}; // [0] fused passes found misbehaving on THIS engine (they stay off for it), [1] fallbacks
    hipEvent_t ev_aux = nullptr; // work that runs on st2 beside st (the RLE1 image beside the cut chain)
    size_t ws_blocks = 0; // blocks the batch workspace holds now (<= max_blocks)
    // own packed buffer / assemble list for the single-GPU convenience call
    DevBuf packed, gathered, asmlist;
    // a batch of inputs (bz_gpu_encode_batch_device): the one-block inputs' records, their streams' frames and their bit
    // strings (the inputs that may take several blocks go through `packed` one at a time while these are still needed)
    DevBuf batch_items, batch_frames, batch_packed;
    u64 batch_stats[4] = {0, 0, 0, 0}; // last batch: inputs through k_rle_batch, through the one-input path, blocks, sub-batches
    unsigned long long *h_active = nullptr; // pinned
    // results of the last encode
    std::vector<BlockOut> h_out;
    std::vector<u32> h_out_nblock;
    std::vector<u32> h_out_pass; // 32 words per block: k_huff_sweep's per-pass figures (bz_gpu_debug_block_sections)
    double t_stage[6] = {0, 0, 0, 0, 0, 0};
    KernelProf prof;
    // last bz_gpu_encode_sharded: wait for the hop, hop -> hand-on, gather, assembly; entry -> ready for the hop (scan,
    // counts, the slab's image offsets, its image and the cut tables under way), the chain kernel or table look-ups alone,
    // the whole call
    double shard_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    u64 bwt_stats[4] = {0, 0, 0, 0};
    u64 round_active[64] = {};

    struct Span {
        int stage;
        hipStream_t st;
        hipEvent_t a, b;
    };
    std::vector<Span> spans;
    // self-check (bz_gpu_engine_set_verify / BZ_VERIFY=1): the blocks of every bz_gpu_encode_blocks call are decoded on
    // the device and compared with the input they cover before the call returns
    bool verify = false;
    bool debug_figures = false; // bz_gpu_profile_enable(g, 2 | ..): k_huff_sweep sums the per-pass figures of bz_gpu_debug_block_sections
    u64 verify_stats[4] = {0, 0, 0, 0}; // since creation: blocks checked, calls redone, redone calls that failed again, ns
    DevBuf vstream, vout, vseg, vmis;
    DecWorkspace *dec = nullptr; // decode workspace, created by the first decode call
    DevBuf dec_in, oneshot_out;  // bz_decode_buffer / df_encode_buffer: the caller's bytes on the device and the result (kept with the cached engine)
    DfWorkspace *df = nullptr;   // Deflate encode workspace, created by the first df_gpu_encode_device call
    LzhWorkspace *lzh = nullptr; // LZHUF decode workspace, created by the first bz_gpu_lzh_decode_batch_device call
    LhaWorkspace *lha = nullptr; // LHA archive reader's workspace, created by the first bz_gpu_lha_read_device call
};

#include "one_shot.h" // (behind the engine: its round trip uses dec_in and oneshot_out)
