/*
 * bz2_mi355x.h -- C ABI of the MI355X-native BZip2 block-encode path (sections
 * 1-2) and of the matching decode path (section 3).
 *
 * This is the drop-in boundary for ONE hot path of chalharu/rust-compression:
 *   `iter.encode(&mut BZip2Encoder::new(level), action)`  (BZip2 encode),
 * widened by its inverse `iter.decode(&mut BZip2Decoder::new())`.
 * The reference is pure Rust and has no FFI of its own; each entry point below
 * names the reference interface it replaces (paths relative to the reference
 * repo).  A Rust shim re-implements `Encoder::next` on top
 * of these calls; host/compression.hpp is the same shim in C++.
 *
 * Plain C types only: pointers, sizes, ints.  No torch / HIP types appear in
 * any signature; device pointers are `void*`/`const void*` and a HIP stream is
 * an opaque `void*` (0 = the engine's own stream).
 *
 * Stream ordering: an engine launches its kernels on its OWN HIP stream, and every device-pointer
 * call returns after that stream has drained.  The caller makes sure that the input behind a device
 * pointer is complete before the call (synchronise the stream that produced it), and does not hand
 * the engine a buffer that a stream-ordered allocator may still be reading on another stream (a
 * PyTorch tensor allocated right after asynchronous work that freed its inputs is such a buffer:
 * torch.cuda.synchronize() first).
 *
 * Results are bit-identical to the reference encoder (checked against the CPU
 * oracle in oracle/).  There is NO CPU fallback: without a gfx950 device every
 * compute entry point returns BZ_E_NOGPU.
 */
#ifndef BZ2_MI355X_H
#define BZ2_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------
 * 0 = ok.  -1..-3 mirror CompressionError::{DataError,UnexpectedEof,Unexpected}
 * (src/error.rs:10-15); -4/-5 are BZip2Error::{DataErrorMagicFirst,DataErrorMagic}
 * (src/bzip2/error.rs:5-11, produced by the decoder entry points of section 3).  The encoder can
 * only fail with BZ_E_UNEXPECTED in the reference (src/bzip2/encoder.rs:623);
 * HIP failures map to it too. */
#define BZ_OK 0
#define BZ_E_DATA (-1)
#define BZ_E_EOF (-2)
#define BZ_E_UNEXPECTED (-3)
#define BZ_E_MAGIC_FIRST (-4)
#define BZ_E_MAGIC (-5)
#define BZ_E_PARAM (-6)  /* invalid level: BZip2Encoder::new panics (src/bzip2/encoder.rs:59-61) */
#define BZ_E_NOGPU (-7)  /* no gfx950 device / HIP runtime unusable: the path fails loudly */
#define BZ_E_NOMEM (-8)
#define BZ_E_CAPACITY (-9) /* caller's output buffer too small */

/* src/action.rs:8-13 */
#define BZ_ACTION_RUN 0
#define BZ_ACTION_FLUSH 1
#define BZ_ACTION_FINISH 2

const char *bz_strerror(int code);
const char *bz_version(void);
/* number of usable gfx950 devices (0 when none; never initialises a context) */
int bz_device_count(void);

/* ========================================================================
 * 1. Streaming encoder context  ==  `BZip2Encoder`  (src/bzip2/encoder.rs:40-49)
 * ======================================================================== */
typedef struct bz_enc bz_enc;

/* BZip2Encoder::new(level) (src/bzip2/encoder.rs:58-72).  level 1..=9 else
 * BZ_E_PARAM (the shim turns that back into the reference's panic).
 * `device` is the HIP device ordinal.  The GPU is first touched lazily, at the
 * first call that has work for it. */
int bz_enc_create(bz_enc **out, int level, int device);

/* The same encoder over SEVERAL devices of one process (SURVEY.md 8(b) "Surface"; in the shims
 * `BZip2Encoder::with_devices(level, &[0, 1, ..])`, still src/bzip2/encoder.rs:58-72 for the caller, who drives it
 * through the unchanged Encoder::next of src/traits/encoder.rs:41-79).  Every entry of `devices` (HIP ordinals; an
 * ordinal may be listed more than once) gets two LANES (BZ_ENC_LANES in the environment: 2 .. 8) -- an engine with its
 * own streams and buffers each; the input is cut into chunks (BZ_ENC_CHUNK_MIB, default 192), chunk q is uploaded to and
 * encoded on lane q mod (2 n_devices), the unconsumed tail of a
 * chunk's input crosses to the next lane's device (hipMemcpyPeerAsync: xGMI between the GPUs of a node), and the
 * block bit strings are concatenated in chunk order with the BitWriter carry, the combined CRC and "a block has
 * been written" handed from chunk to chunk on the host.  The bytes are those of bz_enc_create for any device list
 * and any chunk size.  bz_enc_create(out, level, d) == bz_enc_create_multi(out, level, &d, 1). */
int bz_enc_create_multi(bz_enc **out, int level, const int *devices, int n_devices);

/* The input iterator yielded `n` more bytes (src/bzip2/encoder.rs:80-85,
 * EncoderInner::next :671-697).  Bytes are copied; complete blocks may be
 * encoded immediately. */
int bz_enc_write(bz_enc *e, const uint8_t *in, size_t n);

/* The input iterator returned None while the caller's Action is `action`
 * (src/bzip2/encoder.rs:86-110 and :129-146): Run = nothing is flushed,
 * Flush = current block without the pending run, then zero-pad to a byte,
 * Finish = pending run, last block, trailer, pad.  Runs the reference's
 * state machine up to the point where `Encoder::next` would return None. */
int bz_enc_end(bz_enc *e, int action);

/* Output bytes in stream order (the bytes `Encoder::next` hands out,
 * src/bzip2/encoder.rs:149-157).  Returns the number of bytes copied (0 = none
 * ready) or a negative status. */
long bz_enc_read(bz_enc *e, uint8_t *out, size_t cap);
/* bytes currently readable */
size_t bz_enc_pending(const bz_enc *e);

void bz_enc_destroy(bz_enc *e);

/* Self-check (opt-in; BZ_VERIFY=1 in the environment turns it on for every context and engine of the process).  The
 * reference encoder is sequential code that cannot emit a stream which does not decode to its input
 * (src/bzip2/encoder.rs:224-291); a GPU pipeline with look-back words, ticket counters and stream-ordered clears can,
 * if one of them is ever wrong.  With the check on, the blocks of every job are decoded again on the same device (the
 * decode path of section 3) and compared byte for byte with the input they cover BEFORE their bytes can be read; a job
 * that fails is encoded again without any look-back pass and checked again, and if that fails too bz_enc_write /
 * bz_enc_end return BZ_E_UNEXPECTED.  Costs about one decode per encode (encode 12.6 GB/s, decode 22 GB/s).
 * stats: [0] blocks checked, [1] jobs that failed the check and were redone, [2] redone jobs that failed again (the
 * context is in error), [3] nanoseconds spent checking. */
int bz_enc_set_verify(bz_enc *e, int on);
int bz_enc_verify_stats(bz_enc *e, uint64_t out[4]);

/* Where the time of a stream went (milliseconds, summed over its jobs; a diagnostic -- the bytes do not depend on it):
 * [0] the caller's copies into pinned staging memory  [1] the caller waiting for a free staging buffer
 * [2] SPLIT sections (compose + RLE1 + block cuts; serial from job to job)  [3] ENCODE (jobs side by side on the lanes)
 * [4] ASSEMBLE sections (serial)  [5] downloads  [6] number of jobs  [7] workers waiting for their turn in the two serial
 * sections.  bz_encode_buffer_last_phases: the same for the last one-shot call of the process. */
int bz_enc_phase_stats(bz_enc *e, double out_ms[8]);
int bz_encode_buffer_last_phases(double out_ms[8]);

/* One-shot over host buffers:
 * `in.iter().cloned().encode(&mut BZip2Encoder::new(level), Action::Finish).collect()`.
 * *out is malloc'ed by the library; release with bz_free. */
int bz_encode_buffer(int level, int device, const uint8_t *in, size_t in_len,
                     uint8_t **out, size_t *out_len);
/* ... over several devices (see bz_enc_create_multi).  A one-shot call knows its length: it cuts the input into
 * equal chunks, a whole number of rounds over the lanes. */
int bz_encode_buffer_multi(int level, const int *devices, int n_devices, const uint8_t *in, size_t in_len,
                           uint8_t **out, size_t *out_len);
/* Many independent inputs in one call: stream i is bz_encode_buffer(level, device, ins[i], lens[i]), bit for bit, and
 * lies at *out + out_off[i] with out_len[i] bytes (streams in input order, each starting at a multiple of 4 bytes, zeros
 * between them).  *out is ONE malloc'ed buffer (release with bz_free); out_off and out_len have `count` entries.  The
 * inputs are packed at 16-byte-aligned offsets into pinned staging memory, uploaded once, encoded by
 * bz_gpu_encode_batch_device (section 2) on an engine of the per-process cache and downloaded once.  BZ_VERIFY=1
 * applies.  count == 0: BZ_OK, *out is an empty buffer. */
int bz_encode_batch(int level, int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                    uint8_t **out, uint64_t *out_off, uint64_t *out_len);
void bz_free(void *p);
/* Contexts and one-shot calls park their engines (batch workspace: about 36.4 MB of HBM per block of the largest
 * chunk seen, i.e. up to ~9 GB per lane with the default 192 MiB chunks, two lanes per listed device), device staging
 * buffers and 2 x BZ_ENC_CHUNK_MIB of pinned host memory in a per-process cache (two device lists at most) when they
 * end, so that the next one does not pay hipMalloc / hipHostMalloc again (fresh device memory costs about 40 ms per
 * GiB on this platform: the FIRST 1 GiB call of a process takes 0.35 s, a later one 0.1 s).  This call releases what
 * is parked (call it between contexts to run without the cache).  The decode and Deflate entry points over host
 * buffers (bz_decode_buffer, bz_dec_*, df_encode_buffer, df_enc_*) park up to TWO engines per device the same way (the
 * lanes of a streaming decoder; a decode workspace is about 13 MB of HBM per block of the largest stream seen; a call
 * takes an engine that holds its kind of workspace, else the one parked last), and bz_dec_* contexts leave up to four of
 * their chunk buffers (64 MiB of host memory each by default): released here too. */
void bz_release_cached_resources(void);
/* Diagnostic for hosts with several devices (no reference counterpart: the reference has no devices).  What a context
 * over `devices` does when a job's unconsumed tail changes device -- hipMemcpyPeerAsync, across xGMI where peer access
 * can be enabled, through the host where not -- done once per neighbour pair devices[i] -> devices[i + 1 mod n] with
 * `bytes` (1 ... 2^30) of a known pattern, there and back, compared on the host.  peer_access[i] (may be NULL): 1 direct
 * access enabled, 0 not offered, -1 both on one device (nothing copied); out_ms[i] (may be NULL): the round trip's wall
 * time, -1 if the pair failed.  BZ_OK when every pair's bytes came back intact; a failing pair is named on stderr. */
int bz_peer_copy_selftest(const int *devices, int n_devices, size_t bytes, int *peer_access, double *out_ms);

/* ========================================================================
 * 2. Device-resident engine (what bz_enc drives; also the bench / multi-GPU
 *    surface: input and output stay in HBM).
 *    Stages == src/bzip2/encoder.rs: RLE1+split+CRC (:671-716), write_blockdata
 *    (:300-639: BWT src/suffix_array/sais.rs:266, MTF src/bzip2/mtf.rs:16-39,
 *    ZLE :653-669, table selection :370-509, code lengths
 *    src/huffman/cano_huff_table.rs:198-225, canonical codes
 *    src/huffman/mod.rs:22-67, emission :527-629) and stream framing
 *    write_block (:224-291) + BitWriter<Left> (src/bitio/writer.rs:186-243).
 * ======================================================================== */
typedef struct bz_gpu_engine bz_gpu_engine;

/* max_blocks_in_flight bounds the workspace (about 36.4 MB of HBM per
 * block); inputs with more blocks are processed in several batches. */
int bz_gpu_engine_create(bz_gpu_engine **out, int device, size_t max_blocks_in_flight);
void bz_gpu_engine_destroy(bz_gpu_engine *g);
/* The batch workspace (about 36.4 MB per block in flight) is made by the first call that needs it and grows with the
 * largest call seen; a caller who knows the size of the calls to come reserves it once (fresh device memory costs about
 * 40 ms per GiB here: growing means freeing and paying again). */
int bz_gpu_engine_reserve(bz_gpu_engine *g, size_t blocks);

/* The self-check of section 1 for the device-resident calls: the blocks of every bz_gpu_encode_blocks (and so of
 * bz_gpu_encode_device / bz_gpu_encode_sharded on each rank) are decoded on the device and compared with the input they
 * cover before the call returns; stats as for bz_enc_verify_stats, since the engine's creation. */
int bz_gpu_engine_set_verify(bz_gpu_engine *g, int on);
int bz_gpu_verify_stats(bz_gpu_engine *g, uint64_t out[4]);

/* Upper bound of the .bz2 size for n input bytes (for sizing d_out). */
size_t bz_encode_bound(size_t n);

/* Whole stream on one GPU: d_in[n] (HBM, 16-byte aligned) -> d_out (HBM,
 * 4-byte aligned, cap bytes).  *out_len receives the stream length.
 * Equivalent to the one-shot above minus the PCIe copies. */
int bz_gpu_encode_device(bz_gpu_engine *g, int level, const void *d_in, size_t n,
                         void *d_out, size_t cap, size_t *out_len);

/* Many independent inputs, one stream each, in one pass of the pipeline.  Input i is the h_in_len[i] bytes at
 * d_in + h_in_off[i] (d_in 16-byte aligned, every offset a multiple of 16, ranges in ascending order without overlap);
 * stream i is the bytes of bz_gpu_encode_device(g, level, d_in + h_in_off[i], h_in_len[i], ...), bit for bit, and is
 * written to d_out + h_out_off[i] (h_out_len[i] bytes; d_out 4-byte aligned; streams in input order, each at a multiple
 * of 4 bytes, zeros between them).  The four arrays are HOST arrays of `count` entries.
 * An input of n bytes with 5 * (n / 4) + n % 4 <= 100000 * level - 19 is certainly one block (RLE1 grows it by at most
 * one byte per four, src/bzip2/encoder.rs:699-716, and the cut at :692 only fires behind a run that is not the last):
 * all such inputs are split by one launch and encoded together as the blocks of one bz_gpu_encode_blocks call, whatever
 * their number; an empty input is the 14 bytes of header and trailer.  Every other input takes the path of
 * bz_gpu_encode_device, one at a time.  bz_encode_batch_bound: a `cap` that always suffices (the sum of
 * bz_encode_bound, each rounded up to 4).
 * BZ_E_PARAM: level outside 1..9, a null array with count > 0, a misaligned offset, ranges that overlap or are out of
 * order.  BZ_E_CAPACITY: cap too small (nothing is promised about d_out then).  count == 0: BZ_OK, nothing is touched. */
size_t bz_encode_batch_bound(const uint64_t *in_len, size_t count);
int bz_gpu_encode_batch_device(bz_gpu_engine *g, int level, const void *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                               void *d_out, size_t cap,
                               uint64_t *h_out_off, uint64_t *h_out_len);
/* The last bz_gpu_encode_batch_device call: [0] inputs split by the batch front end (k_rle_batch)  [1] inputs that took
 * the one-input path  [2] blocks of the inputs of [0]  [3] sub-batches the pipeline ran them in (the workspace holds
 * max_blocks_in_flight blocks). */
int bz_gpu_last_batch_stats(bz_gpu_engine *g, uint64_t out[4]);

/* ---- the same, split into the three steps a multi-GPU job needs ---------- */

/* (a) RLE1 + block split over the whole input (every rank runs it: it is
 * <2 % of the work and keeps block boundaries a pure function of the input).
 * mode: BZ_ACTION_FINISH = all chunks, tail block emitted;
 *       BZ_ACTION_FLUSH  = like FINISH over the bytes given (the caller has
 *                          already removed the pending run);
 *       BZ_ACTION_RUN    = only blocks closed by a cut; *consumed tells how
 *                          many input bytes they cover.
 * Returns the number of blocks in *n_blocks; *tail_block = 1 when the last of
 * them is the unfinished tail rather than a block closed by a cut (the
 * streaming context needs that to replay write_block's call sequence). */
int bz_gpu_partition(bz_gpu_engine *g, int level, const void *d_in, size_t n, int mode,
                     size_t *n_blocks, size_t *consumed, int *tail_block);

/* (a') The same split sharded over ranks by SLABS of 4 KiB input tiles (rank r owns tiles
 * [tile0, tile1); every rank sees the whole input d_in[n] but touches only its slab plus the tail
 * of the block that straddles its left edge).  Three steps with two tiny exchanges in between:
 *   _slab_begin  run starts + tile CRCs of the slab; *slab_last_start = last run start inside it
 *                (-1: none).              [exchange: all-gather of that one value]
 *   _slab_count  carry_run = the last run start BEFORE the slab (max over lower ranks, -1: none);
 *                RLE1 byte counts of the slab.
 *   _slab_finish start_in = first input byte of this rank's first block (rank 0: 0; else the
 *                next_in handed over by rank-1: a serial chain of one 8-byte message per rank);
 *                is_last: the last rank also emits the unfinished tail block.  Produces this rank's
 *                blocks (stream order = rank order) for bz_gpu_encode_blocks(g, 0, 1, ...).
 * RLE1 restarted at a block cut equals RLE1 continued (a cut is a chunk start, encoder.rs:689-693),
 * so a rank codes its first block afresh from the cut it is handed.
 * bz_gpu_partition == these three calls over all tiles. */
int bz_gpu_partition_slab_begin(bz_gpu_engine *g, int level, const void *d_in, size_t n,
                                uint64_t tile0, uint64_t tile1, int64_t *slab_last_start);
int bz_gpu_partition_slab_count(bz_gpu_engine *g, int64_t carry_run);
int bz_gpu_partition_slab_finish(bz_gpu_engine *g, uint64_t start_in, int is_last, size_t *n_blocks,
                                 uint64_t *next_in, int *tail_block);

/* Blocks of the last partition (what *n_blocks returned): sizes the host arrays of (b). */
size_t bz_gpu_block_count(const bz_gpu_engine *g);

/* (b) Encode blocks first, first+stride, ... (< n_blocks) of the last
 * partition.  Each block's bit string (block magic .. last payload bit,
 * MSB-first) is appended to d_packed as host-endian uint32 words whose bit 31
 * is the earliest bit, zero padded to a whole word (cap_words words).  For the k-th local block:
 * h_word_off[k] = first word in d_packed, h_bit_len[k] = length in bits,
 * h_crc[k] = block CRC.  Arrays are HOST arrays with room for the local
 * block count ceil((n_blocks-first)/stride). *words_used = words written. */
int bz_gpu_encode_blocks(bz_gpu_engine *g, size_t first, size_t stride,
                         void *d_packed, size_t cap_words,
                         uint64_t *h_word_off, uint64_t *h_bit_len, uint32_t *h_crc,
                         size_t *words_used);

/* (c) Assemble a stream from block bit strings held in d_packed (in STREAM
 * order k = 0..n_blocks-1, described by the three host arrays): optional
 * "BZh<level>" header, blocks back to back at bit granularity, optional
 * trailer (0x177245385090 + combined CRC) and zero padding to a byte.
 * `carry_bits` (0..7) bits of `carry_byte` (left aligned) precede the
 * output -- the BitWriter carry of a previous call; *out_carry_* return the
 * new carry when no padding is requested.  combined_crc_in/out carry
 * src/bzip2/encoder.rs:237-238 across calls. */
int bz_gpu_assemble(bz_gpu_engine *g, int level, size_t n_blocks,
                    const void *d_packed, const uint64_t *h_word_off,
                    const uint64_t *h_bit_len, const uint32_t *h_crc,
                    int write_header, int write_trailer, int pad_to_byte,
                    unsigned carry_bits, unsigned carry_byte,
                    uint32_t combined_crc_in, uint32_t *combined_crc_out,
                    void *d_out, size_t cap, size_t *out_len,
                    unsigned *out_carry_bits, unsigned *out_carry_byte);

/* ---- the whole stream over several GPUs (BASELINE.json configs[2]) ----------------
 * One process (one engine) per GPU; every rank calls bz_gpu_encode_sharded with the same level and n.
 * Rank r splits its SLAB of the input -- a contiguous range of the 4 KiB tiles, bz_shard_slab_tiles: nearly equal
 * shares, shrinking a little from rank to rank (BZ_SHARD_SKEW) because rank r starts its blocks r links of
 * the cut chain later than rank 0 --, encodes the blocks that END in its slab
 * (stream order == rank order) and the block bit strings are gathered to rank 0, which assembles the
 * serial stream (bz_gpu_assemble).  The cuts (encoder.rs:692) are the only serial dependency between the slabs, and a
 * rank prepares its link of that chain before the cut of the rank in front arrives: with the slabs' image sizes
 * all-gathered every rank knows where its slab lies in the RLE1 image of the whole input, the k-th block of the whole
 * input can only start at one of 4 k + 1 offsets of that image, and the rank resolves the cut behind every such start
 * inside its slab in parallel (tables; bz_gpu_cut_stats).  The link itself is then about a hundred table look-ups.  d_in is addressed as the whole input, but a rank only reads its
 * slab and, in front of it, the input bytes of the block that straddles its left edge (a level-9
 * block covers at most 900000 * 255 / 5 = 45.9 MB of input), so the rest need not be backed by memory.
 * The transport is the caller's: RCCL (ncclAllGather / ncclSend / ncclRecv over xGMI), MPI or
 * torch.distributed behind four C callbacks, each returning 0 on success.  Every rank takes part in
 * every exchange; a rank-local error is carried in the exchanged status words and returned by ALL
 * ranks (no rank is left waiting in a collective).
 *   allgather(ctx, send, bytes, recv)   HOST memory: `bytes` bytes of every rank, in rank order, into recv
 *   send(ctx, dst, buf, bytes) / recv(ctx, src, buf, bytes)   HOST memory, 32 bytes along the cut chain
 *   gatherv(ctx, d_send, send_bytes, d_recv, recv_off, recv_bytes)   DEVICE memory: rank r's send_bytes
 *       bytes land at d_recv + recv_off[r] on rank 0 (recv_bytes[r] == that rank's send_bytes; the
 *       two arrays are valid on every rank, d_recv only on rank 0; rank 0's own part included).  The transfer
 *       must be OVER when the callback returns: the library reads d_recv (rank 0) and overwrites d_send (every
 *       rank, at its next call) on its own stream right away; a transport that queues the transfer on a stream
 *       synchronises that stream first (an RCCL request's wait only orders streams).
 * d_packed / d_gather: optional caller-owned device buffers (e.g. registered with the transport) for
 * this rank's bit strings and, on rank 0, everybody's; NULL = the engine's own.  On rank 0 *out_len
 * receives the stream length and d_out the stream; the other ranks get *out_len = 0. */
typedef struct bz_shard_comm {
    void *ctx;
    int rank, world;
    int (*allgather)(void *ctx, const void *send, size_t bytes, void *recv);
    int (*send)(void *ctx, int dst, const void *buf, size_t bytes);
    int (*recv)(void *ctx, int src, void *buf, size_t bytes);
    int (*gatherv)(void *ctx, const void *d_send, size_t send_bytes, void *d_recv,
                   const uint64_t *recv_off, const uint64_t *recv_bytes);
} bz_shard_comm;
int bz_gpu_encode_sharded(bz_gpu_engine *g, int level, const void *d_in, size_t n,
                          const bz_shard_comm *comm, void *d_packed, size_t packed_cap_words,
                          void *d_gather, size_t gather_cap_words, void *d_out, size_t cap,
                          size_t *out_len);

/* The same call for a rank that holds only a WINDOW of the input (a rank of a large job need not back the bytes it
 * never reads): d_window[0 .. window_bytes) are the input bytes [window_off, window_off + window_bytes) of the n-byte
 * input (d_window 16-byte aligned, window_off a multiple of 16).  The window must hold the rank's slab, the bytes of
 * the block that straddles its left edge (from the start of their 4 KiB tile on) and the 4 KiB tile behind the slab (or
 * all there is): bz_shard_window returns one that always does -- the slab plus bz_shard_halo_bytes(level) in front (a
 * level-9 block covers at most 899981 * 255 / 5 = 45.9 MB of input) and one tile behind.  A window that turns out
 * too short (the cut handed over by the rank before lies in front of it) makes every rank return BZ_E_CAPACITY.
 * bz_gpu_encode_sharded(g, level, d_in, n, ...) == bz_gpu_encode_sharded_window(g, level, d_in, 0, n, n, ...). */
int bz_shard_slab_tiles(size_t n, int rank, int world, uint64_t *tile0, uint64_t *tile1); /* the rank's tiles [tile0, tile1) */
size_t bz_shard_halo_bytes(int level);
int bz_shard_window(int level, size_t n, int rank, int world, uint64_t *window_off, size_t *window_bytes);
int bz_gpu_encode_sharded_window(bz_gpu_engine *g, int level, const void *d_window, uint64_t window_off,
                                 size_t window_bytes, size_t n, const bz_shard_comm *comm, void *d_packed,
                                 size_t packed_cap_words, void *d_gather, size_t gather_cap_words,
                                 void *d_out, size_t cap, size_t *out_len);

/* Where the last bz_gpu_encode_sharded[_window] call of this rank spent its wall time around the exchanges (ms):
 * [0] waiting for the cut from the rank before (rank 0: 0)  [1] from that cut's arrival to the hand-on of this rank's own
 * cut -- its LINK of the one serial chain across the ranks (left halo, tile offsets, the cut chain over its slab)
 * [2] the gather of the bit strings  [3] the assembly (rank 0). */
int bz_gpu_last_shard_timings(bz_gpu_engine *g, double out_ms[4]);
/* The same four and: [4] entry -> ready for the cut of the rank in front (scan, counts, the slab's image offsets, its
 * image and the cut tables under way: nothing of it waits for another rank's cuts), [5] the cuts themselves once the
 * hop is there (table look-ups, or the chain kernel), [6] unused, [7] the whole call. */
int bz_gpu_last_shard_phases(bz_gpu_engine *g, double out_ms[8]);

/* A ready-made transport: the four callbacks over RCCL (xGMI inside a node).  These three entry points are
 * exported by a SECOND library, libbz2_mi355x_rccl.so (it links librccl; the codec library does not):
 * rank 0 draws an id and ships its BZ_RCCL_ID_BYTES bytes to the other ranks by any means; every rank then
 * creates its communicator (collective: ncclCommInitRank) on the device its engine lives on.  Small host-byte
 * exchanges go through a pinned + a device staging buffer, the bit strings travel as one group of
 * ncclSend / ncclRecv between the callers' device buffers. */
#define BZ_RCCL_ID_BYTES 128
int bz_rccl_unique_id(uint8_t id[BZ_RCCL_ID_BYTES]);
int bz_rccl_comm_create(bz_shard_comm **out, const uint8_t id[BZ_RCCL_ID_BYTES], int rank, int world, int device);
void bz_rccl_comm_destroy(bz_shard_comm *comm);
/* ranks of the communicator as RCCL counts them (ncclCommCount), or a negative status */
int bz_rccl_comm_count(const bz_shard_comm *comm);
/* No exchange of this transport waits for ever: each one polls its stream, the communicator's asynchronous
 * error state and a deadline (BZ_RCCL_TIMEOUT_S in the environment, default 300 s); on an error or a timeout
 * the communicator is aborted (ncclCommAbort), the callback fails and bz_gpu_encode_sharded returns
 * BZ_E_UNEXPECTED on this rank. */

/* Runs known patterns through a transport's four callbacks, shaped like the exchanges above (every
 * rank calls it): BZ_OK, BZ_E_DATA (bytes arrived wrong somewhere; the same verdict on every rank) or
 * BZ_E_UNEXPECTED (a callback failed).  host_memory != 0: the buffers handed to gatherv are host
 * memory (a CPU transport under test; needs no GPU), else device memory. */
int bz_shard_comm_selftest(const bz_shard_comm *comm, int host_memory);

/* Seconds of GPU time spent in the kernels of the last bz_gpu_encode_device /
 * bz_gpu_encode_blocks call, by stage (HIP events on the engine's stream):
 * [0] rle1+crc+split [1] bwt [2] mtf+zle [3] huffman [4] emit+assemble [5] total. */
int bz_gpu_last_timings(bz_gpu_engine *g, double out_seconds[6]);
/* [0] BWT rounds executed (prefix doubling), [1] total sorted elements, [2] batches of the last call; [3] sorts of
 * this engine since its creation that fell back from the fused radix passes to the three-kernel passes (a
 * look-back gave up or tile tickets were not handed out evenly: the engine then stays on the three-kernel passes) */
int bz_gpu_last_bwt_stats(bz_gpu_engine *g, uint64_t out[4]);
/* The block cuts (encoder.rs:692), since the engine's creation: [0] partitions whose cuts came from the tables of
 * candidate cuts (every cut a block start can lead to, resolved in parallel; BZ_CUT_TABLES=0 turns them off),
 * [1] partitions that took the chain kernel instead although the tables were asked (never seen). */
int bz_gpu_cut_stats(bz_gpu_engine *g, uint64_t out[2]);
/* rotations still unordered after the initial 4-byte sort (out[0]) and after each doubling
 * round (out[1..]), summed over the blocks of the last encode */
int bz_gpu_last_bwt_rounds(bz_gpu_engine *g, uint64_t out[64]);

/* Per-kernel timing of the BWT kernels (HIP events around every launch, on the engine's
 * stream).  Enable, run encodes, then read: kernel name (all template instances of one
 * kernel are pooled), launches, summed duration, summed ALGORITHMIC bytes.
 * bz_gpu_profile_enable also clears the counters.  `on`: bit 0 the kernel timing, bit 1 the per-pass figures of
 * bz_gpu_debug_block_sections (a few ballots per group in the Huffman sweeps: off by default). */
int bz_gpu_profile_enable(bz_gpu_engine *g, int on);
int bz_gpu_profile_kernels(bz_gpu_engine *g);
int bz_gpu_profile_get(bz_gpu_engine *g, int idx, const char **name, uint64_t *launches,
                       double *seconds, uint64_t *algorithmic_bytes);

/* ---- stage probes for the parity tests (device results copied to host) ---- */

/* Rotation order of ONE block (src/suffix_array/sais.rs:266 `bwt`). */
int bz_gpu_debug_bwt(bz_gpu_engine *g, const uint8_t *h_block, size_t n, uint32_t *h_sa);
/* The MTF + zero-run stage alone on `nb` last columns (column i: h_cols + h_off[i], h_len[i] bytes, 1 .. 900000),
 * run as an encode runs it on a batch of nb blocks; the bytes in use are taken from the columns.  heads: 1 / 0 force
 * the form that ranks only the run heads / every position, -1 follows BZ_MTF_HEADS.  Per column: its symbols (RUNA 0,
 * RUNB 1, rank r > 0 as r + 1, EOB last) at h_sym + i * sym_stride (sym_stride > every h_len[i]), their number, the
 * number of bytes in use and the 258 symbol counts at h_freq + 258 i.  nb is bounded by max_blocks_in_flight. */
int bz_gpu_debug_mtf(bz_gpu_engine *g, size_t nb, const uint8_t *h_cols, const uint64_t *h_off, const uint32_t *h_len,
                     int heads, uint16_t *h_sym, size_t sym_stride, uint32_t *h_mtf_count, uint32_t *h_in_use,
                     uint32_t *h_freq);
/* Code lengths of one table (EncoderInner::create_huffman,
 * src/bzip2/encoder.rs:641-651) through the device code.  alpha <= 258 and a total of
 * less than 2^20 occurrences (a block holds 900 001 symbols at most; the device's weights
 * are 32-bit, the reference's usize: equal below 2^24 occurrences per package), else
 * BZ_E_PARAM. */
int bz_gpu_debug_code_lengths(bz_gpu_engine *g, const uint32_t *h_freq, size_t alpha,
                              uint8_t *h_len, int *took_length_limited_path);
/* Per-block statistics of the last bz_gpu_encode_blocks / encode_device call,
 * the numbers behind the reference's log::debug! lines
 * (src/bzip2/encoder.rs:240-243, :360-365): 8 x uint32 per block:
 * nblock, crc, origPtr, mtf_count, in_use_count, group_num, n_selectors, max_len */
int bz_gpu_debug_block_stats(bz_gpu_engine *g, uint32_t *h_stats, size_t cap_blocks,
                             size_t *n_blocks);
/* ... and the figures behind the other two debug lines of write_blockdata
 * (src/bzip2/encoder.rs:483-498 "pass k: size is .., grp uses are ..", :556-636
 * "bits: mapping .., selectors .., code lengths .., codes .."): 32 x uint32 per
 * block: [0..3] totc / 8 of the four refinement passes, [4 + 6 k + t] groups that
 * chose table t in pass k, [28] bits of the mapping table, [29] of the
 * selectors, [30] of the code lengths, [31] of the symbols.  The per-pass
 * figures need bz_gpu_profile_enable(g, 2) in force during the encode (else 0). */
int bz_gpu_debug_block_sections(bz_gpu_engine *g, uint32_t *h_sections, size_t cap_blocks,
                                size_t *n_blocks);

/* ========================================================================
 * 3. Decoder  ==  `BZip2Decoder`  (src/bzip2/decoder.rs:583-612; the work is
 *    BZip2DecoderBase::init_block / next, src/bzip2/decoder.rs:163-581)
 *
 * The decode calls return the DECODER'S verdict: BZ_OK, BZ_E_DATA
 * (BZip2Error::DataError), BZ_E_MAGIC_FIRST / BZ_E_MAGIC (bad level digit of
 * the first / a later stream header), or an infrastructure status
 * (BZ_E_NOGPU, BZ_E_NOMEM, BZ_E_CAPACITY, BZ_E_UNEXPECTED).  With a decoder
 * error the bytes of all blocks in front of the failing record are still
 * produced -- exactly the items the reference's iterator yields before its
 * Err (a block whose CRC is wrong is handed out first, src/bzip2/decoder.rs:189-201).
 * Multi-stream files decode to the concatenation (src/bzip2/decoder.rs:503-516).
 * ======================================================================== */

/* Whole file on one GPU: d_in[n] (HBM, 4-byte aligned) -> d_out (HBM, cap
 * bytes).  *out_len = bytes decoded.  d_out == NULL: sizes only (nothing is
 * written, CRCs are not checked), to learn the capacity a second call needs. */
int bz_gpu_decode_device(bz_gpu_engine *g, const void *d_in, size_t n,
                         void *d_out, size_t cap, size_t *out_len);
/* The same over several GPUs (one process per GPU, every rank holds the whole
 * compressed file): rank r decodes the r-th contiguous share of the blocks
 * into ITS OWN d_out.  *out_len = bytes of this rank's slice, *out_offset =
 * where the slice sits in the decoded file, *total_len = decoded bytes over all
 * ranks; the verdict is the same on every rank.  `allgather` is the only
 * collective the path needs (called twice, with a few bytes per block): it must
 * copy `bytes` bytes from `send` of every rank, in rank order, into `recv`
 * (world * bytes) -- RCCL, MPI or torch.distributed behind a C callback; return
 * 0 on success.  Blocks must carry their full 48-bit magic (every encoder's do). */
typedef int (*bz_allgather_fn)(void *ctx, const void *send, size_t bytes, void *recv);
int bz_gpu_decode_device_sharded(bz_gpu_engine *g, const void *d_in, size_t n,
                                 void *d_out, size_t cap, int rank, int world,
                                 bz_allgather_fn allgather, void *ctx,
                                 size_t *out_len, size_t *out_offset, size_t *total_len);
/* Seconds of GPU time of the last decode by stage (HIP events):
 * [0] magic scan + Huffman [1] zero runs + inverse MTF [2] inverse BWT
 * [3] RLE1 undo + CRC [4] total. */
int bz_gpu_last_decode_timings(bz_gpu_engine *g, double out_seconds[5]);
/* [0] block-magic candidates [1] blocks decoded [2] streams [3] blocks that
 * started without the full 48-bit magic */
int bz_gpu_last_decode_stats(bz_gpu_engine *g, uint64_t out[4]);

/* Many independent streams in one call.  Entry i is the h_in_len[i] bytes at d_in + h_in_off[i] (d_in 4-byte aligned,
 * every offset a multiple of 4, ranges in ascending order without overlap, the allocation reaches to the next multiple
 * of 4 behind the last entry; bytes between entries are never read as input of any entry) -- exactly what
 * bz_gpu_encode_batch_device writes: its (d_out, h_out_off, h_out_len) are valid (d_in, h_in_off, h_in_len) here.
 * The result of entry i is that of bz_gpu_decode_device on its bytes ALONE: the same bytes in front of the verdict
 * (those of a block whose CRC is wrong included), written to d_out + h_out_off[i] (h_out_len[i] bytes), and the same
 * verdict -- BZ_OK, BZ_E_DATA, BZ_E_MAGIC_FIRST or BZ_E_MAGIC -- in h_verdict[i].  An entry may hold several streams (its
 * stream count starts at 1); an empty entry is BZ_E_MAGIC_FIRST without bytes; no entry's verdict changes another
 * entry's result.  The RETURN VALUE is the infrastructure status only: BZ_OK also when entries carry decoder errors.
 * The five arrays are HOST arrays of `count` entries.
 * Every h_out_off[i] is a multiple of 16 and the ranges do not overlap, so (d_out, h_out_off, h_out_len) are valid
 * inputs of bz_gpu_encode_batch_device.  Offsets follow each entry's rebuilt length BEFORE its CRCs are looked at.
 * The scan, the Huffman stage and the record chains run over all entries of a GROUP (consecutive entries whose
 * block-magic candidates fit the workspace: BZ_DEC_BATCH, default 4096) in one launch each, and their true blocks are
 * rebuilt together; these entries lie in input order.  An entry with more candidates than a group holds, or with a
 * block that lacks its full 48-bit magic, takes the path of bz_gpu_decode_device on its own range: those lie behind all
 * the others, in input order among themselves.  Bytes of d_out outside the reported ranges are unspecified; nothing is
 * written at or behind d_out + cap.
 * d_out == NULL: sizes only (nothing is written, CRCs are not checked): h_out_off are those of the real call,
 * h_out_len[i] can exceed the real call's only for entries that a CRC turns into BZ_E_DATA, and the capacity the real
 * call needs is the largest h_out_off[i] + h_out_len[i] of this one.
 * BZ_E_CAPACITY: cap too small.  BZ_E_PARAM: a null engine, a null array with count > 0, a misaligned d_in or offset,
 * ranges that overlap or are out of order.  count == 0: BZ_OK, nothing is touched.
 * bz_gpu_last_decode_timings and bz_gpu_last_decode_stats hold sums over the call afterwards. */
int bz_gpu_decode_batch_device(bz_gpu_engine *g, const void *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                               void *d_out, size_t cap,
                               uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict);
/* The last bz_gpu_decode_batch_device call: [0] entries decoded by the batch path  [1] entries that took the
 * one-stream path  [2] blocks rebuilt for the entries of [0]  [3] groups. */
int bz_gpu_last_decode_batch_stats(bz_gpu_engine *g, uint64_t out[4]);

/* One-shot over host buffers: `in.iter().cloned().decode(&mut BZip2Decoder::new())`
 * collected until None or the first Err.  *out (malloc'ed, release with
 * bz_free) holds the bytes yielded before the verdict, also when that is an error.
 * 1 GiB of decoded bytes in 0.068 s (15.6 GB/s; rounds 1-4: 0.11 s) from the second call of a process on: the engine
 * and its workspace are kept between calls (bz_release_cached_resources), the bytes land once, in huge-page-backed memory,
 * sub-batch by sub-batch beside the kernels of the next one. */
int bz_decode_buffer(int device, const uint8_t *in, size_t in_len,
                     uint8_t **out, size_t *out_len);

/* The same for many independent streams (the host form of bz_gpu_decode_batch_device, mirroring bz_encode_batch):
 * entry i is bz_decode_buffer(device, ins[i], lens[i]) -- its bytes at *out + out_off[i] (out_len[i] of them), its
 * verdict in verdict[i]; the return value is the infrastructure status only.  The entries are packed at 4-byte-aligned
 * offsets, uploaded once and decoded on an engine of the decode cache; the bytes come down group by group into ONE
 * malloc'ed buffer (release with bz_free; offsets are multiples of 16, relative to it).  count == 0: BZ_OK, *out is an
 * empty buffer, no device is touched. */
int bz_decode_batch(int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                    uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict);

/* Streaming context == BZip2Decoder as the DecodeIterator drives it
 * (src/traits/decoder.rs:73-86): compressed bytes in (bz_dec_write), end of
 * the input iterator (bz_dec_end), decoded bytes out in order (bz_dec_read:
 * > 0 bytes copied; 0 = nothing ready yet; once the verdict is final and
 * nothing is left, the verdict -- 0 = `None`, negative = the `Err` item).
 * Decoding is incremental and runs BESIDE the caller, on a thread of the
 * context: whenever BZ_DEC_CHUNK bytes (environment; default 64 MiB, the first
 * chunk of a stream 16 MiB) have been written, the records that are wholly
 * there are decoded and their bytes queued as they land in host memory, and the
 * chain state (bit position, stream number, level, combined CRC) is carried to
 * the next chunk; chunks of less than 4 MiB are decoded before bz_dec_write
 * returns.  bz_dec_end hands over the rest and does not wait for the decode --
 * it returns the verdict if it is already final, else BZ_OK; like bz_dec_write
 * it waits only while two chunks are already queued, and for a last chunk of
 * less than 4 MiB, which is decoded inside the call -- and from then on
 * bz_dec_read WAITS for the next bytes or the final verdict instead of
 * answering "nothing yet" (a caller that polls between other work must not
 * call it behind bz_dec_end until it can afford to block): a consumer reads the
 * head of the file while its tail is being decoded (the verdict follows the
 * last byte, as the reference's iterator yields it).  INPUT memory is bounded
 * by the chunks in flight (three); decoded bytes wait in host segments until
 * they are read, without a limit -- a caller that writes a whole file before
 * its first read holds the whole decoded output (back-pressure on the worker
 * would dead-lock exactly that caller: its writes wait for the worker).
 * The reference decodes lazily block by block -- same items, coarser moments.
 * 1 GiB written in 1 MiB pieces and read in 4 MiB pieces: see bench.py
 * extra.decode.end_to_end.streaming (rounds 1-4, which decoded inside
 * bz_dec_write: 4.2 GB/s). */
typedef struct bz_dec bz_dec;
int bz_dec_create(bz_dec **out, int device);        /* BZip2Decoder::new, src/bzip2/decoder.rs:588-594 */
int bz_dec_write(bz_dec *d, const uint8_t *data, size_t n);
int bz_dec_end(bz_dec *d);
long bz_dec_read(bz_dec *d, uint8_t *out, size_t cap);
size_t bz_dec_pending(const bz_dec *d);
void bz_dec_destroy(bz_dec *d);

/* ========================================================================
 * 4. Deflate / zlib / gzip ENCODE
 *
 * Replaces `Inflater` (src/deflate/encoder.rs:92-260: LzssEncoder with window
 * 0x8000, matches 3..258, lazy level 3, hash chains of 255, src/lzss/encoder.rs,
 * src/lzss/slidedict.rs; blocks of <= 0xFFFF bytes, stored / fixed / dynamic
 * chosen by size, src/deflate/encoder.rs:454-547), `ZlibEncoder`
 * (src/zlib/encoder.rs:55-157: 78 DA, Adler-32 big endian) and `GZipEncoder`
 * (src/gzip/encoder.rs:50-135: 10-byte header, CRC-32 and ISIZE little endian),
 * driven with Action::Finish.  The stream is the reference's, bit for bit.
 * `kind`: 0 raw Deflate, 1 zlib, 2 gzip.
 * Action::Flush inside a stream is offered for Inflater through the streaming context (df_enc_end):
 * the stream becomes a sequence of byte-aligned segments (src/deflate/encoder.rs:170-195, :227-235,
 * :638-647).  The zlib / gzip wrappers end their container at the first None of their inner Inflater whatever
 * the Action (src/zlib/encoder.rs:138-150, src/gzip/encoder.rs:120-133): df_enc_end(Run) / (Flush) on kinds 1 / 2
 * write header + what the Inflater yields under that Action + trailer, and the context is finished.  Inputs of
 * any length: a call works through a long segment in parts of BZ_DF_PART_MIB (default 1024) MiB.
 * ======================================================================== */
#define DF_KIND_DEFLATE 0
#define DF_KIND_ZLIB 1
#define DF_KIND_GZIP 2

/* Upper bound of the stream length for n input bytes (every block stored). */
size_t df_encode_bound(size_t n);
/* d_in[n] (HBM, 4-byte aligned) -> d_out (HBM, cap bytes); *out_len = stream
 * bytes.  d_out == NULL: length only.  Uses the engine's stream; workspace
 * (about 20 bytes per input byte) is created by the first call and kept. */
int df_gpu_encode_device(bz_gpu_engine *g, int kind, const void *d_in, size_t n,
                         void *d_out, size_t cap, size_t *out_len);
/* The same with a preset dictionary == Inflater::with_dict / ZlibEncoder::with_dict
 * (src/deflate/encoder.rs:134-153, src/zlib/encoder.rs:74-93): `dict` is HOST
 * memory; its last 0x8000 bytes are the window in front of the input
 * (src/lzss/encoder.rs:104-130), the zlib header becomes 78 F9 + Adler-32 of the
 * whole dictionary.  kind 2 (gzip) has no with_dict: BZ_E_PARAM. */
int df_gpu_encode_device_dict(bz_gpu_engine *g, int kind, const void *d_in, size_t n,
                              const uint8_t *dict, size_t dict_len,
                              void *d_out, size_t cap, size_t *out_len);
/* Seconds of GPU time of the last call by stage (HIP events): [0] hash chains
 * (sort) [1] matches [2] parse [3] blocks + tables [4] emission + checksums [5] total. */
int df_gpu_last_timings(bz_gpu_engine *g, double out_seconds[6]);
/* [0] blocks [1] stored [2] fixed [3] dynamic [4] tables that took the
 * length-limited path [5] stream bytes [6] dynamic blocks without any match: for
 * those the reference writes HDIST = 0 and no distance code length
 * (src/deflate/encoder.rs:431-436, 449-451), which RFC 1951 decoders reject; the
 * stream is reproduced as the reference writes it and counted here */
int df_gpu_last_stats(bz_gpu_engine *g, uint64_t out[8]);
/* Test hooks: the LZSS codes of the last call in stream order as (len, pos)
 * pairs, len 0 = the literal `pos` (what LzssEncoder::next yields,
 * src/lzss/encoder.rs:203-234); per block (start offset, bytes, BTYPE, bits). */
int df_gpu_debug_codes(bz_gpu_engine *g, const void *d_in, size_t n,
                       uint32_t *out_pairs, size_t cap, size_t *count);
int df_gpu_debug_blocks(bz_gpu_engine *g, uint64_t *out4, size_t cap, size_t *count);

/* One-shot over host buffers: `in.iter().cloned().encode(&mut Inflater::new(),
 * Action::Finish)` collected (or ZlibEncoder / GZipEncoder).  *out is malloc'ed,
 * release with bz_free.  Inputs of 64 MiB and more are uploaded, encoded (in parts: 64 MiB, then 256 MiB each) and
 * downloaded side by side: 1 GiB in 0.079 s (13.6 GB/s); *out is then a buffer of the stream's upper bound in
 * huge-page-backed memory of which only the pages the stream fills have been touched. */
int df_encode_buffer(int kind, int device, const uint8_t *in, size_t in_len,
                     uint8_t **out, size_t *out_len);
int df_encode_buffer_dict(int kind, int device, const uint8_t *in, size_t in_len,
                          const uint8_t *dict, size_t dict_len,
                          uint8_t **out, size_t *out_len);

/* Many independent inputs, one stream each, in one call (the Deflate counterpart of bz_gpu_encode_batch_device).
 * Input i is the h_in_len[i] bytes at d_in + h_in_off[i]: d_in 16-byte aligned, every offset a multiple of 16, the ranges
 * ascending and disjoint; bytes outside the ranges are never read as part of any input.  Stream i -- the bytes of
 * df_gpu_encode_device(g, kind, d_in + h_in_off[i], h_in_len[i], ...), bit for bit -- is written at d_out + h_out_off[i]
 * (h_out_len[i] bytes): input order, each stream at a multiple of 4 bytes, zeros between them, nothing at or behind
 * d_out + cap.  One `kind` for the call.  Inputs of at most 0xFFFF bytes are exactly one Deflate block
 * (MAX_BLOCK_SIZE, src/deflate/encoder.rs:577-597) and are encoded together, whatever their number, in sub-batches of
 * BZ_DF_BATCH_MIB (default 64) MiB of 4 KiB-aligned slots: one pass of the pipeline, one host round trip and one placement
 * per sub-batch, the container checksums, headers and trailers written on the device.  Every other input takes the path
 * of df_gpu_encode_device, in its turn, inside the same call.  BZ_E_PARAM: kind outside 0..2, a null engine, a null array
 * with count > 0, a misaligned d_in or offset, ranges that overlap or are out of order; BZ_E_CAPACITY: cap too small
 * (df_encode_batch_bound always suffices: the sum of df_encode_bound, each rounded up to 4); count == 0: BZ_OK, nothing
 * touched.  BZ_DF_MATCH=walk and BZ_DF_PARSE=doubling do not apply to the batch path. */
size_t df_encode_batch_bound(const uint64_t *in_len, size_t count);
int df_gpu_encode_batch_device(bz_gpu_engine *g, int kind, const void *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                               void *d_out, size_t cap, uint64_t *h_out_off, uint64_t *h_out_len);
/* The last df_gpu_encode_batch_device call: [0] inputs taken by the batch path [1] inputs that took the one-input path
 * [2] sub-batches, and of the batch-path inputs' blocks [3] stored [4] fixed [5] dynamic [6] tables on the length-limited
 * path [7] dynamic blocks without any match (see df_gpu_last_stats [6]).  After such a call df_gpu_last_timings holds the
 * batch path's stages summed over the sub-batches. */
int df_gpu_last_batch_stats(bz_gpu_engine *g, uint64_t out[8]);
/* The host form (mirrors bz_encode_batch): the inputs are packed at 16-byte-aligned offsets, uploaded once, encoded by one
 * df_gpu_encode_batch_device call on an engine of the per-process cache and downloaded once.  Stream i is
 * (*out)[out_off[i] .. + out_len[i]); *out is one malloc'ed buffer, release with bz_free.  count == 0: BZ_OK, *out an
 * empty buffer, no device is touched. */
int df_encode_batch(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                    uint8_t **out, uint64_t *out_off, uint64_t *out_len);
/* The same with ONE preset dictionary for every input (`Inflater::with_dict` / `ZlibEncoder::with_dict`; dict is host
 * memory).  Stream i is, byte for byte, df_encode_buffer_dict(kind, input i, dict, dict_len): the last 32 768 bytes of the
 * dictionary are history in front of EVERY input; zlib (kind 1) writes the six-byte header 78 F9 + DICTID (the Adler-32 of the
 * whole dictionary), and its trailer covers the input alone.  dict_len == 0 is no dictionary: the calls above, same bytes
 * (they ARE these calls with (NULL, 0)).  BZ_E_PARAM: dict == NULL with dict_len > 0; kind 2 with dict_len > 0 (GZipEncoder
 * has no with_dict).  An input of at most 0xFFFF bytes is still exactly one block (the dictionary is history, not output,
 * src/deflate/encoder.rs:293-308) and takes the batch path: the dictionary's window lies in the sub-batch's image in front
 * of every slot, so a sub-batch of BZ_DF_BATCH_MIB holds up to 32 KiB less input per slot.  Layout of the output,
 * df_encode_batch_bound (its 64 bytes of slack per input cover the longer header), df_gpu_last_batch_stats: as above.
 * What df_gpu_encode_batch_device_dict writes is valid input of df_gpu_decode_batch_device_dict with the same offsets,
 * lengths and dictionary. */
int df_gpu_encode_batch_device_dict(bz_gpu_engine *g, int kind, const void *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                                    const uint8_t *dict, size_t dict_len,
                                    void *d_out, size_t cap, uint64_t *h_out_off, uint64_t *h_out_len);
int df_encode_batch_dict(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                         const uint8_t *dict, size_t dict_len,
                         uint8_t **out, uint64_t *out_off, uint64_t *out_len);

/* Streaming context == the Encoder::next contract of the three encoders:
 * df_enc_write feeds bytes, df_enc_end(action) marks the end of an input
 * iterator (0 Run, kind 0: nothing comes out yet -- the blocks the reference hands out while it
 * consumes input come with the next Flush / Finish, the bytes are the same;
 * 1 Flush: the bytes written since the last segment come out as one segment:
 * LZSS stage drained, current block closed without the final bit, padded to a byte, window and
 * decompress_len carried over; 2 Finish: the last segment, final bit, container trailer;
 * kinds 1 / 2 (ZlibEncoder / GZipEncoder): ANY action ends the container -- Run: header, the whole bytes of
 * the blocks the Inflater has closed with 261 bytes of look-ahead held back, trailer; Flush: header, the
 * flushed segment, trailer -- and the encoder is finished: later input is not even pulled
 * (src/zlib/encoder.rs:130-136)), df_enc_read drains.  The stream so far stays in device memory until the
 * context is finished.  df_enc_finished: 1 once the final block (kind 0) / the trailer (kinds 1, 2) is out. */
typedef struct df_enc df_enc;
int df_enc_create(df_enc **out, int kind, int device);
int df_enc_create_dict(df_enc **out, int kind, int device, const uint8_t *dict, size_t dict_len); /* ::with_dict */
int df_enc_write(df_enc *e, const uint8_t *in, size_t n);
int df_enc_end(df_enc *e, int action);
int df_enc_finished(const df_enc *e);
long df_enc_read(df_enc *e, uint8_t *out, size_t cap);
size_t df_enc_pending(const df_enc *e);
void df_enc_destroy(df_enc *e);

/* ========================================================================
 * 5. Deflate / zlib / gzip DECODE  ==  `Deflater`, `ZlibDecoder`, `GZipDecoder`
 *    (src/deflate/decoder.rs, src/zlib/decoder.rs, src/gzip/decoder.rs) on
 *    streams that are well-formed; RFC 1951 / 1950 / 1952 decide everywhere else.
 *
 * Many independent streams in one call, one wave per stream; an entry of
 * BZ_DF_INF_SPLIT_KIB KiB or more (default 1024, 0 = never; read per call) is
 * split: its compressed bytes are cut into pieces of BZ_DF_INF_PIECE_KIB KiB
 * (default 16: profiles/r14_inflate_split.md), a search finds a block header in every piece,
 * one wave decodes from each, and a chain keeps exactly the pieces that start
 * where the piece in front of them ended (DESIGN_deflate.md, "One large stream
 * across many waves").  A split entry gets the bytes, the length and the verdict
 * of the one-wave path under every clause of the contract below.  `kind` as in
 * section 4 (one kind per call; the _dict forms take one preset dictionary for
 * every entry of the call: clause (c)).
 *
 * THE CONTRACT (DESIGN_deflate.md, "Decoding many streams in one call", says why
 * the reference's decoder cannot be the standard on malformed input):
 * (a) a stream that is well-formed under RFC 1951 (kind 1: inside an RFC 1950
 *     container, kind 2: an RFC 1952 member) gets BZ_OK and its bytes -- what
 *     zlib's inflate yields for it.  Bytes behind the end of the stream or its
 *     trailer are ignored, and only the first gzip member is decoded
 *     (section 6 decodes every member).
 * (b) every other entry gets an error verdict and the bytes produced in front of
 *     the failing code or block header.  BZ_E_EOF: the entry ends before the
 *     final block's end-of-block code (kinds 1 / 2: before the trailer is
 *     complete, or inside the container header: no bytes).  BZ_E_DATA: BTYPE 3; a
 *     stored block with LEN ^ NLEN != 0xFFFF; more than 286 literal/length or 30
 *     distance code lengths; a repeat code 16 with nothing in front of it; a run
 *     past HLIT + HDIST; an over-subscribed code-length set; an incomplete one
 *     (accepted: no distance code at all, and exactly one distance code of
 *     length 1); no end-of-block code; a length symbol 286 / 287; a distance
 *     symbol 30 / 31; a distance that reaches in front of the entry's output; a
 *     container header the reference rejects (zlib: CM != 8, CINFO > 7, FCHECK;
 *     gzip: ID1, ID2, CM != 8, a reserved FLG bit, a wrong header CRC); FDICT
 *     set; a wrong Adler-32; a wrong CRC-32 or ISIZE -- with a wrong trailer
 *     value all bytes have been produced and h_out_len is the full length.
 *     A failure that only the zero bits behind the entry's end made possible is
 *     BZ_E_EOF, never BZ_E_DATA.  A stored block that the entry's end cuts short
 *     yields none of its bytes.
 * (c) WITH A PRESET DICTIONARY (the _dict forms; `Deflater::with_dict`,
 *     `ZlibDecoder::with_dict`, src/deflate/decoder.rs:358-404,
 *     src/zlib/decoder.rs:32-39, 66-101) every clause above holds, and:
 *     dict_len == 0 is exactly the call without one, whatever `dict` is: FDICT
 *     stays BZ_E_DATA.  (As the encoder, where an empty dictionary writes 78 DA;
 *     a deliberate difference from the reference's with_dict(b""), which wants
 *     FDICT and the DICTID 1.)  dict == NULL with dict_len > 0, and kind 2 with
 *     dict_len > 0 (GZipDecoder has no with_dict), are BZ_E_PARAM; the host forms
 *     return them before any device is touched.  `dict` is HOST memory; one
 *     dictionary serves every entry; its last W = min(dict_len, 32768) bytes are
 *     uploaded once per call, and they are history in front of position 0 of every
 *     entry's output.
 *     kind 0: a distance d at output position p is valid iff d <= p + W; d > p + W
 *     is BZ_E_DATA with the bytes in front of the failing code.  Source byte
 *     q = p - d + i (p - d + i % d for d < length) with q < 0 is window byte
 *     W + q.  A wrong dictionary of the same length cannot be detected: BZ_OK with
 *     the bytes that dictionary gives.  zlib's decompressobj(-15, zdict=dict) is
 *     the arbiter.
 *     kind 1: the header is the reference's.  CMF and FLG: fewer than 2 bytes is
 *     BZ_E_EOF.  FDICT clear is BZ_E_DATA with no bytes (the reference refuses it;
 *     zlib would ignore the dictionary).  FDICT set: the header is six bytes, and
 *     fewer than six in the entry is BZ_E_EOF with no bytes even when CM, CINFO or
 *     FCHECK are wrong already; with all six present CM != 8, CINFO > 7, FCHECK,
 *     or a DICTID (big endian) that is not the Adler-32 of the WHOLE dictionary is
 *     BZ_E_DATA with no bytes.  Behind the header the body is decoded as kind 0
 *     with the window; the trailer's Adler-32 covers the output bytes only.
 *     The bits and "compressed bytes consumed" of an entry include the six header
 *     bytes.  No byte of the dictionary is ever written to d_out; placement, cap,
 *     the sizes-only call, the isolation of the entries' verdicts and "nothing
 *     outside the reported ranges is written" hold as they are.
 * ======================================================================== */

/* Entry i is the h_in_len[i] bytes at d_in + h_in_off[i]: d_in 16-byte aligned, every offset a multiple of 4, the ranges
 * ascending and disjoint, each shorter than 4 GiB -- exactly what df_gpu_encode_batch_device writes: its (d_out, h_out_off,
 * h_out_len) go in unchanged.  No bit outside an entry's range influences that entry, and nothing at or behind the end of
 * the last range is read (an entry's last, partial 4-byte word is read byte by byte).
 * Entry i's bytes go to d_out + h_out_off[i] (h_out_len[i] of them): input order, every offset a multiple of 16 (d_out
 * itself 16-byte aligned), the ranges disjoint -- valid input of df_gpu_encode_batch_device and
 * bz_gpu_encode_batch_device.  NOTHING outside the reported ranges is written: the bytes between them, and everything at
 * or behind d_out + cap, keep what they held.  h_verdict[i] is BZ_OK, BZ_E_DATA or BZ_E_EOF (CompressionError::DataError /
 * UnexpectedEof); no entry's verdict or bytes change another entry's.  The RETURN VALUE is the infrastructure status only:
 * BZ_OK also when entries carry errors.  The five arrays are HOST arrays of `count` entries.
 * Two launches: the first decodes every entry and writes only its length and verdict; the host places the outputs (one
 * round trip, in which cap is checked: BZ_E_CAPACITY leaves d_out untouched); the second decodes again and writes.
 * Kinds 1 / 2: a third kernel sums the decoded bytes and compares with the trailers.
 * d_out == NULL: sizes only -- the offsets, lengths and verdicts of the real call, except that Adler-32, CRC-32 and ISIZE
 * are not looked at (such an entry is BZ_OK here); the capacity the real call needs is the largest h_out_off[i] +
 * h_out_len[i].  Positions inside an entry are 32-bit: an entry whose output would reach 4 GiB makes the call return
 * BZ_E_PARAM.  BZ_E_PARAM also: kind outside 0..2, a null engine, a null array with count > 0, a misaligned d_in, d_out or
 * offset, ranges that overlap or are out of order.  count == 0: BZ_OK, nothing touched.
 * Afterwards df_gpu_last_timings holds [0] the sizes launch [1] the writing launch [2] the checksum kernel [5] their sum. */
int df_gpu_decode_batch_device(bz_gpu_engine *g, int kind, const void *d_in,
                               const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                               void *d_out, size_t cap,
                               uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict);
/* ... with a preset dictionary (clause (c)); df_gpu_decode_batch_device is this call with (NULL, 0). */
int df_gpu_decode_batch_device_dict(bz_gpu_engine *g, int kind, const void *d_in,
                                    const uint64_t *h_in_off, const uint64_t *h_in_len, size_t count,
                                    const uint8_t *dict, size_t dict_len,
                                    void *d_out, size_t cap,
                                    uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict);
/* The last df_gpu_decode_batch_device call: [0] entries decoded clean [1] entries with an error verdict, and of the
 * blocks decoded whole [2] stored [3] fixed [4] dynamic; [5] decoded bytes [6] compressed bytes consumed (to the end of
 * the stream or trailer, or to the failing code) [7] kernel launches. */
int df_gpu_last_decode_batch_stats(bz_gpu_engine *g, uint64_t out[8]);
/* The split entries of the last df_gpu_decode_batch_device call: [0] entries split [1] pieces with a candidate [2] pieces
 * confirmed without repair (every entry's first piece is one) [3] repair rounds [4] output bytes decoded by the serial tail
 * [5] bytes the writing launch left unresolved (their value lies in an earlier piece) [6] jump rounds [7] kernel launches
 * of the split entries (not counted in df_gpu_last_decode_batch_stats [7]).  df_gpu_last_timings [0] / [1] / [2] include
 * their search, sizes and repair / writing, jump rounds and gather / checksum. */
int df_gpu_last_decode_split_stats(bz_gpu_engine *g, uint64_t out[8]);
/* ... and their phases in seconds, summed over the split entries (a host clock around launches that are waited for):
 * [0] search [1] sizes [2] chain and repair [3] writing [4] jump rounds [5] gather [6] checksum. */
int df_gpu_last_decode_split_timings(bz_gpu_engine *g, double out_seconds[7]);
/* The host form (mirrors bz_decode_batch): the entries are packed at 4-byte-aligned offsets, uploaded once and decoded by
 * one device call on an engine of the per-process cache; entry i's bytes are (*out)[out_off[i] .. + out_len[i]), its
 * verdict verdict[i]; *out is ONE malloc'ed buffer (release with bz_free; offsets are multiples of 16, relative to it).
 * count == 0: BZ_OK, *out an empty buffer, no device is touched.  Without a GPU: BZ_E_NOGPU (there is no CPU path). */
int df_decode_batch(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                    uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict);
/* The batch of one == `in.iter().cloned().decode(&mut Deflater::new())` (ZlibDecoder / GZipDecoder) collected until None
 * or the first Err under the contract above: returns BZ_OK with the bytes, or the verdict with the bytes in front of it
 * (as bz_decode_buffer does). */
int df_decode_buffer(int kind, int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len);
/* The two host forms with a preset dictionary (clause (c)) == `Deflater::with_dict(dict)` / `ZlibDecoder::with_dict(dict)`;
 * df_decode_batch and df_decode_buffer are these calls with (NULL, 0). */
int df_decode_batch_dict(int kind, int device, const uint8_t *const *ins, const size_t *lens, size_t count,
                         const uint8_t *dict, size_t dict_len,
                         uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict);
int df_decode_buffer_dict(int kind, int device, const uint8_t *in, size_t in_len,
                          const uint8_t *dict, size_t dict_len, uint8_t **out, size_t *out_len);

/* ========================================================================
 * 6. EVERY MEMBER of a gzip file (RFC 1952 section 2.2: a file is a series of
 *    members) -- what gzip(1), Python's gzip.decompress and flate2's
 *    MultiGzDecoder yield: BGZF (.bam, .vcf.gz), `cat a.gz b.gz`, pigz -i.
 *    Section 5 and DF_KIND_GZIP keep decoding the first member only, as the
 *    reference's GZipDecoder does (src/gzip/decoder.rs:204-216).
 *
 * THE CONTRACT.  The stream's bytes and verdict are those of this loop over the
 * one-member contract of section 5 (zlib is the arbiter of each member):
 *
 *     pos = 0
 *     repeat:
 *         skip zero bytes at pos          (zero padding between and behind members)
 *         if pos == len: BZ_OK, stop      (a file of no bytes, or of zeros only: BZ_OK, no bytes)
 *         decode ONE member from the bytes [pos, len) under section 5, kind 2
 *         append its bytes                (the bytes in front of the fault, if it fails)
 *         if its verdict is not BZ_OK: that is the stream's verdict, stop
 *         pos = the byte behind its trailer
 *
 * So: junk behind a member that is neither zeros nor a valid header is
 * BZ_E_DATA, with every byte of the members in front of it; a file cut inside a
 * later member's header, body or trailer is BZ_E_EOF with the bytes in front of
 * the cut; a wrong CRC-32 or ISIZE in member k is BZ_E_DATA with all of member
 * k's bytes and nothing of member k + 1; an empty member (BGZF's 28-byte EOF
 * marker) contributes no bytes; a truncated member followed by an intact one is
 * decoded on into the bytes of the next (the loop knows no other end of a
 * member).  Input of 4 GiB or more is BZ_E_PARAM, as is a member whose output
 * would reach 4 GiB; the output length is summed in 64 bits.
 *
 * HOW (DESIGN_deflate.md, "Every member of a gzip file").  A search lists every
 * position that holds 1f 8b 08 and a FLG byte without reserved bits (a
 * CANDIDATE: every member starts at one, but a stored block may hold some too).
 * The spans between candidates are decoded as one batch by the kernels of
 * section 5, BZ_DF_GZ_BATCH candidates (default 16384) per launch; a walk keeps
 * the candidates at which the member in front ended (zeros skipped), and decodes
 * a member that a false candidate cut short again over 1, 2, 4, ... candidates
 * more.  Speculation may cost time, never a byte.  Members of
 * BZ_DF_INF_SPLIT_KIB or more go across many waves as in section 5.
 * ======================================================================== */

/* d_in[in_len] (HBM, 16-byte aligned; nothing at or behind d_in + in_len is read) -> the members' bytes side by side at
 * d_out (any alignment): *out_len bytes, *verdict BZ_OK, BZ_E_DATA or BZ_E_EOF.  NOTHING at or behind d_out + *out_len is
 * written.  The RETURN VALUE is the infrastructure status only: BZ_OK also when the stream carries an error.
 * Two passes: the first finds the members and their lengths; cap is then checked (BZ_E_CAPACITY leaves d_out untouched,
 * *out_len holds the capacity needed); the second decodes the members into a buffer of the engine, compares CRC-32 and
 * ISIZE, and copies the bytes up to the first member that is not clean into d_out.
 * d_out == NULL: sizes only -- the trailers are not looked at, so *out_len is the capacity the real call needs (and its
 * *out_len, unless a trailer value is wrong).  BZ_E_PARAM: a null engine or result pointer, d_in null with in_len > 0
 * or misaligned, in_len >= 4 GiB.  Afterwards df_gpu_last_timings holds [0] sizes [1] writing [2] checksums [3] search,
 * gather and zero skip [4] compaction [5] their sum, and df_gpu_last_decode_batch_stats / _split_stats describe the members. */
int df_gpu_decode_members_device(bz_gpu_engine *g, const void *d_in, size_t in_len,
                                 void *d_out, size_t cap, uint64_t *out_len, int32_t *verdict);
/* The last df_gpu_decode_members_device call: [0] members decoded, the first that is not clean included (sizes only: members
 * found, trailers not looked at) [1] candidates found [2] candidates never confirmed
 * [3] decodes of a member again after a span extension [4] zero bytes skipped [5] members that took the split path
 * [6] sub-batches of candidates [7] launches of the kernels of this section (search, gather, zero skip, compaction). */
int df_gpu_last_decode_members_stats(bz_gpu_engine *g, uint64_t out[8]);
/* ... and the stages of this section in seconds (a host clock around launches that are waited for): [0] search
 * [1] gather [2] zero skip [3] compaction. */
int df_gpu_last_decode_members_timings(bz_gpu_engine *g, double out_seconds[4]);
/* Host to host: one upload, one device call on an engine of the per-process cache, one download.  Returns BZ_OK with the
 * bytes, or the stream's verdict with the bytes in front of it (as df_decode_buffer does); *out is malloc'ed, release
 * with bz_free.  in_len == 0: BZ_OK, an empty buffer, no device is touched.  Without a GPU: BZ_E_NOGPU. */
int df_decode_members_buffer(int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len);

/* ========================================================================
 * 7. WRITING BGZF (the blocked gzip of .bam, .vcf.gz and bgzip; SAM
 *    specification section 4.1): one contiguous input as a series of gzip
 *    members of at most 65 280 input bytes each -- the file that section 6
 *    decodes member-parallel and that htslib seeks in.  The reference has no
 *    such writer; its GZipEncoder (section 4) writes one member.
 *
 * THE FILE.  With B = block_bytes (0 means DF_BGZF_BLOCK; any value from 1 to
 * 65 280, not only multiples of 16), block k holds the input bytes
 * [k * B, min(n, (k + 1) * B)).  The file is the blocks in order, byte against
 * byte, no padding; with eof != 0 the standard 28-byte EOF marker follows
 * (1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 and eight zero
 * bytes).  n == 0 writes the marker alone, or nothing.
 *
 * A BLOCK is the 18-byte header 1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6,
 * 42 43 02 00, BSIZE = block length - 1 (little-endian u16); then ONE final
 * Deflate block; then CRC-32 and ISIZE of the block's input, little endian.
 * The Deflate block is, bit for bit, the reference's one-block stream of that
 * input alone (section 4, kind 0: window, chains and matches inside the block,
 * as in the batch path) with one exception, THE STRICT RULE: where the reference
 * chooses a dynamic block although the block has no match, it writes HDIST = 0
 * and no distance code length (df_gpu_last_stats [6]), which zlib and section 5
 * refuse.  Such a block -- literals only -- is written stored if
 * 8 * len + 34 <= fixed, otherwise fixed, where fixed = 2 + the fixed code lengths
 * of its literals + 7 for the end-of-block code.  Every Deflate block is at most
 * len + 5 bytes, so a block is at most len + 31 bytes and BSIZE fits.
 * ======================================================================== */
#define DF_BGZF_BLOCK 65280u          /* htslib's block size, the default and the maximum */
size_t df_bgzf_block_count(size_t n, uint32_t block_bytes);      /* ceil(n / B); 0 for n == 0 */
size_t df_bgzf_bound(size_t n, uint32_t block_bytes, int eof);   /* n + 31 * count + (eof ? 28 : 0) */
/* d_in[n] (HBM, 16-byte aligned; nothing at or behind d_in + n is read) -> the file at d_out (HBM, any alignment):
 * *out_len bytes.  h_block_off, when not NULL, receives count + 1 file offsets: entry k is where block k starts, the last
 * one where the EOF marker starts (*out_len when there is none) -- with k * B beside it the .gzi table, and the coffset
 * half of a virtual offset.  The blocks go through the batch pipeline of section 4 in sub-batches of BZ_DF_BATCH_MIB
 * (default 64 MiB of 4 KiB-aligned slots: 1 024 blocks of 65 280 bytes), each placed at the running byte total; n is a
 * size_t and the offsets are 64-bit.  BZ_E_PARAM: a null engine or out_len, d_in null with n > 0 or not 16-byte aligned,
 * block_bytes > 65 280; BZ_E_CAPACITY: the file does not fit in cap (df_bgzf_bound always suffices).  Nothing at or
 * behind d_out + cap is ever written, and on success nothing at or behind d_out + *out_len. */
int df_gpu_bgzf_encode_device(bz_gpu_engine *g, const void *d_in, size_t n, uint32_t block_bytes, int eof,
                              void *d_out, size_t cap, uint64_t *out_len, uint64_t *h_block_off);
/* The last df_gpu_bgzf_encode_device call: [0] blocks (the marker not counted) [1] sub-batches, and of the blocks
 * [2] stored [3] fixed [4] dynamic [5] tables on the length-limited path [6] blocks the strict rule replaced
 * [7] file bytes.  After such a call df_gpu_last_timings holds the stages summed over the sub-batches. */
int df_gpu_last_bgzf_stats(bz_gpu_engine *g, uint64_t out[8]);
/* Host to host: one upload, one device call on an engine of the per-process cache, one download; *out is malloc'ed,
 * release with bz_free; block_off (may be NULL) as h_block_off above.  The parameters are checked before any device is
 * touched (BZ_E_PARAM: a null out or out_len, in null with n > 0, block_bytes > 65 280), then BZ_E_NOGPU without a
 * GPU.  n == 0: BZ_OK with the marker or an empty buffer, no device is touched. */
int df_bgzf_encode_buffer(int device, const uint8_t *in, size_t n, uint32_t block_bytes, int eof,
                          uint8_t **out, size_t *out_len, uint64_t *block_off);

/* ========================================================================
 * 8. READING BGZF: the block index from BSIZE, range reads, one decode pass
 *    (DESIGN_deflate.md, "Reading BGZF").  Section 6 reads such a file as an
 *    anonymous run of gzip members: it guesses the starts, decodes every member
 *    twice and copies its bytes into place, and it reads the whole file.  A
 *    BGZF block says what that path has to find out: BSIZE is its length, ISIZE
 *    its output's length, so every block's place in the output is a prefix sum
 *    known before the first bit is decoded.
 *
 * A BLOCK HEADER at byte p is htslib's rule with FLG exact: in[p .. p + 16) ==
 * 1f 8b 08 04 ?? ?? ?? ?? ?? ?? 06 00 42 43 02 00 -- MTIME, XFL and OS may be
 * anything, FLG is exactly 4, XLEN exactly 6 with the BC subfield first and
 * alone.  BSIZE = u16 at p + 16, the block is BSIZE + 1 bytes, ISIZE = u32 in
 * its last four bytes.  A gzip file whose members carry other extra subfields
 * is legal gzip, and legal by the letter of the SAM specification; htslib does
 * not read it and neither does this section: such a file goes through section 6.
 *
 * THE CHAIN, from pos = 0, upos = 0, over a file of len bytes:
 *
 *     repeat:
 *         if pos == len: BZ_OK, stop
 *         if len - pos < 18: BZ_E_EOF, stop              (a cut header, whatever its bytes are)
 *         if the header rule fails at pos: BZ_E_DATA, stop
 *         if BSIZE + 1 < 28: BZ_E_DATA, stop             (18 + a 2-byte empty final block + 8)
 *         if pos + BSIZE + 1 > len: BZ_E_EOF, stop
 *         if ISIZE > 65536: BZ_E_DATA, stop
 *         record block (coff = pos, uoff = upos); pos += BSIZE + 1; upos += ISIZE
 *
 * Zero padding is NOT skipped (htslib does not skip it; section 6 does).  THE
 * INDEX is count + 1 pairs (coff[k], uoff[k]); the last pair is the end of the
 * last complete block; on an error verdict the blocks in front of the fault
 * are still indexed.  The 28-byte EOF marker is an ordinary block with ISIZE 0.
 * The two arrays ARE the .gzi table (files of that layout are not read or
 * written here).
 *
 * A BLOCK IS CLEAN iff its Deflate bytes [coff[k] + 18, coff[k + 1] - 8) decode
 * under section 5, kind 0, with NO history in front of the block (a distance
 * that reaches in front of the block's first byte is a fault although, written
 * in place, the previous block's bytes lie right there), produce exactly ISIZE
 * bytes, end in the byte in front of the trailer, and the CRC-32 of the output
 * is the trailer's.  Every fault inside a block is BZ_E_DATA, running out of
 * bits included: the cut is BSIZE's, not the file's end.  BZ_E_EOF comes from
 * the index calls only.
 *
 * So every file this section reads with BZ_OK yields, over [0, total), exactly
 * the bytes of section 6 and of Python's gzip.decompress.  On faulty files the
 * two sections may differ, deliberately in two places: a trailer fault in
 * block k delivers nothing of block k here (section 6 delivers all of member
 * k), and zeros between blocks are an error here.
 *
 * WHAT A RANGE READ IS WORTH.  One wave decodes one block; a 64 KiB block takes
 * milliseconds on the device whatever surrounds it.  Range reads pay off for
 * ranges of many blocks (a region of tens of MiB of a large file), not for one
 * record.  Figures: profiles/r22_bgzf_read.md.
 * ======================================================================== */

/* The chain on the HOST, over host memory (sixteen thousand steps per GiB).  This is parsing, not decoding: it touches no
 * device and works without a GPU -- the one exception to "there is no CPU path".  *coff and *uoff are malloc'ed arrays of
 * *count + 1 entries, release each with bz_free; *verdict is the chain's (BZ_OK, BZ_E_DATA, BZ_E_EOF).  The return value is
 * the infrastructure status only.  BZ_E_PARAM: a null result pointer, in null with in_len > 0. */
int df_bgzf_index_buffer(const uint8_t *in, size_t in_len, uint64_t **coff, uint64_t **uoff, size_t *count, int32_t *verdict);
/* The same index for a file in HBM (d_in 16-byte aligned; nothing at or behind d_in + in_len is read).  h_coff and h_uoff are
 * HOST arrays with room for cap_blocks + 1 entries; BZ_E_CAPACITY with *count set when cap_blocks is too small (cap_blocks
 * == 0 with null arrays asks for the count).  A search lists every position that satisfies the 16-byte header rule with at
 * least 18 bytes behind it (ascending, 64-bit positions, tiles of 4 096 positions, count then scatter), a second kernel
 * fetches BSIZE, and ISIZE where the block fits, per candidate, and the host walks the chain over the list: a chain
 * position that is not in the list is a header-rule failure; false candidates (a stored block whose payload is a BGZF
 * file) are never landed on and cost nothing.  The list is handled in windows of BZ_DF_BGZF_BATCH candidates (environment;
 * default 65 536, read per call). */
int df_gpu_bgzf_index_device(bz_gpu_engine *g, const void *d_in, size_t in_len, uint64_t *h_coff, uint64_t *h_uoff,
                             size_t cap_blocks, size_t *count, int32_t *verdict);
/* The uncompressed bytes [ustart, min(ustart + ulen, uoff[count])) at d_out (any alignment).  Only the blocks that the range
 * touches are decoded: from the block that holds its first byte to the block that holds its last, empty blocks between
 * them included.  The blocks that lie whole inside the range are decoded by ONE launch, one wave per block, straight to
 * d_out + (uoff[k] - ustart); the at most two blocks the range cuts are decoded in the same launch into two 64 KiB slots
 * of the engine's workspace and their slices copied out; a second kernel compares the CRC-32s.  Blocks go to the launch in
 * groups of at most BZ_DF_BGZF_BATCH.
 * THE INDEX is the caller's -- from either index call, from df_gpu_bgzf_encode_device's h_block_off with k * B beside it, or
 * from a .gzi -- count + 1 entries per array; coff is relative to d_in (16-byte aligned), coff[0] need not be 0 and uoff[0]
 * need not be 0 (ustart counts in the same coordinates).  It is checked where it is used: for every block k touched the
 * header rule holds at coff[k], coff[k + 1] - coff[k] == BSIZE + 1 and uoff[k + 1] - uoff[k] == ISIZE, else BZ_E_DATA at
 * block k.  BZ_E_PARAM: a null engine, index, out_len or verdict; d_in misaligned, or null with in_len > 0; arrays that are
 * not ascending (coff strictly); coff[count] > in_len; ustart < uoff[0]; a block longer than 65 536 bytes either way.
 * RESULT.  The return value is the infrastructure status.  *verdict BZ_OK: *out_len is the range's length.  BZ_E_DATA:
 * *out_len is the range's bytes in front of the first faulty block (the lowest k).  Decided before any write: d_out ==
 * NULL gives sizes only (*out_len is the range's length, no kernel is launched); BZ_E_CAPACITY when cap is below the
 * range's length (*out_len holds it), d_out untouched.  ulen == 0 or ustart >= uoff[count]: BZ_OK, no bytes, no launch.
 * THE PRICE OF ONE PASS: on an error verdict the bytes of d_out in [*out_len, range length) are UNSPECIFIED.  Nothing at or
 * behind d_out + range length is ever written, and a block's stores are clipped to its own [uoff[k], uoff[k + 1]).
 * Afterwards df_gpu_last_timings holds [0] search and chain of the last index call [1] decode [2] checksums [3] edge copy
 * [5] their sum. */
int df_gpu_bgzf_read_device(bz_gpu_engine *g, const void *d_in, size_t in_len, const uint64_t *h_coff, const uint64_t *h_uoff,
                            size_t count, uint64_t ustart, uint64_t ulen, void *d_out, size_t cap, uint64_t *out_len,
                            int32_t *verdict);
/* The last df_gpu_bgzf_read_device call: [0] blocks decoded [1] of them written in place [2] edge blocks through the workspace
 * [5] bytes decoded [6] bytes delivered [7] kernel launches; and the last df_gpu_bgzf_index_device call: [3] candidates found
 * [4] candidates never landed on. */
int df_gpu_last_bgzf_read_stats(bz_gpu_engine *g, uint64_t out[8]);
/* Host to host: the index is built on the host, only the compressed bytes of the blocks touched are uploaded, one device
 * call on an engine of the per-process cache, one download; *out is malloc'ed, release with bz_free.  Returns BZ_OK with the
 * bytes, or the verdict with the bytes in front of it (as df_decode_members_buffer does): an index verdict of BZ_E_EOF or
 * BZ_E_DATA in front of or inside the range is the call's verdict, with the bytes of the range that lie in clean indexed
 * blocks in front of it.  ulen = UINT64_MAX reads to the end.  The parameters are checked before any device is touched
 * (BZ_E_PARAM: a null out or out_len, in null with in_len > 0); in_len == 0 or a range without bytes: an empty buffer, no
 * device.  Without a GPU: BZ_E_NOGPU. */
int df_bgzf_read_buffer(int device, const uint8_t *in, size_t in_len, uint64_t ustart, uint64_t ulen,
                        uint8_t **out, size_t *out_len);

/* ========================================================================
 * 9. LZHUF DECODE  ==  `LzhufDecoder` with `LzhufMethod::{Lh4, Lh5, Lh6, Lh7}`
 *    (src/lzhuf/decoder.rs; the LHA methods -lh4- .. -lh7-) on the streams
 *    `LzhufEncoder` writes; the contract below decides everywhere else.
 *
 * Many independent streams in one call, one wave per stream (k_lzhuf.hip;
 * DESIGN_lzhuf.md has the stream format and the reasons).  One method per call:
 *   method            BZ_LZH_LH4  BZ_LZH_LH5  BZ_LZH_LH6  BZ_LZH_LH7
 *   dictionary_bits       12          13          15          16
 *   offset_bits            4           4           5           5
 * The window is 1 << dictionary_bits bytes.
 *
 * THE CONTRACT.  The reference's decoder cannot be the standard on anything but
 * its encoder's streams: it pads the input with zero bits, accepts runs that
 * pass a table's count, reads distances out of a 64 KiB ring nobody wrote, and
 * builds a table from any lengths below 32.
 * (a) THE END.  The format has no end marker.  At a block boundary the stream
 *     ends with BZ_OK when fewer than 16 bits of the entry remain
 *     (decoder.rs:221-237) or when the 16-bit block length is 0; bytes behind
 *     that end are ignored.  An empty entry is BZ_OK without bytes.  So an entry
 *     cut exactly at a block boundary is a clean, shorter stream: only a known
 *     original length (b) can tell.
 * (b) A KNOWN ORIGINAL LENGTH (what an LHA member header carries): h_orig_len
 *     (NULL: no entry has one; an entry of UINT64_MAX: not this one).  With a
 *     length L decoding ends with BZ_OK as soon as L bytes exist: a match that
 *     crosses L is cut at it, nothing behind the code that reached L is read,
 *     L == 0 reads nothing.  When the end (a) comes with fewer than L bytes the
 *     verdict is BZ_E_EOF with the bytes produced.
 * (c) BZ_E_EOF: a field or a code, in a block header or among a block's codes,
 *     uses a bit behind the entry's end.  Every failure that only the zero bits
 *     behind the end made possible is BZ_E_EOF, never BZ_E_DATA (section 5 (b)).
 * (d) BZ_E_DATA, with the bytes in front of the failing code or block header:
 *     a t-count above 19; a skip field that runs past the t-count; a c-count
 *     above 510; a zero run that runs past the c-count (a constant t-code 1 or 2
 *     that does not meet the count exactly is this case); a p-count above
 *     dictionary_bits + 1; a constant t-symbol above 18, c-symbol above 509 or
 *     p-symbol above dictionary_bits; any code length above 16; an explicit
 *     length set whose Kraft sum is not exactly 1 (an all-zero set and a single
 *     code of length 1 included: the encoder writes a lone symbol in the
 *     constant form only); a distance greater than the bytes produced so far
 *     when prefill < 0; a distance greater than 1 << dictionary_bits, always
 *     (the p-count rule already keeps every distance inside the window).
 * (e) PREFILL.  -1: strict, as above.  0 .. 255: every byte in front of position
 *     0 of an entry's output has that value, so any distance up to the window is
 *     valid at any position.  No address in front of the entry's output is ever
 *     formed.  (The reference's ring reads 0 there; LHA's decoders fill their
 *     window with 0x20.)
 * (f) Placement, isolation, capacity and parameter errors are section 5's: d_in
 *     16-byte aligned, input offsets multiples of 4, the ranges ascending and
 *     disjoint, each shorter than 4 GiB; no byte at or behind the end of an
 *     entry's range is read (its last, partial word byte by byte); output offsets
 *     multiples of 16 in input order; NOTHING outside the reported ranges is
 *     written; no entry's verdict or bytes change another's; the return value is
 *     the infrastructure status.  Two launches: sizes, then (cap checked:
 *     BZ_E_CAPACITY leaves d_out untouched) the bytes.  d_out == NULL: sizes
 *     only.  An entry whose output would reach 4 GiB makes the call return
 *     BZ_E_PARAM (a block of constant codes makes 16 MiB from a few bytes).
 *     BZ_E_PARAM also: a method outside 4..7, a prefill outside -1..255, a null
 *     engine, a null array (h_orig_len excepted) with count > 0, a misaligned
 *     d_in, d_out or offset.  count == 0: BZ_OK, nothing touched.
 * (g) ONE LARGE ENTRY ACROSS MANY WAVES.  An entry of BZ_LZH_SPLIT_KIB KiB of
 *     compressed bytes or more (default 1024; 0: never; read per call) is
 *     decoded by one wave per block: every bit position that holds a whole
 *     block header valid under (d) and inside the entry is a candidate, every
 *     candidate is decoded, and the walk from bit 0 keeps the pieces that start
 *     where the piece in front of them stopped (DESIGN_lzhuf.md section 11).
 *     Such an entry obeys (a) to (f) clause by clause: its bytes, length,
 *     verdict and its share of bz_gpu_last_lzh_decode_stats [0..6] are those
 *     of the one-wave path, which it takes after all when its chain has fewer
 *     than two pieces, when it holds more than max(64, in_len /
 *     BZ_LZH_SPLIT_CAND_BYTES) candidates (default 1024) or when the source
 *     map (4 bytes per output byte, for the length of the call) cannot be had.
 * ======================================================================== */
#define BZ_LZH_LH4 4
#define BZ_LZH_LH5 5
#define BZ_LZH_LH6 6
#define BZ_LZH_LH7 7
int bz_gpu_lzh_decode_batch_device(bz_gpu_engine *g, int method, int prefill, const void *d_in,
                                   const uint64_t *h_in_off, const uint64_t *h_in_len, const uint64_t *h_orig_len, size_t count,
                                   void *d_out, size_t cap, uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict);
/* The last bz_gpu_lzh_decode_batch_device call: [0] entries decoded clean [1] entries with an error verdict [2] blocks
 * decoded whole (all their codes) [3] literal codes [4] match codes (one cut by the original length included) [5] decoded
 * bytes [6] compressed bytes consumed by the clean entries (to the end (a), the zero length included, or to the code that
 * completed the original length) [7] kernel launches. */
int bz_gpu_last_lzh_decode_stats(bz_gpu_engine *g, uint64_t out[8]);
/* The split entries (g) of the last call: [0] entries split [1] candidates [2] pieces in chains [3] false pieces (decoded,
 * not in a chain) [4] pieces decoded again with their place known [5] jump rounds [6] bytes filled by the gather (their value
 * lay in an earlier piece) [7] fallbacks to the one-wave path. */
int bz_gpu_last_lzh_decode_split_stats(bz_gpu_engine *g, uint64_t out[8]);
/* Seconds of the last call's split entries in: [0] search [1] sizes launch [2] chain and pieces decoded again [3] writing
 * launch [4] jump rounds [5] gather. */
int bz_gpu_last_lzh_decode_split_timings(bz_gpu_engine *g, double out_seconds[6]);
/* The host form (mirrors df_decode_batch): the entries packed at 4-byte-aligned offsets, one upload, one device call on an
 * engine of the per-process cache, one download; *out is ONE malloc'ed buffer (bz_free), entry i at out_off[i] (multiples
 * of 16).  orig_lens as h_orig_len.  The parameters are checked before any device is touched; count == 0: BZ_OK, an empty
 * buffer, no device.  Without a GPU: BZ_E_NOGPU. */
int bz_lzh_decode_batch(int method, int prefill, int device, const uint8_t *const *ins, const size_t *lens,
                        const uint64_t *orig_lens, size_t count, uint8_t **out, uint64_t *out_off, uint64_t *out_len, int32_t *verdict);
/* The batch of one == `in.iter().cloned().decode(&mut LzhufDecoder::new(&method))` under the contract above (orig_len
 * UINT64_MAX: not known): BZ_OK with the bytes, or the verdict with the bytes in front of it. */
int bz_lzh_decode_buffer(int method, int prefill, int device, const uint8_t *in, size_t in_len,
                         uint64_t orig_len, uint8_t **out, size_t *out_len);

/* ========================================================================
 * 10. LZHUF ENCODE  ==  `LzhufEncoder::new(&method)` driven with Action::Finish
 *     (src/lzhuf/encoder.rs), many independent inputs in one call.
 *
 * Stream i is `input_i.encode(&mut LzhufEncoder::new(&method), Action::Finish)`
 * collected, byte for byte: LzssEncoder with a window of 1 << dictionary_bits,
 * matches of 3 .. 256 bytes, lazy level 3 and Deflate's comparison; blocks of
 * 65 535 CODES (the last one shorter) with their t-, c- and p-table; no end
 * marker; zero bits to the next byte at the end of the stream; an empty input
 * gives an empty stream.  One method per call (section 9's table).
 *
 * Inputs as in df_gpu_encode_batch_device: d_in 16-byte aligned, h_in_off
 * multiples of 16, the ranges ascending and disjoint; every input at most
 * 1 GiB (positions are 32-bit; a longer one is BZ_E_PARAM -- encoding in
 * parts is not offered).  Streams are written to d_out (4-byte aligned) in
 * input order, stream i at h_out_off[i] (a multiple of 4) with h_out_len[i]
 * bytes, zeros between a stream's end and the next multiple of 4, and nothing
 * at or behind d_out + cap.  (d_out, h_out_off, h_out_len) are valid
 * (d_in, h_in_off, h_in_len) of bz_gpu_lzh_decode_batch_device, and that
 * call's outputs (multiples of 16) are valid inputs of this one.
 * BZ_E_CAPACITY: cap is too small (bz_lzh_encode_batch_bound always suffices;
 * bytes in front of d_out + cap may have been written).  BZ_E_PARAM: a method
 * outside 4 .. 7, a null engine, a null array or d_out with count > 0, a
 * misaligned d_in, d_out or offset, ranges out of order, an input above 1 GiB.
 * count == 0: BZ_OK, nothing touched.
 * ======================================================================== */
int bz_gpu_lzh_encode_batch_device(bz_gpu_engine *g, int method, const void *d_in, const uint64_t *h_in_off,
                                   const uint64_t *h_in_len, size_t count, void *d_out, size_t cap, uint64_t *h_out_off,
                                   uint64_t *h_out_len);
/* The last bz_gpu_lzh_encode_batch_device call: [0] inputs [1] sub-batches (BZ_DF_BATCH_MIB of slot image each; an input
 * larger than that has one of its own) [2] blocks [3] literal codes [4] match codes [5] input bytes [6] stream bytes
 * [7] c-tables that took make_table's length-limited path. */
int bz_gpu_last_lzh_encode_stats(bz_gpu_engine *g, uint64_t out[8]);
/* Bytes that always suffice for the streams of inputs of these lengths, each rounded up to 4 (DESIGN_lzhuf.md section 8: a
 * code costs at most 16 bits per input byte, a block header at most 1 084 bytes per 65 535 codes). */
size_t bz_lzh_encode_batch_bound(const uint64_t *in_len, size_t count);
/* The host form (mirrors df_encode_batch): the inputs packed at 16-byte-aligned offsets, one upload, one device call on an
 * engine of the per-process cache, one download; *out is ONE malloc'ed buffer (bz_free), stream i at out_off[i].  The
 * parameters are checked before any device is touched; count == 0: BZ_OK, an empty buffer, no device.  Without a GPU:
 * BZ_E_NOGPU. */
int bz_lzh_encode_batch(int method, int device, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t **out,
                        uint64_t *out_off, uint64_t *out_len);
/* The batch of one == `in.encode(&mut LzhufEncoder::new(&method), Action::Finish).collect()`. */
int bz_lzh_encode_buffer(int method, int device, const uint8_t *in, size_t in_len, uint8_t **out, size_t *out_len);
/* Test hook: the LZSS codes of ONE input (n bytes of device memory, 16-byte aligned) under `method`, in stream order as
 * (len, pos) pairs, len 0 = the literal `pos`, else a match of len bytes at distance pos + 1 (what LzssEncoder::next
 * yields).  At most cap pairs are written; *count is the number of codes. */
int bz_gpu_lzh_debug_codes(bz_gpu_engine *g, int method, const void *d_in, size_t n, uint32_t *out_pairs, size_t cap,
                           size_t *count);
/* Test hook: the block stage's table builder on the host's counts (510 c-counts: literals, then lengths 3 .. 256; 17
 * p-counts by the bit length of distance - 1).  c_len[510], p_len[17], t_len[19]: make_table's lengths (a lone symbol has
 * length 1 and is written in the constant form; t_len is all zero when the c-table is a constant).  res[0]: bits of the
 * block header, the 16-bit code count included; res[1]: bit 0 the c-table is a constant, bit 1 the p-table, bit 2 the
 * t-table; res[2]: tables that took the length-limited path. */
int bz_gpu_lzh_debug_tables(bz_gpu_engine *g, int method, const uint32_t *c_freq, const uint32_t *p_freq, uint8_t *c_len,
                            uint8_t *p_len, uint8_t *t_len, uint32_t res[3]);

/* ========================================================================
 * 11. LHA ARCHIVES (.lzh / .lha), READING: the member table on the host, the
 *     bytes of all members or of a chosen subset in one device call, every
 *     member with its own verdict and its CRC-16 checked on the device.
 *
 * The header rules (levels 0, 1 and 2; DESIGN_lzhuf.md section 12 has the
 * table) stand in csrc/lha_archive.h alone.  Methods: -lh4- .. -lh7- are
 * decoded by section 9's call, -lh0- and -lz4- are stored, -lhd- is a directory
 * (no data, clean without a launch); any other id of the form -???- is listed
 * with BZ_LHA_OTHER and reads as BZ_E_UNEXPECTED without bytes.  Header level 3
 * and the 64-bit size extension are not read.
 * ======================================================================== */
#define BZ_LHA_STORED 0
#define BZ_LHA_DIR 1
#define BZ_LHA_LH4 4 /* .. BZ_LHA_LH7 7: BZ_LZH_LH4 .. BZ_LZH_LH7 */
#define BZ_LHA_LH5 5
#define BZ_LHA_LH6 6
#define BZ_LHA_LH7 7
#define BZ_LHA_OTHER 255
typedef struct bz_lha_member {
    uint64_t header_off; /* where the member's header starts in the archive */
    uint64_t data_off;   /* where its data starts */
    uint64_t packed_len; /* bytes of data */
    uint64_t orig_len;   /* bytes it stands for */
    uint64_t name_off;   /* the name's bytes in the archive (a type-0x01 extended header's when there is one), raw */
    uint64_t dir_off;    /* the directory's (type 0x02, components separated by 0xFF) */
    uint32_t name_len, dir_len;
    uint32_t mtime;      /* levels 0 and 1: MS-DOS time and date; level 2: Unix time; raw */
    uint16_t crc16;      /* CRC-16/ARC of the original bytes */
    uint8_t method;      /* BZ_LHA_* */
    uint8_t level;
    uint8_t os_id;       /* levels 1 and 2; level 0: 0 */
    uint8_t attr;        /* raw */
    uint8_t method_id[5];
    uint8_t pad;
} bz_lha_member;
/* The member table, on the host alone (never BZ_E_NOGPU).  At most cap records are written; members == NULL counts.
 * *count: the members found.  *fault: BZ_OK when the archive ends cleanly (at in_len, or at a header position that holds a
 * 0 byte; bytes behind that are ignored), else the verdict that ended the walk and *fault_pos the header it lies in:
 * BZ_E_EOF, a header or a member's data needs a byte behind in_len; BZ_E_DATA, a wrong byte sum (levels 0, 1) or header
 * CRC (level 2), a level above 2, a method id not of the form -???-, a header size below what its fields need, an extended
 * header of size 1 or 2, a level-1 skip size below its extended headers.  The table lists every member in front of the
 * fault; a member whose data is cut by the end of the archive is listed too (it reads as BZ_E_EOF).  Returns BZ_OK, or
 * BZ_E_PARAM (a null count, fault or fault_pos; in null with in_len > 0). */
int bz_lha_index_buffer(const uint8_t *in, size_t in_len, bz_lha_member *members, size_t cap, size_t *count, int32_t *fault,
                        uint64_t *fault_pos);
/* The members h_sel[0 .. nsel) (indices into h_members[0 .. nmembers), strictly ascending; NULL: all, nsel == nmembers) of
 * the archive d_in[0 .. in_len) (HBM, 16-byte aligned).  Selected members are grouped by method: one gather of their spans
 * (they lie at any byte phase) and ONE call into section 9's decode path per method present, with the members' original
 * lengths and `prefill` (section 9 (e); LHA's encoders match against a window of spaces, so the archive-shaped wrappers
 * default to 0x20); the split path (g), its fallbacks and BZ_LZH_SPLIT_KIB apply as there.  Stored members are copied.
 * Then ONE CRC-16 launch (parts of BZ_LHA_CRC_PART_KIB KiB, default 1024, read per call) and its join run over all clean
 * members of the call.
 * Member k of the selection lies at h_out_off[k], a multiple of 16, in selection order: its slot is its header's original
 * length rounded up to 16 (no bytes for a directory, a BZ_LHA_OTHER member, a stored member whose sizes differ, a member
 * whose data is cut), so the places are known before any launch: cap must reach the end of the last slot's original
 * length, else BZ_E_CAPACITY with d_out untouched.  h_out_len[k] is what was produced (the original length for a clean
 * member).  NOTHING outside the reported ranges is written.  d_out == NULL: sizes and verdicts only (no CRC: a member
 * that decodes is reported clean).
 * h_verdict[k]: BZ_OK only when the member's bytes are whole and their CRC-16 is the header's; BZ_E_DATA: the decoder's
 * (section 9 (d)), a stored member whose packed and original sizes differ, or a CRC mismatch (the bytes are there);
 * BZ_E_EOF: the decoder's, a stream that ends short of the original length (section 9 (b)), or data cut by the end of
 * the archive; BZ_E_UNEXPECTED: a method that is not decoded.  No member's verdict or bytes change another's; the
 * return value is the infrastructure status.
 * BZ_E_PARAM, before any device is touched: a null engine, a null array with nsel > 0, a misaligned d_in or d_out, a
 * selection out of order or out of range, a record whose header or data starts behind in_len or whose packed or
 * original length is 4 GiB or more, a prefill outside -1 .. 255.  nsel == 0: BZ_OK, nothing touched. */
int bz_gpu_lha_read_device(bz_gpu_engine *g, const void *d_in, size_t in_len, const bz_lha_member *h_members, size_t nmembers,
                           const size_t *h_sel, size_t nsel, int prefill, void *d_out, size_t cap, uint64_t *h_out_off,
                           uint64_t *h_out_len, int32_t *h_verdict);
/* The last bz_gpu_lha_read_device call: [0] members read clean [1] with an error verdict [2] stored [3] directories
 * [4] not decodable (BZ_E_UNEXPECTED) [5] CRC mismatches [6] bytes out [7] kernel launches.  (Section 9's figures are
 * those of the call's last decode call.) */
int bz_gpu_last_lha_read_stats(bz_gpu_engine *g, uint64_t out[8]);
/* The host form (the shape of bz_lzh_decode_batch): the table is built here, one upload, one device call on an engine of
 * the per-process cache, one download; *out is ONE malloc'ed buffer (bz_free), member k of the selection at out_off[k].
 * sel == NULL: all members, and nsel must be their count (bz_lha_index_buffer).  *fault: the index's verdict; the members
 * in front of it are read.  The parameters are checked before any device is touched; nsel == 0: BZ_OK, an empty buffer,
 * no device.  Without a GPU: BZ_E_NOGPU. */
int bz_lha_read_buffer(int device, const uint8_t *in, size_t in_len, const size_t *sel, size_t nsel, int prefill, uint8_t **out,
                       uint64_t *out_off, uint64_t *out_len, int32_t *verdict, int32_t *fault);

/* ========================================================================
 * 12. LHA ARCHIVES, WRITING: every member in one device call -- section 10's
 *     streams (or the members' own bytes) behind headers of level 0, 1 or 2,
 *     every member's CRC-16 computed on the device.
 *
 * method: BZ_LHA_LH4 .. BZ_LHA_LH7, or BZ_LHA_STORED (every member -lh0-, no
 * encode call at all).  level: the header level, 0, 1 or 2.  The data of
 * member i is stream i of bz_gpu_lzh_encode_batch_device for that method, byte
 * for byte, with one exception, THE STORED RULE (this project's own; LHA tools
 * decide likewise but no text fixes the tie): a member whose stream is not
 * shorter than its input (stream_len >= in_len, the empty input included; the
 * tie goes to stored) is written as -lh0- with the input's own bytes.  crc16
 * is the CRC-16/ARC of the input bytes.  An is_dir entry is a -lhd- member
 * without data.  The archive ends with one 0 byte; count == 0 gives that byte
 * alone.
 *
 * The header shape is fixed (csrc/lha_archive.h; DESIGN_lzhuf.md section 13):
 * level 0 has the name in the base header and no place for a directory;
 * level 1 has the name in the base header while 25 + N <= 255, else as a
 * type-0x01 extended header with N = 0, and a non-empty dir as type 0x02;
 * level 2 has a type-0x00 header CRC, the name as type 0x01 always, dir as
 * type 0x02 when it is not empty, and one padding byte when the low byte of
 * the header size would be 0.
 * ======================================================================== */
typedef struct bz_lha_entry {
    const uint8_t *name; uint32_t name_len; /* raw bytes */
    const uint8_t *dir;  uint32_t dir_len;  /* raw, components separated by 0xFF; may be empty */
    uint32_t mtime;                         /* raw, as bz_lha_member.mtime */
    uint8_t attr, os_id, is_dir, pad;       /* is_dir: a -lhd- member, no data */
} bz_lha_entry;
/* Bytes that always suffice for the archive: every header's size, every input's length and the end byte (the stored rule
 * keeps a member's data at or below its input's length; header sizes do not depend on packed sizes).  The host alone.
 * 0: a level outside 0 .. 2 or an entry that has no header at that level (see BZ_E_PARAM below). */
size_t bz_lha_write_bound(int level, const bz_lha_entry *e, const uint64_t *in_len, size_t count);
/* Inputs as in bz_gpu_lzh_encode_batch_device: d_in 16-byte aligned, h_in_off multiples of 16, the ranges ascending and
 * disjoint; member i is h_entries[i] with the bytes d_in[h_in_off[i] .. + h_in_len[i]).  One call: the CRC-16 launch and its
 * join over the inputs (parts of BZ_LHA_CRC_PART_KIB KiB as in section 11), section 10's encode call into a buffer of the
 * engine (not for BZ_LHA_STORED, directories and empty inputs), ONE host step (the stored rule, the headers, the places,
 * the capacity check), ONE launch that lays headers and data side by side at any byte phase of d_out.
 * *out_len: the archive's length.  No byte of d_out outside [0, *out_len) is written.  BZ_E_CAPACITY: the finished archive
 * does not fit cap; d_out is untouched (the archive is laid out last, its length known).  h_members (may be NULL; room for
 * count records): the table bz_lha_index_buffer would build from the written bytes, field for field.
 * BZ_E_PARAM, before any device is touched: a null engine, out_len or d_out; a null array with count > 0; a name or dir
 * pointer null with a length; a misaligned d_in or offset, ranges out of order; a method outside the five, a level outside
 * 0 .. 2; a non-empty dir at level 0 (no field a reader would give it back from); a name or directory whose header exceeds
 * its size field (H > 255 at level 0, an extended header or T above 65 535); an input above 1 GiB with a compressing
 * method, or one whose size field would reach 4 GiB - 1 with BZ_LHA_STORED; an is_dir entry with h_in_len != 0. */
int bz_gpu_lha_write_device(bz_gpu_engine *g, int method, int level, const void *d_in, const uint64_t *h_in_off,
                            const uint64_t *h_in_len, const bz_lha_entry *h_entries, size_t count, void *d_out, size_t cap,
                            size_t *out_len, bz_lha_member *h_members);
/* The last bz_gpu_lha_write_device call: [0] members [1] written compressed [2] stored by the rule [3] stored by request
 * (BZ_LHA_STORED) [4] directories [5] input bytes [6] archive bytes [7] kernel launches of the writer itself (CRC, join,
 * layout; section 10's figures are those of the call's encode call). */
int bz_gpu_last_lha_write_stats(bz_gpu_engine *g, uint64_t out[8]);
/* The host form (the shape of bz_lzh_encode_batch): the inputs packed at 16-byte-aligned offsets, one upload, one device call
 * on an engine of the per-process cache, one download; *out is ONE malloc'ed buffer (bz_free) of *out_len bytes.  The
 * parameters are checked before any device is touched; count == 0: BZ_OK, the end byte alone, no device.  Without a GPU:
 * BZ_E_NOGPU. */
int bz_lha_write_buffer(int method, int level, int device, const uint8_t *const *ins, const size_t *lens,
                        const bz_lha_entry *entries, size_t count, uint8_t **out, size_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* BZ2_MI355X_H */
