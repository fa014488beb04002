// k_rle1.hip -- RLE1, block split and block CRC as data-parallel kernels.
//
// Reference being replaced: EncoderInner::next / write_rle
// (src/bzip2/encoder.rs:671-716), the block cut at :692 and the CRC update at
// :701-702 (src/crc32.rs:58-84, 128-149).
//
// Restatement that makes it parallel.  A "chunk" is a maximal same-byte run cut
// every 255 bytes from the run's start (encoder.rs:682).  For input position p
// with run start rs(p):  q = p - rs(p),  c = q mod 255 (position inside its
// chunk).  Position p emits its byte iff c < 4, and a count byte (c-3) iff it
// is the last byte of its chunk and c >= 3.  The RLE1 image of the whole input
// is therefore one exclusive prefix sum away, and blocks are contiguous slices
// of it: a block is cut right after the first chunk whose end brings the block
// to >= 100000*level-19 bytes (encoder.rs:186,692).  Only the cut positions are
// a serial chain (about 1200 per GiB).
//
// HBM traffic: the input is read 3x (tile scan+CRC, count, scatter) and the
// image written once -- all coalesced 16 B/lane.  An engine that codes the whole
// input reads it once (k_rle_onepass); the three kernels are the path of sharded
// slabs and the fallback.
#include "bzgpu.h"

namespace bzgpu {

constexpr u32 RT = 256; // threads per RLE tile

__device__ __forceinline__ i64 block_excl_max64(i64 v, i64 *sh /*[RT/64 + 1]*/, i64 &total)
{
    // exclusive max-scan over the workgroup in thread order
    const u32 l = lane_id(), w = threadIdx.x >> 6;
    i64 inc = wave_incl_max64(v);
    if (l == 63) sh[w] = inc;
    __syncthreads();
    i64 carry = -1;
    for (u32 k = 0; k < w; ++k) carry = sh[k] > carry ? sh[k] : carry;
    i64 tot = -1;
    for (u32 k = 0; k < RT / 64; ++k) tot = sh[k] > tot ? sh[k] : tot;
    total = tot;
    i64 prev = __shfl_up(inc, 1, 64);
    i64 ex = (l == 0) ? (i64)-1 : prev;
    __syncthreads();
    return ex > carry ? ex : carry;
}

__device__ __forceinline__ u32 block_excl_sum(u32 v, u32 *sh /*[RT/64]*/, u32 &total)
{
    const u32 l = lane_id(), w = threadIdx.x >> 6;
    u32 inc = wave_incl_sum(v);
    if (l == 63) sh[w] = inc;
    __syncthreads();
    u32 carry = 0, tot = 0;
    for (u32 k = 0; k < RT / 64; ++k) {
        if (k < w) carry += sh[k];
        tot += sh[k];
    }
    total = tot;
    __syncthreads();
    return carry + inc - v;
}

// load the 16 bytes of this thread (tile t, thread tid) + the byte before and after
struct Seg {
    u8 b[16];
    int prev;  // byte before p0 or -1
    int next;  // byte after the segment or -1 (end of input)
    u64 p0;
    u32 valid; // number of valid bytes (0..16)
    u32 skip;  // leading bytes that lie before the region's first byte (treated as not there)
};

// in_begin: first byte of the region being coded.  RLE1 restarted at a block cut is identical to
// RLE1 continued (a cut is a chunk start), so a rank may start at the cut it was handed.
__device__ __forceinline__ void load_seg(const u8 *__restrict__ in, u64 n, u64 tile, Seg &s, u64 in_begin = 0)
{
    s.p0 = tile * (u64)kRleTile + (u64)threadIdx.x * 16u;
    if (s.p0 + 16 <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(in + s.p0);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) s.b[k] = (u8)(w[k >> 2] >> ((k & 3) * 8));
        s.valid = 16;
    } else {
        s.valid = s.p0 < n ? (u32)(n - s.p0) : 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) s.b[k] = (u32)k < s.valid ? in[s.p0 + k] : (u8)0;
    }
    s.prev = (s.p0 > in_begin && s.valid > 0) ? (int)in[s.p0 - 1] : -1;
    s.next = (s.p0 + s.valid < n && s.valid > 0) ? (int)in[s.p0 + s.valid] : -1;
    s.skip = (in_begin > s.p0) ? (u32)((in_begin - s.p0) < 16u ? (in_begin - s.p0) : 16u) : 0u;
}

// ---- kernel A: per-tile last run start + per-tile raw CRC ---------------------
// crc_tab: 256-entry byte table (src/crc32.rs:58-72); xp16: x^(8*16*k) mod P, k=0..255
__global__ __launch_bounds__(RT) void k_rle_tile_scan(const u8 *__restrict__ in, u64 n, u64 t0, u64 in_begin,
                                                       const u32 *__restrict__ crc_tab,
                                                       const u32 *__restrict__ xp16,
                                                       i64 *__restrict__ tile_last_start,
                                                       u32 *__restrict__ tile_crc)
{
    __shared__ u32 s_tab[256];
    __shared__ i64 s_max[RT / 64];
    __shared__ u32 s_x[RT / 64];
    s_tab[threadIdx.x] = crc_tab[threadIdx.x];
    __syncthreads();

    const u64 tile = t0 + blockIdx.x;
    Seg s;
    load_seg(in, n, tile, s, in_begin);

    i64 last = -1;
    int pb = s.prev;
    u32 crc = 0;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        if (k < s.valid) {
            if (k >= s.skip) {
                if ((int)s.b[k] != pb) last = (i64)(s.p0 + k);
                pb = s.b[k];
            }
            crc = s_tab[(crc >> 24) ^ s.b[k]] ^ (crc << 8); // the tile CRC covers every byte of the tile
        }
    }
    // shift this thread's CRC to the end of the tile: bytes after it inside the tile
    const u64 tile_beg = tile * (u64)kRleTile;
    const u32 tile_len = (u32)((n - tile_beg) < (u64)kRleTile ? (n - tile_beg) : (u64)kRleTile);
    if (s.valid > 0) {
        const u32 after = tile_len - (threadIdx.x * 16u + s.valid);
        if ((after & 15u) == 0) {
            crc = gf_mulmod(crc, xp16[after >> 4]);
        } else { // only in the last, partial tile
            u32 m = gf_mulmod(xp16[after >> 4], 1u);
            for (u32 k = 0; k < (after & 15u); ++k) m = gf_mulmod(m, 0x100u); // * x^8
            crc = gf_mulmod(crc, m);
        }
    } else {
        crc = 0;
    }
    i64 wl = last;
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
        i64 o = __shfl_xor(wl, d, 64);
        wl = o > wl ? o : wl;
    }
    const u32 wx = wave_xor(crc);
    if (lane_id() == 0) {
        s_max[threadIdx.x >> 6] = wl;
        s_x[threadIdx.x >> 6] = wx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        i64 m = -1;
        u32 x = 0;
        for (u32 k = 0; k < RT / 64; ++k) {
            m = s_max[k] > m ? s_max[k] : m;
            x ^= s_x[k];
        }
        tile_last_start[tile] = m;
        tile_crc[tile] = x;
    }
}

// ---- kernels B and D: exclusive scans over the tiles of a range, in three small launches -----------------
// (one workgroup walking 262 144 tiles took 0.44 ms per scan and left the chip idle)
//   _local : a workgroup scans 1024 consecutive tiles, writes the tile's value relative to the workgroup and the
//            workgroup's total;   _parts : one workgroup scans the totals;   _add : every tile takes its workgroup's.
// IS_MAX: max-scan of i64 run starts (identity -1, carried in from `init`); else sum of u32 counts into u64 offsets.
template <bool IS_MAX> struct TileScan;
template <> struct TileScan<true> {
    typedef i64 In;
    typedef i64 Out;
    static __device__ __forceinline__ i64 ident() { return -1; }
    static __device__ __forceinline__ i64 op(i64 a, i64 b) { return a > b ? a : b; }
};
template <> struct TileScan<false> {
    typedef u32 In;
    typedef u64 Out;
    static __device__ __forceinline__ u64 ident() { return 0; }
    static __device__ __forceinline__ u64 op(u64 a, u64 b) { return a + b; }
};
template <bool IS_MAX> __device__ __forceinline__ typename TileScan<IS_MAX>::Out wave_incl(typename TileScan<IS_MAX>::Out v)
{
    typedef TileScan<IS_MAX> S;
    const u32 l = lane_id();
#pragma unroll
    for (u32 d = 1; d < 64; d <<= 1) {
        const typename S::Out t = __shfl_up(v, d, 64);
        if (l >= d) v = S::op(t, v);
    }
    return v;
}
// exclusive scan of one value per thread over a 1024-thread workgroup (thread order); total = the whole
template <bool IS_MAX>
__device__ __forceinline__ typename TileScan<IS_MAX>::Out wg_excl(typename TileScan<IS_MAX>::Out v,
                                                                     typename TileScan<IS_MAX>::Out *sh /*[16]*/,
                                                                     typename TileScan<IS_MAX>::Out &total)
{
    typedef TileScan<IS_MAX> S;
    const u32 l = lane_id(), w = threadIdx.x >> 6;
    const typename S::Out inc = wave_incl<IS_MAX>(v);
    if (l == 63) sh[w] = inc;
    __syncthreads();
    typename S::Out carry = S::ident(), tot = S::ident();
    for (u32 k = 0; k < 16; ++k) {
        if (k < w) carry = S::op(carry, sh[k]);
        tot = S::op(tot, sh[k]);
    }
    total = tot;
    typename S::Out prev = __shfl_up(inc, 1, 64);
    if (l == 0) prev = S::ident();
    __syncthreads();
    return S::op(carry, prev);
}
template <bool IS_MAX>
__global__ __launch_bounds__(1024) void k_tiles_scan_local(const typename TileScan<IS_MAX>::In *__restrict__ in,
                                                           typename TileScan<IS_MAX>::Out *__restrict__ out, u64 t0, u64 t1,
                                                           typename TileScan<IS_MAX>::Out *__restrict__ part)
{
    typedef TileScan<IS_MAX> S;
    __shared__ typename S::Out sh[16];
    const u64 t = t0 + (u64)blockIdx.x * 1024u + threadIdx.x;
    const typename S::Out v = t < t1 ? (typename S::Out)in[t] : S::ident();
    typename S::Out total;
    const typename S::Out ex = wg_excl<IS_MAX>(v, sh, total);
    if (t < t1) out[t] = ex;
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// part[b] <- what is carried into workgroup b (from `init`); *whole (and *whole2, if given) <- the scan's end value
template <bool IS_MAX>
__global__ __launch_bounds__(1024) void k_tiles_scan_parts(typename TileScan<IS_MAX>::Out *__restrict__ part, u32 nparts,
                                                           typename TileScan<IS_MAX>::Out init,
                                                           typename TileScan<IS_MAX>::Out *__restrict__ whole,
                                                           typename TileScan<IS_MAX>::Out *__restrict__ whole2)
{
    typedef TileScan<IS_MAX> S;
    __shared__ typename S::Out sh[16];
    typename S::Out run = init;
    for (u32 b0 = 0; b0 < nparts; b0 += 1024u) {
        const u32 b = b0 + threadIdx.x;
        const typename S::Out v = b < nparts ? part[b] : S::ident();
        typename S::Out total;
        const typename S::Out ex = wg_excl<IS_MAX>(v, sh, total);
        if (b < nparts) part[b] = S::op(run, ex);
        run = S::op(run, total);
    }
    if (threadIdx.x == 0) {
        if (whole) *whole = run;
        if (whole2) *whole2 = run;
    }
}
template <bool IS_MAX>
__global__ __launch_bounds__(1024) void k_tiles_scan_add(typename TileScan<IS_MAX>::Out *__restrict__ out, u64 t0, u64 t1,
                                                         const typename TileScan<IS_MAX>::Out *__restrict__ part)
{
    typedef TileScan<IS_MAX> S;
    const u64 t = t0 + (u64)blockIdx.x * 1024u + threadIdx.x;
    if (t < t1) out[t] = S::op(part[blockIdx.x], out[t]);
}
template <bool IS_MAX>
static void tiles_scan(hipStream_t st, const typename TileScan<IS_MAX>::In *in, typename TileScan<IS_MAX>::Out *out, u64 t0,
                       u64 t1, typename TileScan<IS_MAX>::Out *part, typename TileScan<IS_MAX>::Out init,
                       typename TileScan<IS_MAX>::Out *whole, typename TileScan<IS_MAX>::Out *whole2)
{
    const u32 nparts = (u32)((t1 - t0 + 1023u) / 1024u);
    hipLaunchKernelGGL((k_tiles_scan_local<IS_MAX>), dim3(nparts), dim3(1024), 0, st, in, out, t0, t1, part);
    hipLaunchKernelGGL((k_tiles_scan_parts<IS_MAX>), dim3(1), dim3(1024), 0, st, part, nparts, init, whole, whole2);
    hipLaunchKernelGGL((k_tiles_scan_add<IS_MAX>), dim3(nparts), dim3(1024), 0, st, out, t0, t1, part);
}

// Per-thread RLE1 evaluation of its 16 positions.
//   rs_in : run start that is live when the segment begins (from earlier threads/tiles), -1 if p0==0
// Produces the emitted-byte count, and (optionally) the bytes.
struct SegEval {
    u32 count;      // bytes this segment emits
    u32 c_first;    // chunk phase of the first position
};

__device__ __forceinline__ u32 phase_of(u64 p, i64 rs)
{
    return (u32)((p - (u64)rs) % 255u);
}

// fills e[k] = number of bytes position k emits (0,1,2); returns sum
__device__ __forceinline__ u32 eval_seg(const Seg &s, i64 rs_in, u8 e[16], u8 cph[16])
{
    u32 sum = 0;
    i64 rs = rs_in;
    int pb = s.prev;
    u32 c = 0;
    bool have_c = false;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        u32 ek = 0;
        u32 ck = 0;
        if (k < s.valid && k >= s.skip) {
            const u64 p = s.p0 + k;
            if ((int)s.b[k] != pb) {
                rs = (i64)p;
                c = 0;
                have_c = true;
            } else if (!have_c) {
                c = phase_of(p, rs);
                have_c = true;
            } else {
                c = (c == 254u) ? 0u : c + 1u;
            }
            pb = s.b[k];
            const int nb = (k + 1 < s.valid) ? (int)s.b[k + 1 < 16 ? k + 1 : 15] : s.next;
            const bool chunk_end = (nb != (int)s.b[k]) || (c == 254u);
            ek = (c < 4u ? 1u : 0u) + ((chunk_end && c >= 3u) ? 1u : 0u);
            ck = c;
        }
        e[k] = (u8)ek;
        cph[k] = (u8)ck;
        sum += ek;
    }
    return sum;
}

// run start live at the beginning of each thread's segment
__device__ __forceinline__ i64 seg_run_start(const Seg &s, i64 tile_carry, i64 *sh)
{
    i64 last = -1;
    int pb = s.prev;
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        if (k < s.valid && k >= s.skip) {
            if ((int)s.b[k] != pb) last = (i64)(s.p0 + k);
            pb = s.b[k];
        }
    }
    i64 tot;
    i64 ex = block_excl_max64(last, sh, tot);
    return ex > tile_carry ? ex : tile_carry;
}

// ---- kernel C: bytes emitted per tile -------------------------------------------
// Also records, for each 256-byte sub-tile, the bytes emitted before it inside its tile and the run
// start live at its first byte -- the cut chain uses them to look at 2 KiB instead of whole tiles.
__global__ __launch_bounds__(RT) void k_rle_count(const u8 *__restrict__ in, u64 n, u64 t0, u64 in_begin,
                                                   const i64 *__restrict__ carry_in,
                                                   u32 *__restrict__ tile_count, u16 *__restrict__ sub_off,
                                                   i64 *__restrict__ sub_rs)
{
    __shared__ i64 s_m[RT / 64 + 1];
    __shared__ u32 s_s[RT / 64];
    const u64 tile = t0 + blockIdx.x;
    Seg s;
    load_seg(in, n, tile, s, in_begin);
    const i64 rs = seg_run_start(s, carry_in[tile], s_m);
    u8 e[16], cph[16];
    const u32 cnt = eval_seg(s, rs, e, cph);
    u32 tot;
    const u32 ex = block_excl_sum(cnt, s_s, tot);
    if (threadIdx.x == 0) tile_count[tile] = tot;
    if ((threadIdx.x & 15u) == 0) {
        sub_off[tile * 16u + (threadIdx.x >> 4)] = (u16)ex;
        sub_rs[tile * 16u + (threadIdx.x >> 4)] = rs;
    }
}

// ---- kernel E: scatter the RLE1 image -------------------------------------------
__global__ __launch_bounds__(RT) void k_rle_scatter(const u8 *__restrict__ in, u64 n, u64 t0, u64 in_begin,
                                                     const i64 *__restrict__ carry_in,
                                                     const u64 *__restrict__ tile_off,
                                                     u8 *__restrict__ rle)
{
    __shared__ i64 s_m[RT / 64 + 1];
    __shared__ u32 s_s[RT / 64];
    __shared__ __attribute__((aligned(16))) u8 s_out[2 * kRleTile + 32];
    const u64 tile = t0 + blockIdx.x;
    Seg s;
    load_seg(in, n, tile, s, in_begin);
    const i64 rs = seg_run_start(s, carry_in[tile], s_m);
    u8 e[16], cph[16];
    const u32 cnt = eval_seg(s, rs, e, cph);
    u32 tot;
    // The tile's bytes are staged at the offset their destination has inside a 16-byte line, so that the copy out is
    // aligned 16-byte stores of aligned 16-byte LDS reads (rounds 1-4a: one BYTE per lane and store instruction, sixteen
    // store instructions per thread); only the ragged first and last line go out byte by byte.
    u8 *dst = rle + tile_off[tile];
    const u32 a0 = (u32)(reinterpret_cast<uintptr_t>(dst) & 15u);
    u32 o = a0 + block_excl_sum(cnt, s_s, tot);
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        if (e[k]) {
            if (cph[k] < 4u) s_out[o++] = s.b[k];
            if (e[k] == 2u || cph[k] >= 4u) s_out[o++] = (u8)(cph[k] - 3u);
        }
    }
    __syncthreads();
    u8 *line0 = dst - a0; // 16-byte aligned
    const u32 end = a0 + tot, nlines = (end + 15u) >> 4;
    for (u32 j = threadIdx.x; j < nlines; j += RT) {
        const u32 lo = j * 16u;
        if (lo >= a0 && lo + 16u <= end) {
            *reinterpret_cast<uint4 *>(line0 + lo) = *reinterpret_cast<const uint4 *>(s_out + lo);
        } else {
            const u32 b0 = lo > a0 ? lo : a0, b1 = lo + 16u < end ? lo + 16u : end;
            for (u32 b = b0; b < b1; ++b) line0[b] = s_out[b];
        }
    }
}

// ---- kernel A+C+E in one: the whole front end in one pass over the input ---------------------------------
// For an engine that codes the whole input from byte 0.  A workgroup takes a SPAN of eight consecutive tiles (32 KB),
// handed out in order by a ticket, and writes for them exactly what k_rle_tile_scan, the two tile scans, k_rle_count
// and k_rle_scatter write: the input is read once instead of three times.  What a span needs from the spans in front
// of it -- the run start live at its first byte and the image offset of its first byte -- comes by decoupled
// look-back.  A ticket's predecessors all hold a lower ticket, so they are running or done: a wait ends.
//
// Look-back words.  Spans run on all XCDs, whose L2s are not coherent with each other, so the words are read and
// written with agent-scope atomics (st_sc1_x4 / ld_sc1_x4, for all their name, reach the XCD's own L2 only: the
// sort's and the ZLE stage's tickets keep producer and consumer on one XCD, a span's predecessor is anywhere).  The
// widest single access those give is 8 bytes, so tag, state and value share ONE 64-bit word,
//     epoch << 48 | state << 46 | value        (46 bits: 64 TiB)
// and a word is never seen half-written.  The epoch is the engine's call counter (1 .. 65535; the host clears the
// words when it wraps), so nothing is cleared between calls.  One wave asks for 64 predecessors' words at once.
constexpr u32 kSpanTiles = 8;
constexpr u32 kSpan = kSpanTiles * kRleTile;
constexpr u64 kOpValMask = (1ull << 46) - 1u;
constexpr u32 kOpAgg = 1, kOpIncl = 2; // the span's own figure / the figure of everything up to the span's end
constexpr u32 kOpEpochs = 65535;

__device__ __forceinline__ u64 op_word(u32 epoch, u32 state, u64 v)
{
    return ((u64)epoch << 48) | ((u64)state << 46) | (v & kOpValMask);
}
__device__ __forceinline__ void op_publish(u64 *p, u64 w) { __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Every lane of ONE wave calls this.  IS_MAX: the latest run start published in front of `span` (values are position
// + 1, 0 = the span holds none: such a span is passed over until it has looked back itself and says kOpIncl); else the
// sum of the spans' byte counts.  Span 0 always says kOpIncl.  false: gave up (*err is set).
template <bool IS_MAX> __device__ __forceinline__ bool span_look_back(const u64 *words, u64 span, u32 epoch, u32 *err, u64 &result)
{
    const u32 l = lane_id();
    u64 acc = 0, hi = span; // words [0, hi) are still in front
    u32 spins = 0;
    while (hi > 0) {
        const bool have = (u64)l < hi;
        u64 w = 0;
        if (have) w = __hip_atomic_load(words + (hi - 1u - l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const u32 state = (u32)(w >> 46) & 3u;
        const u64 val = w & kOpValMask;
        const bool ready = have && (u32)(w >> 48) == epoch && state != 0u;
        const bool term = ready && (state == kOpIncl || (IS_MAX && val != 0u));
        const u64 m_wait = __ballot(have && !ready), m_term = __ballot(term);
        const u64 m_stop = m_wait | m_term;
        const u32 first = m_stop ? (u32)__builtin_ctzll(m_stop) : 64u; // the lanes below it hold settled, passable words
        if (!IS_MAX) {
            u64 c = (have && l < first) ? val : 0u;
#pragma unroll
            for (u32 d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
            acc += c;
        }
        if (first < 64u && ((m_term >> first) & 1u)) {
            const u64 tv = __shfl(val, (int)first, 64);
            result = IS_MAX ? tv : acc + tv;
            return true;
        }
        const u64 step = first < 64u ? first : 64u;
        hi -= step < hi ? step : hi;
        if (first < 64u) { // a predecessor has not published yet
            if (lb_give_up(spins, err, kLbSpinMax >> 3)) {
                if (l == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return false;
            }
            __builtin_amdgcn_s_sleep(2);
        }
    }
    result = acc; // (not reached: span 0 ends every walk)
    return true;
}

// RLE1 over the 16 bytes of a segment as bit masks (bit k = byte k).  eval_seg's rule, position by position, is: c = the
// byte's distance from its run's start modulo 255; it emits itself if c < 4 and a count byte (c - 3) if it is the last of
// its chunk (the next byte differs, or c = 254) and c >= 3.  Inside a segment a byte's distance from a run start OF THE
// SEGMENT is below 16, so only the bytes in front of the segment's first run start need the phase c0 of byte 0.
// bit k: byte k equals the byte before it (byte 0: `prev`, -1 = there is none)
__device__ __forceinline__ u32 seg_eq_mask(const uint4 &v, int prev)
{
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u32 m = 0, carry = (u32)prev & 0xFFu;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const u32 y = w[q] ^ ((w[q] << 8) | carry); // a byte of y is zero where the byte equals the one before it
        carry = w[q] >> 24;
        u32 t = (y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
        t = ~(t | y | 0x7F7F7F7Fu); // 0x80 in every zero byte of y
        const u32 u = t >> 7;
        m |= ((u | (u >> 7) | (u >> 14) | (u >> 21)) & 0xFu) << (4 * q);
    }
    return prev < 0 ? m & ~1u : m;
}
// E: seg_eq_mask, V: the valid bytes, c0: phase of byte 0 if it continues a run, next_differs: the byte behind the last
// valid one is another (or the input ends).  lt4: the bytes that emit themselves, cg: those that emit a count byte.
__device__ __forceinline__ void seg_emit_masks(u32 E, u32 V, u32 c0, bool next_differs, u32 &lt4, u32 &cg)
{
    const u32 S = ~E & V;                                       // run starts
    const u32 P = (S ? (1u << __builtin_ctz(S)) - 1u : 0xFFFFu) & V; // the bytes in front of the first one: c = (c0 + k) % 255
    const u32 wrap = 255u - c0;                                 // k at which c0 + k comes round to 0 (>= 16: not in this segment)
    const u32 w4 = wrap < 16u ? (0xFu << wrap) : 0u, w3 = wrap < 16u ? (0x7u << wrap) : 0u;
    const u32 p4 = (c0 < 4u ? (1u << (4u - c0)) - 1u : 0u) | w4, p3 = (c0 < 3u ? (1u << (3u - c0)) - 1u : 0u) | w3;
    lt4 = ((p4 & P) | S | (S << 1) | (S << 2) | (S << 3)) & V;
    const u32 lt3 = ((p3 & P) | S | (S << 1) | (S << 2)) & V;
    const u32 c254 = wrap >= 1u && wrap <= 16u ? (1u << (wrap - 1u)) & P : 0u;
    const u32 top = V ^ (V >> 1);                               // the last valid byte
    const u32 ce = ((S >> 1) | (next_differs ? top : 0u) | c254) & V; // last byte of its chunk
    cg = ce & ~lt3;
}

__global__ __launch_bounds__(RT, 3) void k_rle_onepass(const u8 *__restrict__ in, u64 n, u64 ntiles, u32 nspans, u32 epoch,
                                                     const u32 *__restrict__ crc_tab, const u32 *__restrict__ xp16,
                                                     RleBuffers rb, u8 *__restrict__ rle, i64 *__restrict__ out_last)
{
    __shared__ u32 s_tab[256];
    __shared__ int s_wmax[kSpanTiles][RT / 64];  // per tile and wave: last run start, relative to the span (-1: none)
    __shared__ u32 s_wx[kSpanTiles][RT / 64];    // ... CRC
    __shared__ u32 s_wsum[kSpanTiles][RT / 64];  // ... bytes emitted
    __shared__ int s_fb[kSpanTiles][RT / 64], s_lb[kSpanTiles][RT / 64]; // ... first byte of lane 0, last byte of lane 63
    __shared__ int s_edge[2]; // the byte in front of the span and the byte behind it (-1: none)
    __shared__ u32 s_ticket, s_fail;
    __shared__ i64 s_carry;   // run start live at the span's first byte
    __shared__ u32 s_cphase;  // ... and the span's first byte's distance from it, modulo 255
    __shared__ u64 s_base;    // image offset of the span's first byte
    __shared__ __attribute__((aligned(16))) u8 s_out[kSpan / 4 * 5 + 64]; // (a span that begins inside a chunk can emit a byte more than 5/4 of its own)

    const u32 tid = threadIdx.x, l = lane_id(), wv = tid >> 6;
    if (tid == 0) {
        s_ticket = __hip_atomic_fetch_add(rb.lb_ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_fail = 0;
    }
    s_tab[tid] = crc_tab[tid];
    __syncthreads();
    const u64 span = s_ticket;
    if (span >= nspans) return;
    const u64 B = span * (u64)kSpan;
    u64 *w_rs = rb.lb_rs + span, *w_off = rb.lb_off + span;

    // ---- the span's bytes: eight 16-byte loads per lane, back to back ------------------------------------
    uint4 v[kSpanTiles];
    if (B + kSpan <= n) {
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) v[j] = *reinterpret_cast<const uint4 *>(in + B + j * kRleTile + tid * 16u);
    } else {
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) {
            const u64 p0 = B + j * kRleTile + tid * 16u;
            if (p0 + 16 <= n) {
                v[j] = *reinterpret_cast<const uint4 *>(in + p0);
            } else {
                u32 t[4] = {0, 0, 0, 0};
                const u32 valid = p0 < n ? (u32)(n - p0) : 0u;
                for (u32 k = 0; k < valid; ++k) t[k >> 2] |= (u32)in[p0 + k] << ((k & 3u) * 8u);
                v[j] = make_uint4(t[0], t[1], t[2], t[3]);
            }
        }
    }
    if (tid == 0) {
        s_edge[0] = B > 0 ? (int)in[B - 1] : -1;
        s_edge[1] = B + kSpan < n ? (int)in[B + kSpan] : -1;
    }
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        if (l == 0) s_fb[j][wv] = (int)(v[j].x & 0xFFu);
        if (l == 63) s_lb[j][wv] = (int)(v[j].w >> 24);
    }
    __syncthreads();
    // the byte before and behind every segment: the neighbouring lane's, the neighbouring wave's, the neighbouring tile's
    u32 pn[kSpanTiles];
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        const u64 p0 = B + j * kRleTile + tid * 16u;
        const u32 valid = p0 + 16 <= n ? 16u : (p0 < n ? (u32)(n - p0) : 0u);
        int pb = __shfl_up((int)(v[j].w >> 24), 1, 64);
        int nb = __shfl_down((int)(v[j].x & 0xFFu), 1, 64);
        if (l == 0) pb = wv > 0 ? s_lb[j][wv - 1] : (j > 0 ? s_lb[j > 0 ? j - 1 : 0][RT / 64 - 1] : s_edge[0]);
        if (l == 63) nb = wv + 1 < RT / 64 ? s_fb[j][wv + 1 < RT / 64 ? wv + 1 : 0] : (j + 1 < kSpanTiles ? s_fb[j + 1 < kSpanTiles ? j + 1 : 0][0] : s_edge[1]);
        if (!(p0 > 0 && valid > 0)) pb = -1;
        if (!(valid > 0 && p0 + valid < n)) nb = -1;
        pn[j] = (u32)(pb + 1) | ((u32)(nb + 1) << 9); // (bits 18 ..: the phase of byte 0, step 4)
    }

    // ---- 1. per tile: last run start and CRC (k_rle_tile_scan) --------------------------------------------
    const bool full = B + kSpan <= n;
    u32 E[kSpanTiles];   // seg_eq_mask of the segment, valid bytes only
    int inc[kSpanTiles]; // inclusive max over the wave's lanes of the segments' last run starts (relative to the span)
    u32 crc[kSpanTiles];
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        const u32 rel = j * kRleTile + tid * 16u;
        const u32 valid = full ? 16u : (B + rel + 16 <= n ? 16u : (B + rel < n ? (u32)(n - (B + rel)) : 0u));
        const u32 V = (1u << valid) - 1u;
        E[j] = seg_eq_mask(v[j], (int)(pn[j] & 0x1FFu) - 1) & V;
        const u32 S = ~E[j] & V;
        const int last = S ? (int)(rel + 31u - (u32)__builtin_clz(S)) : -1;
        inc[j] = wave_incl_max32(last);
        if (l == 63) s_wmax[j][wv] = inc[j];
        const u32 w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        u32 c = 0;
#pragma unroll
        for (u32 k = 0; k < 16; ++k)
            if (full || k < valid) c = s_tab[(c >> 24) ^ ((w[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu)] ^ (c << 8);
        crc[j] = c;
    }
    if (full) {
        // the segment's CRC moved to the end of its tile: times x^(8 * 16 * (255 - tid)), the same factor in all eight tiles,
        // so its 32 shifts are made once: a * b = sum over the bits i of a of b x^i
        u32 bx = xp16[255u - tid];
        u32 r[kSpanTiles];
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) r[j] = 0;
#pragma unroll 4
        for (u32 i = 0; i < 32; ++i) {
#pragma unroll
            for (u32 j = 0; j < kSpanTiles; ++j) r[j] ^= (u32)((int)(crc[j] << (31u - i)) >> 31) & bx;
            bx = (bx << 1) ^ ((u32)((int)bx >> 31) & kCrcPoly);
        }
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) crc[j] = r[j];
    } else {
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) {
            const u64 tile_beg = B + (u64)j * kRleTile, p0 = tile_beg + tid * 16u;
            const u32 valid = p0 + 16 <= n ? 16u : (p0 < n ? (u32)(n - p0) : 0u);
            if (valid > 0) {
                const u32 tile_len = (u32)((n - tile_beg) < (u64)kRleTile ? (n - tile_beg) : (u64)kRleTile);
                const u32 after = tile_len - (tid * 16u + valid);
                u32 m = xp16[after >> 4];
                for (u32 k = 0; k < (after & 15u); ++k) m = gf_mulmod(m, 0x100u); // * x^8: only in the last, partial tile
                crc[j] = gf_mulmod(crc[j], m);
            } else {
                crc[j] = 0;
            }
        }
    }
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        const u32 wx = wave_xor(crc[j]);
        if (l == 0) s_wx[j][wv] = wx;
    }
    __syncthreads();
    if (tid < kSpanTiles && span * kSpanTiles + tid < ntiles) {
        int m = -1;
        u32 x = 0;
        for (u32 k = 0; k < RT / 64; ++k) {
            m = s_wmax[tid][k] > m ? s_wmax[tid][k] : m;
            x ^= s_wx[tid][k];
        }
        rb.tile_last[span * kSpanTiles + tid] = m >= 0 ? (i64)(B + (u32)m) : (i64)-1;
        rb.tile_crc[span * kSpanTiles + tid] = x;
    }
    // ---- 2., 3. the span's last run start goes out; the run start live at its first byte comes in -----------
    if (wv == 0) {
        int m = l < kSpanTiles * (RT / 64) ? s_wmax[l >> 2][l & 3u] : -1;
#pragma unroll
        for (u32 d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(m, d, 64);
            m = o > m ? o : m;
        }
        const u64 own = m >= 0 ? B + (u32)m + 1u : 0u;
        // (a span with a run start of its own settles what is live behind it; one without passes on what it finds)
        if (l == 0) op_publish(w_rs, op_word(epoch, own ? kOpIncl : kOpAgg, own));
        u64 before = 0;
        bool ok = true;
        if (span > 0) ok = span_look_back<true>(rb.lb_rs, span, epoch, rb.lb_ctl + 1, before);
        if (ok && !own && l == 0) op_publish(w_rs, op_word(epoch, kOpIncl, before));
        if (l == 0) {
            s_carry = (i64)before - 1;
            s_cphase = before ? (u32)((B - (before - 1u)) % 255u) : 0u;
            if (!ok) s_fail = 1;
            if (ok && span + 1u == nspans && out_last) *out_last = (i64)(own ? own : before) - 1;
        }
    }
    __syncthreads();
    if (s_fail) return;

    // ---- 4. per tile: carries, RLE1 byte counts, sub-tile index (k_rle_count) ------------------------------
    const i64 span_carry = s_carry;
    int tcr[kSpanTiles]; // last run start in the span's tiles in front of tile j (relative to the span, -1: none)
    {
        int run = -1;
#pragma unroll
        for (u32 j = 0; j < kSpanTiles; ++j) {
            tcr[j] = __builtin_amdgcn_readfirstlane(run); // (the same in every lane: a scalar register)
            for (u32 k = 0; k < RT / 64; ++k) run = s_wmax[j][k] > run ? s_wmax[j][k] : run;
        }
    }
    const u32 cphase = s_cphase;
    u32 exw[kSpanTiles]; // bytes the wave's lanes below this one emit
    u32 em[kSpanTiles];  // seg_emit_masks: lt4 | cg << 16
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        const int cr = tcr[j];
        int ex = __shfl_up(inc[j], 1, 64);
        if (l == 0) ex = -1;
        for (u32 k = 0; k < wv; ++k) ex = s_wmax[j][k] > ex ? s_wmax[j][k] : ex;
        if (cr > ex) ex = cr; // the run start live at the segment's first byte, relative to the span (-1: the span's carry)
        const u32 rel = j * kRleTile + tid * 16u;
        const u32 valid = full ? 16u : (B + rel + 16 <= n ? 16u : (B + rel < n ? (u32)(n - (B + rel)) : 0u));
        const u32 V = (1u << valid) - 1u;
        const u32 c0 = (ex >= 0 ? rel - (u32)ex : rel + cphase) % 255u;
        pn[j] |= c0 << 18;
        const int nxt = (int)((pn[j] >> 9) & 0x1FFu) - 1;
        u32 lastb = v[j].w >> 24;
        if (valid != 16u && valid > 0u) {
            const u32 w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            lastb = 0;
#pragma unroll
            for (u32 k = 0; k < 16; ++k)
                if (k + 1u == valid) lastb = (w[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
        }
        u32 lt4, cg;
        seg_emit_masks(E[j], V, c0, nxt != (int)lastb, lt4, cg);
        em[j] = lt4 | (cg << 16);
        const u32 cnt = (u32)__builtin_popcount(em[j]);
        const u32 incs = wave_incl_sum(cnt);
        exw[j] = incs - cnt;
        if (l == 63) s_wsum[j][wv] = incs;
        const u64 tile = span * kSpanTiles + j;
        if (tile < ntiles) {
            if (tid == 0) rb.carry_in[tile] = cr >= 0 ? (i64)(B + (u32)cr) : span_carry;
            if ((tid & 15u) == 0) rb.sub_rs[tile * 16u + (tid >> 4)] = ex >= 0 ? (i64)(B + (u32)ex) : span_carry;
        }
    }
    __syncthreads();
    u32 tile_ex[kSpanTiles]; // bytes the span emits in front of tile j
    u32 span_total = 0;
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        tile_ex[j] = span_total;
        u32 below = 0, tot = 0;
        for (u32 k = 0; k < RT / 64; ++k) {
            if (k < wv) below += s_wsum[j][k];
            tot += s_wsum[j][k];
        }
        exw[j] += (u32)__builtin_amdgcn_readfirstlane((int)below); // (wave-uniform, like tot: scalar registers)
        span_total += (u32)__builtin_amdgcn_readfirstlane((int)tot);
        const u64 tile = span * kSpanTiles + j;
        if (tile < ntiles) {
            if (tid == 0) rb.tile_count[tile] = tot;
            if ((tid & 15u) == 0) rb.sub_off[tile * 16u + (tid >> 4)] = (u16)exw[j];
        }
    }
    // ---- 5., 6., 7. the span's byte count goes out; the image offset of its first byte comes in ------------
    if (wv == 0) {
        if (l == 0) op_publish(w_off, op_word(epoch, span ? kOpAgg : kOpIncl, span_total));
        u64 base = 0;
        bool ok = true;
        if (span > 0) {
            ok = span_look_back<false>(rb.lb_off, span, epoch, rb.lb_ctl + 1, base);
            if (ok && l == 0) op_publish(w_off, op_word(epoch, kOpIncl, base + span_total));
        }
        if (l == 0) {
            s_base = base;
            if (!ok) s_fail = 1;
            if (ok && span + 1u == nspans) {
                rb.tile_off[ntiles] = base + span_total;
                *rb.total = base + span_total;
            }
        }
    }
    __syncthreads();
    if (s_fail) return;
    // ---- 8. tile offsets ------------------------------------------------------------------------------------
    const u64 base = s_base;
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j)
        if (tid == j && span * kSpanTiles + j < ntiles) rb.tile_off[span * kSpanTiles + j] = base + tile_ex[j];

    // ---- 9. the image (k_rle_scatter): staged at the offset its destination has inside a 16-byte line -------
    u8 *dst = rle + base;
    const u32 a0 = (u32)(reinterpret_cast<uintptr_t>(dst) & 15u);
#pragma unroll
    for (u32 j = 0; j < kSpanTiles; ++j) {
        const u32 w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        const u32 lt4 = em[j] & 0xFFFFu, cg = em[j] >> 16, S = ~E[j];
        u32 o = a0 + tile_ex[j] + exw[j];
        u32 c = pn[j] >> 18; // the phase of the byte at hand
#pragma unroll
        for (u32 k = 0; k < 16; ++k) {
            if ((S >> k) & 1u) c = 0;
            if ((lt4 >> k) & 1u) s_out[o++] = (u8)(w[k >> 2] >> ((k & 3u) * 8u));
            if ((cg >> k) & 1u) s_out[o++] = (u8)(c - 3u);
            c = c == 254u ? 0u : c + 1u;
        }
    }
    __syncthreads();
    u8 *line0 = dst - a0; // 16-byte aligned
    const u32 end = a0 + span_total, nlines = (end + 15u) >> 4;
    for (u32 q = tid; q < nlines; q += RT) {
        const u32 lo = q * 16u;
        if (lo >= a0 && lo + 16u <= end) {
            *reinterpret_cast<uint4 *>(line0 + lo) = *reinterpret_cast<const uint4 *>(s_out + lo);
        } else {
            const u32 b0 = lo > a0 ? lo : a0, b1 = lo + 16u < end ? lo + 16u : end;
            for (u32 b = b0; b < b1; ++b) line0[b] = s_out[b];
        }
    }
}

// ---- the front end of a BATCH of one-block inputs: one workgroup per input --------------------------------
// Every input of the batch is certain to be one block (5 * (len / 4) + len % 4 <= 100000 * level - 19), so there is no
// cut to find and nothing to learn from another input: a workgroup walks ITS input in pieces of 4 KiB, 16 bytes per
// thread, with seg_eq_mask / seg_emit_masks as k_rle_onepass, and carries from piece to piece in registers (the same
// value in every thread) the run start that is live at the piece's first byte (the phase of a byte that continues it
// is its distance from there modulo 255), the last byte of the piece in front and the image offset.  No look-back, no
// ticket, no wait.  Nothing crosses an input's edges: the byte in front of the first piece and the byte behind the last
// do not exist for the run detection (-1), and no address outside [in_off, in_off + len) is read.
// Writes the image at rle + rle_off (a slot the host sized by the bound above), the block record and the block CRC =
// CRC-32/BZIP2 of the input's bytes: every thread folds its own 16-byte segments, which lie 4 KiB apart, by Horner's
// rule, and shifts the sum to the input's end once.  An empty input gives a record with n = 0.
__global__ __launch_bounds__(RT) void k_rle_batch(const u8 *__restrict__ in, const RleBatchItem *__restrict__ items,
                                                   const u32 *__restrict__ crc_tab, const u32 *__restrict__ xp2,
                                                   u8 *__restrict__ rle, BlockDesc *__restrict__ blocks,
                                                   u32 *__restrict__ out_crc)
{
    __shared__ u32 s_tab[256];
    __shared__ int s_wmax[RT / 64];                // per wave: last run start of the piece (-1: none)
    __shared__ u32 s_wsum[RT / 64], s_wx[RT / 64]; // ... bytes emitted; (at the end) CRC
    __shared__ int s_fb[RT / 64], s_lb[RT / 64];   // ... first byte of lane 0, last byte of lane 63
    __shared__ int s_next;                         // the first byte of the next piece (-1: the input ends)
    __shared__ __attribute__((aligned(16))) u8 s_out[kRleTile / 4 * 5 + 64]; // (a piece that begins inside a chunk can emit a byte more than 5/4 of its own)

    const u32 tid = threadIdx.x, l = lane_id(), wv = tid >> 6;
    s_tab[tid] = crc_tab[tid];
    const RleBatchItem it = items[blockIdx.x];
    const u8 *src = in + it.in_off;
    const u32 n = (u32)it.len;
    u8 *dst = rle + it.rle_off; // 16-byte aligned
    int run_start = -1, last_byte = -1; // live at the piece's first byte; the byte in front of it
    u32 img = 0;                        // image bytes written so far
    u32 acc = 0, acc_end = 0, crc_part = 0; // CRC of this thread's full segments, moved to position acc_end; of its one short segment
    const u32 x_piece = xp2[12];        // x^(8 * 4096)
    __syncthreads();

    for (u32 base = 0; base < n; base += kRleTile) {
        const u32 p0 = base + tid * 16u;
        const u32 valid = p0 + 16u <= n ? 16u : (p0 < n ? n - p0 : 0u);
        uint4 v = make_uint4(0, 0, 0, 0);
        if (valid == 16u) {
            v = *reinterpret_cast<const uint4 *>(src + p0);
        } else {
            u32 t[4] = {0, 0, 0, 0};
#pragma unroll
            for (u32 k = 0; k < 16; ++k)
                if (k < valid) t[k >> 2] |= (u32)src[p0 + k] << ((k & 3u) * 8u);
            v = make_uint4(t[0], t[1], t[2], t[3]);
        }
        if (tid == 0) s_next = base + kRleTile < n ? (int)src[base + kRleTile] : -1;
        if (l == 0) s_fb[wv] = (int)(v.x & 0xFFu);
        if (l == 63) s_lb[wv] = (int)(v.w >> 24);
        __syncthreads();
        // the byte before and behind the segment: the neighbouring lane's, the neighbouring wave's, the neighbouring piece's
        int pb = __shfl_up((int)(v.w >> 24), 1, 64);
        int nb = __shfl_down((int)(v.x & 0xFFu), 1, 64);
        if (l == 0) pb = wv > 0 ? s_lb[wv > 0 ? wv - 1 : 0] : last_byte;
        if (l == 63) nb = wv + 1 < RT / 64 ? s_fb[wv + 1 < RT / 64 ? wv + 1 : 0] : s_next;
        if (valid == 0u || p0 == 0u) pb = -1;
        if (valid == 0u || p0 + valid >= n) nb = -1;
        const int piece_last_byte = s_lb[RT / 64 - 1]; // (means something only when another piece follows: this one is full then)
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        const u32 V = (1u << valid) - 1u;
        const u32 E = seg_eq_mask(v, pb) & V;
        const u32 S = ~E & V;
        const int last = S ? (int)(p0 + 31u - (u32)__builtin_clz(S)) : -1;
        const int inc = wave_incl_max32(last);
        if (l == 63) s_wmax[wv] = inc;
        // CRC of the segment
        u32 c = 0, lastb = 0;
#pragma unroll
        for (u32 k = 0; k < 16; ++k) {
            const u32 byte = (w[k >> 2] >> ((k & 3u) * 8u)) & 0xFFu;
            if (k < valid) c = s_tab[(c >> 24) ^ byte] ^ (c << 8);
            if (k + 1u == valid) lastb = byte;
        }
        if (valid == 16u) {
            acc = gf_mulmod(acc, x_piece) ^ c;
            acc_end = p0 + 16u;
        } else if (valid > 0u) {
            crc_part = c; // (the input ends with it)
        }
        __syncthreads();
        int ex = __shfl_up(inc, 1, 64); // run start live at the segment's first byte
        if (l == 0) ex = -1;
        int piece_max = -1;
        for (u32 k = 0; k < RT / 64; ++k) {
            if (k < wv) ex = s_wmax[k] > ex ? s_wmax[k] : ex;
            piece_max = s_wmax[k] > piece_max ? s_wmax[k] : piece_max;
        }
        if (run_start > ex) ex = run_start;
        const u32 c0 = ex >= 0 ? (p0 - (u32)ex) % 255u : 0u; // (byte 0 of the input is a run start: c0 is not looked at)
        u32 lt4, cg;
        seg_emit_masks(E, V, c0, nb != (int)lastb, lt4, cg);
        const u32 cnt = (u32)__builtin_popcount(lt4) + (u32)__builtin_popcount(cg);
        const u32 incs = wave_incl_sum(cnt);
        if (l == 63) s_wsum[wv] = incs;
        __syncthreads();
        u32 below = 0, tot = 0;
        for (u32 k = 0; k < RT / 64; ++k) {
            if (k < wv) below += s_wsum[k];
            tot += s_wsum[k];
        }
        // the piece's bytes, staged at the offset their destination has inside a 16-byte line (k_rle_scatter)
        const u32 a0 = img & 15u;
        {
            u32 o = a0 + below + incs - cnt;
            u32 ph = c0; // the phase of the byte at hand
#pragma unroll
            for (u32 k = 0; k < 16; ++k) {
                if ((S >> k) & 1u) ph = 0;
                if ((lt4 >> k) & 1u) s_out[o++] = (u8)(w[k >> 2] >> ((k & 3u) * 8u));
                if ((cg >> k) & 1u) s_out[o++] = (u8)(ph - 3u);
                ph = ph == 254u ? 0u : ph + 1u;
            }
        }
        __syncthreads();
        u8 *line0 = dst + (img - a0); // 16-byte aligned
        const u32 end = a0 + tot, nlines = (end + 15u) >> 4;
        for (u32 q = tid; q < nlines; q += RT) {
            const u32 lo = q * 16u;
            if (lo >= a0 && lo + 16u <= end) {
                *reinterpret_cast<uint4 *>(line0 + lo) = *reinterpret_cast<const uint4 *>(s_out + lo);
            } else {
                const u32 b0 = lo > a0 ? lo : a0, b1 = lo + 16u < end ? lo + 16u : end;
                for (u32 b = b0; b < b1; ++b) line0[b] = s_out[b];
            }
        }
        // what the next piece needs (its first barrier stands between these reads of s_out and its writes)
        if (piece_max > run_start) run_start = piece_max;
        last_byte = piece_last_byte;
        img += tot;
    }

    // the CRC: every thread's sum moved to the input's end, all of them folded, init and final NOT (k_block_crc)
    u32 x = crc_part;
    if (acc_end) x ^= gf_mulmod(acc, gf_xpow_bytes(n - acc_end, xp2));
    x = wave_xor(x);
    if (l == 0) s_wx[wv] = x;
    __syncthreads();
    if (tid == 0) {
        u32 r = 0;
        for (u32 k = 0; k < RT / 64; ++k) r ^= s_wx[k];
        r ^= gf_mulmod(0xFFFFFFFFu, gf_xpow_bytes(n, xp2));
        out_crc[blockIdx.x] = ~r;
        BlockDesc d;
        d.rle_off = it.rle_off;
        d.in_off = it.in_off;
        d.in_end = it.in_off + it.len;
        d.n = img;
        d.pad = 0;
        blocks[blockIdx.x] = d;
    }
}

// ---- kernel F: the chain of block cuts (one workgroup) -------------------------------------
// A cut depends on the previous one, but only weakly: a block holds between L and L+4 bytes
// (L = 100000*level-19; the last chunk adds at most 5), so the k-th next block starts inside
// [s + kL, s + k(L+4)].  Each of the CW waves therefore works on one FUTURE cut speculatively: it
// finds the 256-byte sub-tile holding its earliest possible target, evaluates RLE1 over a window
// from there into LDS, and lane i resolves the cut for the candidate target T+i.  The real chain
// is then CW table lookups.  One round costs the latency of ~4 dependent global loads instead of
// CW x that.  Windows are 2 KiB; data with long runs (63 output bytes can span 3.2 KB of input)
// falls back to 12 KiB windows for the round that needs it.
// Emits BlockDesc records.  emit_tail: also emit the remaining partial block.
constexpr u32 CW = 16;                               // speculative cuts per round (waves)
constexpr u32 CT = CW * 64;                          // threads
constexpr u32 CSW_SMALL = 2, CSW_BIG = 12;           // sweeps of 64 segments (1 KiB) per window
constexpr u32 CSEG = CSW_BIG * 64;                   // LDS slots per wave
constexpr u64 CUT_END = ~0ull, CUT_OUT = ~0ull - 1;

// Tiles [t_begin, ntiles) are in play; tile_off is relative to t_begin; the first block starts at
// input byte in_begin (a cut handed over by the previous rank, or 0).
__global__ __launch_bounds__(CT) void k_rle_cuts(const u8 *__restrict__ in, u64 n, u64 t_begin, u64 in_begin,
                                                  const u16 *__restrict__ sub_off,
                                                  const i64 *__restrict__ sub_rs,
                                                  const u64 *__restrict__ tile_off, u64 ntiles,
                                                  u32 block_max_len, int emit_tail,
                                                  BlockDesc *__restrict__ blocks, u32 max_blocks,
                                                  u64 *__restrict__ out_nblocks_consumed /*[3]*/)
{
    __shared__ u16 s_pre[CW][CSEG];    // inclusive count of emitted bytes, per segment, from the window start
    __shared__ u32 s_eb[CW][CSEG];     // 2 bits per position: bytes it emits
    __shared__ u16 s_ce[CW][CSEG];     // chunk-end mask
    __shared__ u64 s_res_rle[CW][64], s_res_in[CW][64];
    __shared__ u64 s_tlo[CW];

    const u32 w = threadIdx.x >> 6, l = threadIdx.x & 63u;
    const u64 L = block_max_len;
    const u64 M = tile_off[ntiles];
    u64 s_rle = 0, s_in = in_begin;
    u64 cur_tile = t_begin; // tile_off[cur_tile] < every later target
    u32 nb = 0;
    bool broken = false, ended = false; // ended: the next target's chunk ends behind the range (see phase 2b)
    u32 nsw = CSW_SMALL; // sweeps per window in this round

    while (!broken && !ended) {
        if (M < s_rle + L || M == s_rle) break; // no chunk end reaches the limit any more
        // ---- phase 1: this wave's window ------------------------------------------------
        const u64 T_lo = s_rle + (u64)(w + 1) * L; // smallest possible target of step w
        const bool alive = T_lo <= M;
        u64 t_lo = cur_tile;
        u64 in0 = 0, base_off = 0;
        i64 rs_carry = -1;
        if (alive) {
            // largest t with tile_off[t] < T_lo, galloping from cur_tile (tile_off[ntiles] = M >= T_lo)
            u64 base = cur_tile;
            while (true) { // coarse: 64 probes, 64 tiles apart
                u64 t = base + (u64)(l + 1) * 64u;
                if (t > ntiles) t = ntiles;
                const u64 bal = __ballot(tile_off[t] >= T_lo);
                if (bal) {
                    base += (u64)__builtin_ctzll(bal) * 64u;
                    break;
                }
                base += 64u * 64u;
            }
            {
                u64 t = base + (u64)(l + 1);
                if (t > ntiles) t = ntiles;
                const u64 bal = __ballot(tile_off[t] >= T_lo); // lane 63 always hits
                t_lo = base + (u64)__builtin_ctzll(bal);
            }
            // sub-tile: the last of the 16 whose start offset is still below T_lo
            const u64 toff = tile_off[t_lo];
            const u32 so = sub_off[t_lo * 16u + (l & 15u)];
            const u64 bal = __ballot((l < 16u) && (toff + so < T_lo)); // bit 0 always set
            const u32 u = 63u - (u32)__builtin_clzll(bal);
            in0 = t_lo * (u64)kRleTile + (u64)u * 256u;
            base_off = toff + (u64)__shfl(so, (int)u, 64);
            rs_carry = sub_rs[t_lo * 16u + u];
        }
        // ---- phase 2: RLE1 over the window, 64 consecutive segments (1 KiB) per sweep ----------------
        if (alive) {
            u32 off_carry = 0;
            int prev_carry = (in0 > in_begin) ? (int)in[in0 - 1] : -1;
            uint4 cur;
            u32 cur_valid;
            {
                const u64 p0 = in0 + (u64)l * 16u;
                if (p0 + 16 <= n) {
                    cur = *reinterpret_cast<const uint4 *>(in + p0);
                    cur_valid = 16;
                } else {
                    u32 t[4] = {0, 0, 0, 0};
                    cur_valid = p0 < n ? (u32)(n - p0) : 0u;
                    for (u32 k = 0; k < cur_valid; ++k) t[k >> 2] |= (u32)in[p0 + k] << ((k & 3u) * 8u);
                    cur = make_uint4(t[0], t[1], t[2], t[3]);
                }
            }
            for (u32 q = 0; q < nsw; ++q) {
                // prefetch the next sweep while this one is evaluated
                uint4 nxt = make_uint4(0, 0, 0, 0);
                u32 nxt_valid = 0;
                {
                    const u64 p0 = in0 + (u64)((q + 1) * 64u + l) * 16u;
                    if (p0 + 16 <= n) {
                        nxt = *reinterpret_cast<const uint4 *>(in + p0);
                        nxt_valid = 16;
                    } else {
                        u32 t[4] = {0, 0, 0, 0};
                        nxt_valid = p0 < n ? (u32)(n - p0) : 0u;
                        for (u32 k = 0; k < nxt_valid; ++k) t[k >> 2] |= (u32)in[p0 + k] << ((k & 3u) * 8u);
                        nxt = make_uint4(t[0], t[1], t[2], t[3]);
                    }
                }
                Seg sg;
                sg.p0 = in0 + (u64)(q * 64u + l) * 16u;
                sg.valid = cur_valid;
                sg.skip = (in_begin > sg.p0) ? (u32)((in_begin - sg.p0) < 16u ? (in_begin - sg.p0) : 16u) : 0u;
                const u32 wv[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) sg.b[k] = (u8)(wv[k >> 2] >> ((k & 3) * 8));
                // neighbours' bytes by shuffle: previous segment's last byte, next segment's first
                const int lastb = sg.valid ? (int)sg.b[(sg.valid - 1) & 15] : -1;
                const int firstb = sg.valid ? (int)sg.b[0] : -1;
                int pv = __shfl_up(lastb, 1, 64);
                if (l == 0) pv = prev_carry;
                int nx = __shfl_down(firstb, 1, 64);
                const u32 nfw = __shfl(nxt.x, 0, 64), nfv = __shfl(nxt_valid, 0, 64);
                if (l == 63) nx = nfv ? (int)(nfw & 0xFFu) : -1;
                sg.prev = (sg.valid && sg.p0 > in_begin) ? pv : -1;
                sg.next = (sg.valid == 16) ? nx : -1; // a short segment ends the input
                i64 last = -1;
                int pb = sg.prev;
#pragma unroll
                for (u32 k = 0; k < 16; ++k) {
                    if (k < sg.valid && k >= sg.skip) {
                        if ((int)sg.b[k] != pb) last = (i64)(sg.p0 + k);
                        pb = sg.b[k];
                    }
                }
                const i64 inc = wave_incl_max64(last);
                const i64 prv = __shfl_up(inc, 1, 64);
                i64 rs = (l == 0) ? (i64)-1 : prv;
                rs = rs > rs_carry ? rs : rs_carry;
                u8 e[16], cph[16];
                const u32 c = eval_seg(sg, rs, e, cph);
                u32 eb = 0, ce = 0;
#pragma unroll
                for (u32 k = 0; k < 16; ++k) {
                    if (k < sg.valid && k >= sg.skip) {
                        const int nbyte = (k + 1 < sg.valid) ? (int)sg.b[k + 1 < 16 ? k + 1 : 15] : sg.next;
                        if (nbyte != (int)sg.b[k] || cph[k] == 254u) ce |= 1u << k;
                        eb |= (u32)e[k] << (2u * k);
                    }
                }
                const u32 incs = wave_incl_sum(c);
                s_pre[w][q * 64u + l] = (u16)(off_carry + incs);
                s_eb[w][q * 64u + l] = eb;
                s_ce[w][q * 64u + l] = (u16)ce;
                const i64 winc = __shfl(inc, 63, 64);
                rs_carry = winc > rs_carry ? winc : rs_carry;
                off_carry += __shfl(incs, 63, 64);
                prev_carry = __shfl(lastb, 63, 64);
                cur = nxt;
                cur_valid = nxt_valid;
            }
        }
        __syncthreads();
        // ---- phase 2b: lane i resolves the cut for target T_lo + i -----------------------------
        {
            const u32 nseg = nsw * 64u;
            u64 r_rle = CUT_OUT, r_in = 0;
            const u64 tgt = T_lo + l;
            if (!alive || tgt > M) {
                r_rle = CUT_END;
            } else if (tgt - base_off <= (u64)s_pre[w][nseg - 1]) {
                const u32 rel = (u32)(tgt - base_off);
                u32 lo = 0, hi = nseg - 1;
                while (lo < hi) {
                    const u32 mid = (lo + hi) >> 1;
                    if ((u32)s_pre[w][mid] >= rel) hi = mid; else lo = mid + 1;
                }
                u32 seg = lo, k = 0;
                u32 acc = seg ? (u32)s_pre[w][seg - 1] : 0u;
                u32 eb = s_eb[w][seg];
                for (; k < 16; ++k) {
                    acc += (eb >> (2u * k)) & 3u;
                    if (acc >= rel) break;
                }
                // on to the end of the chunk
                bool ok = true;
                while (!((s_ce[w][seg] >> k) & 1u)) {
                    if (++k == 16u) {
                        k = 0;
                        if (++seg == nseg) {
                            ok = false;
                            break;
                        }
                        eb = s_eb[w][seg];
                    }
                    acc += (eb >> (2u * k)) & 3u;
                }
                if (ok) {
                    r_rle = base_off + acc;
                    r_in = in0 + (u64)seg * 16u + k + 1u;
                    // A chunk that BEGINS in the range and ends behind it (a run across the edge of a slab: its count
                    // byte belongs to the run's last input byte, so the range's image ends in mid-chunk) closes no
                    // block of this range: the block it would close begins here and is the next rank's first one
                    // (that rank codes the bytes in front of its slab afresh, from this block's start).
                    if (r_rle > M) r_rle = CUT_END;
                }
            }
            s_res_rle[w][l] = r_rle;
            s_res_in[w][l] = r_in;
            if (l == 0) s_tlo[w] = t_lo;
        }
        __syncthreads();
        // ---- phase 3: the real chain, CW table lookups (every thread does the same) ---------------
        const u64 round_s = s_rle;
        bool need_big = false;
        for (u32 q = 0; q < CW; ++q) {
            const u64 target = s_rle + L;
            if (M < target || M == s_rle) break;
            const u64 idx = target - (round_s + (u64)(q + 1) * L);
            if (idx > 63) { // cannot happen for q <= 15 (jitter <= 4 per step); stop the round
                if (q == 0) broken = true;
                break;
            }
            const u64 r = s_res_rle[q][idx];
            if (r == CUT_END) {
                ended = true;
                break;
            }
            if (r == CUT_OUT) {
                if (q == 0) {
                    if (nsw == CSW_BIG) broken = true; // 12 KiB always hold step 0
                    need_big = true;
                }
                break;
            }
            const u64 cut_in = s_res_in[q][idx];
            if (threadIdx.x == 0 && nb < max_blocks) {
                BlockDesc d;
                d.rle_off = s_rle;
                d.in_off = s_in;
                d.in_end = cut_in;
                d.n = (u32)(r - s_rle);
                d.pad = 0;
                blocks[nb] = d;
            }
            ++nb;
            s_rle = r;
            s_in = cut_in;
            cur_tile = s_tlo[q];
        }
        nsw = need_big ? CSW_BIG : CSW_SMALL;
        __syncthreads();
    }
    u32 tail = 0;
    if (emit_tail && M > s_rle && !broken) {
        tail = 1;
        if (threadIdx.x == 0 && nb < max_blocks) {
            BlockDesc d;
            d.rle_off = s_rle;
            d.in_off = s_in;
            d.in_end = n;
            d.n = (u32)(M - s_rle);
            d.pad = 0;
            blocks[nb] = d;
        }
        ++nb;
        s_in = n;
    }
    if (threadIdx.x == 0) {
        out_nblocks_consumed[0] = broken ? ~0ull : nb;
        out_nblocks_consumed[1] = s_in;
        out_nblocks_consumed[2] = tail; // 1: the last block is the unfinished tail, not one closed by a cut
    }
}

// ---- kernels H: the cuts from tables (no chain of launches-worth of latency, and nothing to wait for) ------
// Block j of the whole input starts at image offset S_j, and S_j lies in [j L, j (L + 4)] (a block holds L ... L + 4
// bytes), so the step S_j -> S_{j+1} -- "the end of the first chunk that ends at or behind the TARGET S_j + L" -- has
// only 4 j + 1 possible arguments.  All of them are resolved in parallel, position by position: a chunk that ends at
// image offset c_e and holds `em` bytes answers every target in (c_e - em, c_e].  A table entry is
//     (c_e - target)  [3 bits: 0 .. 4]   |   (input position behind the chunk - first byte of the step's first tile) << 3
// and the real chain is then one look-up per block -- or one per SIXTEEN blocks through the composed table
// (`k_cut_compose`).  Offsets are those of the image of the WHOLE input (g_base = offset of the range's first byte:
// a rank of a sharded job knows it from an all-gather of the slabs' totals) and so is j: a rank fills the tables for
// the targets inside its slab, (g_base, own_hi], BEFORE the cut of the rank in front of it arrives, and what is left
// of its link of the chain is `k_cut_select`: about a hundred dependent loads.  0xFFFFFFFF = a target of another rank.
__host__ __device__ __forceinline__ u64 cut_tbase(u64 j_lo, u64 j) // entries of the steps j_lo ... j - 1
{
    return 2u * (j * (j - 1u) - j_lo * (j_lo - 1u)) + (j - j_lo);
}
__host__ __device__ __forceinline__ u64 cut_cbase(u64 g_lo, u64 g) // composed entries of the groups g_lo ... g - 1
{
    return 32u * (g * (g - 1u) - g_lo * (g_lo - 1u)) + (g - g_lo);
}

// largest t in [lo, hi] with off[t] < v (off[lo] < v is given)
__device__ __forceinline__ u64 cut_last_below(const u64 *__restrict__ off, u64 lo, u64 hi, u64 v)
{
    while (lo < hi) {
        const u64 mid = (lo + hi + 1) >> 1;
        if (off[mid] < v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one thread per step: the tiles that hold the chunk ends of its targets
__global__ __launch_bounds__(256) void k_cut_steps(CutPlan pl, const u64 *__restrict__ tile_off, u64 *__restrict__ step_t0,
                                                    u32 *__restrict__ step_nt)
{
    const u64 gid = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 j = pl.j_lo + gid;
    if (j > pl.j_hi) return;
    const u64 lb = (j + 1u) * pl.L;
    const u64 w_lo = lb > pl.w_min ? lb : pl.w_min;
    const u64 w_hi = lb + 4u * j < pl.own_hi ? lb + 4u * j : pl.own_hi;
    u64 ta = pl.tb;
    u32 nt = 0;
    if (w_lo <= w_hi) {
        // (targets at or below g_base: the chunk that answers them began in front of the range and ends in its first tiles)
        if (w_lo > pl.g_base) ta = cut_last_below(tile_off, pl.tb, pl.t1, w_lo - pl.g_base);
        u64 te = (w_hi > pl.g_base ? cut_last_below(tile_off, ta, pl.t1, w_hi - pl.g_base) : ta) + 1u; // (a chunk may end in the tile behind)
        if (te > pl.t_eval) te = pl.t_eval;
        if (ta > pl.t_eval) ta = pl.t_eval;
        nt = (u32)(te - ta + 1u);
    }
    step_t0[gid] = ta;
    step_nt[gid] = nt;
}

// exclusive sum of step_nt -> step_w0[0 .. nsteps], one workgroup
__global__ __launch_bounds__(1024) void k_cut_steps_scan(const u32 *__restrict__ step_nt, u64 nsteps, u64 *__restrict__ step_w0)
{
    __shared__ u64 sh[16];
    u64 run = 0;
    for (u64 b0 = 0; b0 < nsteps; b0 += 1024u) {
        const u64 b = b0 + threadIdx.x;
        const u64 v = b < nsteps ? (u64)step_nt[b] : 0u;
        u64 total;
        const u64 ex = wg_excl<false>(v, sh, total);
        if (b < nsteps) step_w0[b] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) step_w0[nsteps] = run;
}

// one workgroup per (step, tile): the RLE1 evaluation of k_rle_count, and every chunk end answers its targets
__global__ __launch_bounds__(RT) void k_cut_table(CutPlan pl, const u8 *__restrict__ in, u64 n_lim,
                                                   const i64 *__restrict__ carry_in, const u64 *__restrict__ tile_off,
                                                   const u64 *__restrict__ step_t0, const u64 *__restrict__ step_w0,
                                                   u64 nsteps, u32 *__restrict__ tab)
{
    __shared__ i64 s_m[RT / 64 + 1];
    __shared__ u32 s_s[RT / 64];
    // the step this workgroup belongs to: last gid with step_w0[gid] <= blockIdx.x
    u64 lo = 0, hi = nsteps - 1u;
    while (lo < hi) {
        const u64 mid = (lo + hi + 1) >> 1;
        if (step_w0[mid] <= (u64)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const u64 gid = lo, j = pl.j_lo + gid;
    const u64 t_first = step_t0[gid];
    const u64 tile = t_first + ((u64)blockIdx.x - step_w0[gid]);
    const u64 lb = (j + 1u) * pl.L;
    const u64 w_lo = lb > pl.w_min ? lb : pl.w_min;
    const u64 w_hi = lb + 4u * j < pl.own_hi ? lb + 4u * j : pl.own_hi;
    const u64 in_ref = t_first * (u64)kRleTile;
    u32 *__restrict__ row = tab + cut_tbase(pl.j_lo, j);

    Seg s;
    load_seg(in, n_lim, tile, s, 0);
    const i64 rs = seg_run_start(s, carry_in[tile], s_m);
    u8 e[16], cph[16];
    const u32 cnt = eval_seg(s, rs, e, cph);
    u32 tot;
    const u32 ex = block_excl_sum(cnt, s_s, tot);
    u64 cum = pl.g_base + tile_off[tile] + ex;
    if (cum + cnt < w_lo || cum > w_hi + 4u) return; // none of this segment's chunk ends answers a target of the step
#pragma unroll
    for (u32 k = 0; k < 16; ++k) {
        if (k < s.valid && k >= s.skip) {
            cum += e[k];
            const int nbyte = (k + 1 < s.valid) ? (int)s.b[k + 1 < 16 ? k + 1 : 15] : s.next;
            if (nbyte != (int)s.b[k] || cph[k] == 254u) {
                const u32 c = cph[k];
                const u64 em = c < 3u ? c + 1u : 5u;
                const u64 t_lo = cum - em + 1u > w_lo ? cum - em + 1u : w_lo;
                const u64 t_hi = cum < w_hi ? cum : w_hi;
                const u32 rel = (u32)(s.p0 + k + 1u - in_ref) << 3;
                for (u64 T = t_lo; T <= t_hi; ++T) row[T - lb] = (u32)(cum - T) | rel;
            }
        }
    }
}

// sixteen steps in one: comp[g][i] = how far a block start with index i at step 16 g has drifted sixteen steps on
// (0xFFFF: one of them leaves this rank's targets)
__global__ __launch_bounds__(256) void k_cut_compose(CutPlan pl, u64 g_lo, const u32 *__restrict__ tab, u16 *__restrict__ comp)
{
    const u64 g = g_lo + blockIdx.y;
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 j0 = g * 16u;
    if (i > 4u * j0) return;
    u64 idx = i;
    bool ok = true;
    for (u32 q = 0; q < 16u; ++q) {
        const u32 en = tab[cut_tbase(pl.j_lo, j0 + q) + idx];
        if (en == 0xFFFFFFFFu) {
            ok = false;
            break;
        }
        idx += en & 7u;
    }
    comp[cut_cbase(g_lo, g) + i] = ok ? (u16)(idx - i) : (u16)0xFFFFu;
}

// The chain itself: from block j0 with image offset s0 (its first input byte: start_in).  Thread 0 follows the
// composed tables and notes where every stretch begins; the threads then walk the stretches and write the records.
// res[0] blocks (~0: the tables did not answer an owned target -- never seen; the caller falls back to k_rle_cuts),
// res[1] input bytes consumed, res[2] tail flag, res[3] image offset and res[4] number of the next rank's first block.
constexpr u32 kCutSegCap = 4096;
__global__ __launch_bounds__(256) void k_cut_select(CutPlan pl, u64 j0, u64 s0, u64 start_in, u64 g_lo, u64 g_hi, u64 n,
                                                    long long rle_bias, int emit_tail, const u32 *__restrict__ tab,
                                                    const u16 *__restrict__ comp, const u64 *__restrict__ step_t0,
                                                    BlockDesc *__restrict__ blocks, u32 max_blocks, u64 *__restrict__ res)
{
    __shared__ u32 sg_j[kCutSegCap]; // relative to j0
    __shared__ u32 sg_idx[kCutSegCap];
    __shared__ u8 sg_n[kCutSegCap];
    __shared__ u64 s_stop[3]; // j, idx at the stop; 1 if the tables failed
    __shared__ u32 s_nseg;
    if (threadIdx.x == 0) {
        u64 j = j0, idx = s0 - j0 * pl.L;
        u32 ns = 0;
        u64 bad = (s0 < j0 * pl.L || idx > 4u * j0) ? 1u : 0u;
        while (!bad) {
            const u64 target = (j + 1u) * pl.L + idx;
            if (target > pl.own_hi) break; // the target lies behind this rank's image
            if (ns >= kCutSegCap) {
                bad = 1;
                break;
            }
            // A target among the last four bytes of this rank's image may belong to a chunk that ends BEHIND the image (a
            // run across the edge of the slab: its count byte is the next slab's): such a chunk is evaluated by the next
            // rank (w_min), the block it closes is that rank's first one, and the chain of this rank stops here.
            if (j > pl.j_hi || j < pl.j_lo) {
                if (target + 4u <= pl.own_hi) bad = 1;
                break;
            }
            if ((j & 15u) == 0 && g_hi >= g_lo && (j >> 4) >= g_lo && (j >> 4) <= g_hi) {
                const u16 c = comp[cut_cbase(g_lo, j >> 4) + idx];
                if (c != 0xFFFFu) {
                    sg_j[ns] = (u32)(j - j0);
                    sg_idx[ns] = (u32)idx;
                    sg_n[ns] = 16;
                    ++ns;
                    idx += c;
                    j += 16u;
                    continue;
                }
            }
            const u32 en = tab[cut_tbase(pl.j_lo, j) + idx];
            if (en == 0xFFFFFFFFu) {
                if (target + 4u <= pl.own_hi) bad = 1; // an owned target without an answer (else: the next rank's, see above)
                break;
            }
            sg_j[ns] = (u32)(j - j0);
            sg_idx[ns] = (u32)idx;
            sg_n[ns] = 1;
            ++ns;
            idx += en & 7u;
            j += 1u;
        }
        s_stop[0] = j;
        s_stop[1] = idx;
        s_stop[2] = bad;
        s_nseg = ns;
    }
    __syncthreads();
    const u64 j_stop = s_stop[0], s_end = j_stop * pl.L + s_stop[1];
    const u32 ns = s_nseg;
    const u64 nb = j_stop - j0;
    const bool tail = emit_tail && !s_stop[2] && pl.own_hi > s_end;
    if (s_stop[2]) {
        if (threadIdx.x == 0) {
            res[0] = ~0ull;
            res[1] = start_in;
            res[2] = 0;
            res[3] = s0;
            res[4] = j0;
        }
        return;
    }
    for (u32 q = threadIdx.x; q < ns; q += 256u) {
        u64 j = j0 + sg_j[q], idx = sg_idx[q];
        for (u32 w = 0; w < sg_n[q]; ++w, ++j) {
            const u32 en = tab[cut_tbase(pl.j_lo, j) + idx];
            const u64 cut_in = step_t0[j - pl.j_lo] * (u64)kRleTile + (u64)(en >> 3);
            const u64 k = j - j0;
            if (k < max_blocks) {
                blocks[k].rle_off = (u64)((long long)(j * pl.L + idx) + rle_bias);
                blocks[k].in_end = cut_in;
                blocks[k].n = (u32)(pl.L + (en & 7u));
                blocks[k].pad = 0;
                if (k == 0) blocks[k].in_off = start_in;
            }
            if (k + 1u < max_blocks) blocks[k + 1u].in_off = cut_in;
            if (j + 1u == j_stop) res[1] = tail ? n : cut_in;
            idx += en & 7u;
        }
    }
    if (threadIdx.x == 0) {
        if (nb == 0) res[1] = tail ? n : start_in;
        if (tail && nb < max_blocks) {
            blocks[nb].rle_off = (u64)((long long)s_end + rle_bias);
            if (nb == 0) blocks[nb].in_off = start_in;
            blocks[nb].in_end = n;
            blocks[nb].n = (u32)(pl.own_hi - s_end);
            blocks[nb].pad = 0;
        }
        res[0] = nb + (tail ? 1u : 0u);
        res[2] = tail ? 1u : 0u;
        res[3] = s_end;
        res[4] = j_stop;
    }
}

// ---- kernel G: block CRC from tile CRCs -------------------------------------------
__global__ __launch_bounds__(RT) void k_block_crc(const u8 *__restrict__ in,
                                                   const BlockDesc *__restrict__ blocks,
                                                   const u32 *__restrict__ crc_tab,
                                                   const u32 *__restrict__ xp2,
                                                   const u32 *__restrict__ tile_crc,
                                                   u32 *__restrict__ out_crc)
{
    __shared__ u32 s_tab[256];
    __shared__ u32 s_x[RT / 64];
    s_tab[threadIdx.x] = crc_tab[threadIdx.x];
    __syncthreads();
    const BlockDesc d = blocks[blockIdx.x];
    const u64 a = d.in_off, b = d.in_end;
    const u64 ft = (a + kRleTile - 1) / kRleTile; // first full tile
    const u64 lt = b / kRleTile;                  // one past the last full tile
    u32 acc = 0;
    if (ft >= lt) {
        // short range: 16-byte pieces straight from the bytes
        for (u64 p = a + (u64)threadIdx.x * 16u; p < b; p += (u64)RT * 16u) {
            const u64 len = (b - p) < 16u ? (b - p) : 16u;
            const u32 c = crc_bytes_raw(in + p, len, s_tab);
            acc ^= gf_mulmod(c, gf_xpow_bytes(b - (p + len), xp2));
        }
    } else {
        const u64 head_end = ft * kRleTile, tail_beg = lt * kRleTile;
        // head and tail pieces
        for (u64 p = a + (u64)threadIdx.x * 16u; p < head_end; p += (u64)RT * 16u) {
            const u64 len = (head_end - p) < 16u ? (head_end - p) : 16u;
            const u32 c = crc_bytes_raw(in + p, len, s_tab);
            acc ^= gf_mulmod(c, gf_xpow_bytes(b - (p + len), xp2));
        }
        for (u64 p = tail_beg + (u64)threadIdx.x * 16u; p < b; p += (u64)RT * 16u) {
            const u64 len = (b - p) < 16u ? (b - p) : 16u;
            const u32 c = crc_bytes_raw(in + p, len, s_tab);
            acc ^= gf_mulmod(c, gf_xpow_bytes(b - (p + len), xp2));
        }
        // full tiles: each thread folds a contiguous run of tiles
        const u64 nt = lt - ft;
        const u64 per = (nt + RT - 1) / RT;
        const u64 t0 = ft + (u64)threadIdx.x * per;
        const u64 t1 = (t0 + per < lt) ? t0 + per : lt;
        if (t0 < t1) {
            const u32 xt = xp2[12]; // x^(8*4096)
            u32 c = 0;
            for (u64 t = t0; t < t1; ++t) c = gf_mulmod(c, xt) ^ tile_crc[t];
            acc ^= gf_mulmod(c, gf_xpow_bytes(b - t1 * kRleTile, xp2));
        }
    }
    const u32 wx = wave_xor(acc);
    if (lane_id() == 0) s_x[threadIdx.x >> 6] = wx;
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 x = 0;
        for (u32 k = 0; k < RT / 64; ++k) x ^= s_x[k];
        // init 0xFFFFFFFF rides through the whole message; final NOT (crc32.rs:128-131)
        x ^= gf_mulmod(0xFFFFFFFFu, gf_xpow_bytes(b - a, xp2));
        out_crc[blockIdx.x] = ~x;
    }
}

// ---- host launchers -----------------------------------------------------------------
// last run start inside tiles [t0,t1) (-1: none)
__global__ __launch_bounds__(1024) void k_slab_last(const i64 *__restrict__ tile_last, u64 t0, u64 t1,
                                                     i64 *__restrict__ out)
{
    __shared__ i64 s_m[1024];
    i64 m = -1;
    for (u64 t = t0 + threadIdx.x; t < t1; t += 1024) m = tile_last[t] > m ? tile_last[t] : m;
    s_m[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 k = 1; k < 1024; ++k) m = s_m[k] > m ? s_m[k] : m;
        *out = m;
    }
}

void launch_slab_last(hipStream_t st, const RleBuffers &rb, u64 t0, u64 t1, i64 *d_out)
{
    hipLaunchKernelGGL(k_slab_last, dim3(1), dim3(1024), 0, st, rb.tile_last, t0, t1, d_out);
}

// The split is driven in three steps so that a multi-GPU job can shard it by slabs of tiles:
//   scan   : tiles [t0,t1): run starts + tile CRCs; *out_last = last run start of the range
//   count  : tiles [t0,t1): carries from `init_carry`, RLE1 byte counts, sub-tile index
//   finish : prefix over [tb,t1), the cut chain from byte in_begin, the RLE1 image
void launch_rle_scan(hipStream_t st, const u8 *d_in, u64 n, u64 t0, u64 t1, u64 in_begin, const u32 *crc_tab,
                     const u32 *xp16, const RleBuffers &rb)
{
    if (t1 <= t0) return;
    hipLaunchKernelGGL(k_rle_tile_scan, dim3((u32)(t1 - t0)), dim3(RT), 0, st, d_in, n, t0, in_begin, crc_tab, xp16,
                       rb.tile_last, rb.tile_crc);
}

void launch_rle_count(hipStream_t st, const u8 *d_in, u64 n, u64 t0, u64 t1, u64 in_begin, i64 init_carry,
                      const RleBuffers &rb, i64 *d_out_last)
{
    if (t1 <= t0) return;
    // carry_in[t] = last run start before tile t (from init_carry); *d_out_last = the range's last run start
    tiles_scan<true>(st, rb.tile_last, rb.carry_in, t0, t1, reinterpret_cast<i64 *>(rb.scan_part), init_carry, d_out_last,
                     nullptr);
    hipLaunchKernelGGL(k_rle_count, dim3((u32)(t1 - t0)), dim3(RT), 0, st, d_in, n, t0, in_begin, rb.carry_in,
                       rb.tile_count, rb.sub_off, rb.sub_rs);
}

void launch_rle_prefix(hipStream_t st, u64 tb, u64 t1, const RleBuffers &rb, bool write_end)
{
    // tile_off[tb] = 0 ... tile_off[t1] = total (offsets are relative to the range); write_end = false leaves
    // tile_off[t1] alone (it is the first offset of a range that has its own)
    if (t1 <= tb) {
        (void)hipMemsetAsync(rb.total, 0, 8, st);
        if (write_end) (void)hipMemsetAsync(rb.tile_off + tb, 0, 8, st);
        return;
    }
    tiles_scan<false>(st, rb.tile_count, rb.tile_off, tb, t1, rb.scan_part, 0ull, rb.total, write_end ? rb.tile_off + t1 : nullptr);
}

// The chain of cuts is one workgroup that reads the input and the tile tables, not the image: the two are
// separate launches (one GPU: side by side on two streams; a rank of a sharded job: the cuts first, the cut is
// handed to the next rank, then the image).
void launch_rle_cuts(hipStream_t st, const u8 *d_in, u64 n, u64 tb, u64 t1, u64 in_begin, const RleBuffers &rb,
                     u32 block_max_len, int emit_tail, BlockDesc *d_blocks, u32 max_blocks)
{
    if (t1 <= tb) {
        (void)hipMemsetAsync(rb.cut_result, 0, 3 * sizeof(u64), st);
        return;
    }
    hipLaunchKernelGGL(k_rle_cuts, dim3(1), dim3(CT), 0, st, d_in, n, tb, in_begin, rb.sub_off, rb.sub_rs,
                       rb.tile_off, t1, block_max_len, emit_tail, d_blocks, max_blocks, rb.cut_result);
}
void launch_rle_image(hipStream_t st, const u8 *d_in, u64 n, u64 tb, u64 t1, u64 in_begin, const RleBuffers &rb, u8 *d_rle)
{
    if (t1 <= tb) return;
    hipLaunchKernelGGL(k_rle_scatter, dim3((u32)(t1 - tb)), dim3(RT), 0, st, d_in, n, tb, in_begin, rb.carry_in,
                       rb.tile_off, d_rle);
}

// The whole front end for an engine that codes the input from byte 0: every table of the three steps above and the
// image, in one launch (k_rle_onepass).  rb.lb_ctl[0] counts the spans handed out and rb.lb_ctl[1] is set by a look-back
// that gave up: the caller reads both.  *d_out_last = the input's last run start, rb.total = bytes of the image.
u64 rle_onepass_spans(u64 ntiles) { return (ntiles + kSpanTiles - 1u) / kSpanTiles; }
u32 rle_onepass_epochs() { return kOpEpochs; }
void launch_rle_onepass(hipStream_t st, const u8 *d_in, u64 n, u64 ntiles, u32 epoch, const u32 *crc_tab, const u32 *xp16,
                        const RleBuffers &rb, u8 *d_rle, i64 *d_out_last)
{
    (void)hipMemsetAsync(rb.lb_ctl, 0, 16, st);
    hipLaunchKernelGGL(k_rle_onepass, dim3((u32)rle_onepass_spans(ntiles)), dim3(RT), 0, st, d_in, n, ntiles,
                       (u32)rle_onepass_spans(ntiles), epoch, crc_tab, xp16, rb, d_rle, d_out_last);
}

// The cuts from tables, in three steps (see "kernels H"): the steps' tiles (the caller reads step_w0[nsteps], the number
// of workgroups of the table kernel), the tables, the chain.
u64 cut_table_entries(const CutPlan &pl) { return pl.j_hi >= pl.j_lo ? cut_tbase(pl.j_lo, pl.j_hi + 1u) : 0u; }
void cut_groups(const CutPlan &pl, u64 *g_lo, u64 *g_hi, u64 *entries)
{
    // groups of sixteen steps that lie inside [j_lo, j_hi]; *g_hi < *g_lo: none
    *g_lo = (pl.j_lo + 15u) / 16u;
    *g_hi = *g_lo;
    *entries = 0;
    if (pl.j_hi < pl.j_lo || pl.j_hi + 1u < (*g_lo + 1u) * 16u) {
        *g_lo = 1;
        *g_hi = 0;
        return;
    }
    *g_hi = (pl.j_hi + 1u) / 16u - 1u;
    *entries = cut_cbase(*g_lo, *g_hi + 1u);
}
u32 cut_seg_cap() { return kCutSegCap; }
void launch_cut_steps(hipStream_t st, const CutPlan &pl, const RleBuffers &rb, const CutBuffers &cb)
{
    const u64 nsteps = pl.j_hi - pl.j_lo + 1u;
    if (nsteps == 0) return; // (cut_tables_prepare does not get here without steps)
    hipLaunchKernelGGL(k_cut_steps, dim3((u32)((nsteps + 255u) / 256u)), dim3(256), 0, st, pl, rb.tile_off, cb.step_t0, cb.step_nt);
    // (the exclusive sum of the steps' tile counts, by the three-kernel scan of the tile offsets instead of one workgroup
    // that walks the steps 1024 at a time (k_cut_steps_scan, rounds 4-5).  For the 1 189 blocks of a GiB there are about
    // 1 200 steps and either form is microseconds of work; the kernel trace shows it at 1.5 ms only because it runs beside
    // k_rle_scatter and waits for a CU -- nothing the step time sees.  The workgroup totals live behind step_w0's
    // nsteps + 1 entries.)
    tiles_scan<false>(st, cb.step_nt, cb.step_w0, 0, nsteps, cb.step_w0 + nsteps + 2, 0ull, cb.step_w0 + nsteps, nullptr);
}
void launch_cut_tables(hipStream_t st, const CutPlan &pl, const u8 *d_in, u64 n_lim, const RleBuffers &rb, const CutBuffers &cb,
                       u64 work_total)
{
    const u64 nsteps = pl.j_hi - pl.j_lo + 1u;
    (void)hipMemsetAsync(cb.tab, 0xFF, cut_table_entries(pl) * 4u, st);
    if (work_total)
        hipLaunchKernelGGL(k_cut_table, dim3((u32)work_total), dim3(RT), 0, st, pl, d_in, n_lim, rb.carry_in, rb.tile_off, cb.step_t0,
                           cb.step_w0, nsteps, cb.tab);
    u64 g_lo, g_hi, ce;
    cut_groups(pl, &g_lo, &g_hi, &ce);
    if (g_hi >= g_lo)
        hipLaunchKernelGGL(k_cut_compose, dim3((u32)((4u * 16u * g_hi + 256u) / 256u), (u32)(g_hi - g_lo + 1u)), dim3(256), 0, st, pl,
                           g_lo, cb.tab, cb.comp);
}
void launch_cut_select(hipStream_t st, const CutPlan &pl, u64 j0, u64 s0, u64 start_in, u64 n, long long rle_bias, int emit_tail,
                       const RleBuffers &rb, const CutBuffers &cb, BlockDesc *d_blocks, u32 max_blocks)
{
    u64 g_lo, g_hi, ce;
    cut_groups(pl, &g_lo, &g_hi, &ce);
    hipLaunchKernelGGL(k_cut_select, dim3(1), dim3(256), 0, st, pl, j0, s0, start_in, g_lo, g_hi, n, rle_bias, emit_tail, cb.tab,
                       cb.comp, cb.step_t0, d_blocks, max_blocks, rb.cut_result);
}

void launch_block_crc(hipStream_t st, const u8 *d_in, const BlockDesc *d_blocks, u32 nblocks,
                      const u32 *crc_tab, const u32 *xp2, const u32 *tile_crc, u32 *d_crc)
{
    if (nblocks == 0) return;
    hipLaunchKernelGGL(k_block_crc, dim3(nblocks), dim3(RT), 0, st, d_in, d_blocks, crc_tab, xp2, tile_crc,
                       d_crc);
}


// The front end of a batch of one-block inputs: one workgroup per input, a record and a CRC per input (k_rle_batch).
void launch_rle_batch(hipStream_t st, const u8 *d_in, const RleBatchItem *d_items, u32 count, const u32 *crc_tab,
                      const u32 *xp2, u8 *d_rle, BlockDesc *d_blocks, u32 *d_crc)
{
    if (count == 0) return;
    hipLaunchKernelGGL(k_rle_batch, dim3(count), dim3(RT), 0, st, d_in, d_items, crc_tab, xp2, d_rle, d_blocks, d_crc);
}

} // namespace bzgpu
