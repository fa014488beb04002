// k_gz_members.hip -- every member of a gzip file (include/bz2_mi355x.h section 6, DESIGN_deflate.md "Every member of a
// gzip file"): where members may start, their spans as a batch image for the decode kernels of k_inflate.hip (which are
// used as they are), the zeros between members, and the members' bytes put side by side.
//
// k_gz_member_search<false>: candidates per tile of gzmem::kTile byte positions; <true>: behind the host's exclusive sum,
//   the candidates numbered [first, first + n) as an ascending list.  A position reads its own four bytes, whichever tile
//   or wave they lie in, and nothing at or behind in + len.
// k_gz_member_gather: spans of the input -> an image in which each starts at a multiple of 4 (whole words are stored; the
//   bytes of a last, partial word that lie behind the span are zero).
// k_gz_zero_skip: a wave per position: the first byte at or behind it that is not zero, in front of a bound.
// k_gz_members_compact: spans that start at multiples of 16 -> contiguous bytes, exactly `len` of each.
#include <hip/hip_runtime.h>

#include "bzgpu.h"
#include "k_deflate.h"
#include "gz_members.h"

namespace dfgpu {
using namespace bzgpu;

namespace {
constexpr u32 kTileWords = gzmem::kTile / 4;
constexpr u32 kCopyChunk = 16384; // bytes of a span per workgroup and step

// the word at `byte` (a multiple of 4; `in` is 16-byte aligned); bytes at and behind len read as zero and are not touched
__device__ __forceinline__ u32 gz_word(const u8 *in, u32 len, u64 byte)
{
    if (byte + 4 <= len) return *reinterpret_cast<const u32 *>(in + byte);
    u32 v = 0;
    for (u32 k = 0; k < 4 && byte + k < len; ++k) v |= (u32)in[byte + k] << (8 * k);
    return v;
}
// bit k: byte position 4 * wi + k is a candidate
__device__ __forceinline__ u32 gz_mask(const u8 *in, u32 len, u64 wi)
{
    const u64 byte = 4 * wi;
    if (byte >= len) return 0;
    const u64 v = (u64)gz_word(in, len, byte) | (u64)gz_word(in, len, byte + 4) << 32;
    u32 m = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        if (byte + k + 4 <= len && gzmem::candidate_word((u32)(v >> (8 * k)))) m |= 1u << k;
    return m;
}
} // namespace

// Thread t looks at words t, t + 256, t + 512, t + 768 of its tile.  <false>: cnt[tile] = candidates.  <true>: base[tile]
// = candidates in front of the tile; candidate number i of the input goes to list[i - first] if first <= i < first + n.
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_gz_member_search(const u8 *__restrict__ in, u32 len, u32 tile0, u32 *cnt, const u32 *__restrict__ base,
                                                          u32 first, u32 n, u32 *list)
{
    __shared__ u32 s_c[256];
    __shared__ u32 s_sum;
    const u32 t = threadIdx.x, tile = tile0 + blockIdx.x;
    if (!SCATTER) {
        if (t == 0) s_sum = 0;
        __syncthreads();
        u32 c = 0;
        for (u32 r = 0; r < 4; ++r) c += (u32)__popc(gz_mask(in, len, (u64)tile * kTileWords + r * 256u + t));
        if (c) atomicAdd(&s_sum, c);
        __syncthreads();
        if (t == 0) cnt[tile] = s_sum;
        return;
    }
    u32 run = base[tile];
    for (u32 r = 0; r < 4; ++r) {
        const u64 wi = (u64)tile * kTileWords + r * 256u + t;
        const u32 m = gz_mask(in, len, wi);
        if (!__syncthreads_or((int)m)) continue; // (nearly every step of nearly every tile)
        s_c[t] = (u32)__popc(m);
        __syncthreads();
        u32 mine = 0, all = 0;
        for (u32 q = 0; q < 256; ++q) {
            if (q == t) mine = all;
            all += s_c[q];
        }
        u32 i = run + mine;
        for (u32 k = 0; k < 4; ++k)
            if (m & (1u << k)) {
                if (i >= first && i - first < n) list[i - first] = (u32)(4 * wi + k);
                ++i;
            }
        run += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_gz_member_gather(const u8 *__restrict__ in, const GzSpan *__restrict__ spans, u8 *image)
{
    const GzSpan s = spans[blockIdx.x];
    const u8 *src = in + s.src;
    u32 *dst = reinterpret_cast<u32 *>(image + s.dst); // (a multiple of 4 in a 16-byte-aligned buffer)
    for (u64 lo = (u64)blockIdx.y * kCopyChunk; lo < s.len; lo += (u64)gridDim.y * kCopyChunk)
        for (u64 b = lo + 4ull * threadIdx.x; b < lo + kCopyChunk && b < s.len; b += 1024u) {
            u32 v = 0;
            for (u32 k = 0; k < 4 && b + k < s.len; ++k) v |= (u32)src[b + k] << (8 * k);
            dst[b >> 2] = v;
        }
}

// out[j] = the first p in [from[j], bound[j]) with in[p] != 0, or bound[j]
__global__ __launch_bounds__(64) void k_gz_zero_skip(const u8 *__restrict__ in, const u32 *__restrict__ from, const u32 *__restrict__ bound, u32 *out)
{
    const u32 lane = threadIdx.x, j = blockIdx.x;
    const u64 hi = bound[j];
    u64 res = hi;
    for (u64 o = from[j]; o < hi; o += 64u) {
        const u64 p = o + lane;
        const u64 m = __ballot(p < hi && in[p] != 0);
        if (m) {
            res = o + (u32)__ffsll((long long)m) - 1u;
            break;
        }
    }
    if (lane == 0) out[j] = (u32)res;
}

__global__ __launch_bounds__(256) void k_gz_members_compact(const u8 *__restrict__ staged, const GzSpan *__restrict__ spans, u8 *out)
{
    const GzSpan s = spans[blockIdx.x];
    const u8 *src = staged + s.src; // (a multiple of 16)
    u8 *dst = out + s.dst;
    const bool aligned = ((uintptr_t)dst & 3u) == 0;
    for (u64 lo = (u64)blockIdx.y * kCopyChunk; lo < s.len; lo += (u64)gridDim.y * kCopyChunk)
        for (u64 b = lo + 4ull * threadIdx.x; b < lo + kCopyChunk && b < s.len; b += 1024u) {
            if (b + 4 <= s.len) {
                const u32 v = *reinterpret_cast<const u32 *>(src + b);
                if (aligned) *reinterpret_cast<u32 *>(dst + b) = v;
                else
                    for (u32 k = 0; k < 4; ++k) dst[b + k] = (u8)(v >> (8 * k));
            } else
                for (u32 k = 0; b + k < s.len; ++k) dst[b + k] = src[b + k];
        }
}

int df_launch_gz_search_count(hipStream_t st, const u8 *in, u32 len, u32 ntiles, u32 *cnt)
{
    hipLaunchKernelGGL((k_gz_member_search<false>), dim3(ntiles), dim3(256), 0, st, in, len, 0u, cnt, nullptr, 0u, 0u, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_gz_search_list(hipStream_t st, const u8 *in, u32 len, u32 tile0, u32 ntiles, const u32 *base, u32 first, u32 n, u32 *list)
{
    hipLaunchKernelGGL((k_gz_member_search<true>), dim3(ntiles), dim3(256), 0, st, in, len, tile0, nullptr, base, first, n, list);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

static u32 gz_copy_rows(u32 max_len)
{
    const u32 rows = max_len / kCopyChunk + 1u;
    return rows < 64u ? rows : 64u;
}

int df_launch_gz_gather(hipStream_t st, const u8 *in, const GzSpan *spans, u32 count, u32 max_len, u8 *image)
{
    hipLaunchKernelGGL(k_gz_member_gather, dim3(count, gz_copy_rows(max_len)), dim3(256), 0, st, in, spans, image);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_gz_zero_skip(hipStream_t st, const u8 *in, const u32 *from, const u32 *bound, u32 count, u32 *out)
{
    hipLaunchKernelGGL(k_gz_zero_skip, dim3(count), dim3(64), 0, st, in, from, bound, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_gz_compact(hipStream_t st, const u8 *staged, const GzSpan *spans, u32 count, u32 max_len, u8 *out)
{
    hipLaunchKernelGGL(k_gz_members_compact, dim3(count, gz_copy_rows(max_len)), dim3(256), 0, st, staged, spans, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace dfgpu
