// k_bgzf_read.hip -- reading BGZF (include/bz2_mi355x.h section 8, DESIGN_deflate.md "Reading BGZF"): the kernels around the
// one-pass decode (k_bgzf_inflate instantiates the decode loop of k_inflate.hip and lives there, with k_bgzf_check).
//
// k_bgzf_search<false>: candidates per tile of bgzf::kTile byte positions; <true>: behind the host's exclusive sum, the
//   candidates numbered [first, first + n) as an ascending list of 64-bit positions.  A candidate is a position at which
//   the 16-byte header rule of bgzf_index.h holds with at least 18 bytes behind it.  A position reads its own bytes,
//   whichever tile or wave they lie in, and nothing at or behind in + len.
// k_bgzf_block_info: BSIZE + 1 of every listed candidate, and its ISIZE where the block lies whole inside the input.
// k_bgzf_edge_copy: the slice of an edge block that belongs to the range, from its slot of the workspace into place.
#include <hip/hip_runtime.h>

#include "bzgpu.h"
#include "k_deflate.h"
#include "bgzf_index.h"

namespace dfgpu {
using namespace bzgpu;

namespace {
constexpr u32 kTileWords = bgzf::kTile / 4;

// the word at `byte` (a multiple of 4; `in` is 16-byte aligned); bytes at and behind len read as zero and are not touched
__device__ __forceinline__ u32 bg_word(const u8 *in, u64 len, u64 byte)
{
    if (byte + 4 <= len) return *reinterpret_cast<const u32 *>(in + byte);
    u32 v = 0;
    for (u32 k = 0; k < 4 && byte + k < len; ++k) v |= (u32)in[byte + k] << (8 * k);
    return v;
}
// bit k: byte position 4 * wi + k is a candidate.  Nearly every word fails on its first four bytes; the rest of the
// sixteen is loaded behind that.
__device__ __forceinline__ u32 bg_mask(const u8 *in, u64 len, u64 wi)
{
    const u64 byte = 4 * wi;
    if (byte + bgzf::kHeader > len) return 0;
    const u64 v = (u64)bg_word(in, len, byte) | (u64)bg_word(in, len, byte + 4) << 32;
    u32 m = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        if ((u32)(v >> (8 * k)) == 0x04088B1Fu && byte + k + bgzf::kHeader <= len) m |= 1u << k;
    if (!m) return 0;
    const u32 w2 = bg_word(in, len, byte + 8), w3 = bg_word(in, len, byte + 12), w4 = bg_word(in, len, byte + 16);
    const u64 a = (u64)w2 | (u64)w3 << 32, b = (u64)w3 | (u64)w4 << 32; // bytes 8 .. 15 and 12 .. 19 behind `byte`
    u32 res = 0;
#pragma unroll
    for (u32 k = 0; k < 4; ++k)
        if ((m & (1u << k)) && bgzf::header_words(0x04088B1Fu, (u32)(a >> (8 * k)), (u32)(b >> (8 * k)))) res |= 1u << k;
    return res;
}
} // namespace

// Thread t looks at words t, t + 256, t + 512, t + 768 of its tile.  <false>: cnt[tile] = candidates.  <true>: base[tile]
// = candidates in front of the tile; candidate number i of the input goes to list[i - first] if first <= i < first + n.
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_bgzf_search(const u8 *__restrict__ in, u64 len, u32 tile0, u32 *cnt, const u64 *__restrict__ base, u64 first,
                                                     u32 n, u64 *list)
{
    __shared__ u32 s_c[256];
    __shared__ u32 s_sum;
    const u32 t = threadIdx.x, tile = tile0 + blockIdx.x;
    if (!SCATTER) {
        if (t == 0) s_sum = 0;
        __syncthreads();
        u32 c = 0;
        for (u32 r = 0; r < 4; ++r) c += (u32)__popc(bg_mask(in, len, (u64)tile * kTileWords + r * 256u + t));
        if (c) atomicAdd(&s_sum, c);
        __syncthreads();
        if (t == 0) cnt[tile] = s_sum;
        return;
    }
    u64 run = base[tile];
    for (u32 r = 0; r < 4; ++r) {
        const u64 wi = (u64)tile * kTileWords + r * 256u + t;
        const u32 m = bg_mask(in, len, wi);
        if (!__syncthreads_or((int)m)) continue; // (nearly every step of nearly every tile)
        s_c[t] = (u32)__popc(m);
        __syncthreads();
        u32 mine = 0, all = 0;
        for (u32 q = 0; q < 256; ++q) {
            if (q == t) mine = all;
            all += s_c[q];
        }
        u64 i = run + mine;
        for (u32 k = 0; k < 4; ++k)
            if (m & (1u << k)) {
                if (i >= first && i - first < n) list[i - first] = 4 * wi + k;
                ++i;
            }
        run += all;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_bgzf_block_info(const u8 *__restrict__ in, u64 len, const u64 *__restrict__ list, u32 n, BgzfInfo *info)
{
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 p = list[i]; // (a candidate: p + 18 <= len)
    BgzfInfo o;
    o.bsize1 = ((u32)in[p + 16] | (u32)in[p + 17] << 8) + 1u;
    o.isize = 0;
    if (o.bsize1 >= bgzf::kMinBlock && o.bsize1 <= len - p) o.isize = bgzf::le32(in + p + o.bsize1 - 4);
    info[i] = o;
}

__global__ __launch_bounds__(256) void k_bgzf_edge_copy(const BgzfDesc *__restrict__ desc, const u8 *__restrict__ slots, u8 *out)
{
    const BgzfDesc q = desc[blockIdx.x];
    const u8 *src = slots + (size_t)(q.slot - 1u) * bgzf::kMaxBlock + q.lo;
    u8 *dst = out + q.dst;
    for (u32 i = threadIdx.x; i < q.n; i += 256u) dst[i] = src[i];
}

int df_launch_bgzf_search_count(hipStream_t st, const u8 *in, u64 len, u32 ntiles, u32 *cnt)
{
    hipLaunchKernelGGL((k_bgzf_search<false>), dim3(ntiles), dim3(256), 0, st, in, len, 0u, cnt, nullptr, 0ull, 0u, nullptr);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_bgzf_search_list(hipStream_t st, const u8 *in, u64 len, u32 tile0, u32 ntiles, const u64 *base, u64 first, u32 n, u64 *list)
{
    hipLaunchKernelGGL((k_bgzf_search<true>), dim3(ntiles), dim3(256), 0, st, in, len, tile0, nullptr, base, first, n, list);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_bgzf_block_info(hipStream_t st, const u8 *in, u64 len, const u64 *list, u32 n, BgzfInfo *info)
{
    hipLaunchKernelGGL(k_bgzf_block_info, dim3((n + 255u) / 256u), dim3(256), 0, st, in, len, list, n, info);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int df_launch_bgzf_edge_copy(hipStream_t st, const BgzfDesc *desc, u32 count, const u8 *slots, u8 *out)
{
    hipLaunchKernelGGL(k_bgzf_edge_copy, dim3(count), dim3(256), 0, st, desc, slots, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace dfgpu
