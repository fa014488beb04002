// k_lha.hip -- the kernels of the LHA archive reader (include/bz2_mi355x.h section 11, DESIGN_lzhuf.md section 12).
//
// k_lha_crc16: CRC-16/ARC (reflected 0xA001, initial value 0, no final XOR) of every member's bytes, piecewise.  The register
//   is linear in the data because it starts at zero: crc(A || B) = crc(A) * x^(8 |B|) mod P ^ crc(B).  Grid (part, member):
//   a workgroup folds one part of a member, thread t the slice [t * s, (t + 1) * s) of it (s a multiple of 16: 16-byte loads
//   from 16-aligned outputs), moves its register to the end of the part and the workgroup XORs the 256 registers.
// k_lha_crc16_join: one thread per member combines its parts and compares with the header's value.
// k_lha_store: stored members from any byte phase of the archive to their 16-aligned places, exactly their bytes.
// k_lha_pack (the writer, section 12): spans of headers, streams and stored inputs to ANY byte phase of the archive.  Two
//   neighbours meet inside one 16-byte line, so a span's ragged head and tail go byte by byte and only its interior lines are
//   whole 16-byte stores, built from aligned source words with funnel shifts; nothing outside a span is written, nothing
//   behind a span's last source byte is read.
#include <hip/hip_runtime.h>

#include "k_lha.h"
#include "../../include/bz2_mi355x.h"

namespace lhagpu {

namespace {
constexpr u32 kPoly = 0xA001u;
constexpr u32 kStoreChunk = 16384; // bytes of a span per workgroup and step

__device__ __forceinline__ u32 lha_gf_mul(u32 a, u32 b) // a * b in GF(2)[x] / P, reflected (bit 15 = x^0)
{
    u32 pr = 0;
    for (u32 m = 1u << 15; m != 0 && a != 0; m >>= 1) {
        if (a & m) { pr ^= b; a &= ~m; }
        b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return pr;
}
__device__ __forceinline__ u32 lha_gf_xpow8(u64 nbytes) // x^(8 * nbytes) mod P
{
    u32 r = 1u << 15, sq = 1u << 7;
    while (nbytes) {
        if (nbytes & 1u) r = lha_gf_mul(r, sq);
        sq = lha_gf_mul(sq, sq);
        nbytes >>= 1;
    }
    return r;
}
__device__ __forceinline__ u32 lha_fold_word(u32 c, u32 w, const u16 *tab)
{
#pragma unroll
    for (u32 k = 0; k < 4; ++k) c = tab[(c ^ (w >> (8 * k))) & 0xFFu] ^ (c >> 8);
    return c;
}
} // namespace

__global__ __launch_bounds__(256) void k_lha_crc16(const u8 *__restrict__ data, const LhaCrcJob *__restrict__ jobs, u32 njobs, u32 part_bytes,
                                                   u32 *__restrict__ part_crc)
{
    __shared__ u16 s_tab[256];
    __shared__ u32 s_red[kCrcThreads / kWave];
    const u32 t = threadIdx.x;
    {
        u32 c = t;
        for (u32 k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
        s_tab[t] = (u16)c;
    }
    __syncthreads();
    for (u32 j = blockIdx.y; j < njobs; j += gridDim.y) {
        const LhaCrcJob job = jobs[j];
        const u64 nparts = lha_crc_parts(job.len, part_bytes);
        for (u64 part = blockIdx.x; part < nparts; part += gridDim.x) {
            const u64 lo = part * part_bytes;
            const u32 n = job.len - lo < part_bytes ? (u32)(job.len - lo) : part_bytes;
            const u32 slice = ((n + kCrcThreads - 1) / kCrcThreads + 15u) & ~15u;
            const u32 a = t * slice < n ? t * slice : n, b = a + slice < n ? a + slice : n;
            const u8 *p = data + job.off + lo; // (16-byte aligned: the output's place, the part and the slice are multiples of 16)
            u32 c = 0, i = a;
#pragma unroll 4
            for (; i + 16 <= b; i += 16) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p + i);
                c = lha_fold_word(c, v.x, s_tab);
                c = lha_fold_word(c, v.y, s_tab);
                c = lha_fold_word(c, v.z, s_tab);
                c = lha_fold_word(c, v.w, s_tab);
            }
            for (; i < b; ++i) c = s_tab[(c ^ p[i]) & 0xFFu] ^ (c >> 8); // (the member's last bytes: nothing behind them is read)
            if (c) c = lha_gf_mul(c, lha_gf_xpow8(n - b));
#pragma unroll
            for (u32 d = kWave / 2; d != 0; d >>= 1) c ^= (u32)__shfl_xor((int)c, (int)d, (int)kWave);
            if ((t & (kWave - 1)) == 0) s_red[t / kWave] = c;
            __syncthreads();
            if (t == 0) part_crc[(u64)job.pbase + part] = s_red[0] ^ s_red[1] ^ s_red[2] ^ s_red[3];
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void k_lha_crc16_join(const LhaCrcJob *__restrict__ jobs, u32 njobs, u32 part_bytes, const u32 *__restrict__ part_crc,
                                                        LhaCrcRes *__restrict__ res)
{
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= njobs) return;
    const LhaCrcJob job = jobs[j];
    const u64 nparts = lha_crc_parts(job.len, part_bytes);
    u32 c = 0;
    const u32 xp = nparts > 1 ? lha_gf_xpow8(part_bytes) : 0u;
    for (u64 k = 0; k < nparts; ++k) { // c holds parts [0, k); part k has nb bytes
        const u64 left = job.len - k * part_bytes;
        const u32 nb = left < part_bytes ? (u32)left : part_bytes;
        if (c) c = lha_gf_mul(c, nb == part_bytes ? xp : lha_gf_xpow8(nb));
        c ^= part_crc[(u64)job.pbase + k];
    }
    res[j].crc = c;
    res[j].verdict = c == job.want ? BZ_OK : BZ_E_DATA;
}

__global__ __launch_bounds__(256) void k_lha_store(const u8 *__restrict__ in, u64 in_len, const dfgpu::GzSpan *__restrict__ spans, u8 *out)
{
    const dfgpu::GzSpan s = spans[blockIdx.x];
    u8 *dst = out + s.dst; // (a multiple of 16 in a 16-byte-aligned buffer)
    for (u64 lo = (u64)blockIdx.y * kStoreChunk; lo < s.len; lo += (u64)gridDim.y * kStoreChunk)
        for (u64 b = lo + 16ull * threadIdx.x; b < lo + kStoreChunk && b < s.len; b += 16u * 256u) {
            const u64 src = s.src + b;
            if (b + 16 <= s.len && src + 20 <= in_len) { // five aligned words hold the sixteen bytes, all inside the archive
                const u32 *w = reinterpret_cast<const u32 *>(in + (src & ~(u64)3));
                const u32 sh = ((u32)src & 3u) * 8u;
                const u32 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                uint4 v;
                v.x = __funnelshift_r(w0, w1, sh);
                v.y = __funnelshift_r(w1, w2, sh);
                v.z = __funnelshift_r(w2, w3, sh);
                v.w = __funnelshift_r(w3, w4, sh);
                *reinterpret_cast<uint4 *>(dst + b) = v;
            } else
                for (u32 k = 0; k < 16 && b + k < s.len; ++k) dst[b + k] = in[src + k];
        }
}

__global__ __launch_bounds__(256) void k_lha_pack(const u8 *__restrict__ blob, const u8 *__restrict__ streams, const u8 *__restrict__ in,
                                                  const LhaPackSpan *__restrict__ spans, u8 *out)
{
    const LhaPackSpan s = spans[blockIdx.x];
    const u8 *src = (s.which == kPackBlob ? blob : s.which == kPackStream ? streams : in) + s.src;
    u8 *dst = out + s.dst;
    const u64 to_line = (0 - (u64)reinterpret_cast<uintptr_t>(dst)) & 15u;
    const u64 head = to_line < s.len ? to_line : s.len, lines = (s.len - head) & ~(u64)15, tail = s.len - head - lines;
    const u32 t = threadIdx.x;
    if (blockIdx.y == 0) { // the bytes that share a line with a neighbour
        if (t < head) dst[t] = src[t];
        if (t < tail) dst[head + lines + t] = src[head + lines + t];
    }
    src += head;
    dst += head; // (a multiple of 16)
    const u32 ph = (u32)reinterpret_cast<uintptr_t>(src) & 15u, sh = (ph & 3u) * 8u; // (the same for every line of the span)
    for (u64 lo = (u64)blockIdx.y * kStoreChunk; lo < lines; lo += (u64)gridDim.y * kStoreChunk)
        for (u64 b = lo + 16ull * t; b < lo + kStoreChunk && b < lines; b += 16u * 256u) {
            uint4 v;
            if (ph == 0) v = *reinterpret_cast<const uint4 *>(src + b);
            else if (sh == 0 || b + 20 - (ph & 3u) <= lines + tail) { // the aligned words end inside the span
                const u32 *w = reinterpret_cast<const u32 *>(src + b - (ph & 3u));
                const u32 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = sh ? w[4] : 0u;
                v.x = __funnelshift_r(w0, w1, sh);
                v.y = __funnelshift_r(w1, w2, sh);
                v.z = __funnelshift_r(w2, w3, sh);
                v.w = __funnelshift_r(w3, w4, sh);
            } else {
                u32 q[4];
#pragma unroll
                for (u32 k = 0; k < 4; ++k)
                    q[k] = (u32)src[b + 4 * k] | (u32)src[b + 4 * k + 1] << 8 | (u32)src[b + 4 * k + 2] << 16 | (u32)src[b + 4 * k + 3] << 24;
                v = make_uint4(q[0], q[1], q[2], q[3]);
            }
            *reinterpret_cast<uint4 *>(dst + b) = v;
        }
}

int lha_launch_crc16(hipStream_t st, const u8 *data, const LhaCrcJob *jobs, u32 njobs, u64 max_parts, u32 part_bytes, u32 *part_crc)
{
    if (njobs == 0 || max_parts == 0) return 0;
    const u32 gx = max_parts < 0x7FFFFFFFull ? (u32)max_parts : 0x7FFFFFFFu, gy = njobs < 65535u ? njobs : 65535u;
    hipLaunchKernelGGL(k_lha_crc16, dim3(gx, gy), dim3(kCrcThreads), 0, st, data, jobs, njobs, part_bytes, part_crc);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lha_launch_crc16_join(hipStream_t st, const LhaCrcJob *jobs, u32 njobs, u32 part_bytes, const u32 *part_crc, LhaCrcRes *res)
{
    if (njobs == 0) return 0;
    hipLaunchKernelGGL(k_lha_crc16_join, dim3((njobs + 255u) / 256u), dim3(256), 0, st, jobs, njobs, part_bytes, part_crc, res);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lha_launch_store(hipStream_t st, const u8 *in, u64 in_len, const dfgpu::GzSpan *spans, u32 count, u32 max_len, u8 *out)
{
    if (count == 0) return 0;
    const u32 rows = max_len / kStoreChunk + 1u;
    hipLaunchKernelGGL(k_lha_store, dim3(count, rows < 64u ? rows : 64u), dim3(256), 0, st, in, in_len, spans, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lha_launch_pack(hipStream_t st, const u8 *blob, const u8 *streams, const u8 *in, const LhaPackSpan *spans, u32 count, u64 max_len, u8 *out)
{
    if (count == 0) return 0;
    const u64 rows = max_len / kStoreChunk + 1u;
    hipLaunchKernelGGL(k_lha_pack, dim3(count, rows < 64u ? (u32)rows : 64u), dim3(256), 0, st, blob, streams, in, spans, out);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

} // namespace lhagpu
