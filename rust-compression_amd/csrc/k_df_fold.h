// k_df_fold.h -- the piecewise checksum folds shared by the Deflate encode kernels (k_df_sums, k_df_batch_wrap:
// k_deflate.hip) and the decode side's checksum kernel (k_df_inflate_check: k_inflate.hip).
// Reflected CRC-32 (crc32.rs:40-55): crc(A || B) = crc(A) * x^(8 |B|) ^ crc(B) for registers that start at zero.
// Adler-32 (adler32.rs:20-66): a piece of `len` bytes contributes (sum of bytes, sum of (len - i) * byte).
#pragma once
#include "k_deflate.h"

namespace dfgpu {
__device__ __forceinline__ u32 df_gf_mul(u32 a, u32 b) // a * b in GF(2)[x] / P, reflected (bit 31 = x^0)
{
    u32 pr = 0;
    for (u32 m = 1u << 31; m != 0 && a != 0; m >>= 1) {
        if (a & m) { pr ^= b; a &= ~m; }
        b = (b & 1u) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return pr;
}
__device__ __forceinline__ u32 df_gf_xpow8(u32 nbytes) // x^(8 * nbytes) mod P
{
    u32 r = 1u << 31, sq = 1u << 23;
    while (nbytes) {
        if (nbytes & 1u) r = df_gf_mul(r, sq);
        sq = df_gf_mul(sq, sq);
        nbytes >>= 1;
    }
    return r;
}

// one byte of a piece: the Adler sums with the byte's weight (bytes from it to the end of the piece) and the CRC register
__device__ __forceinline__ void df_fold_byte(u32 d, u64 weight, const u32 *tab, u64 &a, u64 &b, u32 &c)
{
    a += d;
    b += weight * d;
    c = tab[(c ^ d) & 0xFFu] ^ (c >> 8);
}
// the register of a whole input from the register of its bytes for a zero initial value (crc32.rs:74-78)
__device__ __forceinline__ u32 df_crc_finish(u32 raw, u32 len) { return raw ^ df_gf_mul(0xFFFFFFFFu, df_gf_xpow8(len)) ^ 0xFFFFFFFFu; }
} // namespace dfgpu
