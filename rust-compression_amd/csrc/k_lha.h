// k_lha.h -- what lha_engine.hip launches from k_lha.hip (include/bz2_mi355x.h sections 11 and 12).
#pragma once
#include "bzgpu.h"
#include "k_deflate.h"

namespace lhagpu {
using namespace bzgpu;

constexpr u32 kCrcThreads = 256;
constexpr u32 kCrcPartMin = kCrcThreads * 16u; // bytes: a part is a multiple of this, so every slice is a multiple of 16

// one member's bytes for the CRC launch and its join
struct LhaCrcJob {
    u64 off;   // where its bytes lie in the output (a multiple of 16)
    u64 len;
    u32 pbase; // its first part's place among all partials
    u32 want;  // the header's CRC-16
};
struct LhaCrcRes {
    u32 crc;
    int32_t verdict; // BZ_OK, or BZ_E_DATA: the CRC differs from the header's
};

__host__ __device__ inline u64 lha_crc_parts(u64 len, u32 part_bytes) { return (len + part_bytes - 1) / part_bytes; }

// part_crc[job.pbase + k] = the register of part k of every job (part_bytes: a multiple of kCrcPartMin)
int lha_launch_crc16(hipStream_t st, const u8 *data, const LhaCrcJob *jobs, u32 njobs, u64 max_parts, u32 part_bytes, u32 *part_crc);
int lha_launch_crc16_join(hipStream_t st, const LhaCrcJob *jobs, u32 njobs, u32 part_bytes, const u32 *part_crc, LhaCrcRes *res);
// spans of the archive (any byte phase) -> out + dst (multiples of 16), exactly len bytes of each
int lha_launch_store(hipStream_t st, const u8 *in, u64 in_len, const dfgpu::GzSpan *spans, u32 count, u32 max_len, u8 *out);

// the writer (section 12): `len` bytes from blob, streams or in (`which`) + src to out + dst, at any byte phase
constexpr u32 kPackBlob = 0, kPackStream = 1, kPackInput = 2;
struct LhaPackSpan {
    u64 src, dst, len;
    u32 which, pad;
};
// every span in one launch; exactly the spans' bytes are written, nothing behind a span's last source byte is read
int lha_launch_pack(hipStream_t st, const u8 *blob, const u8 *streams, const u8 *in, const LhaPackSpan *spans, u32 count, u64 max_len, u8 *out);
} // namespace lhagpu
