// k_lzhuf.h -- what the LZHUF decode kernel (k_lzhuf.hip) and its driver (lzhuf_engine.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include "bzgpu.h"

namespace lzhgpu {
using namespace bzgpu;

// what a launch leaves per entry (the sizes launch writes it, the writing launch reads len as its store limit)
struct LzhRec {
    u64 end_bit;  // bits consumed, at most 8 * in_len
    u32 len;      // bytes produced
    int verdict;  // BZ_OK, BZ_E_DATA, BZ_E_EOF
    u32 nblk;     // blocks decoded whole
    u32 nlit;     // literal codes
    u32 nmatch;   // match codes
    u32 flags;    // bit 0: the output would reach 4 GiB
};
static_assert(sizeof(LzhRec) == 32, "LzhRec is copied between host and device as it is");

constexpr u64 kNoLen = ~0ull; // orig_len: not known

// dbits: dictionary_bits, pbits: offset_bits of the method; orig_len: nullptr or one u64 per entry
int lzh_launch_decode(hipStream_t st, bool write, const u8 *in, const u64 *in_off, const u64 *in_len, const u64 *orig_len, u32 count,
                      u32 dbits, u32 pbits, int prefill, u8 *out, const u64 *out_off, LzhRec *rec);
} // namespace lzhgpu
