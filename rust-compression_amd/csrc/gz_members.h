// gz_members.h -- every member of a gzip file (include/bz2_mi355x.h section 6, DESIGN_deflate.md "Every member of a gzip
// file"): the rule that says where a member MAY start (a candidate) and the rules that say whether it DOES (the walk).
// They exist here only: k_gz_member_search (k_gz_members.hip) runs the candidate rule with one byte position per lane,
// df_members_core (deflate_engine.hip) walks.
//
// A candidate is a byte position p with in[p .. p + 3] == 1f 8b 08 and no reserved FLG bit in in[p + 3], all four bytes
// inside the input: the first four header rules of k_df_inflate (kind 2), so every member the one-member decoder accepts
// starts at one.  The converse does not hold (a stored block may hold a whole .gz file), which is what the walk is for.
//
// Plain C++17 without HIP headers (tests/host_stub/gz_members_check.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifndef BZ_HD
#ifdef __HIPCC__
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif
#endif

namespace gzmem {

constexpr uint32_t kTile = 4096;       // byte positions per workgroup of the search
constexpr uint32_t kSubBatch = 16384;  // candidates decoded per sizes launch (BZ_DF_GZ_BATCH)
constexpr uint32_t kJunkBytes = 64;    // what the one-member decoder is shown of a position that is no candidate
constexpr int kOk = 0, kEof = -2;      // BZ_OK, BZ_E_EOF (static_assert'ed where the public header is in sight)

// the four bytes at p as a little-endian word
BZ_HD inline bool candidate_word(uint32_t x) { return (x & 0xE0FFFFFFu) == 0x00088B1Fu; }

BZ_HD inline bool candidate_at(const uint8_t *in, uint64_t len, uint64_t p)
{
    if (p + 4 > len) return false;
    return candidate_word((uint32_t)in[p] | (uint32_t)in[p + 1] << 8 | (uint32_t)in[p + 2] << 16 | (uint32_t)in[p + 3] << 24);
}

// ---- the walk.  What the decoder left for a CONFIRMED member whose span is [start, span_end): its verdict, where it ended
// (start + end_bit / 8: behind the trailer of a clean member) and `nonzero`, the first byte at or behind that end which is
// not zero, looked for up to `bound` -- the next candidate at or behind the end, or the input's end -- and equal to
// `bound` if there is none in front of it.
enum class Step {
    Extend,  // BZ_E_EOF at the span's end with input behind it: a false candidate cut the member short; decode it again
             // over a longer span
    Fault,   // the member's verdict is the stream's
    End,     // clean, and only zeros (or nothing) up to the input's end: BZ_OK
    Next,    // clean, and the next candidate is where the zeros end: it is confirmed
    Junk     // clean, and the zeros end at a byte that is no candidate: the bytes from there are decoded as one more member, so
             // that the decoder's own header rules give the verdict.  kJunkBytes of them are enough: a position that is no
             // candidate fails inside its first four bytes (or the input ends inside them), whatever follows
};

BZ_HD inline Step walk_step(int verdict, uint64_t span_end, uint64_t nonzero, uint64_t bound, uint64_t len)
{
    if (verdict == kEof && span_end < len) return Step::Extend;
    if (verdict != kOk) return Step::Fault;
    if (nonzero < bound) return Step::Junk;
    return bound == len ? Step::End : Step::Next;
}

// The r-th extension (r = 1, 2, ...) of the member at candidate i reaches to candidate i + 2^r: 1, 2, 4, ... candidates
// more each time, so f false candidates inside one member cost ceil(log2(f + 1)) decodes.  At or behind `total` (the
// number of candidates) the span reaches the input's end, where BZ_E_EOF is the truth.
BZ_HD inline uint64_t extend_to(uint64_t i, uint32_t r) { return r >= 63u ? ~0ull : i + (1ull << r); }

} // namespace gzmem
