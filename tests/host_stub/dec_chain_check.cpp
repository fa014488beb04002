// dec_chain_check.cpp -- csrc/dec_chain.h on the host (tests/test_dec_chain_host.py): the record chain's rules driven
// over forged byte strings.  A block is the byte 0x31 and filler bits of a chosen length, described to the chain by a
// hand-written record (start bit, end_bit, stored_crc, next_head, next_bits) the way kernel D1 describes a real one.
// Exits non-zero at the first failure.
#include "../../rust-compression_amd/csrc/dec_chain.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "dec_chain_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                               \
        }                                                                           \
    } while (0)

// the input: `nbits` bits in a heap block of exactly the bytes that hold them (a read past it is the sanitizer's finding)
struct MemBits {
    u8 *p;
    u64 nbits;
    MemBits(const std::vector<u8> &bytes, u64 nb) : p(static_cast<u8 *>(malloc((size_t)((nb + 7) / 8) + !nb))), nbits(nb)
    {
        memcpy(p, bytes.data(), (size_t)((nb + 7) / 8));
    }
    MemBits(const MemBits &) = delete;
    ~MemBits() { free(p); }
    u32 read(u64 &pos, u32 n) // the short-read contract
    {
        const u64 avail = nbits > pos ? nbits - pos : 0;
        const u32 k = avail < n ? (u32)avail : n;
        u32 v = 0;
        for (u32 i = 0; i < k; ++i) v = (v << 1) | ((p[(pos + i) >> 3] >> (7u - (u32)((pos + i) & 7u))) & 1u);
        pos += k;
        return v;
    }
};

struct Rec {
    u64 start, end_bit;
    u32 stored_crc, status, next_head, next_bits;
};

struct Forge {
    std::vector<u8> bytes;
    u64 nbits = 0;
    std::vector<Rec> recs;
    u32 combined = 0;
    void put(u32 v, u32 n)
    {
        for (u32 i = n; i-- > 0; ++nbits) {
            if ((nbits & 7) == 0) bytes.push_back(0);
            bytes.back() |= (u8)(((v >> i) & 1u) << (7u - (u32)(nbits & 7)));
        }
    }
    void header(u32 digit = 0x39u, const char *bzh = "BZh")
    {
        for (int i = 0; i < 3; ++i) put((u8)bzh[i], 8);
        put(digit, 8);
        combined = 0;
    }
    void block(u32 filler_bits, u32 crc, u32 head = 0x31u)
    {
        Rec r = {nbits, 0, crc, 0, 0, 0};
        put(head, 8);
        for (u32 i = 0; i < filler_bits; ++i) put((i * 7u + 3u) % 5u == 0, 1);
        r.end_bit = nbits;
        recs.push_back(r);
        combined = ((combined << 1) | (combined >> 31)) ^ crc; // (this file's own rotate-xor)
    }
    void trailer(u32 head = 0x17u) { trailer_crc(combined, head); }
    void trailer_crc(u32 crc, u32 head = 0x17u)
    {
        static const u8 rest[5] = {0x72, 0x45, 0x38, 0x50, 0x90};
        put(head, 8);
        for (u8 b : rest) put(b, 8);
        put(crc, 32);
        while (nbits & 7) put(0, 1);
    }
};

struct Result {
    int verdict; // 0 clean end, 1 Data, 2 MagicFirst, 3 Magic, 4 a block without a record
    u32 stream_no, blocks;
    u64 pos;
    bool operator==(const Result &o) const { return verdict == o.verdict && stream_no == o.stream_no && blocks == o.blocks && pos == o.pos; }
};

// what D1 says of every block for an input of `nbits` bits: a block that does not end inside it fails; the 8 bits behind
// one are read like every other read
static std::vector<Rec> describe(const Forge &f, MemBits &rd)
{
    std::vector<Rec> recs = f.recs;
    for (Rec &r : recs) {
        r.status = r.end_bit > rd.nbits;
        u64 p = r.end_bit;
        r.next_head = rd.read(p, 8);
        r.next_bits = r.status ? 0 : (u32)(p - r.end_bit);
    }
    return recs;
}
static const Rec *find(const std::vector<Rec> &recs, u64 start)
{
    for (const Rec &r : recs)
        if (r.start == start) return &r;
    return nullptr;
}

// the chain through dec_chain.h; use_next false: every head byte comes from the reader
static Result run_chain(const Forge &f, u64 nbits, bool use_next)
{
    MemBits rd(f.bytes, nbits);
    const std::vector<Rec> recs = describe(f, rd);
    ChainState s;
    Result r = {0, 0, 0, 0};
    for (;;) {
        const ChainEvent ev = chain_open_record(s, rd, nbits);
        if (ev == ChainEvent::StreamEnd) {
            if (s.combined != 0 || !s.need_header || s.have_next) r.verdict = 99;
            else continue;
        } else if (ev == ChainEvent::Block) {
            const Rec *b = find(recs, s.pos);
            if (b && !b->status) {
                chain_take_block(s, b->end_bit, b->stored_crc, b->next_head, b->next_bits);
                if (!use_next) s.have_next = false;
                r.blocks += 1;
                continue;
            }
            r.verdict = b ? 1 : 4;
        } else {
            r.verdict = ev == ChainEvent::End ? 0 : ev == ChainEvent::Data ? 1 : ev == ChainEvent::MagicFirst ? 2 : 3;
        }
        break;
    }
    r.stream_no = s.stream_no;
    r.pos = s.pos;
    return r;
}

// The expectation: the host loop of decode_core as it stood before dec_chain.h, transcribed statement by statement
// (one batch, no partial input, no shards).  It is this test's table, not library code.
static Result expect_chain(const Forge &f, u64 nbits)
{
    MemBits rd(f.bytes, nbits);
    const std::vector<Rec> recs = describe(f, rd);
    u64 pos = 0;
    u32 stream_no = 1, combined = 0, blocks = 0, next_head = 0, next_bits = 0;
    bool need_header = true, have_next = false;
    int term = 0;
    for (;;) {
        if (need_header) {
            (void)rd.read(pos, 8);
            (void)rd.read(pos, 8);
            (void)rd.read(pos, 8);
            const u32 lv = rd.read(pos, 8);
            if (lv < 0x31u || lv > 0x39u) {
                term = (stream_no == 1) ? 2 : 3;
                break;
            }
            need_header = false;
        }
        u64 p = pos;
        u32 head;
        if (have_next) {
            head = next_head;
            p = pos + next_bits;
            have_next = false;
        } else {
            head = rd.read(p, 8);
        }
        if (head == 0x31u) {
            const Rec *bi = find(recs, pos);
            if (!bi) {
                term = 4;
                break;
            }
            if (bi->status) {
                term = 1;
                break;
            }
            blocks += 1;
            combined = ((combined << 1) | (combined >> 31)) ^ bi->stored_crc;
            pos = bi->end_bit;
            have_next = true;
            next_head = bi->next_head;
            next_bits = bi->next_bits;
        } else if (head == 0x17u) {
            pos = p;
            for (int k = 0; k < 5; ++k) (void)rd.read(pos, 8);
            const u32 stored = rd.read(pos, 32);
            if (stored != combined) {
                term = 1;
                break;
            }
            pos = (pos + 7ull) & ~7ull;
            if (pos > nbits) pos = nbits;
            if (nbits - pos >= 8) {
                need_header = true;
                combined = 0;
                stream_no += 1;
            } else {
                break; // the clean end
            }
        } else {
            term = 1;
            break;
        }
    }
    return Result{term, stream_no, blocks, pos};
}

// both head-byte paths against the transcription; -> the result
static int g_bad = 0;
static Result chain(const Forge &f, u64 nbits)
{
    const Result a = run_chain(f, nbits, true), b = run_chain(f, nbits, false), e = expect_chain(f, nbits);
    if (!(a == e) || !(b == e)) {
        fprintf(stderr, "dec_chain_check: %llu bits: verdict %d/%d, expected %d; stream %u/%u, %u; blocks %u/%u, %u; pos %llu/%llu, %llu\n",
                (unsigned long long)nbits, a.verdict, b.verdict, e.verdict, a.stream_no, b.stream_no, e.stream_no, a.blocks, b.blocks,
                e.blocks, (unsigned long long)a.pos, (unsigned long long)b.pos, (unsigned long long)e.pos);
        g_bad += 1;
    }
    return a;
}
static Result chain(const Forge &f) { return chain(f, f.nbits); }

// one stream of `nblocks` blocks whose last one ends at bit phase `phase`
static void stream(Forge &f, u32 nblocks, u32 phase, u32 digit = 0x39u, const char *bzh = "BZh")
{
    f.header(digit, bzh);
    for (u32 b = 0; b < nblocks; ++b) {
        u32 fill = 11 + 5 * b;
        if (b + 1 == nblocks) fill += (8 + phase - (u32)((f.nbits + 8 + fill) & 7)) & 7;
        f.block(fill, 0x80000001u * (b + 1) + 0x1234567u);
    }
    f.trailer();
}

static int run()
{
    // bit phases: the trailer is unaligned and still pads to a byte
    for (u32 nblocks : {0u, 1u, 3u})
        for (u32 phase = 0; phase < 8; ++phase) {
            Forge f;
            stream(f, nblocks, phase);
            CHECK(nblocks == 0 || (f.recs.back().end_bit & 7) == phase);
            CHECK(f.nbits % 8 == 0 && f.nbits < 8 * 64);
            CHECK((chain(f) == Result{0, 1, nblocks, f.nbits}));
        }
    // several streams
    {
        Forge f;
        stream(f, 2, 3);
        stream(f, 0, 0);
        stream(f, 1, 5);
        CHECK((chain(f) == Result{0, 3, 3, f.nbits}));
    }
    // level digits; 'B','Z','h' are read, not compared
    for (u32 digit : {0x30u, 0x3Au}) {
        Forge f;
        stream(f, 1, 2, digit);
        CHECK((chain(f) == Result{2, 1, 0, 32}));
        Forge h;
        stream(h, 1, 2);
        const u64 second = h.nbits;
        stream(h, 1, 2, digit);
        CHECK((chain(h) == Result{3, 2, 1, second + 32}));
    }
    for (u32 digit = 0x31u; digit <= 0x39u; ++digit) {
        Forge f;
        stream(f, 1, 6, digit, "\x00\xff!");
        stream(f, 1, 1, digit, "xyz");
        CHECK((chain(f) == Result{0, 2, 2, f.nbits}));
    }
    // the combined CRC: over 33 blocks and more the rotation wraps
    for (u32 nblocks : {33u, 40u}) {
        Forge f;
        f.header();
        for (u32 b = 0; b < nblocks; ++b) f.block(3 + b % 9, 0x80000000u | (0x9E3779B9u * (b + 1)));
        Forge bad = f;
        f.trailer();
        CHECK((chain(f) == Result{0, 1, nblocks, f.nbits}));
        const u64 at = bad.nbits;
        bad.trailer_crc(bad.combined ^ 1u);
        CHECK((chain(bad) == Result{1, 1, nblocks, at + 80}));
        u32 x = 0; // xor without the rotation is a different number
        for (const Rec &r : f.recs) x ^= r.stored_crc;
        CHECK(x != f.combined);
    }
    // an unknown head byte, where a block and where a trailer may stand
    for (u32 head : {0x00u, 0x30u, 0x32u, 0x16u, 0x18u, 0xFFu}) {
        Forge f;
        f.header();
        f.block(13, 7);
        const u64 at = f.nbits;
        f.block(9, 8, head);
        f.trailer();
        CHECK((chain(f) == Result{1, 1, 1, at}));
        Forge t;
        t.header();
        t.block(13, 7);
        const u64 at2 = t.nbits;
        t.trailer(head);
        CHECK((chain(t) == Result{1, 1, 1, at2}));
    }
    // a block head without a record (no full magic): the caller's business
    {
        Forge f;
        f.header();
        f.block(5, 1);
        f.recs.clear();
        CHECK(chain(f).verdict == 4);
    }
    // truncation: cut at every byte of the last 12, and at every bit of them (next_bits 0..8 behind the last block)
    for (u32 nblocks : {0u, 1u, 3u})
        for (u32 phase = 0; phase < 8; ++phase) {
            Forge f;
            stream(f, 2, 4);
            stream(f, nblocks, phase);
            for (u64 cut = 0; cut <= 12 * 8 && cut <= f.nbits; ++cut) {
                const Result r = chain(f, f.nbits - cut);
                CHECK(r.pos <= f.nbits - cut);
                if (nblocks && cut >= 8 && cut <= 80 && cut % 8 == 0) CHECK(r.verdict == 1 && r.stream_no == 2); // (no block: a CRC cut to nothing reads 0)
            }
        }
    // the clean end: 7 bits behind the padded trailer end the input, 8 are another header
    for (u32 phase = 0; phase < 8; ++phase) {
        Forge f;
        stream(f, 1, phase);
        const u64 end = f.nbits;
        f.put(0xFFu, 8);
        for (u32 left = 0; left < 8; ++left) CHECK((chain(f, end + left) == Result{0, 1, 1, end}));
        CHECK((chain(f, end + 8) == Result{3, 2, 1, end + 8}));
    }
    CHECK(g_bad == 0);
    return 0;
}

int main()
{
    if (run()) return 1;
    printf("ok\n");
    return 0;
}
