// dec_chain.h -- the record chain of a .bz2 file (stream header, block, end-of-stream record, next stream ...) as the
// reference walks it: BZip2DecoderBase::init_block / the end of a stream (src/bzip2/decoder.rs:171-221, 487-520).
// These rules decide every decoder verdict, and they exist here only: the host loop of decode_core (dec_engine.hip) and
// k_dec_chain_batch (k_dec.hip, one lane per entry) both open their records through chain_open_record.  Blocks are
// opaque to the chain: what it needs of one is where it ends, its stored CRC and the 8 bits behind it (DecBlockInfo).
//
// Plain C++17 without HIP headers (tests/host_stub/dec_chain_check.cpp compiles it with g++).
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define BZ_HD __host__ __device__
#else
#define BZ_HD
#endif

// BZip2DecoderBase's state (decoder.rs:93-108) as far as the chain needs it.  `pos` is the bit position of the next
// record; have_next: the block in front of it already looked at its head byte (next_bits of its 8 bits were there).
struct ChainState {
    uint64_t pos = 0;
    uint32_t stream_no = 1, level = 0, combined = 0;
    bool need_header = true, have_next = false;
    uint32_t next_head = 0, next_bits = 0;
};

enum class ChainEvent {
    Block,      // state.pos is where a block starts: the caller finds its candidate and calls chain_take_block
    StreamEnd,  // trailer consumed, combined CRC right, padded to a byte; another stream follows
    End,        // ... fewer than 8 bits follow: the clean end
    MagicFirst, // level digit of the first stream's header
    Magic,      // ... of a later one
    Data,       // unknown head byte, or a wrong combined CRC
};

// Reader: u32 read(u64 &pos, u32 nbits), nbits <= 32, like BitReader<Left> (bitio/reader.rs:70-186): at the end of
// the input the bits that are left come back as a shorter number and pos stops there.
template <class Reader>
BZ_HD ChainEvent chain_open_record(ChainState &s, Reader &rd, uint64_t nbits)
{
    if (s.need_header) { // 'B','Z','h' are read, not compared; the level digit is (decoder.rs:171-187)
        (void)rd.read(s.pos, 24);
        const uint32_t lv = rd.read(s.pos, 8);
        if (lv < 0x31u || lv > 0x39u) return s.stream_no == 1 ? ChainEvent::MagicFirst : ChainEvent::Magic;
        s.level = lv - 0x30u;
        s.need_header = false;
    }
    uint64_t p = s.pos;
    uint32_t head;
    if (s.have_next) {
        head = s.next_head;
        p = s.pos + s.next_bits;
        s.have_next = false;
    } else {
        head = rd.read(p, 8);
    }
    if (head == 0x31u) return ChainEvent::Block; // only the first byte of the block magic is compared (decoder.rs:204-221)
    if (head != 0x17u) return ChainEvent::Data;
    // end of stream, decoder.rs:487-520: the other five bytes of its magic are skipped, then the combined CRC
    s.pos = p;
    (void)rd.read(s.pos, 24);
    (void)rd.read(s.pos, 16);
    const uint32_t stored = rd.read(s.pos, 32);
    if (stored != s.combined) return ChainEvent::Data;
    s.pos = (s.pos + 7ull) & ~7ull;
    if (s.pos > nbits) s.pos = nbits;
    if (nbits - s.pos < 8) return ChainEvent::End;
    s.need_header = true;
    s.combined = 0;
    s.stream_no += 1;
    return ChainEvent::StreamEnd;
}

// the block at state.pos is one of the chain (decoder.rs:199-200: the combined CRC is rotated, then xored)
BZ_HD inline void chain_take_block(ChainState &s, uint64_t end_bit, uint32_t stored_crc, uint32_t next_head, uint32_t next_bits)
{
    s.combined = ((s.combined << 1) | (s.combined >> 31)) ^ stored_crc;
    s.pos = end_bit;
    s.have_next = true;
    s.next_head = next_head;
    s.next_bits = next_bits;
}
