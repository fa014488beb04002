"""The BGZF file that df_gpu_bgzf_encode_device must write (section 7 of include/bz2_mi355x.h), built from the oracle and
zlib.crc32 alone -- never from the library.

A file is its blocks side by side, then the 28-byte EOF marker.  Block k carries the input bytes [k*B, min(n, (k+1)*B)):
the 18-byte header with the `BC` subfield and BSIZE, one final Deflate block, CRC-32 and ISIZE.  The Deflate block is the
oracle's one-block stream of that chunk alone (oracle.deflate_encode(chunk, 0)) with one exception, THE STRICT RULE: where
the reference chooses a dynamic block although the chunk has no match at all, it writes HDIST = 0 and no distance code
length, which zlib refuses; such a block is written stored if 8 * len + 34 <= fixed, else fixed, `fixed` being
2 + the fixed code lengths of the literals + 7 for the end-of-block code."""
import struct
import zlib

BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def block_count(n, block_bytes=0):
    b = block_bytes or BLOCK
    return (n + b - 1) // b


def bound(n, block_bytes=0, eof=True):
    return n + 31 * block_count(n, block_bytes) + (28 if eof else 0)


def fixed_bits(chunk):
    """the kernel's count for a block of literals only: BTYPE, the literals, the end-of-block code"""
    hi = sum(1 for b in chunk if b >= 144)
    return 2 + 8 * len(chunk) + hi + 7


def stored_body(chunk):
    n = len(chunk)
    return bytes([1]) + struct.pack("<HH", n, n ^ 0xFFFF) + chunk


def fixed_body(chunk):
    """BFINAL = 1, BTYPE = 1, every byte as a literal of the fixed code (RFC 1951 3.2.6), end of block, LSB first"""
    acc, nacc = 0b011, 3                    # BFINAL, then BTYPE 01 from its low bit
    out = bytearray()

    def put_code(code, length):             # Huffman codes go out from their most significant bit
        nonlocal acc, nacc
        for i in range(length - 1, -1, -1):
            acc |= ((code >> i) & 1) << nacc
            nacc += 1
    for b in chunk:
        if b < 144:
            put_code(0x30 + b, 8)
        else:
            put_code(0x190 + (b - 144), 9)
        while nacc >= 8:
            out.append(acc & 0xFF)
            acc >>= 8
            nacc -= 8
    put_code(0, 7)
    while nacc > 0:
        out.append(acc & 0xFF)
        acc >>= 8
        nacc -= 8
    return bytes(out)


def literals_only(oracle, chunk):
    return bool((oracle.lzss_tokens_raw(chunk)[:, 0] == 0).all())   # (oracle.lzss_tokens as an array of (len, pos))


def body(oracle, chunk):
    """-> (the Deflate block, its BTYPE, whether the strict rule replaced the oracle's)"""
    ref = oracle.deflate_encode(chunk, 0)
    btype = (ref[0] >> 1) & 3
    if btype == 2 and literals_only(oracle, chunk):
        if 8 * len(chunk) + 34 <= fixed_bits(chunk):
            return stored_body(chunk), 0, True
        return fixed_body(chunk), 1, True
    return ref, btype, False


def wrap(chunk, deflate):
    bsize = 18 + len(deflate) + 8 - 1
    assert bsize <= 0xFFFF
    head = bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", bsize)
    return head + deflate + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def build(oracle, data, block_bytes=0, eof=True):
    """-> (file, block offsets: count + 1 entries, per-block (btype, replaced))"""
    b = block_bytes or BLOCK
    assert 1 <= b <= BLOCK
    data = bytes(data)
    out, offs, kinds = bytearray(), [], []
    for a in range(0, len(data), b):
        chunk = data[a:a + b]
        d, btype, replaced = body(oracle, chunk)
        assert len(d) <= len(chunk) + 5
        offs.append(len(out))
        kinds.append((btype, replaced))
        out += wrap(chunk, d)
    offs.append(len(out))
    if eof:
        out += EOF
    assert len(out) <= bound(len(data), b, eof)
    return bytes(out), offs, kinds


def walk(file):
    """the BSIZE chain from offset 0: -> the members' offsets; the chain must end exactly at the file's end"""
    pos, offs = 0, []
    while pos < len(file):
        assert file[pos:pos + 4] == b"\x1f\x8b\x08\x04" and file[pos + 10:pos + 16] == b"\x06\x00BC\x02\x00", pos
        offs.append(pos)
        pos += struct.unpack_from("<H", file, pos + 16)[0] + 1
    assert pos == len(file)
    return offs
