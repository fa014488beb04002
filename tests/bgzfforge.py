"""Test helper (not collected by pytest): BGZF files made by hand, block by block, for the reader of section 8 of
include/bz2_mi355x.h -- bgzfref.wrap around raw Deflate streams of zlib.compressobj(level, DEFLATED, -15) and around dfforge
streams, and the same with a header byte, BSIZE, CRC-32 or ISIZE forged.  Nothing here comes from the library: the expected
bytes of a file are the plain chunks it was built from, its offsets are the lengths of the blocks put side by side, and
tests/test_bgzfforge.py pins both against gzip.decompress and bgzfref.walk.

chain() is the BSIZE chain written from the contract's words; the library's index calls are compared with it."""
import struct
import zlib

import bgzfref
import dfforge

OK, E_DATA, E_EOF = 0, -1, -2
HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
FIXED_BYTES = (0, 1, 2, 3, 10, 11, 12, 13, 14, 15)   # the header bytes the rule pins (4 .. 9 are free)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(bytes(data)) + c.flush()


def stored(data):
    return raw_deflate(data, 0)


def fixed(data):
    return raw_deflate(data, 6, zlib.Z_FIXED)


def dynamic(data):
    d = raw_deflate(data, 9)
    assert (d[0] >> 1) & 3 == 2, "zlib did not choose a dynamic block"
    return d


def three_blocks(data):
    """one Deflate stream of three Deflate blocks: a full flush behind each third"""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    n = len(data) // 3
    return c.compress(data[:n]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[n:2 * n]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[2 * n:]) + c.flush()


def block(deflate, data, crc=None, isize=None, bsize=None, head=HEAD):
    """18-byte header, the Deflate bytes, CRC-32 and ISIZE of `data`; each of them forged when given"""
    n = 18 + len(deflate) + 8
    assert n <= 65536
    crc = zlib.crc32(bytes(data)) if crc is None else crc
    return head + struct.pack("<H", n - 1 if bsize is None else bsize) + deflate + struct.pack("<II", crc, len(data) if isize is None else isize)


def zblock(data, level=6):
    return bgzfref.wrap(bytes(data), raw_deflate(data, level))


class File:
    """blocks side by side: .file, .chunks (the bytes each block stands for), .coff / .uoff (count + 1 entries), .data"""

    def __init__(self, parts, tail=b""):
        self.blocks = [bytes(b) for b, _ in parts]
        self.chunks = [bytes(d) for _, d in parts]
        self.coff, self.uoff = [0], [0]
        for b, d in zip(self.blocks, self.chunks):
            self.coff.append(self.coff[-1] + len(b))
            self.uoff.append(self.uoff[-1] + len(d))
        self.file = b"".join(self.blocks) + tail
        self.data = b"".join(self.chunks)

    @property
    def count(self):
        return len(self.blocks)


def of_chunks(chunks, level=6, eof=False):
    parts = [(zblock(c, level), c) for c in chunks]
    if eof:
        parts.append((bgzfref.EOF, b""))
    return File(parts)


def forged_clean_file():
    """every clean raw stream of the Deflate forge (dfforge.clean_cases) that fits a block, a block each, in the forge's order
    -> (File, the names of the cases that do not fit)"""
    cases = [c for c in dfforge.clean_cases() if c.kind == dfforge.RAW]
    fit = [c for c in cases if len(c.stream) + 26 <= 65536 and len(c.data) <= 65536]
    return File([(bgzfref.wrap(c.data, c.stream), c.data) for c in fit]), [c.name for c in cases if c not in fit]


def text(n, seed=1):
    """compressible, not periodic"""
    words = (b"the ", b"block ", b"index ", b"of ", b"a ", b"file ", b"read ", b"range ", b"gzip ", b"member ", b"\n")
    out, x = bytearray(), seed * 2654435761 % (1 << 32)
    while len(out) < n:
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out += words[(x >> 16) % len(words)]
        if (x >> 8) % 7 == 0:
            out += b"%d " % (x % 1000)
    return bytes(out[:n])


def chain(file):
    """THE CHAIN of the contract -> (coff, uoff, verdict): count + 1 entries each, the clean prefix on a fault"""
    n, pos, upos, coff, uoff = len(file), 0, 0, [], []
    while True:
        if pos == n:
            v = OK
            break
        if n - pos < 18:
            v = E_EOF
            break
        h = file[pos:pos + 16]
        if not (h[:4] == b"\x1f\x8b\x08\x04" and h[10:] == b"\x06\x00BC\x02\x00"):
            v = E_DATA
            break
        size = struct.unpack_from("<H", file, pos + 16)[0] + 1
        if size < 28:
            v = E_DATA
            break
        if pos + size > n:
            v = E_EOF
            break
        isize = struct.unpack_from("<I", file, pos + size - 4)[0]
        if isize > 65536:
            v = E_DATA
            break
        coff.append(pos)
        uoff.append(upos)
        pos += size
        upos += isize
    return coff + [pos], uoff + [upos], v


def clean_files():
    """name -> File: every one decodes with gzip.decompress (an empty file aside) and walks with bgzfref.walk"""
    out = {}
    out["no_blocks"] = File([])
    out["one_block"] = of_chunks([text(700, 1)])
    out["forty_blocks"] = of_chunks([text(50 + 37 * k, k) for k in range(40)], eof=True)
    out["marker_alone"] = File([(bgzfref.EOF, b"")])
    out["empty_in_the_middle"] = File([(zblock(text(300, 2)), text(300, 2)), (bgzfref.EOF, b""), (zblock(text(301, 3)), text(301, 3))])
    parts = []
    for r in range(8):   # block lengths of every residue mod 4 (twice over): stored blocks are their payload + 31 bytes
        d = text(90 + r, 10 + r)
        parts.append((bgzfref.wrap(d, stored(d)), d))
    out["length_residues"] = File(parts)
    assert {len(b) % 4 for b in out["length_residues"].blocks} == {0, 1, 2, 3}
    return out


def phase_file():
    """payload lengths such that coff mod 4 and uoff mod 16 take every value (stored blocks: length = payload + 31)"""
    parts, k = [], 0
    while True:
        f = File(parts)
        if {c % 4 for c in f.coff[:-1]} == {0, 1, 2, 3} and {u % 16 for u in f.uoff[:-1]} == set(range(16)) and k >= 20:
            return f
        d = text(61 + (k * 7) % 13, 40 + k)   # lengths 61 .. 73: every step of uoff mod 16 is odd or even by turns
        parts.append((bgzfref.wrap(d, stored(d) if k % 3 else fixed(d)), d))
        k += 1
        assert k < 64


def nested():
    """a stored block whose payload is a whole BGZF file: its headers are candidates that the chain never lands on"""
    inner = of_chunks([text(60 + k, 70 + k) for k in range(64)])
    assert inner.count == 64 and len(inner.file) < 65000
    return File([(bgzfref.wrap(inner.file, stored(inner.file)), inner.file), (zblock(text(100, 5)), text(100, 5))]), inner


def chain_faults():
    """-> [(name, file bytes, verdict, clean prefix: blocks indexed)]: every verdict of the chain"""
    base = of_chunks([text(200 + 11 * k, 20 + k) for k in range(4)])
    f, c = base.file, base.coff
    out = []
    for cut, v in ((1, E_EOF), (17, E_EOF), (18, E_EOF), (19, E_EOF)):
        out.append(("cut_%d_into_block_2" % cut, f[:c[2] + cut], v, 2))
    out.append(("cut_one_short_of_block_2_end", f[:c[3] - 1], E_EOF, 2))
    out.append(("cut_at_block_2_end", f[:c[3]], OK, 3))
    for i in FIXED_BYTES:
        b = bytearray(f)
        b[c[2] + i] ^= 0x01
        out.append(("header_byte_%d_spoilt" % i, bytes(b), E_DATA, 2))
    for i in range(4, 10):   # MTIME, XFL, OS: anything goes
        b = bytearray(f)
        b[c[2] + i] ^= 0xA5
        out.append(("free_byte_%d_changed" % i, bytes(b), OK, 4))
    d = text(100, 30)
    raw = raw_deflate(d)
    # FLG = 0x0c with an FNAME behind the extra field: legal gzip, not BGZF
    named = b"\x1f\x8b\x08\x0c" + HEAD[4:] + struct.pack("<H", 18 + 5 + len(raw) + 8 - 1) + b"name\x00" + raw + struct.pack("<II", zlib.crc32(d), len(d))
    assert zlib.decompress(named, 31) == d
    out.append(("flg_0c_with_fname", f[:c[2]] + named + f[c[2]:], E_DATA, 2))
    # XLEN = 10: a second subfield behind BC
    two = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x0a\x00BC\x02\x00" + struct.pack("<H", 22 + len(raw) + 8 - 1) + b"XY\x00\x00" + raw + struct.pack("<II", zlib.crc32(d), len(d))
    assert zlib.decompress(two, 31) == d
    out.append(("xlen_10_two_subfields", f[:c[2]] + two + f[c[2]:], E_DATA, 2))
    b = bytearray(f)
    struct.pack_into("<H", b, c[2] + 16, 26)
    out.append(("bsize_plus_1_is_27", bytes(b), E_DATA, 2))
    b = bytearray(f)
    struct.pack_into("<I", b, c[3] - 4, 65537)
    out.append(("isize_65537", bytes(b), E_DATA, 2))
    out.append(("four_zeros_between_blocks", f[:c[2]] + bytes(4) + f[c[2]:], E_DATA, 2))
    out.append(("eighteen_zeros_behind", f + bytes(18), E_DATA, 4))
    out.append(("three_zeros_behind", f + bytes(3), E_EOF, 4))
    return [(name, data, v, n, base) for name, data, v, n in out]


def bsize_spoilt():
    """the two header bytes that the rule does not pin by value, spoilt: the chain lands one byte (256 bytes) off and the
    next step fails -> [(name, file bytes)]; what is indexed in front of the fault is chain()'s to say"""
    base = of_chunks([text(200 + 11 * k, 20 + k) for k in range(4)])
    out = []
    for i in (16, 17):
        b = bytearray(base.file)
        b[base.coff[2] + i] ^= 0x01
        out.append(("header_byte_%d_spoilt" % i, bytes(b)))
    return out
