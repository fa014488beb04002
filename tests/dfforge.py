"""Test helper (not collected by pytest): a Deflate / zlib / gzip stream WRITER that builds streams code by code, for
forging streams that no encoder writes -- in the spirit of bzforge.py.

Written from the formats themselves (RFC 1951, 1950, 1952):

    stream  := block*                      bits are packed LSB first; Huffman codes are sent MSB first
    block   := BFINAL1 BTYPE2 body
    stored  := pad-to-byte LEN16 NLEN16 byte{LEN}
    fixed   := code* EOB                   lengths 8 / 9 / 7 / 8 for 0-143 / 144-255 / 256-279 / 280-287, distances 5 bits
    dynamic := HLIT5 HDIST5 HCLEN4 (len3){HCLEN + 4} cl-code* code* EOB
               cl-code: 0..15 a length; 16 = repeat the previous 3..6 times (2 bits); 17 = 3..10 zeros (3 bits);
               18 = 11..138 zeros (7 bits); the HLIT + 257 and HDIST + 1 lengths are ONE sequence (a run may cross over)
    zlib    := CMF FLG [DICTID4] stream ADLER32-big-endian
    gzip    := 1F 8B CM FLG MTIME4 XFL OS [XLEN2 extra] [name 0] [comment 0] [HCRC2] stream CRC32 ISIZE  (little endian)

Every builder returns a Case: the stream, the bytes it should decode to -- for a malformed one the bytes in front of the
failing code or block header -- and the verdict class.  tests/test_dfforge.py pins all of it against Python's zlib before
any GPU sees a stream.  Pure Python.

Every builder of cases takes the stream to begin from (`begin`, a callable; default: an empty Stream).  preamble() makes
one whose last block starts at a candidate of csrc/inf_split.h in a later piece of the entry: what a case appends behind
it is decoded, in a split entry, by a wave that did not start at the entry's first bit (behind(), source_map_cases()).
"""
import functools
import zlib

OK, E_DATA, E_EOF = 0, -1, -2
RAW, ZLIB, GZIP = 0, 1, 2
WBITS = {RAW: -15, ZLIB: 15, GZIP: 31}

CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Case:
    """name; kind (RAW / ZLIB / GZIP); stream; data: the bytes yielded (in front of the fault for a malformed stream);
    verdict: OK, E_DATA or E_EOF; note: what zlib is expected to do when that is not "decode" / "raise" / "eof False"."""

    def __init__(self, name, kind, stream, data, verdict=OK, note=""):
        self.name, self.kind, self.stream, self.data, self.verdict, self.note = name, kind, bytes(stream), bytes(data), verdict, note

    def __repr__(self):
        return "Case(%s, kind %d, %d -> %d bytes, verdict %d)" % (self.name, self.kind, len(self.stream), len(self.data), self.verdict)


class Bits:
    """LSB-first bit writer"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, n):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code: most significant bit first"""
        if length:
            self.put(int(format(code & ((1 << length) - 1), "0%db" % length)[::-1], 2), length)   # (an over-subscribed set's codes overflow)

    def align(self, fill=0):
        if self.n:
            self.put(fill & ((1 << (8 - self.n)) - 1), 8 - self.n)

    @property
    def bit_length(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        assert self.n == 0, "align first"
        return bytes(self.out)


def canonical(lengths):
    """codes of a (not necessarily complete) set of code lengths, RFC 1951 3.2.2"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    codes = []
    for l in lengths:
        codes.append(nxt[l] if l else None)
        if l:
            nxt[l] += 1
    return codes


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - l) for l in lengths if l)


def balanced(symbols, size):
    """a complete set of code lengths over `size` symbols in which exactly `symbols` (two or more) have codes"""
    k = len(symbols)
    assert k >= 2
    m = k.bit_length() - 1
    longer = 2 * (k - (1 << m))
    lens = [0] * size
    for i, s in enumerate(sorted(symbols)):
        lens[s] = m + 1 if i >= k - longer else m
    assert kraft(lens) == 32768
    return lens


def ladder(symbols, size):
    """a complete set with code lengths 1, 2, .., 15, 15 (16 symbols, in the order given): codes longer than any
    first-level lookup"""
    assert len(symbols) == 16
    lens = [0] * size
    for i, s in enumerate(symbols):
        lens[s] = min(i + 1, 15)
    assert kraft(lens) == 32768
    return lens


def rle_ops(seq, runs=True):
    """the code-length sequence as cl-code operations (symbol, extra value): greedy runs of 18 / 17 / 16"""
    ops, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if runs and v == 0 and run >= 3:
            take = min(run, 138)
            ops.append((18, take - 11) if take >= 11 else (17, take - 3))
            i += take
        elif runs and i > 0 and seq[i - 1] == v and run >= 3:
            take = min(run, 6)
            ops.append((16, take - 3))
            i += take
        else:
            ops.append((v, None))
            i += 1
    return ops


class Stream:
    """A raw Deflate stream under construction; `out` collects the bytes it decodes to."""

    def __init__(self):
        self.w = Bits()
        self.out = bytearray()
        self.root = []     # per byte of `out`: the position of the literal or stored byte its value was first written at
        self.marks = []    # (bit, mode, len(out)) of the block starts that to_next_piece() promises as candidates
        self.lit_codes = self.lit_lens = self.dist_codes = self.dist_lens = None

    def clone(self):
        c = Stream()
        c.w.acc, c.w.n, c.w.out = self.w.acc, self.w.n, bytearray(self.w.out)
        c.out, c.root, c.marks = bytearray(self.out), list(self.root), list(self.marks)
        c.lit_codes, c.lit_lens, c.dist_codes, c.dist_lens = self.lit_codes, self.lit_lens, self.dist_codes, self.dist_lens
        return c

    # -- blocks
    def header(self, final, btype):
        self.w.put(1 if final else 0, 1)
        self.w.put(btype, 2)

    def stored(self, data, final=False, ln=None, nlen=None, pad=0):
        self.header(final, 0)
        self.w.align(pad)
        ln = len(data) if ln is None else ln
        self.w.put(ln, 16)
        self.w.put(ln ^ 0xFFFF if nlen is None else nlen, 16)
        assert self.w.n == 0
        self.w.out += data
        self.root += range(len(self.out), len(self.out) + len(data))
        self.out += data
        return self

    def fixed(self, final=False):
        self.header(final, 1)
        self._tables(FIXED_LIT, FIXED_DIST)
        return self

    def _tables(self, lit_lens, dist_lens):
        self.lit_lens, self.dist_lens = list(lit_lens), list(dist_lens)
        self.lit_codes, self.dist_codes = canonical(self.lit_lens), canonical(self.dist_lens)

    def dynamic(self, lit_lens, dist_lens, final=False, ops=None, runs=True, cl_lens=None, hclen=None, hlit=None, hdist=None):
        """lit_lens: 257..286 (or more, to forge HLIT > 286 via hlit) code lengths, dist_lens: 1..30.  ops: the cl-code
        operations (default: rle_ops of the joint sequence); cl_lens: the 19 code lengths of the cl-code (default: a
        complete set over the symbols the operations use); hclen: how many of them are written (default: up to the last
        one in use, at least 4); hlit / hdist: the header FIELDS (default: len - 257, len - 1)."""
        self.header(final, 2)
        ops = rle_ops(list(lit_lens) + list(dist_lens), runs) if ops is None else ops
        if cl_lens is None:
            used = sorted({s for s, _ in ops})
            for extra in (0, 18, 17):
                if len(used) < 2 and extra not in used:
                    used = sorted(used + [extra])
            cl_lens = balanced(used, 19)
        cl_codes = canonical(cl_lens)
        if hclen is None:
            hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]) + 1)
        self.w.put(len(lit_lens) - 257 if hlit is None else hlit, 5)
        self.w.put(len(dist_lens) - 1 if hdist is None else hdist, 5)
        self.w.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.w.put(cl_lens[s], 3)
        for s, extra in ops:
            assert cl_codes[s] is not None, "cl symbol %d has no code" % s
            self.w.code(cl_codes[s], cl_lens[s])
            if s >= 16:
                self.w.put(extra, {16: 2, 17: 3, 18: 7}[s])
        self._tables(lit_lens, dist_lens)
        return self

    # -- codes
    def sym(self, s):
        """a literal/length symbol, raw"""
        assert self.lit_codes[s] is not None, "symbol %d has no code" % s
        self.w.code(self.lit_codes[s], self.lit_lens[s])
        return self

    def dsym(self, s):
        assert self.dist_codes[s] is not None, "distance symbol %d has no code" % s
        self.w.code(self.dist_codes[s], self.dist_lens[s])
        return self

    def lit(self, data):
        for b in (data if isinstance(data, (bytes, bytearray)) else bytes([data])):
            self.sym(b)
            self.root.append(len(self.out))
            self.out.append(b)
        return self

    def match(self, length, dist, emit=True):
        """one (length, distance) pair; emit=False: the codes only (the pair is the fault)"""
        li = max(i for i in range(29) if LEN_BASE[i] <= length)
        if length == 258:
            li = 28
        self.sym(257 + li)
        self.w.put(length - LEN_BASE[li], LEN_EXTRA[li])
        di = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dsym(di)
        self.w.put(dist - DIST_BASE[di], DIST_EXTRA[di])
        if emit:
            assert dist <= len(self.out)
            for _ in range(length):
                self.out.append(self.out[-dist])
                self.root.append(self.root[-dist])
        return self

    def eob(self):
        return self.sym(256)

    def raw(self, pad=0):
        w = self.w
        keep = (w.acc, w.n, bytearray(w.out))
        w.align(pad)
        b = w.bytes()
        w.acc, w.n, w.out = keep
        return b


def adler32(data):
    return zlib.adler32(bytes(data)) & 0xFFFFFFFF


def crc32(data):
    return zlib.crc32(bytes(data)) & 0xFFFFFFFF


def zlib_wrap(raw, data, cinfo=7, flevel=2, fdict=False, cm=8, fcheck=None, adler=None, tail=b""):
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (0x20 if fdict else 0)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31 if fcheck is None else fcheck
    a = adler32(data) if adler is None else adler
    return bytes([cmf, flg]) + (b"\x00\x00\x00\x01" if fdict else b"") + raw + a.to_bytes(4, "big") + tail


def gzip_wrap(raw, data, extra=None, name=None, comment=None, hcrc=None, text=False, crc=None, isize=None, id1=0x1F, id2=0x8B, cm=8,
              reserved=0, tail=b""):
    """hcrc: None = no FHCRC, True = the right one, an int = that value"""
    flg = (1 if text else 0) | (2 if hcrc is not None else 0) | (4 if extra is not None else 0) | (8 if name is not None else 0)
    flg |= (16 if comment is not None else 0) | reserved
    h = bytearray([id1, id2, cm, flg, 0x12, 0x34, 0x56, 0x78, 2, 3])
    if extra is not None:
        h += len(extra).to_bytes(2, "little") + extra
    if name is not None:
        h += name + b"\x00"
    if comment is not None:
        h += comment + b"\x00"
    if hcrc is not None:
        h += ((crc32(h) & 0xFFFF) if hcrc is True else hcrc).to_bytes(2, "little")
    c = crc32(data) if crc is None else crc
    n = (len(data) & 0xFFFFFFFF) if isize is None else isize
    return bytes(h) + raw + c.to_bytes(4, "little") + n.to_bytes(4, "little") + tail


def wrap(kind, raw, data, **kw):
    return raw if kind == RAW else zlib_wrap(raw, data, **kw) if kind == ZLIB else gzip_wrap(raw, data, **kw)


# ------------------------------------------------------------------------------------------------- the cases
@functools.lru_cache(maxsize=None)
def text(n, seed=1):
    """n bytes without any repeat of three bytes in the last 300 (so a forged copy is the only way to get a repeat)"""
    out, x = bytearray(), seed * 2654435761 % (1 << 32)
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(32 + (x >> 16) % 95)
    return bytes(out)


COPY_DIST = (1, 2, 3, 4, 7, 8, 63, 64, 65, 127, 128, 129, 258, 259, 32767, 32768)
COPY_LEN = (3, 4, 63, 64, 65, 257, 258)


def copy_grid(begin=Stream):
    """every distance x every length, each its own entry behind a literal prefix just long enough (fixed Huffman; the
    prefixes of the two long distances come as stored blocks to keep the streams short)"""
    cases = []
    for d in COPY_DIST:
        for ln in COPY_LEN:
            s = begin()
            pre = text(d, d + ln)
            if d > 600:
                s.stored(pre)
                s.fixed(final=True)
            else:
                s.fixed(final=True).lit(pre)
            s.match(ln, d).lit(b"!").eob()
            cases.append(Case("copy_d%d_l%d" % (d, ln), RAW, s.raw(), s.out))
    return cases


def copy_chains(begin=Stream):
    """overlapping copies whose source is the previous copy's output, with literals between some of them"""
    cases = []
    for k, plan in enumerate((
            [(3, 1), (4, 3), (64, 7), (65, 64), (258, 65), (257, 258), (63, 2), (258, 1)],
            [(258, 5), (258, 258), (258, 259), (258, 129), (258, 63), (3, 258)],
            [(5, 4), (7, 5), (9, 7), (64, 9), (65, 64), (66, 65), (130, 66), (131, 130)],
            [(ln, d) for d in (1, 2, 3, 63, 64, 65) for ln in (64, 65, 3)])):
        s = begin().fixed(final=True).lit(text(9, k))
        for i, (ln, d) in enumerate(plan):
            while len(s.out) < d:
                s.lit(text(1, i))
            s.match(ln, d)
            if i % 3 == 2:
                s.lit(text(2, i))
        s.eob()
        cases.append(Case("copy_chain_%d" % k, RAW, s.raw(), s.out))
    return cases


def copy_residues(begin=Stream):
    """the destination of a copy at every residue mod 16 (a literal prefix of 0..15 bytes behind 16 stored bytes)"""
    cases = []
    for r in range(16):
        s = begin().fixed(final=True).lit(text(16 + r, r))
        s.match(70, 16).match(200, 3).lit(b"#").match(258, 100).eob()
        cases.append(Case("copy_residue_%d" % r, RAW, s.raw(), s.out))
    for r in range(16):  # ... and a literal run of more than 64 bytes starting there
        s = begin().fixed(final=True).lit(text(r + 3, r)).match(3, 3).lit(text(150, 100 + r)).eob()
        cases.append(Case("literal_run_residue_%d" % r, RAW, s.raw(), s.out))
    return cases


def _ladder_tables():
    lit_syms = [ord(c) for c in "etaoinshrdlu"] + [257, 265, 285, 256]   # EOB carries a 15-bit code
    dist_syms = [0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 25, 29]
    return ladder(lit_syms, 286), ladder(dist_syms, 30)


def table_shapes(begin=Stream):
    cases = []
    # codes of up to 15 bits on both alphabets
    ll, dl = _ladder_tables()
    s = begin().dynamic(ll, dl, final=True)
    s.lit(b"etaoinshrdluetaoinshrdlu" * 3)
    for ln, d in ((3, 1), (3, 2), (3, 3), (3, 4), (3, 5), (3, 7), (3, 9), (3, 17), (3, 33), (11, 65), (12, 40), (258, 3)):
        s.match(ln, d)
    s.lit(b"ul")
    s.eob()
    cases.append(Case("lengths_up_to_15", RAW, s.raw(), s.out))
    # one literal and end-of-block; no distance code at all (one length of zero)
    lens = [0] * 257
    lens[ord("x")] = lens[256] = 1
    s = begin().dynamic(lens, [0], final=True).lit(b"x" * 77).eob()
    cases.append(Case("single_literal_plus_eob", RAW, s.raw(), s.out))
    # exactly one distance code of length 1 (zlib's exception to "incomplete")
    lens = balanced([ord("a"), ord("b"), 256, 257, 258], 259)
    s = begin().dynamic(lens, [0, 0, 1], final=True).lit(b"aba").match(3, 3).match(4, 3).lit(b"b").eob()
    cases.append(Case("one_distance_code_of_length_1", RAW, s.raw(), s.out))
    # HLIT = 286, HDIST = 30; HCLEN = 19 and the smallest HCLEN that can carry a non-zero length (5: symbols 16 17 18 0 8)
    lit8 = [8] * 255 + [0, 8] + [0] * 29      # 256 codes of 8 bits: literals 0..254 and end-of-block
    cl5 = [0] * 19
    cl5[16] = cl5[17] = 3
    cl5[18] = cl5[0] = cl5[8] = 2
    s = begin()
    at = s.w.bit_length
    s.dynamic(lit8, [0] * 30, final=True, cl_lens=cl5).lit(bytes(range(255))).eob()
    assert int.from_bytes(s.raw()[at >> 3:(at >> 3) + 4], "little") >> (at & 7) >> 13 & 15 == 1   # HCLEN field 1: five lengths
    cases.append(Case("hlit286_hdist30_hclen5", RAW, s.raw(), s.out))
    full = balanced(list(range(256)) + list(range(256, 286)), 286)
    cl19 = [5] * 6 + [4] * 13
    assert kraft(cl19) == 32768
    s = begin().dynamic(full, balanced(list(range(30)), 30), final=True, cl_lens=cl19, hclen=19, runs=False)
    s.lit(bytes(range(256))).match(258, 256).match(3, 1).match(10, 24577 // 64).eob()
    cases.append(Case("hlit286_hdist30_hclen19", RAW, s.raw(), s.out))
    # HCLEN = 4 can only say "zero": no end-of-block code
    cl4 = [0] * 19
    cl4[16] = cl4[17] = cl4[18] = cl4[0] = 2
    s = begin().dynamic([0] * 257, [0], final=True, cl_lens=cl4, hclen=4)
    cases.append(Case("hclen4_all_zero", RAW, s.raw(), s.out, E_DATA))
    # a run across the HLIT boundary, with each of the three repeat codes (HLIT = 260: symbols 0..259)
    for rep in (16, 17, 18):
        lit = [0] * 260
        if rep == 16:     # 257: "3", then 16 x 5 = 258, 259 | distance symbols 0, 1, 2; then 3: "3", 4: "2", 5: "2"
            for sy, l in ((ord("p"), 3), (ord("q"), 3), (ord("r"), 2), (256, 3), (257, 3), (258, 3), (259, 3)):
                lit[sy] = l
            dist = [3, 3, 3, 3, 2, 2]
            ops = rle_ops(lit[:257]) + [(3, None), (16, 2), (3, None), (2, None), (2, None)]
            far = 2
        else:             # 17 / 18 x zeros = 258, 259 | the first distance symbols; then two distance codes of length 1
            for sy in (ord("p"), ord("q"), 256, 257):
                lit[sy] = 2
            zeros = 4 if rep == 17 else 12
            dist = [0] * (zeros - 2) + [1, 1]
            ops = rle_ops(lit[:258]) + [(rep, zeros - (3 if rep == 17 else 11)), (1, None), (1, None)]
            far = DIST_BASE[len(dist) - 2]
        assert kraft(lit) == 32768 and kraft(dist) == 32768
        s = begin().dynamic(lit, dist, final=True, ops=ops)
        s.lit((b"pqqp" * 10)[:far + 1]).match(3, far).lit(b"q").eob()
        cases.append(Case("run_across_hlit_%d" % rep, RAW, s.raw(), s.out))
    # stored blocks: 65 535 bytes, and an empty one between two others
    big = text(65535, 9)
    s = begin().stored(big, final=True)
    cases.append(Case("stored_65535", RAW, s.raw(), s.out))
    s = begin().stored(b"abc").stored(b"").fixed().lit(b"de").eob().stored(b"", final=True)
    cases.append(Case("stored_empty", RAW, s.raw(), s.out))
    # the final bit of the stream at bit 7 and at bit 0 of the entry's last byte
    for want in (7, 0):
        for k in range(8):     # (literals from 144 on take 9 bits: each moves the end by one bit)
            s = begin().fixed(final=True).lit(text(5, 3)).lit(bytes([200]) * k).eob()
            if (s.w.bit_length - 1) % 8 == want:
                break
        else:
            raise AssertionError("no such stream")
        cases.append(Case("last_bit_at_%d" % want, RAW, s.raw(pad=0xFF), s.out))
    return cases


def containers(begin=Stream):
    body = text(300, 4)
    s = begin().fixed(final=True).lit(body[:200]).match(50, 200).lit(body[200:]).eob()
    raw, data = s.raw(), bytes(s.out)
    cases = []
    g = lambda label, verdict=OK, d=data, **kw: cases.append(Case("gzip_" + label, GZIP, gzip_wrap(raw, data, **kw), d, verdict))
    z = lambda label, verdict=OK, d=data, **kw: cases.append(Case("zlib_" + label, ZLIB, zlib_wrap(raw, data, **kw), d, verdict))
    g("plain")
    g("extra", extra=b"ab\x04\x00wxyz")
    g("extra_empty", extra=b"")
    g("name", name=b"file.txt")
    g("comment", comment=b"a comment")
    g("hcrc", hcrc=True)
    g("text", text=True)
    g("all", extra=b"q" * 300, name=b"n", comment=b"", hcrc=True, text=True)
    g("hcrc_wrong", E_DATA, b"", hcrc=(crc32(gzip_wrap(raw, data)[:10]) & 0xFFFF) ^ 0x100)
    g("all_hcrc_wrong", E_DATA, b"", extra=b"q" * 300, name=b"n", comment=b"", hcrc=1)
    g("id1", E_DATA, b"", id1=0x1E)
    g("id2", E_DATA, b"", id2=0x8A)
    g("cm", E_DATA, b"", cm=7)
    for bit in (0x20, 0x40, 0x80):
        g("reserved_%02x" % bit, E_DATA, b"", reserved=bit)
    g("trailing_garbage", tail=b"\xFF\x00garbage" * 3)
    g("second_member", tail=gzip_wrap(Stream().fixed(final=True).lit(b"second").eob().raw(), b"second"))
    for bit in (0, 13, 31):
        g("crc_bit_%d" % bit, E_DATA, crc=crc32(data) ^ (1 << bit))
    g("isize_plus_1", E_DATA, isize=len(data) + 1)
    g("isize_minus_1", E_DATA, isize=len(data) - 1)
    for cinfo in range(8):
        z("cinfo_%d" % cinfo, cinfo=cinfo)
    for flevel in (0, 1, 3):
        z("flevel_%d" % flevel, flevel=flevel)
    z("cinfo_8", E_DATA, b"", cinfo=8)
    z("cm_7", E_DATA, b"", cm=7)
    z("fcheck", E_DATA, b"", fcheck=(zlib_wrap(raw, data)[1] & 31) ^ 1)
    cases.append(Case("zlib_fdict", ZLIB, zlib_wrap(raw, data, fdict=True), b"", E_DATA, note="zlib asks for a dictionary"))
    z("trailing_garbage", tail=b"\x01\x02\x03")
    for bit in (0, 16, 31):
        z("adler_bit_%d" % bit, E_DATA, adler=adler32(data) ^ (1 << bit))
    # the empty stream in each container
    e = begin().fixed(final=True).eob()
    cases.append(Case("zlib_empty", ZLIB, zlib_wrap(e.raw(), e.out), e.out))
    cases.append(Case("gzip_empty", GZIP, gzip_wrap(e.raw(), e.out), e.out))
    return cases


def malformed(begin=Stream):
    """one stream for every class of BZ_E_DATA in the contract (the container classes are in containers()), each with
    some good bytes in front of the fault, and a few BZ_E_EOF shapes that are not plain cuts of an encoder's stream"""
    cases = []
    pre = text(40, 6)
    add = lambda name, s, verdict=E_DATA, pad=0, note="": cases.append(Case(name, RAW, s.raw(pad), s.out, verdict, note))
    start = lambda: begin().fixed().lit(pre).eob()
    s = start()
    s.header(True, 3)
    add("btype3", s, pad=0xFF)
    s = start()
    s.stored(b"", final=True, ln=5, nlen=0xFFFA ^ 1)
    s.w.put(0x1234567890, 40)
    add("stored_len_nlen", s)
    ok_lit = balanced([ord("a"), 256], 257)
    s = start().dynamic(ok_lit + [0] * 30, [1, 1], final=True, hlit=30)          # 287 lengths
    add("hlit_287", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1] + [0] * 29, final=True, hdist=30)          # 31 lengths
    add("hdist_31", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1], final=True, ops=[(16, 0)] + rle_ops(ok_lit[3:] + [1, 1]), cl_lens=balanced([0, 1, 16, 17, 18], 19))
    add("repeat_16_first", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1], final=True, ops=rle_ops(ok_lit) + [(1, None), (18, 0)], cl_lens=balanced([0, 1, 17, 18], 19))
    add("run_overshoots", s, pad=0xFF)
    over = list(ok_lit)
    over[ord("b")] = 1
    s = start().dynamic(over, [1, 1], final=True)
    add("lit_oversubscribed", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1, 1], final=True)
    add("dist_oversubscribed", s, pad=0xFF)
    inc = [0] * 257
    inc[ord("a")], inc[ord("b")], inc[256] = 2, 2, 2
    s = start().dynamic(inc, [1, 1], final=True)
    add("lit_incomplete", s, pad=0xFF)
    s = start().dynamic(ok_lit, [2, 2, 2], final=True)
    add("dist_incomplete", s, pad=0xFF)
    s = start().dynamic(ok_lit, [0, 2], final=True)
    add("dist_single_code_of_length_2", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1], final=True, cl_lens=[3 if i in (0, 1, 18) else 0 for i in range(19)])
    add("cl_incomplete", s, pad=0xFF)
    s = start().dynamic(ok_lit, [1, 1], final=True, cl_lens=[1 if i in (0, 1, 18) else 0 for i in range(19)])
    add("cl_oversubscribed", s, pad=0xFF)
    noeob = [0] * 257
    noeob[ord("a")] = noeob[ord("b")] = 1
    s = start().dynamic(noeob, [1, 1], final=True)
    add("no_end_of_block_code", s, pad=0xFF)
    for sy in (286, 287):
        s = start().fixed(final=True).lit(b"zz").sym(sy)
        s.w.put(0x3FFFFFFF, 30)
        add("length_symbol_%d" % sy, s, pad=0xFF)
    for sy in (30, 31):
        s = start().fixed(final=True).lit(b"zz").sym(257).dsym(sy)
        s.w.put(0x3FFFFFFF, 30)
        add("distance_symbol_%d" % sy, s, pad=0xFF)
    s = begin().fixed(final=True).lit(pre)          # one byte in front of ALL output so far
    good = bytes(s.out)
    assert len(good) + 1 <= 32768
    s.match(5, len(good) + 1, emit=False).lit(b"never").eob()
    cases.append(Case("distance_too_far", RAW, s.raw(0xFF), good, E_DATA))
    s = begin().fixed(final=True)                    # one byte in front of the entry's output
    good = bytes(s.out)
    s.match(3, len(good) + 1, emit=False).eob()
    cases.append(Case("distance_at_the_start", RAW, s.raw(0xFF), good, E_DATA))
    # the unused code of a one-code distance set, and a distance code where there is none at all
    lens = balanced([ord("a"), ord("b"), 256, 257], 258)
    s = start().dynamic(lens, [1], final=True).lit(b"ab").sym(257)
    s.w.put(1, 1)
    s.w.put(0x3FFFFFFF, 30)
    add("unused_distance_code", s, pad=0xFF, note="zlib raises before it hands out the last literals")
    s = start().dynamic(lens, [0], final=True).lit(b"ab").sym(257)
    s.w.put(0x3FFFFFFF, 30)
    add("no_distance_codes", s, pad=0xFF, note="zlib raises before it hands out the last literals")
    # ---- BZ_E_EOF shapes
    s = begin()
    cases.append(Case("empty_entry", RAW, s.raw(), s.out, E_EOF))
    s = start()
    cases.append(Case("no_final_block", RAW, s.raw(), s.out, E_EOF))
    s = start()
    s.header(True, 0)
    cases.append(Case("stored_without_len", RAW, s.raw(), s.out, E_EOF))
    s = start().stored(b"0123456789", final=True)
    cases.append(Case("stored_cut_short", RAW, s.raw()[:-3], start().out, E_EOF, note="zlib yields the bytes that are there"))
    s = start().fixed(final=True).lit(b"abc")
    if s.w.n == 1:         # (seven padding bits of zero would BE the end-of-block code: a 9-bit literal leaves six)
        s.lit(bytes([200]))
    cases.append(Case("no_end_of_block", RAW, s.raw(), s.out, E_EOF))
    s = start().dynamic(ok_lit, [1, 1], final=True)
    cases.append(Case("cut_in_dynamic_header", RAW, s.raw()[:len(start().raw()) + 3], start().out, E_EOF))
    return cases


def quirk_like(begin=Stream):
    """what the reference's encoder writes for a dynamic block without any match: HDIST = 0 and NO distance code length
    at all (src/deflate/encoder.rs:431-436, 449-451) -- one length short of what the header announces, so the first code
    of the data is read as that length and everything behind it is shifted"""
    lens = balanced([ord("a"), ord("b"), ord("c"), 256], 257)
    s = begin()
    good = bytes(s.out)
    s.dynamic(lens, [0], final=True, ops=rle_ops(lens))   # (the operations stop after the 257 lengths)
    s.lit(b"abcabc").eob()
    return Case("match_free_dynamic_block_of_the_reference", RAW, s.raw(), good, E_DATA, note="verdict class and prefix are whatever the contract gives")


# ------------------------------------------------------------------------------------------------- preambles
# A case built behind a preamble is decoded, in an entry that is split into pieces (csrc/inf_split.h), by a wave that did
# not start at the entry's first bit: the preamble's last block starts at a candidate of a later piece.
def piece_tables():
    """the tables of a preamble's dynamic blocks: printable ASCII, end-of-block, all 29 length and all 30 distance symbols"""
    return balanced(list(range(32, 127)) + list(range(256, 286)), 286), balanced(list(range(30)), 30)


def to_next_piece(s, phase, mode, piece=1024, lead=0, skip=0, seed=1):
    """Behind a closed block of `s`: a stored block of text() -- printable ASCII holds no LEN / NLEN pair -- whose payload
    runs 40 bytes into the next piece (`skip` pieces further; the entry starts `lead` bytes in front of the stream), then
    a fixed block: a stored block in front of a fixed one is no candidate, and nothing in a fixed block is.  mode 0: the
    fixed block's 9-bit literals move the next block header to a bit = phase (mod 32) of the entry.  mode 1: its 8-bit
    literals move the LEN field of a five-byte stored block behind it to a byte = phase (mod 4); the caller's next block
    has to be a dynamic one, which makes that LEN field a candidate.  The caller's next block is decoded from the mark."""
    len_at = lead + (s.w.bit_length + 3 + 7) // 8
    n = ((len_at + 4) // piece + 1 + skip) * piece - (len_at + 4) + 40
    s.stored(text(n, seed))
    s.fixed()
    if mode == 0:
        here = 8 * lead + s.w.bit_length + 7          # (+ 7: the end-of-block code)
        s.lit(bytes([200]) * ((phase - here) * 25 % 32))      # 9 * 25 = 1 (mod 32)
        s.eob()
        assert (8 * lead + s.w.bit_length) % 32 == phase
        s.marks.append((s.w.bit_length, 0, len(s.out)))
    else:
        here = lead + (s.w.bit_length + 7 + 3 + 7) // 8     # the LEN field without any literal
        s.lit(b"=" * ((phase - here) % 4))
        s.eob()
        at = (s.w.bit_length + 3 + 7) // 8
        assert (lead + at) % 4 == phase
        s.marks.append((8 * at, 1, len(s.out)))
        s.stored(text(5, seed + 1))
    return s


def preamble(phase, mode, piece=1024, lead=0, skip=0):
    """A stream of at least one piece and (without skip) about 1 KiB of output whose last block D, a non-final dynamic one,
    is decoded by a wave that starts at the first candidate of a later piece: mode 0, the header of D at a bit = phase
    (mod 32); mode 1, the LEN field of a short stored block in front of D at a byte = phase (mod 4).  marks[0] names it."""
    s = Stream().fixed().lit(b"in front").eob()
    to_next_piece(s, phase, mode, piece, lead, skip)
    ll, dl = piece_tables()
    return s.dynamic(ll, dl).lit(b"a later piece ").match(6, 3).eob()


def source_map_cases(piece=1024):
    """What a piece's source map has to get right at its start.  Behind a preamble a filler to the next piece, then the
    dynamic block D2: k literals (0, 1, 2), one match of every COPY_DIST x COPY_LEN with a distance above k -- it lies
    wholly in front of the piece, or for d < len straddles its start: sources in front of the piece and (k > 0) the
    piece's own literals take turns -- then 70 bytes at distance len, a copy of what that match gave (unresolved bytes,
    whole or in part), a literal, end of block.  A filler again, and D3 in the third piece copies 40 of those bytes: a
    pointer to a pointer.  Case.unresolved: the bytes whose value lies in front of the piece they are in."""
    ll, dl = piece_tables()
    cases = []
    for k in (0, 1, 2):
        for d in COPY_DIST:
            for ln in COPY_LEN:
                if d <= k:
                    continue
                s = preamble(13, 0, piece, skip=32 if d > 2000 else 0)
                to_next_piece(s, (7 * d + ln) % 32, 0, piece, seed=2)
                s.dynamic(ll, dl).lit(text(k, 5))
                at = len(s.out)
                s.match(ln, d).match(70, ln).lit(b"+").eob()
                to_next_piece(s, (3 * d + ln + k) % 32, 0, piece, seed=3)
                s.dynamic(ll, dl).match(40, len(s.out) - at).lit(b".").eob()
                s.fixed(final=True).lit(b"end").eob()
                c = Case("source_map_k%d_d%d_l%d" % (k, d, ln), RAW, s.raw(), s.out)
                starts = [0] + [m[2] for m in s.marks]
                c.pieces = len(starts)
                c.marks = [m[:2] for m in s.marks]
                c.unresolved = sum(r < max(b for b in starts if b <= i) for i, r in enumerate(s.root))
                cases.append(c)
    return cases


def clean_cases(begin=Stream):
    return copy_grid(begin) + copy_chains(begin) + copy_residues(begin) + [c for c in table_shapes(begin) + containers(begin) if c.verdict == OK]


def malformed_cases(begin=Stream):
    return [c for c in table_shapes(begin) + containers(begin) if c.verdict != OK] + malformed(begin)


BUILDERS = (copy_grid, copy_chains, copy_residues, table_shapes, containers, malformed)


@functools.lru_cache(maxsize=None)
def _builder_of():
    return {c.name: b for b in BUILDERS for c in b()}


def behind(phase, mode, piece=1024, names=None):
    """(clean, malformed): the corpus -- or its cases `names` -- built behind preamble(phase, mode), each name with the
    preamble's in front (Case.base: the name without it); quirk_like() is one of the malformed ones"""
    first = preamble(phase, mode, piece)
    begin = first.clone
    if names is None:
        clean, bad = clean_cases(begin), malformed_cases(begin) + [quirk_like(begin)]
    else:
        made = [c for b in BUILDERS if any(_builder_of()[n] is b for n in names) for c in b(begin)]
        clean, bad = [c for c in made if c.verdict == OK], [c for c in made if c.verdict != OK]
    for c in clean + bad:
        c.base, c.name = c.name, "p%dm%d_%s" % (phase, mode, c.name)
    keep = lambda cs: [c for c in cs if names is None or c.base in names]
    return keep(clean), keep(bad)


TAILS = (1024, 1025, 2049)


def tailed(cases):
    """the cases (none of them E_EOF) with 0xFF bytes behind their stream, up to 1 024, 1 025 or 2 049 bytes in turn -- a
    piece, a piece + 1, two pieces + 1; a stream that is longer than that already takes the next of them, or none.  Bytes
    behind a stream are ignored, behind a fault they could only turn an EOF into the DATA the case names already, and
    0xFF bytes hold no candidate: neither three header bits 0 1 0 nor a LEN ^ NLEN of 0xFFFF."""
    out = []
    for i, c in enumerate(cases):
        assert c.verdict != E_EOF
        want = [TAILS[(i + k) % 3] for k in range(3)]
        n = next((t for t in want if t >= len(c.stream)), len(c.stream))
        out.append(Case(c.name + "_tail", c.kind, c.stream + b"\xFF" * (n - len(c.stream)), c.data, c.verdict, c.note))
    return out


def cut_points(n):
    """where a stream of n bytes is cut: every byte of its first 64 and its last 64, and 32 places spread evenly between"""
    pts = set(range(min(64, n))) | set(range(max(0, n - 64), n))
    pts |= {64 + (n - 128) * k // 33 for k in range(1, 33)} if n > 128 else set()
    return sorted(pts)
