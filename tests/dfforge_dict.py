"""Test helper (not collected by pytest): forged Deflate / zlib streams that need a PRESET DICTIONARY, built with
dfforge.Stream (which stays as it is).  A stream's `out` and `root` are pre-seeded with the window -- the last 32 768 bytes
of the dictionary (Seeded) -- so match() accepts distances that reach into it; the data of a case is out[W:].

Every case is a dfforge.Case with more attributes: `dict` (the whole dictionary), `zlib` (what Python's zlib does with it
when that is not "decode to the data" for OK, "raise" for E_DATA, "eof stays False" for E_EOF: one of "raises", "ignores
the dictionary" -- then `zlib_data` is what it yields) and, for the split cases, `unresolved` and `pieces`.
tests/test_dfforge_dict.py pins all of it against zlib.decompressobj(wbits, zdict=dict) before any GPU sees a stream.
Pure Python.

The contract: include/bz2_mi355x.h section 5, clause (c)."""
import functools

import dfforge as F
from dfforge import E_DATA, E_EOF, OK, RAW, ZLIB

DICT_LEN = (1, 2, 258, 32767, 32768, 40000)      # the last: only its final 32 768 bytes are window
PREFIX = (0, 1, 5, 63, 64, 65)
MAX_DIST = 32768


@functools.lru_cache(maxsize=None)
def dictionary(n):
    return F.text(n, 1000 + n)


def window(dict_):
    return bytes(dict_[-MAX_DIST:])


class Seeded(F.Stream):
    """A dfforge.Stream whose `out` and `root` begin with the window (`W` bytes).  A byte that a match takes from the window
    is its own root, as a literal is -- the decoder has it at once, whatever piece of a split entry it is in -- and byte k
    of a match has the root of ITS source byte, out[p - d + k mod d] (the copy the decoder makes; byte by byte, as
    Stream.match takes it, the roots of an overlapping copy would come from the copy itself)."""

    def __init__(self, dict_=b""):
        super().__init__()
        w = window(dict_)
        self.W = len(w)
        self.out, self.root = bytearray(w), list(range(len(w)))

    def match(self, length, dist, emit=True):
        at = len(self.out)
        super().match(length, dist, emit)
        if emit:
            for k in range(length):
                q = at - dist + (k % dist if dist < length else k)
                self.root[at + k] = at + k if q < self.W else self.root[q]
        return self


def zlib_wrap(raw, data, dictid, cinfo=7, flevel=2, cm=8, fcheck=None, adler=None):
    """dictid: the DICTID field (FDICT set), None: FDICT clear and no such field"""
    cmf = (cinfo << 4) | cm
    flg = (flevel << 6) | (0x20 if dictid is not None else 0)
    flg |= (31 - ((cmf << 8) | flg) % 31) % 31 if fcheck is None else fcheck
    a = F.adler32(data) if adler is None else adler
    return bytes([cmf, flg]) + (dictid.to_bytes(4, "big") if dictid is not None else b"") + raw + a.to_bytes(4, "big")


def case(name, kind, stream, data, dict_, verdict=OK, zl=""):
    c = F.Case(name, kind, stream, data, verdict)
    c.dict, c.zlib = dict_, zl
    return c


def _begin(dict_, p):
    """a stream whose final fixed block holds p literals so far (a prefix of more than 600 bytes: a stored block in front)"""
    s = Seeded(dict_)
    pre = F.text(p, 7 + p)
    if p > 600:
        s.stored(pre)
        s.fixed(final=True)
    else:
        s.fixed(final=True).lit(pre)
    return s


def _one(name, dict_, p, ln, d):
    W = len(window(dict_))
    s = _begin(dict_, p)
    if d > p + W:
        good = bytes(s.out[W:])
        s.match(ln, d, emit=False).lit(b"never").eob()
        return case(name, RAW, s.raw(0xFF), good, dict_, E_DATA)
    s.match(ln, d).lit(b"!").eob()
    return case(name, RAW, s.raw(), s.out[W:], dict_)


@functools.lru_cache(maxsize=None)
def copy_cases(n):
    """one match behind a literal prefix, for the dictionary of n bytes: the source wholly in the window, straddling its
    end with d >= len and with d < len (the period taken from window and output bytes in turn), and the edge distances"""
    dict_ = dictionary(n)
    W = min(n, MAX_DIST)
    plan = set()
    for p in PREFIX:
        for ln in F.COPY_LEN:
            # wholly in the window: d - p >= len -- ending at its last byte, one byte in front of that, starting at its first
            plan |= {(p, ln, p + ln), (p, ln, p + ln + 1), (p, ln, p + W)} if W >= ln else set()
            # straddling, d >= len: the source starts in the window and ends in the prefix
            plan |= {(p, ln, d) for d in (ln, p + 1, p + ln - 1) if p < d and d >= ln and d - p < ln}
            # straddling, d < len: the period holds window bytes and (p > 0) output bytes
            plan |= {(p, ln, d) for d in (p + 1, p + 2, p + W, ln - 1) if p < d < ln}
        for ln in (3, 258):
            plan |= {(p, ln, p + W), (p, ln, p + W + 1)}         # the furthest distance, and one too far
    plan |= {(60, 64, 64), (1, 258, 258), (1, 258, 3), (700, 65, 701), (700, 258, 700 + W)}
    plan |= {(0, ln, d) for d in (1, 2, 3, 63, 64, 65) for ln in (64, 65, 258)}
    cases = []
    for p, ln, d in sorted(plan):
        if d > MAX_DIST or d > p + W + 1:      # (no code for a distance above 32 768)
            continue
        cases.append(_one("dict%d_p%d_l%d_d%d" % (n, p, ln, d), dict_, p, ln, d))
    # a chain: a copy from the window, a copy of that copy, a copy that reaches across both into the window
    if W >= 64:
        s = _begin(dict_, 5)
        s.match(64, 5 + 64).match(64, 64).lit(b"-").match(258, 5 + 64 + 64 + 1 + 30).lit(b"!").eob()
        cases.append(case("dict%d_chain" % n, RAW, s.raw(), s.out[W:], dict_))
    assert len({c.name for c in cases}) == len(cases)
    return cases


def as_zlib(c):
    """the raw case inside a zlib container with the right DICTID"""
    return case("zlib_" + c.name, ZLIB, zlib_wrap(c.stream, c.data, F.adler32(c.dict)), c.data, c.dict, c.verdict, c.zlib)


@functools.lru_cache(maxsize=None)
def zlib_cases(n):
    """the header and trailer of a zlib stream that is decoded with the dictionary of n bytes"""
    dict_ = dictionary(n)
    W = min(n, MAX_DIST)
    did = F.adler32(dict_)
    s = _begin(dict_, 5).match(3, min(5 + W, MAX_DIST)).match(70, 4).lit(b"!").eob()
    raw, data = s.raw(), bytes(s.out[W:])
    plain = F.Stream().fixed(final=True).lit(b"no need of it ").match(9, 3).eob()      # (no reference to the dictionary)
    z = lambda name, stream, d=data, verdict=OK, zl="": case("zlib%d_%s" % (n, name), ZLIB, stream, d, dict_, verdict, zl)
    good = zlib_wrap(raw, data, did)
    cases = [z("right_dictid", good), z("right_dictid_cinfo_0", zlib_wrap(raw, data, did, cinfo=0)),
             z("wrong_dictid", zlib_wrap(raw, data, did ^ 0x10000), b"", E_DATA),
             z("dictid_little_endian", zlib_wrap(raw, data, int.from_bytes(did.to_bytes(4, "little"), "big")), b"", E_DATA),
             z("fdict_clear", zlib_wrap(plain.raw(), plain.out, None), b"", E_DATA, "ignores the dictionary"),
             z("cm_7_six_bytes", zlib_wrap(raw, data, did, cm=7), b"", E_DATA),
             z("cm_7_cut_4", zlib_wrap(raw, data, did, cm=7)[:4], b"", E_EOF, "raises"),
             z("cinfo_8", zlib_wrap(raw, data, did, cinfo=8), b"", E_DATA),
             z("fcheck", zlib_wrap(raw, data, did, fcheck=(good[1] & 31) ^ 1), b"", E_DATA),
             z("fcheck_cut_5", zlib_wrap(raw, data, did, fcheck=(good[1] & 31) ^ 1)[:5], b"", E_EOF, "raises"),
             z("wrong_adler", zlib_wrap(raw, data, did, adler=F.adler32(data) ^ 0x80), data, E_DATA),
             z("adler_of_dict_and_data", zlib_wrap(raw, data, did, adler=F.adler32(window(dict_) + data)), data, E_DATA),
             z("trailer_cut", good[:-1], data, E_EOF)]
    cases += [z("cut_%d" % k, good[:k], b"", E_EOF) for k in (0, 1, 2, 3, 4, 5)]
    cases.append(z("cut_6", good[:6], b"", E_EOF))       # the whole header and not one bit of the body
    # a wrong dictionary of the same length cannot be told by kind 0, but the DICTID tells it
    cases.append(case("zlib%d_other_dictionary" % n, ZLIB, good, b"", bytes(dict_[:-1]) + bytes([dict_[-1] ^ 1]), E_DATA))
    for c in cases:
        c.zlib_data = bytes(plain.out) if c.zlib == "ignores the dictionary" else c.data
    return cases


# ------------------------------------------------------------------------------------------------- the split path
def _unresolved(s, W):
    """bytes of the output whose value was first written in an earlier piece of the ENTRY (a byte taken from the window is its own root: Seeded)"""
    starts = [W] + [m[2] for m in s.marks]
    return sum(r < max(b for b in starts if b <= i) for i, r in enumerate(s.root) if i >= W)


def _finish(name, s, dict_, W, verdict=OK, good=None):
    """behind the case's block: stored filler (the entry has to reach the split threshold of the tests: 4 KiB), the end"""
    s.stored(F.text(3300, 11))
    s.fixed(final=True).lit(b"end").eob()
    data = bytes(s.out[W:]) if good is None else good
    c = case(name, RAW, s.raw(0xFF if verdict != OK else 0), data, dict_, verdict)
    c.unresolved = _unresolved(s, W) if verdict == OK else None
    c.pieces = 1 + len(s.marks)
    assert len(c.stream) >= 4096
    return c


def _later_piece(dict_, piece):
    """A match at p = 0 into the window in the first piece, then a dynamic block decoded by a wave of a later piece."""
    s = Seeded(dict_)
    W = len(s.out)
    s.fixed().match(8, 3).lit(b"in front").eob()
    F.to_next_piece(s, 13, 0, piece)
    ll, dl = F.piece_tables()
    return s.dynamic(ll, dl).lit(b"a later piece "), W


@functools.lru_cache(maxsize=None)
def split_cases(n, piece=1024):
    """(b) in a LATER piece matches with d = base + p + k, k in {1, W}: valid, and in front of the entry;
    (c) d = base + p + W + 1 there: BZ_E_DATA at that code with every byte in front of it;
    (d) a straddle in a later piece: the source starts in the window, runs through the first piece's bytes into the piece
        itself (d < len): the first piece gives 16 bytes, empty stored blocks carry the stream into the next piece."""
    dict_ = dictionary(n)
    cases = []
    s, W = _later_piece(dict_, piece)
    for k in (1, W, 1, 2, W - 1):
        s.match(6, len(s.out) - W + k).lit(b"+")
    s.match(258, len(s.out) - W + W).lit(b"+").eob()
    cases.append(_finish("split%d_into_the_window" % n, s, dict_, W))
    s, W = _later_piece(dict_, piece)
    s.match(6, len(s.out) - W + W)
    good = bytes(s.out[W:])
    s.match(5, len(s.out) - W + W + 1, emit=False).lit(b"never").eob()
    cases.append(_finish("split%d_one_too_far" % n, s, dict_, W, E_DATA, good))
    for lits in (0, 1, 70):
        s = Seeded(dict_)
        s.fixed().match(8, 3).lit(b"in front").eob()
        for _ in range(piece // 5 + 8):
            s.stored(b"")
        s.marks.append((None, 1, len(s.out)))       # (the next piece starts at one of these LEN fields: all at this output position)
        ll, dl = F.piece_tables()
        s.dynamic(ll, dl).lit(F.text(lits, 3))
        s.match(258, len(s.out) - W + 5).lit(b"+").match(258, 258 + 1 + 5).eob()
        cases.append(_finish("split%d_straddle_%d" % (n, lits), s, dict_, W))
    return cases
