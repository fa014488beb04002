"""Test helper (not collected by pytest): the split LZHUF decoder restated in plain Python, and a forge of small streams
whose blocks have ANY size, so that a stream of a few KB has many blocks and splits at BZ_LZH_SPLIT_KIB=1.

The RULES (csrc/lzh_split.h, DESIGN_lzhuf.md section 11) restated on the model's own parts (lzhref._Bits, _read_len, _table,
_sym):
    header_end(stream, bit, method)    the bit behind a whole valid block header at `bit`, inside the entry; None: none
    candidates(stream, method)         every such bit, ascending
    piece(...)                         one piece: from a bit to the first block boundary at or behind `stop` that holds a
                                       valid header, or to the stream's end; bytes in front of the piece are references
    decode(stream, method, ...)        search, pieces, chain walk, the pieces decoded again, the bytes resolved
`decode` with no candidate rule at all (one piece from bit 0, no stop) is lzhref.decode_full restated; tests/test_lzhsplit.py
holds the two against each other on the forged corpus of tests/lzhforge.py, so the restatement is anchored there.  EXPECTED
VALUES of every test come from lzhref.decode_full alone.

`mutate` names deliberate faults of the rules; tests/test_lzhsplit.py shows that each changes some case.

The FORGE: blocks are token lists [("sym", b) | ("ref", len, pos)] (distance pos + 1) written by lzhref.block_fields, so every
header is what the encoder would write for those codes.  cases() builds the streams, each with the true block starts and with
what it was designed for (`expect`); tests/test_lzhsplit.py::test_cases_hit_their_targets COMPUTES from the rules above that a
case is what its name says -- nothing is claimed.  Pure Python.
"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lzhref as R  # noqa: E402

OK, E_DATA, E_EOF = R.OK, R.E_DATA, R.E_EOF
MUTATIONS = ("kraft_le", "header_past_end", "n0_ok", "skip_at_2", "stop_gt")


def _nothing(*_):
    pass


# ---------------------------------------------------------------------------------------------------- the rules
def _tables(b, method, mut=()):
    """the three tables of a block header behind its 16-bit count, as lzhref.decode_full reads them (same fields, same order,
    same failures); raises lzhref._Eof / _Data"""
    dbits, pbits = R.DICT_BITS[method], R.OFFSET_BITS[method]
    lm = {m for m in mut if m == "kraft_le"}
    n = b.take(5)
    if n == 0:
        ttab = b.take(5)
        if ttab > 18:
            raise R._Data()
    else:
        if n > R.NT:
            raise R._Data()
        ll, skip_at = [], (2 if "skip_at_2" in mut else 3)
        while len(ll) < n:
            if len(ll) == skip_at:
                ll += [0] * b.take(2)
                if len(ll) > n:
                    raise R._Data()
                if len(ll) == n:
                    break
            ll.append(R._read_len(b, lm, _nothing, "t"))
        ttab = R._table(ll, lm, _nothing, "t")
    n = b.take(9)
    if n == 0:
        ctab = b.take(9)
        if ctab > R.NC - 1:
            raise R._Data()
    else:
        if n > R.NC:
            raise R._Data()
        ll = []
        while len(ll) < n:
            k = R._sym(b, ttab)
            run = 1 if k == 0 else 3 + b.take(4) if k == 1 else 20 + b.take(9) if k == 2 else 0
            if len(ll) + max(run, 1) > n:
                raise R._Data()
            ll += [0] * run if run else [k - 2]
        ctab = R._table(ll, lm, _nothing, "c")
    n = b.take(pbits)
    if n == 0:
        ptab = b.take(pbits)
        if ptab > dbits:
            raise R._Data()
    else:
        if n > dbits + 1:
            raise R._Data()
        ptab = R._table([R._read_len(b, lm, _nothing, "p") for _ in range(n)], lm, _nothing, "p")
    b.check()
    return ctab, ptab


def header_end(stream, bit, method, mut=()):
    """The candidate rule: a whole block header at `bit` that is valid and lies inside the entry -> the bit behind it."""
    b = R._Bits(stream, late=True)  # (zeros behind the end; the end is looked at once, below)
    b.pos = bit
    if b.take(16) == 0 and "n0_ok" not in mut:
        return None
    try:
        _tables(b, method, mut)
    except R._Data:
        return None
    except R._Eof:
        if "header_past_end" not in mut:
            return None
    if b.pos > b.total and "header_past_end" not in mut:
        return None
    return b.pos


def candidates(stream, method, mut=()):
    return [bit for bit in range(8 * len(stream)) if header_end(stream, bit, method, mut) is not None]


class Piece:
    """what the sizes launch leaves for one piece; out: byte values, or -k for "the byte k in front of the piece's start"."""

    def __init__(self):
        self.out, self.verdict, self.end, self.ended, self.reach = [], OK, 0, True, 0
        self.blocks = self.literals = self.matches = 0


def piece(stream, method, start, stop=None, base=None, limit=None, has_len=False, prefill=-1, mut=()):
    dbits = R.DICT_BITS[method]
    b, r = R._Bits(stream), Piece()
    b.pos = start
    out, L = r.out, limit
    try:
        while True:
            if L is not None and len(out) >= L:
                break
            if b.total - b.pos < 16:
                if has_len and len(out) < L:
                    r.verdict = E_EOF
                break
            boundary = b.pos
            ncodes = b.take(16)
            if ncodes == 0:
                if has_len and len(out) < L:
                    r.verdict = E_EOF
                break
            ctab, ptab = _tables(b, method)
            if stop is not None and (boundary > stop if "stop_gt" in mut else boundary >= stop):
                r.end, r.ended = boundary, False
                return r
            for _ in range(ncodes):
                b.check()
                if L is not None and len(out) >= L:
                    break
                s = R._sym(b, ctab)
                if s < 256:
                    out.append(s)
                    r.literals += 1
                    continue
                ln, v = s - 253, R._sym(b, ptab)
                pos = (1 << (v - 1)) | b.take(v - 1) if v > 1 else v
                d, p = pos + 1, len(out)
                if d > (1 << dbits):
                    raise R._Data()
                if d > p:
                    if prefill < 0 and base is not None and d > base + p:
                        raise R._Data()
                    r.reach = max(r.reach, d - p)
                if L is not None and ln > L - p:
                    ln = L - p
                for i in range(ln):
                    q = p - d + i % d
                    if q >= 0:
                        out.append(out[q])
                    elif base is not None and base + q < 0:
                        out.append(prefill)
                    else:
                        out.append(q)
                r.matches += 1
            else:
                b.check()
                r.blocks += 1
                continue
            break
    except R._Eof:
        r.verdict = E_EOF
    except R._Data:
        r.verdict = E_DATA
    r.end = min(b.pos, b.total)
    return r


class Split(R.Result):
    pass


def sizes(stream, method, orig_len=None, prefill=-1, mut=(), cands=None):
    """the sizes launch: -> (the candidates behind bit 0, the piece from bit 0 and from each of them, each to the next)"""
    L = orig_len
    if cands is None:
        cands = candidates(stream, method, mut)
    cands = [c for c in cands if c > 0]
    prs = [piece(stream, method, s, e, 0 if k == 0 else None, L if k == 0 else None, k == 0 and L is not None, prefill, mut)
           for k, (s, e) in enumerate(zip([0] + cands, cands + [None]))]
    return cands, prs


def plain_walk(cands, prs):
    """the chain walk alone over what the sizes launch left: the pieces' numbers, then "done" or "broken" """
    walk, cur = [], 0
    while True:
        walk.append(cur)
        if prs[cur].ended:
            return walk + ["done"]
        if prs[cur].end not in cands:
            return walk + ["broken"]
        cur = 1 + cands.index(prs[cur].end)


def decode(stream, method, orig_len=None, prefill=-1, mut=(), cands=None):
    """The split decoder: -> Split with out, verdict, bits, blocks, literals, matches as lzhref.Result, and what
    lzh_decode_split_stats counts: candidates, chain, false, again, filled; depth: the longest chain of pointers from a
    byte to the byte that holds its value; ends: where the chain's pieces ended."""
    L = orig_len
    cands, prs = sizes(stream, method, orig_len, prefill, mut, cands)
    starts = [0] + cands
    stops = cands + [None]
    res = Split()
    res.candidates, res.again, res.filled, res.depth, res.ends, res.broken = len(cands), 0, 0, 0, [], False
    out, depth, cur, chain = [], [], 0, 0
    while True:
        pr, base = prs[cur], len(out)
        if cur:
            left = None if L is None else L - base
            if ((prefill < 0 and pr.reach > base) or (left is not None and (len(pr.out) > left or (len(pr.out) == left and pr.ended)))):
                pr = piece(stream, method, starts[cur], stops[cur], base, left, left is not None, prefill, mut)
                res.again += 1
            elif left is not None and pr.ended and pr.verdict == OK and len(pr.out) < left:
                pr.verdict = E_EOF
        chain += 1
        for v in pr.out:  # (the writing launch knows the base: what lies in front of the ENTRY is the constant)
            if v >= 0:
                out.append(v)
                depth.append(0)
            elif base + v < 0:
                out.append(prefill)
                depth.append(0)
            else:
                out.append(out[base + v])
                depth.append(depth[base + v] + 1)
                res.filled += 1
        res.blocks += pr.blocks
        res.literals += pr.literals
        res.matches += pr.matches
        res.verdict, res.bits = pr.verdict, pr.end
        res.ends.append(pr.end)
        if pr.ended or (L is not None and len(out) >= L):
            break
        nxt = [k for k, c in enumerate(cands) if c == pr.end]
        if not nxt:
            res.broken = True
            break
        cur = 1 + nxt[0]
    res.out = bytearray(out)
    res.chain, res.false = chain, len(prs) - chain
    res.depth = max(depth) if depth else 0
    res.fallback = res.broken or chain < 2
    return res


def same(a, b):
    """a split result against the model's"""
    return (bytes(a.out), a.verdict, a.bits, a.blocks, a.literals, a.matches) == (bytes(b.out), b.verdict, b.bits, b.blocks, b.literals, b.matches)


# ---------------------------------------------------------------------------------------------------- the forge
def lits(data):
    return [("sym", x) for x in bytes(data)]


def ref(ln, dist):
    return ("ref", ln, dist - 1)


def build(blocks, method, tail=b""):
    """-> (stream, true block starts): the blocks bit against bit, zero bits to the next byte, then `tail`"""
    fields, starts, n = [], [], 0
    for toks in blocks:
        starts.append(n)
        f = R.block_fields(toks, R.OFFSET_BITS[method])
        fields += f
        n += sum(w for _, w in f)
    return R.pack_bits(fields) + tail, starts


def text(rng, n):
    words = [b"lorem", b"ipsum", b"dolor", b"sit", b"amet", b"sed", b"do", b"eiusmod", b"tempor", b"ut", b"labore"]
    out = b""
    while len(out) < n:
        out += rng.choice(words) + b" "
    return out[:n]


def parse(data, method):
    """an LZSS parse of `data` with the reference's parser (the token lists the encoder would code)"""
    from oracle import oracle
    return oracle.lzss_tokens(bytes(data), window=1 << R.DICT_BITS[method], max_match=R.MAX_MATCH)


def cut(toks, sizes):
    """the token list in blocks of the given sizes, the last size repeated"""
    out, i, k = [], 0, 0
    while i < len(toks):
        n = sizes[min(k, len(sizes) - 1)]
        out.append(toks[i:i + n])
        i += n
        k += 1
    return out


HEADER_IMAGE_BITS = 52


def header_image(ncodes, csym, psym, method):
    """a whole valid header of three constant tables as bytes: 16 + 10 + 18 + 2 * offset_bits bits, zero bits behind"""
    pb = R.OFFSET_BITS[method]
    return R.pack_bits([(ncodes, 16), (0, 5), (0, 5), (0, 9), (csym, 9), (0, pb), (psym, pb)])


def flat_block(images, rng, per=8):
    """A block of all 256 literals, each `per` times, no match: every c-code is the byte itself (8 bits), so the payload is
    the literals' bytes and can carry header images.  images: [(offset in the payload, bytes)]."""
    n = 256 * per
    body = [None] * n
    left = {v: per for v in range(256)}
    for off, img in images:
        for i, x in enumerate(img):
            assert body[off + i] is None and left[x] > 0
            body[off + i] = x
            left[x] -= 1
    rest = [v for v in range(256) for _ in range(left[v])]
    rng.shuffle(rest)
    it = iter(rest)
    return lits(bytes(x if x is not None else next(it) for x in body))


def payload_bit(stream, method, start):
    """the bit of the first code of the block at `start`"""
    return header_end(stream, start, method)


class Case:
    def __init__(self, name, method, stream, starts, orig_len=None, prefill=-1, expect=None):
        self.name, self.method, self.stream, self.starts = name, method, stream, starts
        self.orig_len, self.prefill = orig_len, prefill
        self.expect = expect or {}  # what the forge designed: checked by tests/test_lzhsplit.py against the rules

    def model(self):
        return R.decode_full(self.stream, self.method, self.orig_len, self.prefill)

    def __repr__(self):
        return "Case(%s)" % self.name


def _phase_blocks(rng, method):
    """blocks of 1 .. 40 codes until a block has started at every bit phase of a word"""
    blocks, seen = [], set()
    while len(seen) < 32 or len(blocks) < 70:
        t = text(rng, rng.randrange(1, 41))
        toks = lits(t) if len(blocks) % 3 else parse(t + t[:9], method)
        blocks.append(toks[:rng.randrange(1, len(toks) + 1)])
        _, starts = build(blocks, method)
        seen = {s % 32 for s in starts}
        assert len(blocks) < 400
    return blocks


def run_blocks(nblocks, per_block, first=b"a"):
    """a period-1 run: one literal, then nothing but matches of 256 at distance 1, `per_block` codes a block"""
    return [lits(first) + [ref(256, 1)] * (per_block - 1)] + [[ref(256, 1)] * per_block for _ in range(nblocks - 1)]


def cases():
    rng = random.Random(29)
    cs = []

    def add(name, method, blocks, tail=b"", **kw):
        s, starts = build(blocks, method)
        c = Case(name, method, s + tail, starts, kw.pop("orig_len", None), kw.pop("prefill", -1), kw)
        cs.append(c)
        return c

    # a block start at each of the 32 bit phases of a word (more than 64 blocks: over the default candidate cap as well)
    for m in (5, 7):
        add("phases_m%d" % m, m, _phase_blocks(rng, m), phases=32)
    # the first code of a later piece: a match with d == base, with d == base + 1 (strict and with prefill 0x20)
    head = [lits(text(rng, 50)), lits(text(rng, 30))]
    add("d_eq_base", 5, head + [[ref(10, 80)] + lits(b"xyz")] + [lits(text(rng, 20))])
    add("d_base_plus_1_strict", 5, head + [[ref(10, 81)] + lits(b"xyz")] + [lits(text(rng, 20))], fault_block=2)
    add("d_base_plus_1_prefill", 5, head + [[ref(10, 81)] + lits(b"xyz")] + [lits(text(rng, 20))], prefill=0x20)
    # a period-1 run across ten blocks: byte i's value lies nine pieces back
    add("run_ten_blocks", 5, run_blocks(10, 3), depth=9)
    # a match straddling a piece's start: its source begins in front of the piece and goes on inside it
    add("straddle", 5, [lits(text(rng, 50)), [ref(30, 10)] + lits(b"q") + [ref(100, 41)], lits(text(rng, 9))], straddle=True)
    # lh7: a distance of 65 536 into the piece two back
    far = [lits(b"ab") + [ref(256, 2)] * 255, lits(text(rng, 300)), [ref(7, 65536), ref(3, 65536)] + lits(b"!")]
    add("lh7_window_two_back", 7, far, far=True)
    # pending literals at a piece's end (blocks of 70 and 130 literals: one and two stores of 64 and a rest)
    add("pending_at_end", 5, [lits(text(rng, 70)), lits(text(rng, 130)), [ref(5, 200)] + lits(text(rng, 3))])
    # embedded false candidates: a header image inside a block, and one whose piece runs past the next true start
    for m in (5, 7):
        # (an image of one literal code ends at once; one of 100 matches with 12 extra bits each runs 1 200 bits on)
        img1, img2 = header_image(1, 0x41, 0, m), header_image(100, 256, 13, m)
        blk = flat_block([(40, img1), (256 * 8 - 60, img2)], rng)
        add("false_candidates_m%d" % m, m, [lits(text(rng, 20)), blk, lits(text(rng, 200)), lits(text(rng, 40))],
            images=[(1, 40), (1, 256 * 8 - 60)])
    # a fault in block k: a bad header (t-count 20), and a distance in front of the output
    good = cut(parse(text(rng, 900), 5), [37, 11, 64])
    cs.append(Case("bad_header_in_block_k", 5, _append_bits(good, 5, [(5, 16), (20, 5), (0, 43)]), build(good, 5)[1], None, -1,
                   {"verdict": E_DATA}))
    add("distance_fault_in_block_k", 5, good[:3] + [[ref(5, 4000)]] + good[3:], verdict=E_DATA, fault_block=3)
    # a header cut by the end
    s, starts = build(good, 5)
    cutat = (starts[-1] + 30) // 8
    cs.append(Case("header_cut_by_end", 5, s[:cutat], starts, None, -1, {"verdict": E_EOF}))
    # the ends: fewer than 16 bits left; N = 0 followed by junk that holds candidates
    add("end_under_16_bits", 5, good, tail=b"\x00")
    cs.append(Case("zero_count_then_junk", 5, _append_bits(good[:4], 5, [(0, 16)]) + build(good, 5)[0], build(good[:4], 5)[1], None, -1,
                   {"junk": True}))
    # the known length: in piece 0, exactly at a seam, mid-match in a later piece, beyond the end
    ol = [lits(text(rng, 40)), lits(text(rng, 25)) + [ref(30, 50)] + lits(b"zz"), lits(text(rng, 33)), lits(text(rng, 12))]
    for name, n in (("ol_in_piece_0", 17), ("ol_at_seam", 40), ("ol_at_second_seam", 97), ("ol_mid_match", 40 + 25 + 11), ("ol_at_end", 142),
                    ("ol_beyond", 143), ("ol_zero", 0)):
        add(name, 5, ol, orig_len=n)
    add("ol_before_fault", 5, head + [[ref(10, 81)] + lits(b"xyz")], orig_len=80)
    add("ol_behind_fault", 5, head + [[("sym", 107), ref(10, 82)]], orig_len=85, fault_block=2)
    # all four methods where the p-table rules differ: a p-count of dictionary_bits + 1 (a distance of the whole window)
    for m in (4, 5, 6, 7):
        w = 1 << R.DICT_BITS[m]
        blocks = [lits(b"ab") + [ref(256, 2)] * (w // 256), lits(text(rng, 30)), [ref(9, w), ref(4, 3)] + lits(b"."), lits(text(rng, 10))]
        add("p_count_max_m%d" % m, m, blocks, p_max=2)
    return cs


def _append_bits(blocks, method, fields):
    """the blocks' stream with further fields bit against its last block"""
    f = []
    for toks in blocks:
        f += R.block_fields(toks, R.OFFSET_BITS[method])
    return R.pack_bits(f + list(fields))


PREFIXES = os.path.join(ROOT, "tests", "golden", "lzh_split_prefixes.json")


def prefix_stream():
    """one multi-block stream of about 3 KiB, every prefix of which is a case"""
    rng = random.Random(2929)
    toks = parse(text(rng, 2700) + bytes(rng.randrange(256) for _ in range(2000)) + text(rng, 1500), 5)
    return build(cut(toks, [120, 150, 77, 90, 140, 33, 101] * 12), 5)  # (short blocks: a piece is a wave's serial work)


def prefix_row(stream, n):
    r = R.decode_full(stream[:n], 5)
    return [len(r.out), r.verdict, r.bits, r.blocks, r.literals, r.matches]


def prefix_results(regen=False):
    """What lzhref.decode_full gives for every prefix of prefix_stream(), recorded (the model takes a minute for all of them):
    [bytes, verdict, bits, blocks, literals, matches] per prefix length; the bytes are that many of the whole stream's.
    tests/test_lzhsplit.py decodes a sample again and holds the SHA-256 of the stream."""
    import hashlib
    import json
    s, _ = prefix_stream()
    if regen:
        rows = [prefix_row(s, n) for n in range(len(s) + 1)]
        with open(PREFIXES, "w") as f:
            json.dump({"sha256": hashlib.sha256(s).hexdigest(), "rows": rows}, f, separators=(",", ":"))
            f.write("\n")
    with open(PREFIXES) as f:
        d = json.load(f)
    assert d["sha256"] == hashlib.sha256(s).hexdigest() and len(d["rows"]) == len(s) + 1
    return s, d["rows"]


def over_cap_stream():
    """more than 64 true block starts in about 1 KiB: over max(64, in_len / 1024) candidates at the default"""
    return [c for c in cases() if c.name == "phases_m5"][0]


if __name__ == "__main__":
    if "--regen" in sys.argv:
        print(len(prefix_results(regen=True)[1]), "prefixes recorded")
