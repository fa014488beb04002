"""Test helper (not collected by pytest): a bit-level WRITER of hand-made LZHUF streams, for the shapes at which a decoder
can go wrong and that no encoder writes -- in the spirit of dfforge.py / dfshapes.py.

    stream := block*                    bits are packed MSB first; a block is N16, the t-, c- and p-table, then N codes
    t      := n5 (len | skip2 at index 3){..}   or   0_5 s5          len: 3 bits, 7 extended by ones up to a zero
    c      := n9 t-code{..}                      or   0_9 s9          t-code 0: a zero, 1: 3 + x4 zeros, 2: 20 + x9 zeros,
                                                                       k >= 3: length k - 2
    p      := nP len{n}                          or   0_P sP          P = 4 (lh4, lh5) or 5 (lh6, lh7)
    code   := c-code [p-code extra{v - 1}]       a c-symbol >= 256 is a match of sym - 253 bytes at pos + 1 back

A case is PARAMETERS: {name, method, shape, args, k, orig_len, prefill}: `shape` names a builder below, `k` the preamble (a
first block of k one-bit literal codes, so that the case's block header and every field behind it meet another bit phase;
the fixture holds the base cases, expand() puts each small one behind k = 0 .. 32).
`build(case)` makes the stream; `hits(case)` lists, from a traced run of the MODEL decoder (tests/lzhref.py) over that
stream, which of the targets the stream really meets; `REQUIRED` is the set the committed cases must cover.  The cases live
in tests/golden/lzh_shapes.json with the SHA-256 of their streams (parameters only, never the bytes);
`python tests/lzhforge.py --regen` rewrites it.  Pure Python.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lzhref  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lzh_shapes.json")
OK, E_DATA, E_EOF = lzhref.OK, lzhref.E_DATA, lzhref.E_EOF
METHODS = (4, 5, 6, 7)


def _required():
    r = {"end_rem_0", "end_rem_8", "end_rem_15", "end_zero_len", "end_zero_len_junk", "hdr_phase_0",
         "t_const", "c_const", "p_const", "all_const", "t_const_19", "c_const_510", "p_const_over",
         "t_count_1", "t_count_2", "t_count_3", "t_count_4", "t_count_19", "t_count_20",
         "t_skip_0", "t_skip_1", "t_skip_2", "t_skip_3", "t_skip_past", "t_len_7", "t_len_8", "t_len_16", "t_len_17",
         "run_1", "run_2", "run_3", "run_18", "run_19_as_18_1", "run_19_as_1_18", "run_20", "run_531", "run_past",
         "c_count_1", "c_count_510", "c_count_511", "p_len_7", "p_len_16", "p_len_17",
         "p_sym_0", "p_sym_1", "dist_eq_p", "dist_p_plus_1_strict", "dist_p_plus_1_prefill", "match_reads_pending",
         "stage_cross", "block_2", "block_3",
         "ol_0", "ol_mid_literals", "ol_mid_match", "ol_at_block_end", "ol_beyond"}
    r |= {"hdr_phase_%d" % k for k in range(32)}
    r |= {"c_code_%d" % l for l in range(1, 17)}
    r |= {"%s_kraft_%s" % (t, w) for t in "tcp" for w in ("over", "under")} | {"c_kraft_zero"}
    r |= {"len_%d" % l for l in (3, 4, 63, 64, 65, 255, 256)} | {"dist_%d" % d for d in (1, 2, 3, 63, 64, 65)}
    for m in METHODS:
        r |= {"p_sym_max_m%d" % m, "p_count_over_m%d" % m, "dist_window_m%d" % m}
    return frozenset(r)


REQUIRED = _required()


# ------------------------------------------------------------------------------------------------------ the writer
class W:
    """MSB-first bit writer"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, width):
        assert 0 <= value < (1 << width) or width == 0, (value, width)
        self.acc = (self.acc << width) | value
        self.n += width
        return self

    def code(self, cw):  # (code, length) of lzhref.canonical; None: a constant table, no bits
        if cw is not None:
            self.put(*cw)

    def length(self, ln):
        for v, w in lzhref.len_fields(ln):
            self.put(v, w)

    def bytes(self, fill=0):
        pad = -self.n % 8
        acc = (self.acc << pad) | (((1 << pad) - 1) if fill else 0)
        return acc.to_bytes((self.n + pad) // 8, "big")


def balanced(symbols):
    """{symbol: length} of a complete set over two or more symbols, lengths as equal as they get"""
    k = len(symbols)
    assert k >= 2
    e = (k - 1).bit_length()
    short = (1 << e) - k
    return {s: (e - 1 if i < short else e) for i, s in enumerate(sorted(symbols))}


def lens_list(d, n=None):
    n = max(d) + 1 if n is None else n
    return [d.get(i, 0) for i in range(n)]


def zero_toks(gap):
    """the encoder's spelling of a run of `gap` zero lengths"""
    if gap > 19:
        return [(2, gap - 20)] if gap <= 531 else [(2, 511)] + zero_toks(gap - 531)
    if gap == 19:
        return [(1, 15), (0, 0)]
    if gap > 2:
        return [(1, gap - 3)]
    return [(0, 0)] * gap


def c_toks(clens):
    toks, gap = [], 0
    for l in clens:
        if l == 0:
            gap += 1
        else:
            toks += zero_toks(gap) + [(l + 2, 0)]
            gap = 0
    return toks  # (trailing zeros are not written: the count ends at the last code)


def put_t(w, tlens, skip=None):
    """tlens: a list (the count is its length) or an int (the constant form).  skip: the 2-bit field, None = as many of the
    zeros at index 3 .. 5 as there are"""
    if isinstance(tlens, int):
        return w.put(0, 5).put(tlens, 5)
    w.put(len(tlens), 5)
    i = 0
    while i < len(tlens):
        if i == 3:
            sk = skip
            if sk is None:
                sk = 0
                while sk < 3 and 3 + sk < len(tlens) and tlens[3 + sk] == 0:
                    sk += 1
            w.put(sk, 2)
            i += sk
            if i >= len(tlens):
                break
        w.length(tlens[i])
        i += 1
    return w


def put_c(w, n, toks, tcode):
    """n: the count, or ("const", s); toks: (t-symbol, extra) in stream order; tcode: canonical codes, or None (constant t)"""
    if isinstance(n, tuple):
        return w.put(0, 9).put(n[1], 9)
    w.put(n, 9)
    for k, x in toks:
        if tcode is not None:
            w.code(tcode[k])
        if k == 1:
            w.put(x, 4)
        elif k == 2:
            w.put(x, 9)
    return w


def put_p(w, plens, pbits):
    if isinstance(plens, int):
        return w.put(0, pbits).put(plens, pbits)
    w.put(len(plens), pbits)
    for l in plens:
        w.length(l)
    return w


def block(w, method, codes, clens=None, plens=None, tlens=None, toks=None, ccount=None, ncodes=None, skip=None):
    """One block.  codes: ("lit", b) | ("match", len, dist).  clens / plens: {symbol: length}, an int (the constant form),
    or None (derived: balanced over the symbols in use, constant for one).  toks / ccount / tlens: the c-table's t-codes,
    its count and the t-table, when they are not to be derived."""
    pbits = lzhref.OFFSET_BITS[method]
    csyms, psyms, conv = set(), set(), []
    for c in codes:
        if c[0] == "lit":
            csyms.add(c[1])
            conv.append((c[1],))
        else:
            po, sub = lzhref.convert_pos(c[2] - 1)
            csyms.add(c[1] + 253)
            psyms.add(po)
            conv.append((c[1] + 253, po, sub))
    if clens is None:
        clens = balanced(csyms) if len(csyms) > 1 else (min(csyms) if csyms else 0)
    if plens is None:
        plens = balanced(psyms) if len(psyms) > 1 else (min(psyms) if psyms else 0)
    w.put(len(codes) if ncodes is None else ncodes, 16)
    if isinstance(clens, int):
        put_t(w, 0 if tlens is None else tlens, skip)
        put_c(w, ("const", clens), None, None)
        ccode = None
    else:
        cl = lens_list(clens)
        if toks is None:
            toks = c_toks(cl)
        if tlens is None:
            used = {k for k, _ in toks}
            tlens = lens_list(balanced(used)) if len(used) > 1 else min(used)
        put_t(w, tlens, skip)
        put_c(w, len(cl) if ccount is None else ccount, toks, None if isinstance(tlens, int) else lzhref.canonical(tlens))
        ccode = lzhref.canonical(cl)
    if isinstance(plens, int):
        put_p(w, plens, pbits)
        pcode = None
    else:
        put_p(w, lens_list(plens), pbits)
        pcode = lzhref.canonical(lens_list(plens))
    for c in conv:
        if ccode is not None:
            w.code(ccode[c[0]])
        if len(c) == 3:
            if pcode is not None:
                w.code(pcode[c[1]])
            if c[1] > 1:
                w.put(c[2], c[1] - 1)
    return w


def preamble(w, method, k):
    """a block of k one-bit literal codes ('p' and 'q' alternating; k == 1: 'p' and one 'q' ... k >= 1)"""
    if k:
        block(w, method, [("lit", 0x70 + (i & 1)) for i in range(k)], clens={0x70: 1, 0x71: 1})
    return w


def lits(s):
    return [("lit", b) for b in bytes(s)]


# ------------------------------------------------------------------------------------------------------ the shapes
# every shape: f(w, method, *args) writes its blocks into w and returns the fill of the padding bits (0 / 1) or None
def sh_raw(w, m, hexbytes):
    w.put(int(hexbytes, 16), 4 * len(hexbytes)) if hexbytes else None


def sh_lits(w, m, text, tail_bits=0, tail_val=0):
    """a block of literals and tail_bits more bits; the text grows until the stream ends on a byte with them"""
    text = text.encode()
    while True:
        t = W()
        block(t, m, lits(text))
        if (t.n + tail_bits) % 8 == 0:
            break
        text += bytes([0x61 + len(text) % 26])
    block(w, m, lits(text))
    w.put(tail_val, tail_bits)


def sh_all_const_lits(w, m, n):
    block(w, m, [("lit", 0x41)] * n)


def sh_all_const_matches(w, m, n):
    block(w, m, [("lit", 0x42)])
    block(w, m, [("match", 256, 1)] * n)


def sh_t_count(w, m, n, skip=None):
    """a t-table of n lengths: the c-table uses t-symbols below n only (n <= 3: zeros and runs cannot spell a length, so
    such a table is met with a c-table that must fail or with lengths via symbol n - 1 >= 3)"""
    if n <= 3:
        tl = [1, 1][:n] if n == 2 else ([0] if n == 1 else [1, 2, 2])
        w.put(1, 16)
        put_t(w, tl, skip)
        put_c(w, 4, [(0, 0)] * 4, lzhref.canonical(tl) if n >= 2 else None)
        put_p(w, 0, lzhref.OFFSET_BITS[m])
        w.put(0, 8)
        return
    if n == 4:  # t-symbols 0 (a zero) and 3 (a length of 1): the c-symbols 1 and 2
        block(w, m, lits(b"\x01\x02\x02\x01"), clens={1: 1, 2: 1}, tlens=[1, 0, 0, 1], toks=[(0, 0), (3, 0), (3, 0)], skip=skip)
        return
    if n == 19:
        cl = {0x61: 1, 0x62: 2, 0x63: 3, 0x64: 4, 0x65: 5, 0x66: 6, 0x67: 7, 0x68: 8, 0x69: 9, 0x6A: 10, 0x6B: 11, 0x6C: 12, 0x6D: 13,
              0x6E: 14, 0x6F: 15, 0x70: 16, 0x71: 16}
        tl = None
    else:  # 20: refused
        w.put(1, 16).put(20, 5).put(0, 32)
        return
    block(w, m, lits(bytes(range(0x61, 0x72))), clens=cl, tlens=tl, skip=skip)


def sh_t_skip(w, m, sk, n):
    """the skip field with value sk in a t-table of n lengths (n < 3 + sk: past the count)"""
    tl = [1, 2, 0] + [0] * sk + [2]
    tl = tl[:n] if n < len(tl) else tl
    if n < 3 + sk:  # past the count
        w.put(1, 16).put(n, 5)
        for l in tl[:3]:
            w.length(l)
        w.put(sk, 2).put(0, 32)
        return
    # t-symbols 0 (len 1), 1 (len 2), 3 + sk (len 2): three zeros, then 2^L c-lengths of L = 1 + sk
    L = 1 + sk
    cl = {3 + i: L for i in range(1 << L)}
    block(w, m, lits(bytes(range(3, 3 + (1 << L)))), clens=cl, tlens=tl, toks=[(1, 0)] + [(3 + sk, 0)] * (1 << L))


def sh_t_unary(w, m, top):
    """t-lengths 1, 2, .. top - 1, top, top (top <= 16 complete; 17: refused)"""
    tl = list(range(1, top)) + [top, top]
    if top > 16:
        w.put(1, 16).put(len(tl[:19]), 5)
        i = 0
        for l in tl[:19]:
            if i == 3:
                w.put(0, 2)
            w.length(l)
            i += 1
        w.put(0, 32)
        return
    # t-symbols 0 .. top: symbol 0 (a zero) has the 1-bit code; the c-table is 'a' and 'b' of length 1 spelled with symbol 3
    n = len(tl)
    toks = [(2, 0x61 - 20), (3, 0), (3, 0)]
    tl2 = tl + [0] * max(0, 4 - n)
    block(w, m, lits(b"abba"), clens={0x61: 1, 0x62: 1}, tlens=tl2[:19], toks=toks)


def sh_runs(w, m, spell):
    """c-tables whose zero runs are spelled as `spell` says, between codes of length 1 .. : the symbols in use follow"""
    toks, pos = [], 0
    syms = []
    for item in spell:
        for k, x in item:
            toks.append((k, x))
            pos += 1 if k == 0 else 3 + x if k == 1 else 20 + x
        syms.append(pos)
        toks.append(None)  # a length goes here
        pos += 1
    ks = len(syms)
    cl = balanced(syms)
    out, it = [], iter(sorted(syms))
    for t in toks:
        out.append((cl[next(it)] + 2, 0) if t is None else t)
    block(w, m, lits(bytes(s for s in syms if s < 256)), clens=cl, toks=out)
    return ks


def sh_run_past(w, m, tconst=None):
    if tconst == "big":  # the longest run there is: 531 zeros, more than any count allows
        tl = [0, 0, 1, 1]
        w.put(1, 16)
        put_t(w, tl)
        put_c(w, 510, [(2, 511)], lzhref.canonical(tl))
        w.put(0, 32)
    elif tconst is None:
        block(w, m, lits(b"ab"), clens={0x61: 1, 0x62: 1}, toks=[(2, 0x61 - 20), (3, 0), (3, 0), (1, 5)], ccount=0x64)
    else:  # a constant t-code of 1 or 2 that does not meet the count exactly
        w.put(1, 16)
        put_t(w, tconst)
        w.put(100, 9)
        for _ in range(40):
            w.put(0, 9 if tconst == 2 else 4)
        w.put(0, 32)


def sh_c_count(w, m, n):
    if n == 1:      # one length: symbol 0 with length 1 alone is under-subscribed -- the count itself is legal
        w.put(1, 16)
        put_t(w, 3)
        w.put(1, 9)
        put_p(w, 0, lzhref.OFFSET_BITS[m])
        w.put(0, 8)
    elif n == 510:
        block(w, m, lits(b"a") + [("match", 256, 1), ("match", 3, 1)], clens={0x61: 2, 256: 2, 509: 1})
    else:  # 511: refused, though the lengths behind it are a complete set
        block(w, m, lits(b"\x00\x01"), clens={0: 1, 1: 1}, toks=[(3, 0), (3, 0), (2, 489)], ccount=511)


def sh_c_lengths(w, m):
    cl = {0x61 + i: i + 1 for i in range(16)}
    cl[0x71] = 16
    block(w, m, lits(bytes(range(0x61, 0x72)) * 2), clens=cl)


def sh_kraft(w, m, table, how):
    bad = [1, 1, 1] if how == "over" else [1, 2] if how == "under" else [0, 0]
    if table == "t":
        w.put(1, 16)
        put_t(w, bad if how != "under" else [1, 2, 0])
        w.put(0, 32)
    elif table == "c":
        w.put(1, 16)
        tl = [1, 0, 0, 2, 2]
        put_t(w, tl)
        put_c(w, len(bad), [(0, 0) if l == 0 else (l + 2, 0) for l in bad], lzhref.canonical(tl))
        w.put(0, 32)
    else:
        w.put(1, 16)
        put_t(w, 0)
        put_c(w, ("const", 0x61), None, None)
        put_p(w, bad if how != "zero" else [0, 0], lzhref.OFFSET_BITS[m])
        w.put(0, 32)


def sh_const_limits(w, m, table):
    w.put(1, 16)
    if table == "t":
        w.put(0, 5).put(19, 5).put(0, 32)
    elif table == "c":
        w.put(0, 5).put(0, 5).put(0, 9).put(510, 9).put(0, 32)
    else:
        pb = lzhref.OFFSET_BITS[m]
        w.put(0, 5).put(0, 5).put(0, 9).put(0x61, 9).put(0, pb).put(min(lzhref.DICT_BITS[m] + 1, (1 << pb) - 1), pb).put(0, 32)


def sh_p_count_over(w, m):
    pb = lzhref.OFFSET_BITS[m]
    n = lzhref.DICT_BITS[m] + 2
    w.put(1, 16).put(0, 5).put(0, 5).put(0, 9).put(0x61, 9)
    if n < (1 << pb):
        w.put(n, pb)
        for i in range(n):
            w.length(1 if i < 2 else 0)
    else:
        w.put((1 << pb) - 1, pb)
    w.put(0, 32)


def sh_p_lens(w, m, top):
    """p-lengths 1 .. top - 1, top, top over the p-symbols 0 .. top (top <= dictionary_bits); 17: refused"""
    db = lzhref.DICT_BITS[m]
    if top > 16:
        w.put(1, 16).put(0, 5).put(0, 5).put(0, 9).put(0x61, 9).put(2, lzhref.OFFSET_BITS[m])
        w.length(17)
        w.put(0, 32)
        return
    top = min(top, db)
    pl = {i: i + 1 for i in range(top)}
    pl[top] = top
    block(w, m, lits(b"x" * 40) + [("match", 3, 1), ("match", 3, 2)], plens={0: 1, 1: 1})
    # distances with p-symbol v need 1 << (v - 1) bytes in front of them
    need = (1 << (top - 1)) + 1 if top > 1 else 2
    fillers = []
    have = 46
    while have < need:
        fillers.append(("match", 256, 1))
        have += 256
    block(w, m, fillers + [("match", 3, (1 << (v - 1)) + 1 if v > 1 else v + 1) for v in range(top + 1)], plens=pl)


def sh_matches(w, m, pairs, lead=70):
    """`lead` literals, then the (length, distance) pairs"""
    block(w, m, lits(bytes((i * 7 + 3) & 0xFF for i in range(lead))) + [("match", l, d) for l, d in pairs])


def sh_dist_at_p(w, m, extra):
    """five literals, then a match at distance 5 + extra"""
    block(w, m, lits(b"hello") + [("match", 4, 5 + extra)])


def sh_window(w, m, over):
    """more than a window of output, then a match at the window's distance (the largest the format can say)"""
    win = 1 << lzhref.DICT_BITS[m]
    n = win // 256 + 2
    block(w, m, lits(b"wxyz") + [("match", 256, 4)] * n + [("match", 5, win)])


def sh_pending(w, m):
    block(w, m, lits(b"0123456789") + [("match", 6, 3)] + lits(b"ab") + [("match", 3, 1)])


def sh_stage_cross(w, m):
    """long codes (16 bits) in a row across bit 2048"""
    cl = {0x61 + i: i + 1 for i in range(16)}
    cl[0x71] = 16
    block(w, m, lits(bytes([0x70, 0x71] * 80)), clens=cl)


def sh_blocks(w, m, n):
    texts = [b"first block, ", b"second one with other letters; ", b"THIRD 0123456789"]
    for i in range(n):
        block(w, m, lits(texts[i]) + [("match", 3 + i, 2 + i)])


def sh_entry_mod(w, m, r):
    """a stream of 4k + r bytes whose last bits matter"""
    text = b"the quick brown fox jumps over the lazy dog"
    for cut in range(len(text), 8, -1):
        t = W()
        block(t, m, lits(text[:cut]))
        if len(t.bytes()) % 4 == r and t.n % 8 == 0:
            break
    else:
        for cut in range(len(text), 8, -1):
            t = W()
            block(t, m, lits(text[:cut]))
            if len(t.bytes()) % 4 == r:
                break
    block(w, m, lits(text[:cut]))


SHAPES = {f.__name__[3:]: f for f in (sh_raw, sh_lits, sh_all_const_lits, sh_all_const_matches, sh_t_count, sh_t_skip, sh_t_unary, sh_runs,
                                      sh_run_past, sh_c_count, sh_c_lengths, sh_kraft, sh_const_limits, sh_p_count_over, sh_p_lens,
                                      sh_matches, sh_dist_at_p, sh_window, sh_pending, sh_stage_cross, sh_blocks, sh_entry_mod)}
BIG = ("all_const_lits", "all_const_matches", "window")  # shapes that are not repeated behind every preamble


def build(case):
    w = W()
    preamble(w, case["method"], case.get("k", 0))
    SHAPES[case["shape"]](w, case["method"], *case.get("args", []))
    s = w.bytes(case.get("fill", 0))
    cut = case.get("cut")
    return s if cut is None else s[:cut]


def expected(case, stream=None, trace=None):
    """(bytes, verdict, Result) of the MODEL for the case"""
    r = lzhref.decode_full(build(case) if stream is None else stream, case["method"], case.get("orig_len"), case.get("prefill", -1), trace=trace)
    return bytes(r.out), r.verdict, r


def hits(case):
    t = set()
    expected(case, trace=t)
    return t & REQUIRED


def case_id(c):
    return "%s-m%d-k%d" % (c["name"], c["method"], c.get("k", 0))


# ------------------------------------------------------------------------------------------------------ the cases
def base_cases():
    C = []

    def add(name, shape, args=(), methods=(5,), **kw):
        for m in methods:
            C.append(dict(name=name, method=m, shape=shape, args=list(args), **kw))

    # ends
    for n, hx in enumerate(("", "00", "0000", "000000", "0001", "000100", "0000deadbeef", "0000ab")):
        add("raw%d" % n, "raw", [hx])
    add("rem8", "lits", ["ab", 8, 0x5A])
    add("rem15", "lits", ["ab", 15, 0x5A5A >> 1])
    add("rem16", "lits", ["ab", 16, 0])
    add("rem16junk", "lits", ["ab", 16, 0x8001])
    add("zero_junk", "lits", ["abc", 48, 0xBEEF])
    # table forms
    add("const_lits_16", "all_const_lits", [16], methods=METHODS)
    add("const_lits_max", "all_const_lits", [65535])
    add("const_matches_small", "all_const_matches", [3])
    add("const_matches_max", "all_const_matches", [65535], methods=(7,))
    for t in "tcp":
        add("const_limit_%s" % t, "const_limits", [t], methods=METHODS if t == "p" else (5,))
    # t-table
    for n in (1, 2, 3, 4, 19, 20):
        add("t_count_%d" % n, "t_count", [n])
    for sk in range(4):
        add("t_skip_%d" % sk, "t_skip", [sk, 4 + sk])
    add("t_skip_past", "t_skip", [3, 5])
    for top in (7, 8, 16, 17):
        add("t_unary_%d" % top, "t_unary", [top])
    # c-table
    one = lambda k, x=0: [(k, x)]  # noqa: E731
    add("runs_small", "runs", [[one(2, 0x61 - 20), one(0), one(0) + one(0), one(1, 0), one(1, 15), one(1, 15) + one(0), one(0) + one(1, 15), one(2, 0)]])
    add("runs_long", "runs", [[one(2, 0x61 - 20), one(2, 300)]])
    add("run_531", "run_past", ["big"])
    add("run_past", "run_past")
    add("run_past_tconst1", "run_past", [1])
    add("run_past_tconst2", "run_past", [2])
    for n in (1, 510, 511):
        add("c_count_%d" % n, "c_count", [n])
    add("c_lengths", "c_lengths")
    for t in "tcp":
        for how in ("over", "under"):
            add("kraft_%s_%s" % (t, how), "kraft", [t, how])
    add("kraft_c_zero", "kraft", ["c", "zero"])
    add("kraft_p_zero", "kraft", ["p", "zero"])
    # p-table
    add("p_count_over", "p_count_over", methods=METHODS)
    add("p_lens_max", "p_lens", [16], methods=METHODS)
    add("p_lens_7", "p_lens", [7])
    add("p_lens_17", "p_lens", [17])
    # matches
    add("match_lengths", "matches", [[(3, 1), (4, 70), (63, 64), (64, 63), (65, 65), (255, 2), (256, 3)]])
    add("match_dists", "matches", [[(5, 1), (5, 2), (5, 3), (70, 63), (70, 64), (70, 65), (130, 64), (3, 128)]])
    for extra in (0, 1):
        add("dist_p_%d_strict" % extra, "dist_at_p", [extra])
        add("dist_p_%d_prefill" % extra, "dist_at_p", [extra], prefill=0x20)
    add("dist_far_prefill", "dist_at_p", [200], prefill=0)
    add("window", "window", [0], methods=METHODS)
    add("window_prefill", "window", [0], methods=(4,), prefill=0x20)
    add("pending", "pending")
    add("stage_cross", "stage_cross")
    # entry shapes
    for r in (1, 2, 3):
        add("entry_mod_%d" % r, "entry_mod", [r])
    add("blocks_2", "blocks", [2], methods=METHODS)
    add("blocks_3", "blocks", [3])
    # orig_len
    add("ol_0", "blocks", [2], orig_len=0)
    add("ol_mid_literals", "blocks", [2], orig_len=5)
    add("ol_mid_match", "blocks", [2], orig_len=15)
    add("ol_block_end", "blocks", [2], orig_len=16)
    add("ol_all", "blocks", [2], orig_len=16 + 31 + 4)
    add("ol_beyond", "blocks", [2], orig_len=16 + 31 + 4 + 1)
    add("ol_mid_match_prefill", "dist_at_p", [3], orig_len=7, prefill=0x20)
    return C


def preambles(c):
    """the preambles a base case is met behind: none, and for a small one k = 1 .. 32"""
    return [0] if c["shape"] in BIG else list(range(33))


def expand(cases):
    """every (base case, preamble) as a case of its own"""
    return [dict({f: v for f, v in c.items() if f not in ("sha256", "hits")}, k=k) for c in cases for k in preambles(c)]


def all_cases():
    return expand(base_cases())


def digest(c):
    """the SHA-256 over the streams of a base case behind each of its preambles, every stream behind its length"""
    h = hashlib.sha256()
    for k in preambles(c):
        s = build(dict(c, k=k))
        h.update(len(s).to_bytes(4, "big") + s)
    return h.hexdigest()


def truncations():
    """every prefix of two small streams: (method, stream) pairs; verdict and bytes come from the model"""
    out = []
    for m, text in ((5, b"abracadabra abracadabra abracadabra!"), (7, bytes(range(40)) + b"\0" * 30)):
        z = lzhref.encode(text, m)
        out += [(m, z[:n]) for n in range(len(z) + 1)]
    return out


def load():
    """the committed base cases (expand() makes the corpus of them)"""
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/lzhforge.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    cases, got = [], set()
    for c in base_cases():
        c = dict(c)
        c["sha256"] = digest(c)
        c["hits"] = sorted(set().union(*[hits(dict(c, k=k)) for k in preambles(c)]))
        got |= set(c["hits"])
        cases.append(c)
    missing = sorted(REQUIRED - got)
    if missing:
        print("targets no case hits:", missing)
        return 1
    with open(FIXTURE, "w") as f:
        json.dump({"about": "tests/lzhforge.py --regen: forged LZHUF streams as parameters (shape, args, preamble k, "
                            "orig_len, prefill), the SHA-256 over each case's streams (lzhforge.digest) and the targets they hit", "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases, %d targets" % (len(cases), len(got & REQUIRED)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
