"""LZHUF encoder inputs placed at the shapes where the encode kernels branch (CPU only: Python, numpy, the oracle).

Each case is a small dict -- a generator name and its parameters, the methods it is meant for -- plus what `--regen`
recorded about the bytes it builds: their SHA-256, and per method the targets the model says they hit.  `build(case)`
rebuilds the bytes; `hits(case, oracle, method)` recomputes the targets from the model's codes (oracle.lzss_tokens, and
for the lazy step a plain restatement of SlideDict + LzssEncoder::encode that is held against those codes) and from the
model's tables (oracle.make_tab_with_fn, the run coding of tests/lzhref.py); `REQUIRED` is the set the committed cases
must cover.  `python tests/lzhshapes.py --regen` rewrites tests/golden/lzh_enc_shapes.json.

Families (csrc/k_deflate.hip, "LZHUF encode", and the batch front end it shares with Deflate):
  E  ends: lengths 0 .. 4, the reference's a*11 and a*260, a match cut by the end of the input, a run of 259
  L  every match length 3 .. 256
  D  per method both ends of every p-symbol's range of distances; distance W taken and W + 1 not; more than 255 earlier
     positions of one trigram; a source that lh4's window cuts and lh5's does not
  Z  the lazy step: lazy_index 1 and 2, a candidate of exactly 3 bytes at p + 1 that must not win, a step whose first match
     has 256 bytes (the lazy step is skipped), and both sides of (len << 3) + pos for a candidate one byte longer
  T  tables: each constant form, gaps of 1, 2, 3, 18, 19, 20, 21 and 508 (the largest: symbols 0 and 509), the skip field
     by the first t-index in use (3, 4, 6, 7), t-index 18 (a c-code of 16 bits), p-lengths of 7 and more, a c-table on the
     length-limited path, t-lengths of 7 and more (unary), a p-code of 16 bits, and the widest code word the format has: 47
     bits (a c-code of 16, a p-code of 16, 15 more bits), at several bit phases, one of which reaches a third 32-bit word
  B  blocks: parses of exactly 65 534, 65 535, 65 536 and 131 071 codes, and a block cut between a step's literal and
     its reference
  S  seams: inputs of 4 095, 4 096, 4 097, 65 535 and 65 536 bytes, and an lh7 input whose matches are more than 32 KiB
     long in distance (tests/test_gpu_lzh_encode.py places it across a sort-chunk seam of the image)

Not reachable by an encoder and therefore not required: a t-table whose LAST index is 2 (every c-table with two symbols
lists their lengths, t-indices of 3 and more; the skip field looks at the FIRST index in use of 3 or more, which is what
the T family varies), and a lazy step after a first match of 256 bytes (a later candidate is never better than one that
reached the limit), and a SHORTER candidate at p + 1 that wins by its distance (the source of the first match, one byte on,
is a candidate of at least len - 1 bytes at the same distance, and the search keeps the nearest of the longest).
(k_lzh_emit writes a code as two pieces of at most 32 bits, each across at most two words; the 47-bit cases put the widest
second piece, 31 bits, at the phases the fixture records under "wide_phases".)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import dfshapes as DS  # noqa: E402  (Builder, counter, uniform, Rng)
import lzhref as R  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "lzh_enc_shapes.json")
METHODS = (4, 5, 6, 7)
WIN = {m: 1 << R.DICT_BITS[m] for m in METHODS}
BLOCK = R.BLOCK_CODES
GAPS = (1, 2, 3, 18, 19, 20, 21, 508)
T_FIRST = (3, 4, 6, 7)
S_LENS = (4095, 4096, 4097, 65535, 65536)
B_CODES = (65534, 65535, 65536, 131071)


def p_bounds(method):
    """both ends of every p-symbol's range of distances: 1, 2, 3, 4, 5, 8, 9, 16, .., W"""
    out = [1, 2]
    for v in range(2, R.DICT_BITS[method] + 1):
        out += [(1 << (v - 1)) + 1, 1 << v]
    return sorted(set(out))


def _required():
    req = {"E len=%d" % n for n in range(5)} | {"E a*11", "E a*260", "E match ends input", "E run259"}
    req |= {"L len=%d" % n for n in range(3, 257)}
    for m in METHODS:
        req |= {"D m%d dist=%d" % (m, d) for d in p_bounds(m)}
        req |= {"D m%d W taken" % m, "D m%d W+1 not" % m}
    req |= {"D chain255 cut", "D lh4 cut lh5 sees"}
    req |= {"Z lazy=1", "Z lazy=2", "Z len3 at p+1 loses", "Z first match 256", "Z longer+1 loses", "Z longer+1 wins"}
    req |= {"T c const", "T p empty", "T p const", "T t const", "T all const", "T c limited", "T c len=16", "T tlast=18",
            "T p len>=7", "T t len>=7", "T code>32 bits", "T code=47 bits", "T code=47 third word", "T p len=16"}
    req |= {"T gap=%d" % g for g in GAPS} | {"T tfirst=%d" % k for k in T_FIRST}
    req |= {"B codes=%d" % n for n in B_CODES} | {"B cut inside a step"}
    req |= {"S len=%d" % n for n in S_LENS} | {"S far match lh7"}
    return frozenset(req)


REQUIRED = _required()


# ------------------------------------------------------------------------------------------------------- generators
def gen_bytes(hex):
    return bytes.fromhex(hex)


def gen_rep(byte, n):
    return bytes([byte]) * n


def gen_values(values):
    return bytes(values)


def gen_counter(n, tail=""):
    return DS.counter(n) + bytes.fromhex(tail)


def gen_wedge(method, extra):
    """abc, a run of d, abc again at distance W + extra"""
    return b"abc" + b"d" * (WIN[method] - 3 + extra) + b"abc"


def gen_small(seed, k, n):
    r = DS.Rng(seed)
    return bytes(r.below(k) for _ in range(n))


def gen_text(seed, n):
    """words of a small vocabulary: compressible, with matches of many lengths and distances"""
    r = DS.Rng(seed)
    vocab = [bytes(97 + r.below(26) for _ in range(2 + r.below(9))) for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        out += vocab[r.below(len(vocab)) if r.below(4) else r.below(12)] + b" "
    return bytes(out[:n])


def gen_lengths(seed, lo, hi):
    """one planted match of every length lo .. hi, each a copy of the fresh literals in front of it (distance L + 2:
    every method sees them)"""
    b = DS.Builder(seed)
    for L in range(lo, hi + 1):
        b.lits(DS.uniform(0, 256, L + 3))
        b.plant(L, L + 2, list(range(256)))
    b.lits(DS.uniform(0, 256, 3))
    return bytes(b.out)


def gen_dists(seed, method):
    """planted matches of 3 .. 6 bytes at both ends of every p-symbol's range of the method"""
    b = DS.Builder(seed)
    b.lits(DS.uniform(0, 256, WIN[method] + 64))
    for d in reversed(p_bounds(method)):
        b.plant(3 + b.rng.below(4), d, list(range(256)))
        b.lits(DS.uniform(0, 256, 4))
    return bytes(b.out)


def gen_chain(n):
    """the trigram xyz at n earlier positions, each followed by another byte pair; the first of them is followed by a long
    tail that the last occurrence repeats: with n > 255 the search never reaches it"""
    out = bytearray(b"xyzQRSTUVWQRS")
    for i in range(n):
        out += b"xyz" + bytes([1 + i % 250, 1 + i // 250])
    return bytes(out + b"xyzQRSTUVWQRS" + b"!")


def gen_far(seed, n, d):
    """n bytes without a repeated trigram, then their first n - d .. again: matches at distance n"""
    return DS.counter(n) + DS.counter(n)[:d] + b"\0"


def gen_pfib(seed, counts):
    """planted matches whose p-symbols have Fibonacci-like counts: counts[i] matches of p-symbol 2 + i"""
    b = DS.Builder(seed)
    b.lits(DS.uniform(0, 256, (1 << (len(counts) + 1)) + 64))
    for i, c in enumerate(counts):
        for _ in range(c):
            b.plant(3, (1 << (i + 1)) + 1 + b.rng.below(1 << (i + 1)), list(range(256)))
            b.lits(DS.uniform(0, 256, 2))
    return bytes(b.out)


def gen_lfib(seed, counts, far=0):
    """planted matches whose lengths have Fibonacci counts (counts[i] matches of 3 + i bytes, the commonest first)
    among literals of all 256 values: a c-table deeper than 16.  far: this many of the rarest (longest) ones copy literals
    laid down at the very start, tens of thousands of bytes back: the longest c-code with a long p-code and 15 more bits."""
    b = DS.Builder(seed)
    todo = [3 + i for i, c in enumerate(counts) for _ in range(c)]
    late = [todo.pop() for _ in range(far)]
    b.rng.shuffle(todo)
    b.alpha = list(range(256))
    zones = []
    for L in late:
        b.lits([b.rng.below(256) for _ in range(L + 4)])
        zones.append(len(b.out) - L - 2)
    for L in todo:
        b.lits([b.rng.below(256) for _ in range(L + 3)])
        b.plant(L, L + 2, list(range(256)))
    for L, s in zip(late, zones):
        b.lits([b.rng.below(256) for _ in range(3)])
        while not b._edge_ok(s, L):
            b.lits([b.rng.below(256)])
        b.ref(L, len(b.out) - s)
    b.lits(DS.uniform(0, 256, 3))
    return bytes(b.out)


def gen_tdeep(seed, spec):
    """literals only, no repeated trigram: spec = [(symbols, count of each)] with counts that are powers of two, so the
    c-lengths are exact and the NUMBER of symbols per length is as uneven as spec says -- which is what makes the t-table
    deep (t-lengths of 7 and more, the unary form, in the header and in the c-table's list)"""
    b = DS.Builder(seed)
    vals = list(range(256))
    b.rng.shuffle(vals)
    pool, k = [], 0
    for nsym, cnt in spec:
        for _ in range(nsym):
            pool += [vals[k]] * cnt
            k += 1
    b.lits(pool)
    return bytes(b.out)


def gen_wide(seed, pcounts, lcounts):
    """planted matches (lh7) whose p-symbols AND lengths have Fibonacci counts: pcounts[v] matches of p-symbol v, lcounts[i]
    of length 3 + i; the one match of p-symbol 16 has the rarest length.  With the p-code and the c-code at 16 bits that
    code is 16 + 16 + 15 = 47 bits wide, the format's limit.  Near matches copy literals laid down just in front of them;
    the far ones come last and copy literals no match has used."""
    b = DS.Builder(seed)
    b.alpha = list(range(256))
    r = b.rng
    lens = [3 + i for i, c in enumerate(lcounts) for _ in range(c)]
    rare = lens.pop()  # the longest, once
    r.shuffle(lens)
    near, far = [], []
    for v, c in enumerate(pcounts):
        (near if v <= 6 else far).extend([v] * c)
    r.shuffle(near)
    far.sort()

    def dist(v):
        return v + 1 if v < 2 else (1 << (v - 1)) + 1 + r.below(1 << (v - 1))

    for v in near:
        L, D = lens.pop(), dist(v)
        if D >= L + 2:
            b.lits([r.below(256) for _ in range(D + 2)])
        b.plant(L, D, b.alpha)
        b.lits([r.below(256)])
    for v in far:
        L = rare if v == 16 else lens.pop()
        b.lits([r.below(256) for _ in range(2)])
        b.plant(L, dist(v), b.alpha)
    b.lits([r.below(256) for _ in range(3)])
    return bytes(b.out)


GENS = {"tdeep": gen_tdeep, "wide": gen_wide, "bytes": gen_bytes, "rep": gen_rep, "values": gen_values, "counter": gen_counter, "wedge": gen_wedge, "small": gen_small,
        "text": gen_text, "lengths": gen_lengths, "dists": gen_dists, "chain": gen_chain, "far": gen_far, "pfib": gen_pfib,
        "lfib": gen_lfib}


def build(case):
    return GENS[case["gen"]](**case["args"])


# ------------------------------------------------------------------------------------------------------- the model
def naive_steps(data, window, max_match=R.MAX_MATCH, mutate=(), start=0, stop=None):
    """SlideDict::search_dic + LzssEncoder::encode restated plainly: [(position, lazy_index, m0, m1, m2, chosen)] with
    m = (len, pos) or None.  Quadratic in the worst case: for the small Z cases and the tails of the B cases.
    start / stop: the steps from position `start` (it must be the first byte of a step; everything in front of it is
    history) to the first one at or behind `stop` (tests/dfseams.py: the steps around a part seam)."""
    n = len(data)
    chains = {}

    def hash3(p):
        h = (data[p] << 16) | (data[p + 1] << 8) | data[p + 2]
        return ((h * 0x7A7C4F9F7A7C4F9F) & 0xFFFFFFFFFFFFFFFF) >> 48

    pushed = [0]

    def push_to(p):  # every position in front of p is in the dictionary
        while pushed[0] < p:
            q = pushed[0]
            if q + 3 <= n:
                chains.setdefault(hash3(q), []).append(q)
            pushed[0] += 1

    def search(p):
        if p + 3 > n:
            return None
        push_to(p)
        limit = min(max_match, n - p)
        best, cnt = None, 0
        for q in reversed(chains.get(hash3(p), [])):
            if p - q > window or cnt >= 255:
                break
            cnt += 1
            ln = 0
            while ln < limit and data[q + ln] == data[p + ln]:
                ln += 1
            if ln >= R.MIN_MATCH and (best is None or ln > best[0]):
                best = (ln, p - q - 1)
            if ln == limit:
                break
        return best

    def key(m):
        return (m[0] << 3) + (0 if "no_pos_term" in mutate else m[1])

    floor = R.MIN_MATCH - 1 if "lazy_accepts_3" in mutate else R.MIN_MATCH

    steps, p = [], start
    while p < n and (stop is None or p < stop):
        m0 = search(p)
        m1 = m2 = None
        out, li = m0, 0
        if m0 is not None:
            if out[0] < max_match and p + 1 < n:
                m1 = search(p + 1)
                if m1 is not None and m1[0] > floor and key(m1) > key(out):
                    out, li = m1, 1
            if out[0] < max_match and p + 2 < n:
                m2 = search(p + 2)
                if m2 is not None and m2[0] > floor and key(m2) > key(out):
                    out, li = m2, 2
        steps.append((p, li, m0, m1, m2, out))
        p += 1 if out is None else out[0] + li
    return steps


def steps_tokens(data, steps):
    toks = []
    for p, li, m0, m1, m2, out in steps:
        if out is None:
            toks.append(("sym", data[p]))
        else:
            toks += [("sym", data[p + i]) for i in range(li)] + [("ref", out[0], out[1])]
    return toks


def block_info(oracle, codes, pbits):
    """what write_block makes of one block's codes: tables, gaps, and the bit width of every code"""
    sfreq, ofreq = [0] * R.NC, [0] * 17
    for c in codes:
        if c[0] == "sym":
            sfreq[c[1]] += 1
        else:
            sfreq[c[1] + 256 - R.MIN_MATCH] += 1
            ofreq[R.convert_pos(c[2])[0]] += 1
    stab, lm = oracle.make_tab_with_fn(sfreq, 16, 0)
    otab, _ = oracle.make_tab_with_fn(ofreq, 16, 0)
    cused = [(i, l) for i, l in enumerate(stab) if l]
    pused = [(i, l) for i, l in enumerate(otab) if l]
    gaps, ttab = [], []
    if len(cused) > 1:
        tfreq, i = [0] * R.NT, 0
        for ind, ln in cused:
            gap = ind - i
            i = ind + 1
            gaps.append(gap)
            if gap > 19:
                tfreq[2] += 1
            elif gap == 19:
                tfreq[1] += 1
                tfreq[0] += 1
            elif gap > 2:
                tfreq[1] += 1
            elif gap > 0:
                tfreq[0] += gap
            tfreq[ln + 2] += 1
        ttab, _ = oracle.make_tab_with_fn(tfreq, 16, 0)
    tused = [(i, l) for i, l in enumerate(ttab) if l]
    fields = R.block_fields(codes, pbits)
    widths = []
    for c in codes:
        w = stab[c[1] if c[0] == "sym" else c[1] + 256 - R.MIN_MATCH] if len(cused) > 1 else 0
        if c[0] == "ref":
            v = R.convert_pos(c[2])[0]
            w += (otab[v] if len(pused) > 1 else 0) + max(v - 1, 0)
        widths.append(w)
    bits = sum(w for _, w in fields)
    return dict(stab=stab, otab=otab, ttab=ttab, cused=cused, pused=pused, tused=tused, gaps=gaps, lm=lm, widths=widths, bits=bits,
                hdr_bits=bits - sum(widths), nlit=sum(1 for c in codes if c[0] == "sym"), nref=sum(1 for c in codes if c[0] == "ref"))


def tables_of_counts(oracle, cfreq, pfreq, pbits):
    """the model's answer to bz_gpu_lzh_debug_tables: make_table's c-, p- and t-lengths (padded with zeros to 510, 17 and
    19), the bits of the block header with its 16-bit count, and whether the c-table took the length-limited path"""
    stab, lm = oracle.make_tab_with_fn(list(cfreq), 16, 0)
    otab, _ = oracle.make_tab_with_fn(list(pfreq), 16, 0)
    sf, _ = R._symb_tab_fields(stab)
    of, _ = R._offset_tab_fields(otab, pbits)
    ttab = []
    cused = [(i, l) for i, l in enumerate(stab) if l]
    if len(cused) > 1:
        tfreq, i = [0] * R.NT, 0
        for ind, ln in cused:
            gap, i = ind - i, ind + 1
            if gap > 19:
                tfreq[2] += 1
            elif gap == 19:
                tfreq[1] += 1
                tfreq[0] += 1
            elif gap > 2:
                tfreq[1] += 1
            elif gap > 0:
                tfreq[0] += gap
            tfreq[ln + 2] += 1
        ttab, _ = oracle.make_tab_with_fn(tfreq, 16, 0)

    def pad(t, n):
        return list(t) + [0] * (n - len(t))
    return pad(stab, R.NC), pad(otab, 17), pad(ttab, R.NT), 16 + sum(w for _, w in sf + of), lm


def t_deep_counts(seed=1):
    """510 c-counts, powers of two, with the number of symbols per count growing unevenly: the c-lengths then have very
    uneven counts of their own and the t-table reaches lengths of 7 and more (unary).  No parse was found that makes them,
    so they go to the table builder as they are."""
    r = DS.Rng(seed)
    k = 8 + r.below(6)
    cf, syms, idx = [0] * R.NC, list(range(R.NC)), 0
    r.shuffle(syms)
    for l in range(k):
        for _ in range(1 + r.below(1 << min(l, 6))):
            if idx < R.NC:
                cf[syms[idx]] = 1 << (k - l)
                idx += 1
    return cf


def model(oracle, data, method):
    """-> (tokens, [block_info], stream) of tests/lzhref.py:encode"""
    toks = oracle.lzss_tokens(bytes(data), window=WIN[method], max_match=R.MAX_MATCH)
    infos = [block_info(oracle, toks[i:i + BLOCK], R.OFFSET_BITS[method]) for i in range(0, len(toks), BLOCK)]
    fields = []
    for i in range(0, len(toks), BLOCK):
        fields += R.block_fields(toks[i:i + BLOCK], R.OFFSET_BITS[method])
    return toks, infos, R.pack_bits(fields)


def hits(case, oracle, method, data=None):
    """the targets the case's bytes hit under `method`, from the model alone"""
    data = build(case) if data is None else data
    n, W = len(data), WIN[method]
    toks, infos, stream = model(oracle, data, method)
    got = set()
    refs = [t for t in toks if t[0] == "ref"]
    # ---- E, S, B
    if n <= 4:
        got.add("E len=%d" % n)
    if data == b"a" * 11:
        got.add("E a*11")
    if data == b"a" * 260:
        got.add("E a*260")
    if toks and toks[-1][0] == "ref" and toks[-1][1] < R.MAX_MATCH:
        got.add("E match ends input")
    if n == 259 and len(set(data)) == 1 and [t[0] for t in toks] == ["sym", "ref", "sym", "sym"] and toks[1][1] == 256:
        got.add("E run259")
    if n in S_LENS and refs:
        got.add("S len=%d" % n)
    if len(toks) in B_CODES:
        got.add("B codes=%d" % len(toks))
    if method == 7 and any(t[2] >= 0x8000 for t in refs):
        got.add("S far match lh7")
    # ---- L, D
    for t in refs:
        got.add("L len=%d" % t[1])
        if t[2] + 1 in p_bounds(method):
            got.add("D m%d dist=%d" % (method, t[2] + 1))
    if case["gen"] == "wedge" and case["args"]["method"] == method:
        if case["args"]["extra"] == 0 and toks[-1] == ("ref", 3, W - 1):
            got.add("D m%d W taken" % method)
        if case["args"]["extra"] == 1 and [t[0] for t in toks[-3:]] == ["sym"] * 3:
            got.add("D m%d W+1 not" % method)
    if case["gen"] == "chain" and n - 14 - 5 * case["args"]["n"] == 13:
        p = n - 14  # the last occurrence: its 13-byte source is the first one, behind n nearer candidates
        if case["args"]["n"] > 255 and p - 0 <= W and ("ref", 13, p - 1) not in toks and ("ref", 3, 4) in toks:
            got.add("D chain255 cut")
    if case["gen"] == "far" and method == 5:
        t4 = oracle.lzss_tokens(bytes(data), window=WIN[4], max_match=R.MAX_MATCH)
        if t4 != toks and any(4096 <= t[2] < 8192 for t in refs) and not any(t[0] == "ref" and t[2] >= 4096 for t in t4):
            got.add("D lh4 cut lh5 sees")
    # ---- Z (and the step a block cuts): the plain restatement, held against the oracle's codes
    tail = case.get("tail_from")
    if case["family"] == "Z" or tail is not None:
        base = 0 if tail is None else tail
        steps = naive_steps(data[base:], W)
        st = steps_tokens(data[base:], steps)
        assert st == toks[len(toks) - len(st):], "the restated parse is not the oracle's"
        k = len(toks) - len(st)  # code index of the tail's first code
        for p, li, m0, m1, m2, out in steps:
            if case["family"] == "Z":
                if li:
                    got.add("Z lazy=%d" % li)
                if m0 and m0[0] == R.MAX_MATCH:
                    got.add("Z first match 256")
                if m0 and m0[0] < R.MAX_MATCH and m1 and m1[0] == 3 and (m1[0] << 3) + m1[1] > (m0[0] << 3) + m0[1] and li != 1:
                    got.add("Z len3 at p+1 loses")
                if m0 and m0[0] < R.MAX_MATCH and m1 and m1[0] == m0[0] + 1:
                    got.add("Z longer+1 wins" if li == 1 else "Z longer+1 loses" if (m1[0] << 3) + m1[1] <= (m0[0] << 3) + m0[1] else "Z -")
            if li and k + li == BLOCK and tail is not None:
                got.add("B cut inside a step")
            k += 1 if out is None else li + 1
        got.discard("Z -")
    # ---- T
    bit, wide_phases = 0, []
    for b in infos:
        nc, npu, nt = len(b["cused"]), len(b["pused"]), len(b["tused"])
        if nc == 1:
            got.add("T c const")
            if npu == 0:
                got.add("T all const")
        if npu == 0:
            got.add("T p empty")
        if npu == 1 and nc > 1:
            got.add("T p const")
        if nc > 1 and nt == 1:
            got.add("T t const")
        if b["lm"]:
            got.add("T c limited")
        if nc > 1 and max(b["stab"]) == 16:
            got.add("T c len=16")
        if nt > 1:
            first = min(i for i, _ in b["tused"] if i >= 3)
            if first in T_FIRST:
                got.add("T tfirst=%d" % first)
            if b["tused"][-1][0] == 18:
                got.add("T tlast=18")
        if npu > 1 and max(b["otab"]) >= 7:
            got.add("T p len>=7")
        for g in b["gaps"]:
            if g in GAPS:
                got.add("T gap=%d" % g)
        if max(b["widths"]) > 32:
            got.add("T code>32 bits")
        if nt > 1 and max(b["ttab"]) >= 7:
            got.add("T t len>=7")
        if npu > 1 and max(b["otab"]) == 16:
            got.add("T p len=16")
        at = bit + b["hdr_bits"]
        for w in b["widths"]:
            if w == 47:
                got.add("T code=47 bits")
                wide_phases.append(at % 32)
                if at % 32 + w > 64:
                    got.add("T code=47 third word")
            at += w
        bit += b["bits"]
    return got, dict(tokens=toks, blocks=infos, stream=stream, data=data, wide_phases=wide_phases)


# ------------------------------------------------------------------------------------------------------- named faults
MUTATIONS = ("gap19_as_run_of_19", "skip_from_index_7", "lazy_accepts_3", "block_65536", "max_match_258", "no_pos_term",
             "run1_base_2", "p_count_is_last", "lsb_first_extra")


def _symb_tab_fields_mut(oracle, tab, mut):
    """tests/lzhref.py:_symb_tab_fields with the faults of `mut` (none: the same fields, which the tests hold it to)"""
    used = [(i, l) for i, l in enumerate(tab) if l]
    if len(used) == 1:
        return [(0, 5), (0, 5), (0, 9), (used[0][0], 9)], None
    sym_list, freq, i = [], [0] * R.NT, 0
    for ind, ln in used:
        gap = ind - i
        i = ind + 1
        if gap > 19:
            sym_list.append((2, gap - 20))
            freq[2] += 1
        elif gap == 19 and "gap19_as_run_of_19" in mut:  # 0, then a run of 18
            sym_list += [(0, 0), (1, 15)]
            freq[1] += 1
            freq[0] += 1
        elif gap == 19:
            sym_list += [(1, 15), (0, 0)]
            freq[1] += 1
            freq[0] += 1
        elif gap > (1 if "run1_base_2" in mut else 2):
            sym_list.append((1, gap - 3 if gap >= 3 else 0))
            freq[1] += 1
        elif gap > 0:
            sym_list += [(0, 0)] * gap
            freq[0] += gap
        sym_list.append((3, ln + 2))
        freq[ln + 2] += 1
    ttab, _ = oracle.make_tab_with_fn(freq, 16, 0)
    tused = [(i, l) for i, l in enumerate(ttab) if l]
    ret = []
    if len(tused) == 1:
        ret += [(0, 5), (tused[0][0], 5)]
        tcode = None
    else:
        ret.append((tused[-1][0] + 1, 5))
        i = 0
        for ind, ln in tused:
            while ind >= i:
                if i == 3:
                    skip = 3 if ind > (7 if "skip_from_index_7" in mut else 6) else ind - 3
                    ret.append((skip, 2))
                    i += skip
                ret += [(0, 3)] if ind != i else R.len_fields(ln)
                i += 1
        tcode = R.canonical(ttab)
    ret.append((used[-1][0] + 1, 9))
    for sy, l in sym_list:
        k = l if sy == 3 else sy
        if tcode is not None:
            ret.append(tcode[k])
        if sy == 1:
            ret.append((l, 4))
        elif sy == 2:
            ret.append((l, 9))
    return ret, R.canonical(tab)


def encode_mut(oracle, data, method, mutate=()):
    """tests/lzhref.py:encode with named faults of the ENCODER; mutate=() is encode itself.  The faults of the parse run
    the plain restatement (naive_steps): small inputs only."""
    mut = set(mutate)
    assert mut <= set(MUTATIONS)
    W, pbits = WIN[method], R.OFFSET_BITS[method]
    if mut & {"lazy_accepts_3", "no_pos_term"}:
        toks = steps_tokens(data, naive_steps(data, W, mutate=mut))
    else:
        toks = oracle.lzss_tokens(bytes(data), window=W, max_match=258 if "max_match_258" in mut else R.MAX_MATCH)
    per = 65536 if "block_65536" in mut else BLOCK
    f = []
    for i in range(0, len(toks), per):
        codes = toks[i:i + per]
        sfreq, ofreq, conv = [0] * (R.NC + 2), [0] * 32, []
        for c in codes:
            if c[0] == "sym":
                sfreq[c[1]] += 1
                conv.append((c[1],))
            else:
                po, sub = R.convert_pos(c[2])
                if "lsb_first_extra" in mut and po > 1:
                    sub = int(format(sub, "0%db" % (po - 1))[::-1], 2)
                sfreq[c[1] + 256 - R.MIN_MATCH] += 1
                ofreq[po] += 1
                conv.append((c[1] + 256 - R.MIN_MATCH, po, sub))
        stab, _ = oracle.make_tab_with_fn(sfreq, 16, 0)
        otab, _ = oracle.make_tab_with_fn(ofreq, 16, 0)
        f.append((len(codes) & 0xFFFF, 16))
        sf, scode = _symb_tab_fields_mut(oracle, stab, mut)
        of, ocode = R._offset_tab_fields(otab, pbits)
        if "p_count_is_last" in mut and ocode is not None:
            of[0] = (of[0][0] - 1, pbits)
        f += sf + of
        for c in conv:
            if scode is not None:
                f.append(scode[c[0]])
            if len(c) == 3:
                if ocode is not None:
                    f.append(ocode[c[1]])
                if c[1] > 1:
                    f.append((c[2], c[1] - 1))
    return R.pack_bits(f)


# ------------------------------------------------------------------------------------------------------- the corpus
def cases():
    c = []

    def add(family, name, gen, args, methods=METHODS, **kw):
        c.append(dict(family=family, name=name, gen=gen, args=args, methods=list(methods), **kw))

    for n in range(5):
        add("E", "len%d" % n, "bytes", dict(hex=b"abcd"[:n].hex()))
    add("E", "a11", "rep", dict(byte=97, n=11))
    add("E", "a260", "rep", dict(byte=97, n=260))
    add("E", "run259", "rep", dict(byte=0, n=259))
    add("E", "zero257", "rep", dict(byte=0, n=257))
    add("L", "lengths", "lengths", dict(seed=1, lo=3, hi=256))
    for m in METHODS:
        add("D", "dists_m%d" % m, "dists", dict(seed=10 + m, method=m), methods=[m])
        add("D", "wedge_m%d" % m, "wedge", dict(method=m, extra=0), methods=[m])
        add("D", "wedge1_m%d" % m, "wedge", dict(method=m, extra=1), methods=[m])
    add("D", "chain300", "chain", dict(n=300))
    add("D", "far5000", "far", dict(seed=0, n=5000, d=600), methods=[4, 5])
    for seed in (3, 11, 21):
        add("Z", "small%d" % seed, "small", dict(seed=seed, k=3, n=400))
    add("Z", "text2", "text", dict(seed=2, n=3000))
    add("Z", "run300", "rep", dict(byte=7, n=300))
    add("T", "gaps", "values", dict(values=[0, 2, 5, 9, 28, 48, 69, 91]))
    add("T", "bytes256", "values", dict(values=list(range(256))))
    add("T", "abc", "values", dict(values=[1, 2, 3]))
    add("T", "five", "values", dict(values=[1, 2, 3, 4, 5]))
    add("T", "seventeen", "values", dict(values=list(range(17))))
    add("T", "thirtythree", "values", dict(values=list(range(33))))
    add("T", "pfib", "pfib", dict(seed=4, counts=[21, 13, 8, 5, 3, 2, 1, 1]), methods=[5, 7])
    add("T", "lfib", "lfib", dict(seed=6, counts=[1597, 987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1, 1]), methods=[4, 7])
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597]
    pc = [0] * 17
    for v, f in zip([16, 0, 15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 1, 5, 4, 3, 2], fib):
        pc[v] = f
    for seed in (1, 2, 3, 4):
        add("T", "wide47_%d" % seed, "wide", dict(seed=seed, pcounts=pc, lcounts=fib[::-1]), methods=[7])
    add("T", "tdeep", "tdeep", dict(seed=0, spec=[[128, 1], [64, 2], [16, 8], [8, 8], [4, 16], [1, 64]]))
    add("T", "wide", "lfib", dict(seed=8, counts=[1597, 987, 610, 377, 233, 144, 89, 55, 34, 21, 13, 8, 5, 3, 2, 1, 1], far=4), methods=[7])
    for n in (65534, 65535, 65536):
        add("B", "codes%d" % n, "counter", dict(n=n), methods=[5])
    add("B", "codes131071", "counter", dict(n=131071), methods=[7])
    for n in S_LENS:
        add("S", "text%d" % n, "text", dict(seed=n, n=n), methods=METHODS if n < 60000 else [4, 7])
    add("S", "far40000", "far", dict(seed=0, n=40000, d=30000), methods=[6, 7])
    return c


def cut_case(oracle):
    """counter bytes, then a tail over {0, 1, 2} whose parse has a lazy step: the counter's length puts the step's literal
    at code 65 534 and its reference at 65 535, the first code of the second block.  (No trigram with a byte below 3 occurs
    in the counter: the tail's parse is its own.)"""
    for seed in range(1, 200):
        tail = gen_small(seed, 3, 60)
        k = 0
        for p, li, m0, m1, m2, out in naive_steps(tail, WIN[5]):
            if li == 1 and k + 1 < 60:
                n = BLOCK - 1 - k
                return dict(family="B", name="cut_in_step", gen="counter", args=dict(n=n, tail=tail.hex()), methods=[5], tail_from=n)
            k += 1 if out is None else li + 1
    raise ValueError("no lazy step found")


def regen(oracle, log=print):
    out = []
    for c in cases() + [cut_case(oracle)]:
        data = build(c)
        c["sha256"] = hashlib.sha256(data).hexdigest()
        c["len"] = len(data)
        c["targets"] = {}
        for m in c["methods"]:
            got, _ = hits(c, oracle, m, data)
            keep = sorted(t for t in got if t in REQUIRED)
            c["targets"][str(m)] = keep
            if _["wide_phases"]:
                c["wide_phases"] = _["wide_phases"]
        log("%-16s %7d bytes  %s" % (case_id(c), len(data), {m: len(t) for m, t in c["targets"].items()}))
        out.append(c)
    hit = set().union(*(set(t) for c in out for t in c["targets"].values()))
    missing = sorted(REQUIRED - hit)
    log("missing: %r" % missing)
    return dict(cases=out, total_bytes=sum(c["len"] for c in out)), missing


def load():
    with open(FIXTURE) as f:
        return json.load(f)


def case_id(c):
    return "%s-%s" % (c["family"], c["name"])


def main(argv):
    from oracle import oracle
    oracle.lib()
    if "--regen" in argv:
        fix, missing = regen(oracle)
        if missing:
            print("NOT written: targets missing")
            return 1
        with open(FIXTURE, "w") as f:
            json.dump(fix, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s: %d cases, %d bytes" % (FIXTURE, len(fix["cases"]), fix["total_bytes"]))
        return 0
    print(__doc__)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
