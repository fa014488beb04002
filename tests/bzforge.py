"""Test helper (not collected by pytest): a bzip2 stream parser and writer, for forging streams that no
encoder writes.

Written from the format itself:

    stream  := "BZh" level-digit block* trailer padding
    block   := magic48 crc32 randomised1 orig_ptr24 in_use16 (in_use group 16)*
               n_groups3 n_selectors15 selector-mtf-unary* (start5 (("10" | "11")* "0")*){n_groups}
               symbol-codes*            (table selectors[i // 50] codes symbol i; the last symbol is EOB)
    trailer := magic48 combined_crc32, then zero bits (or whatever `pad` holds) up to the byte edge

Symbols are the MTF ranks with zero runs coded in bijective base 2 (RUNA = 0 adds 1 << k, RUNB = 1 adds 2 << k),
a rank r > 0 as r + 1, and EOB = len(in_use) + 1.  Code lengths are delta coded: a 5-bit start value, then per
symbol "10" (+1) or "11" (-1) steps and a "0".  Codes are canonical: lengths ascending, symbols ascending inside a
length, each code one more than the last, shifted left when the length grows.

Pure Python and numpy; the oracle (oracle/oracle.py) is used only by the builders that need a BWT or a CRC.
"""
import numpy as np

BLOCK_MAGIC = 0x314159265359
EOS_MAGIC = 0x177245385090
G_SIZE = 50
RUNA, RUNB = 0, 1
E_DATA = -1


class Block:
    """One block.  `symbols` holds the MTF/ZLE symbols with EOB; `lengths` one list of code lengths per table;
    `selectors` the table of each 50-symbol group (all written ones, also beyond what the symbols need);
    `in_use` the byte values in use, ascending.  Overrides: `n_groups` / `n_selectors` (the header fields; the
    first `n_selectors` selectors are written), `length_codes` (per table: (start, [bit string per symbol, with
    its closing "0"])), `magic` (48 bits), `groups16` (the 16-bit group map; by default the groups that hold an
    in-use byte).  `crc` None means "fill it in" (fill_crcs)."""

    def __init__(self, symbols, lengths, selectors, in_use, orig_ptr, randomised=False, crc=None, n_groups=None,
                 n_selectors=None, length_codes=None, magic=None, groups16=None):
        self.symbols = symbols
        self.lengths = [list(t) for t in lengths]
        self.selectors = list(selectors)
        self.in_use = sorted(in_use)
        self.orig_ptr = orig_ptr
        self.randomised = randomised
        self.crc = crc
        self.n_groups = n_groups
        self.n_selectors = n_selectors
        self.length_codes = length_codes
        self.magic = magic
        self.groups16 = groups16

    @property
    def alpha(self):
        return len(self.in_use) + 2

    def copy(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Block(**d)


class Stream:
    """`level` is the digit (1-9; anything else is written as is); `combined_crc` None means "compute it";
    `pad` is the value of the bits behind the trailer up to the byte edge."""

    def __init__(self, level, blocks, combined_crc=None, header=b"BZh", eos_magic=None, pad=0):
        self.level = level
        self.blocks = list(blocks)
        self.combined_crc = combined_crc
        self.header = header
        self.eos_magic = eos_magic
        self.pad = pad


# ---------------------------------------------------------------------------- codes
def canonical_codes(lengths):
    """Canonical codes of a table (length 0 = unused: None).  An over-subscribed table gets codes that do not
    fit their lengths, exactly as the assignment rule makes them; the writer keeps their low bits."""
    codes = [None] * len(lengths)
    c_len = c_code = 0
    for ln in range(1, max(list(lengths) + [0]) + 1):
        for s, l in enumerate(lengths):
            if l != ln:
                continue
            cd = c_code << (ln - c_len) if c_len < ln else c_code
            c_len, c_code = ln, cd + 1
            codes[s] = cd
    return codes


def kraft(lengths):
    """sum 2^-l over the used symbols, as a fraction of 2^21 (== 1 << 21: complete; above: over-subscribed)"""
    return sum(1 << (21 - l) for l in lengths if l)


def default_length_codes(lengths):
    """the shortest delta string: start at the first length, walk straight to each next one"""
    curr = lengths[0]
    out = []
    for l in lengths:
        s = ("10" * (l - curr)) if l > curr else ("11" * (curr - l))
        out.append(s + "0")
        curr = l
    return (lengths[0], out)


def lengths_from_codes(length_codes):
    start, steps = length_codes
    curr, out = start, []
    for s in steps:
        assert s.endswith("0") and len(s) % 2 == 1
        for i in range(0, len(s) - 1, 2):
            assert s[i] == "1"
            curr += 1 if s[i + 1] == "0" else -1
        out.append(curr)
    return out


# ---------------------------------------------------------------------------- writer
class _Bits:
    """(value, width) pieces; packed once with numpy"""

    def __init__(self):
        self.vals, self.lens = [], []
        self.big = []  # (vals array, lens array) pieces from the symbol coder, kept in order

    def put(self, v, k):
        if k:
            self.vals.append(v & ((1 << k) - 1))
            self.lens.append(k)

    def put_str(self, s):
        for i in range(0, len(s), 32):
            part = s[i:i + 32]
            self.put(int(part, 2), len(part))

    def put_arrays(self, vals, lens):
        self.flush()
        self.big.append((np.asarray(vals, np.uint64), np.asarray(lens, np.int64)))

    def flush(self):
        if self.vals:
            self.big.append((np.array(self.vals, np.uint64), np.array(self.lens, np.int64)))
            self.vals, self.lens = [], []

    def nbits(self):
        return sum(int(l.sum()) for _, l in self.big) + sum(self.lens)

    def bits(self):
        self.flush()
        if not self.big:
            return np.zeros(0, np.uint8)
        vals = np.concatenate([v for v, _ in self.big])
        lens = np.concatenate([l for _, l in self.big])
        keep = lens > 0
        vals, lens = vals[keep], lens[keep]
        idx = np.repeat(np.arange(len(lens)), lens)
        starts = np.cumsum(lens) - lens
        k = np.arange(int(lens.sum()), dtype=np.int64) - starts[idx]
        shift = (lens[idx] - 1 - k).astype(np.uint64)
        return ((vals[idx] >> shift) & np.uint64(1)).astype(np.uint8)


def _selector_mtf(selectors, n_groups):
    lst = list(range(max(n_groups, 1)))
    out = []
    for s in selectors:
        j = lst.index(s)
        lst.insert(0, lst.pop(j))
        out.append(j)
    return out


def _write_block(w, b):
    w.put(BLOCK_MAGIC if b.magic is None else b.magic, 48)
    w.put(0 if b.crc is None else b.crc, 32)
    w.put(1 if b.randomised else 0, 1)
    w.put(b.orig_ptr, 24)
    used = [False] * 256
    for v in b.in_use:
        used[v] = True
    g16 = b.groups16
    if g16 is None:
        g16 = sum(1 << (15 - i) for i in range(16) if any(used[16 * i:16 * i + 16]))
    w.put(g16, 16)
    for i in range(16):
        if g16 >> (15 - i) & 1:
            w.put(sum(1 << (15 - j) for j in range(16) if used[16 * i + j]), 16)
    n_groups = len(b.lengths) if b.n_groups is None else b.n_groups
    n_sel = len(b.selectors) if b.n_selectors is None else b.n_selectors
    assert n_sel <= len(b.selectors)
    w.put(n_groups, 3)
    w.put(n_sel, 15)
    for j in _selector_mtf(b.selectors[:n_sel], max(n_groups, len(b.lengths))):
        w.put_str("1" * j + "0")
    for t, lens in enumerate(b.lengths):
        start, steps = b.length_codes[t] if b.length_codes is not None else default_length_codes(lens)
        w.put(start, 5)
        w.put_str("".join(steps))
    # symbols: table selectors[i // 50] codes symbol i (vectorised: one code and width per table and symbol)
    sym = np.asarray(b.symbols, np.int64)
    if len(sym):
        ntab = len(b.lengths)
        width = max(len(t) for t in b.lengths)
        ctab = np.zeros((ntab, width + 1), np.uint64)
        ltab = np.zeros((ntab, width + 1), np.int64)
        for t, lens in enumerate(b.lengths):
            for s, c in enumerate(canonical_codes(lens)):
                if c is not None:
                    ctab[t, s] = c & ((1 << lens[s]) - 1)
                    ltab[t, s] = lens[s]
            if any(lens) and kraft(lens) < 1 << 21:  # symbol -1: a codeword no symbol owns
                ctab[t, width], ltab[t, width] = hole_code(lens)
        sym = np.where(sym < 0, width, sym)
        sel = np.asarray(b.selectors, np.int64)[np.arange(len(sym)) // G_SIZE]
        assert np.all(ltab[sel, sym] > 0), "a symbol without a code"
        w.put_arrays(ctab[sel, sym], ltab[sel, sym])


def write_bits(streams):
    """the bits of the streams (numpy uint8 0/1), each stream padded to its byte edge"""
    parts = []
    for st in streams:
        w = _Bits()
        for ch in st.header:
            w.put(ch, 8)
        w.put(0x30 + st.level, 8)
        comb = 0
        for b in st.blocks:
            _write_block(w, b)
            comb = (((comb << 1) | (comb >> 31)) & 0xFFFFFFFF) ^ (b.crc or 0)
        w.put(EOS_MAGIC if st.eos_magic is None else st.eos_magic, 48)
        w.put(comb if st.combined_crc is None else st.combined_crc, 32)
        w.put(st.pad, (-w.nbits()) % 8)
        parts.append(w.bits())
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def write(streams):
    if isinstance(streams, Stream):
        streams = [streams]
    return np.packbits(write_bits(streams)).tobytes()


# ---------------------------------------------------------------------------- parser
class _Reader:
    def __init__(self, z):
        self.z = bytes(z) + b"\0" * 16
        self.nbits = 8 * len(z)
        self.pos = 0

    def peek(self, k):
        p = self.pos
        b = p >> 3
        word = int.from_bytes(self.z[b:b + 8], "big")
        return (word >> (64 - (p & 7) - k)) & ((1 << k) - 1)

    def read(self, k):
        if k > 32:
            hi = self.read(k - 32)
            return (hi << 32) | self.read(32)
        v = self.peek(k)
        self.pos += k
        return v


def _decoder_lut(lens):
    """(lut indexed by max_len bits -> symbol | length << 16, max_len)"""
    ml = max(lens)
    lut = np.full(1 << ml, -1, np.int64)
    for s, c in enumerate(canonical_codes(lens)):
        if c is not None:
            sh = ml - lens[s]
            lut[c << sh:(c + 1) << sh] = s | (lens[s] << 16)
    return lut.tolist(), ml


def _parse_block(r):
    magic = r.read(48)
    crc = r.read(32)
    rnd = r.read(1) == 1
    orig = r.read(24)
    g16 = r.read(16)
    in_use, empty_group = [], False
    for i in range(16):
        if g16 >> (15 - i) & 1:
            m = r.read(16)
            empty_group |= m == 0
            in_use += [16 * i + j for j in range(16) if m >> (15 - j) & 1]
    alpha = len(in_use) + 2
    n_groups = r.read(3)
    n_sel = r.read(15)
    lst = list(range(n_groups))
    selectors = []
    for _ in range(n_sel):
        j = 0
        while r.read(1):
            j += 1
        t = lst.pop(j)
        lst.insert(0, t)
        selectors.append(t)
    lengths, codes, custom = [], [], False
    for _ in range(n_groups):
        start = r.read(5)
        steps = []
        for _ in range(alpha):
            s = ""
            while r.read(1):
                s += "1" + str(r.read(1))
            steps.append(s + "0")
        lens = lengths_from_codes((start, steps))
        custom |= default_length_codes(lens) != (start, steps)
        lengths.append(lens)
        codes.append((start, steps))
    luts = [_decoder_lut(t) for t in lengths]
    eob = alpha - 1
    symbols = []
    i = 0
    while True:
        lut, ml = luts[selectors[i // G_SIZE]]
        e = lut[r.peek(ml)]
        assert e >= 0, "a code hole in a stream the parser was given"
        r.pos += e >> 16
        symbols.append(e & 0xFFFF)
        i += 1
        if (e & 0xFFFF) == eob:
            break
    return Block(symbols, lengths, selectors, in_use, orig, randomised=rnd, crc=crc,
                 length_codes=codes if custom else None, magic=None if magic == BLOCK_MAGIC else magic,
                 groups16=g16 if empty_group else None)


def parse(z):
    """list of Streams; write(parse(z)) == z for every well-formed stream (padding included)"""
    r = _Reader(z)
    streams = []
    while r.pos < r.nbits:
        header = bytes([r.read(8), r.read(8), r.read(8)])
        level = r.read(8) - 0x30
        blocks = []
        while True:
            head = r.peek(48)
            if head >> 40 == 0x31:
                blocks.append(_parse_block(r))
                continue
            eos = r.read(48)
            comb = r.read(32)
            k = (-r.pos) % 8
            pad = r.read(k) if k else 0
            streams.append(Stream(level, blocks, combined_crc=comb, header=header,
                                  eos_magic=None if eos == EOS_MAGIC else eos, pad=pad))
            break
    return streams


# ---------------------------------------------------------------------------- builders
def zle_digits(run):
    """RUNA/RUNB digits of a run of `run` zeros (bijective base 2, least significant first)"""
    out = []
    while run > 0:
        if run & 1:
            out.append(RUNA)
            run = (run - 1) >> 1
        else:
            out.append(RUNB)
            run = (run - 2) >> 1
    return out


def symbols_from_last_column(L, in_use=None):
    """MTF + RUNA/RUNB symbols (with EOB) of a last column; `in_use` may name bytes that never occur"""
    L = np.asarray(bytearray(L) if isinstance(L, (bytes, bytearray)) else L, np.uint8)
    if in_use is None:
        in_use = sorted(set(np.unique(L).tolist()))
    in_use = sorted(in_use)
    seq = np.full(256, -1, np.int64)
    seq[in_use] = np.arange(len(in_use))
    s = seq[L]
    assert np.all(s >= 0), "a byte outside in_use"
    # equal neighbours give rank 0 without a look at the MTF list: only the changes walk it
    n = len(s)
    change = np.ones(n, bool)
    change[1:] = s[1:] != s[:-1]
    pos = np.flatnonzero(change)
    lst = list(range(len(in_use)))
    ranks = np.zeros(n, np.int64)
    rk = []
    for v in s[pos].tolist():
        j = lst.index(v)
        if j:
            lst.insert(0, lst.pop(j))
        rk.append(j)
    ranks[pos] = rk
    out = []
    nz = np.flatnonzero(ranks)
    prev = 0
    for p, r in zip(nz.tolist(), ranks[nz].tolist()):
        if p > prev:
            out += zle_digits(p - prev)
        out.append(r + 1)
        prev = p + 1
    if n > prev:
        out += zle_digits(n - prev)
    out.append(len(in_use) + 1)
    return out


def code_lengths(symbols, alpha, limit=17):
    """complete lengths for the symbol frequencies (the oracle's length-limited Huffman, as the encoders use)"""
    from oracle import oracle
    freq = np.bincount(np.asarray(symbols, np.int64), minlength=alpha)[:alpha].tolist()
    return oracle.bzip2_code_lengths(freq, limit)[0]


def block_from_column(L, orig_ptr, in_use=None, n_tables=2, randomised=False, limit=17):
    """a block for a last column (any, BWT or not): lengths built from its symbols, table 0 everywhere"""
    if in_use is None:
        in_use = sorted(set(bytes(L)))
    sym = symbols_from_last_column(L, in_use)
    lens = code_lengths(sym, len(in_use) + 2, limit)
    ng = (len(sym) + G_SIZE - 1) // G_SIZE
    return Block(sym, [lens] * n_tables, [0] * ng, in_use, orig_ptr, randomised=randomised)


def blocks_from_bytes(data, level=9):
    """the blocks an encoder would cut `data` into, each with a true BWT and its CRC"""
    from oracle import oracle
    rle, ends, _, crcs = oracle.rle1_blocks(data, level)
    out, start = [], 0
    for e, crc in zip(ends, crcs):
        blk = rle[start:e]
        start = e
        sa = oracle.bwt(blk)
        sym, freq, orig, n_in_use = oracle.mtf_zle(blk, sa)
        in_use = sorted(set(blk))
        assert len(in_use) == n_in_use
        lens = oracle.bzip2_code_lengths(freq[:n_in_use + 2], 17)[0]
        ng = (len(sym) + G_SIZE - 1) // G_SIZE
        out.append(Block(sym, [lens, lens], [0] * ng, in_use, orig, crc=crc))
    return out


def block_from_bytes(data, level=9):
    b = blocks_from_bytes(data, level)
    assert len(b) == 1
    return b[0]


def lf_map(L):
    """T of the decoder: the stable argsort of L (slot j of the first column -> its row in L)"""
    return np.argsort(np.asarray(bytearray(L), np.uint8), kind="stable")


def cycle_of(T, p):
    """the cycle of T through p, in walk order starting at T[p]"""
    out, q = [], int(T[p])
    out.append(q)
    while q != p:
        q = int(T[q])
        out.append(q)
    return out


def column_from_perm(T, seed=None):
    """the last column whose stable argsort is T, a permutation with at most 256 rising runs: the bucket number
    goes up by one at every descent of T (and, with a seed, at random cuts as well, up to 256 buckets), and the
    buckets are spread over the byte values"""
    T = np.asarray(T, np.int64)
    n = len(T)
    cut = np.zeros(n, bool)
    cut[1:] = T[1:] < T[:-1]
    if seed is not None and n > 1:
        rng = np.random.default_rng(seed)
        free = np.flatnonzero(~cut[1:]) + 1
        extra = 255 - int(cut.sum())
        if extra > 0 and len(free):
            cut[rng.choice(free, min(extra, len(free)), replace=False)] = True
    bucket = np.cumsum(cut)
    k = int(bucket[-1]) + 1 if n else 1
    assert k <= 256, "too many rising runs for one byte alphabet"
    spread = (np.arange(k) * 255) // max(k - 1, 1) if k > 1 else np.array([97])
    L = np.zeros(n, np.uint8)
    L[T] = spread[bucket]
    assert np.array_equal(lf_map(L.tobytes()), T)
    return L.tobytes()


def _one_cycle(m, rng, alpha):
    """T (length m, one cycle) with at most `alpha` rising runs: the LF map of a random primitive word"""
    from oracle import oracle
    if m == 1:
        return np.zeros(1, np.int64)
    while True:
        w = rng.integers(0, max(2, alpha), m, dtype=np.uint8)
        w[0], w[-1] = 0, 1  # two letters at least
        L = np.frombuffer(bytes(w), np.uint8)
        sa = np.array(oracle.bwt(bytes(w)), np.int64)
        Lc = L[(sa - 1) % m]
        T = lf_map(Lc.tobytes())
        if len(cycle_of(T, 0)) == m:
            return T


def last_column_with_cycles(n, spec, seed, alpha=4):
    """(L, orig_ptr): a last column of n bytes that is NOT a BWT in general.  `spec` lists cycle lengths
    (their sum is n); orig_ptr lies on the first one.  Each cycle lives on its own byte range (the LF map of
    a column made of parts over disjoint, rising alphabets is the union of the parts' maps), and the parts
    are laid out in a seeded order.  spec = ("rows", k): one cycle over the rows 1..127 of the slots (slot
    = 128 * row_index + row), with a slot of row 0 put between every k rows and the rest of row 0 a cycle of
    its own -- orig_ptr on the long cycle, whose stretches between slots that are multiples of 128 are k
    rows long.  (n a multiple of 128.)"""
    rng = np.random.default_rng(seed)
    if isinstance(spec, tuple) and spec[0] == "rows":
        return _rows_column(n, spec[1], seed)
    assert sum(spec) == n and len(spec) <= 256
    budget = 256 - len(spec)
    parts = []
    for m in spec:
        a = 1 if m == 1 else min(alpha, 1 + budget // len(spec)) if m > 2 else 2
        parts.append(_one_cycle(m, rng, a))
    order = rng.permutation(len(spec))
    T = np.zeros(n, np.int64)
    base = 0
    where = {}
    for i in order.tolist():
        m = spec[i]
        T[base:base + m] = parts[i] + base
        where[i] = base
        base += m
    orig = where[0] + int(rng.integers(0, spec[0]))
    return column_from_perm(T, seed), orig


def _rows_column(n, k, seed):
    assert n % 128 == 0
    m = n // 128
    D = int(m * 0.618)
    while np.gcd(D, m) != 1:
        D += 1
    j = np.arange(n, dtype=np.int64)
    T = (j + 128 * D) % n  # residue r = slot % 128 is a cycle of m slots: row index i -> i + D (mod m)
    node = lambda r, i: r + 128 * (i % m)
    # residues 1..127 joined into one cycle; after every k-th one, a detour through one slot of residue 0
    detours = []
    for r in range(1, 128):
        nxt = node(r + 1 if r < 127 else 1, 0)
        last = node(r, m - D)  # the slot whose image was node(r, 0)
        if r % k == 0:
            s = node(0, 1 + 2 * len(detours))
            detours.append(s)
            T[last], T[s] = s, nxt
        else:
            T[last] = nxt
    # residue 0 without the detour slots stays one cycle of its own
    rest = [node(0, i * D) for i in range(m)]
    rest = [x for x in rest if x not in set(detours)]
    for a, b in zip(rest, rest[1:] + rest[:1]):
        T[a] = b
    return column_from_perm(T, seed), 1


_RNUMS = []


def rnums():
    """the format's 512 de-randomisation numbers (the table the oracle's C source holds)"""
    if not _RNUMS:
        import os
        import re
        here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        with open(os.path.join(here, "oracle", "bz2_rnums.h")) as f:
            body = f.read().split("{", 1)[1].split("}", 1)[0]
        _RNUMS.extend(int(x) for x in re.findall(r"\d+", body))
        assert len(_RNUMS) == 512
    return _RNUMS


def walk_output(L, orig_ptr, randomised=False):
    """the n bytes the decoder's walk yields (before the RLE1 undo), de-randomised"""
    L = np.frombuffer(bytes(L), np.uint8)
    T = lf_map(bytes(L))
    n = len(L)
    cyc = np.array(cycle_of(T, orig_ptr), np.int64)
    seq = np.resize(cyc, n)
    out = L[seq].copy()
    if randomised:
        q, t = 0, 0
        while True:
            step = rnums()[t]
            t = (t + 1) & 511
            if q + step - 2 >= n:
                break
            out[q + step - 2] ^= 1
            q += step
    return out


def rle1_ends_in_count(out):
    """True when the RLE1 undo of `out` ends right after four equal bytes (the decoder would then read a count
    byte from beyond the block, so a forged block must not end that way)"""
    out = np.asarray(out, np.uint8)
    last, cnt = 0x100, 0
    # only the tail matters, but the state entering it needs the whole prefix: walk the runs with numpy
    n = len(out)
    if n == 0:
        return False
    i = 0
    brk = np.flatnonzero(np.diff(out.astype(np.int16)) != 0) + 1
    starts = np.concatenate([[0], brk]).tolist()
    ends = np.concatenate([brk, [n]]).tolist()
    for s, e in zip(starts, ends):
        i = s
        while i < e:
            if cnt == 4:
                cnt, last = 0, 0x100
                i += 1
                continue
            if out[i] == last:
                take = min(e - i, 4 - cnt)
                cnt += take
                i += take
            else:
                last, cnt = int(out[i]), 1
                i += 1
    return cnt == 4


def fill_crcs(streams, oracle):
    """set every block CRC left None (and every combined CRC left None) from the bytes the oracle decodes for
    the block alone, under a placeholder CRC.  A block the oracle cannot decode keeps CRC 0."""
    single = isinstance(streams, Stream)
    for st in [streams] if single else streams:
        for i, b in enumerate(st.blocks):
            if b.crc is not None:
                continue
            b.crc = 0
            out, status = oracle.decode(write(Stream(st.level, [b])), 256 << 20)
            if status in (0, E_DATA):
                b.crc = oracle.crc32_bzip2(out)
    return streams


# ---------------------------------------------------------------------------- case families
# Shared by tests/test_bzforge.py (the oracle's verdict of every case, on the CPU) and
# tests/test_gpu_decode_forged.py (the GPU against the oracle).  Every case is (name, stream bytes, expected
# status, expected bytes or None = "whatever the oracle says"); everything is drawn from fixed seeds.
class Case:
    def __init__(self, name, z, status, data=None, multi=False, cap=None):
        self.name, self.z, self.status, self.data, self.multi, self.cap = name, z, status, data, multi, cap
        self.images = self.flips = None  # families h and i: the block images, and what is xored into each CRC
        self.no_oracle = False           # True: the oracle has no answer for this stream (see family_h)

    def __repr__(self):
        return "Case(%s, %d bytes, status %d)" % (self.name, len(self.z), self.status)


def _rand_bytes(rng, n, k=256):
    return rng.integers(0, k, n, dtype=np.uint8).tobytes()


def hole_code(lengths):
    """(code, width) of a codeword no symbol owns (the table must be incomplete)"""
    codes = canonical_codes(lengths)
    ml = max(lengths)
    last = max((c << (ml - lengths[s]), s) for s, c in enumerate(codes) if c is not None)
    nxt = ((codes[last[1]] + 1) << (ml - lengths[last[1]]))
    assert nxt < (1 << ml), "the table is complete"
    return nxt, ml


def deep_lengths(alpha, max_len):
    """complete lengths for `alpha` symbols with the deepest levels filled first: most codes are max_len or
    max_len - 1 bits long, a few are short (ascending)"""
    lens = list(range(1, max_len)) + [max_len, max_len]
    assert alpha >= len(lens) and alpha <= (1 << max_len)
    while len(lens) < alpha:
        l = max(x for x in lens if x < max_len)
        lens.remove(l)
        lens += [l + 1, l + 1]
    assert kraft(lens) == 1 << 21
    return sorted(lens)


def assign_by_use(symbols, alpha, lens, rng=None):
    """give the shortest lengths to the least used symbols, so that the long codes carry the block"""
    freq = np.bincount(np.asarray(symbols, np.int64), minlength=alpha)[:alpha]
    key = freq.astype(np.float64) + (rng.random(alpha) * 0.5 if rng is not None else 0)
    order = np.argsort(key, kind="stable")
    out = [0] * alpha
    for s, l in zip(order.tolist(), sorted(lens)):
        out[s] = l
    return out


def with_selectors(b, n_tables, rng, tables=None):
    """one table per group, a different one at every group (seeded); `tables` or b's first table for all"""
    ng = (len(b.symbols) + G_SIZE - 1) // G_SIZE
    sel, prev = [], -1
    for _ in range(ng):
        t = int(rng.integers(0, n_tables - 1))
        t = t + 1 if t >= prev and prev >= 0 else t
        sel.append(t)
        prev = t
    return b.copy(selectors=sel, lengths=tables or [b.lengths[0]] * n_tables)


def _stream(oracle, blocks, level=9):
    st = Stream(level, blocks)
    fill_crcs(st, oracle)
    return write(st)


def family_a(oracle):
    """long and odd codes"""
    rng = np.random.default_rng(101)
    out = []
    # lengths 1, 2, ..., 19, 20, 20 (21 symbols: 19 bytes in use), used uniformly
    d = _rand_bytes(rng, 30000, 19)
    b = block_from_bytes(d)
    lens = [int(x) for x in rng.permutation(list(range(1, 21)) + [20])]
    out.append(Case("A1-1..20", write(Stream(9, [b.copy(lengths=[lens, lens])])), 0, d))
    # dense long codes: max 11, 12, 13, 17, 20 over all 256 bytes; the 17-bit one over 120 000 symbols
    for ml, n in ((11, 20000), (12, 20000), (13, 20000), (17, 120000), (20, 20000)):
        d = _rand_bytes(rng, n)
        b = block_from_bytes(d)
        t1 = assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, ml))
        t2 = assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, ml), rng)
        out.append(Case("A2-max%d" % ml, write(Stream(9, [with_selectors(b, 2, rng, [t1, t2])])), 0, d))
    # lengths 21 and 0 through the delta coding (a step is allowed from 20 and from 1; none from 21 or 0)
    d = _rand_bytes(rng, 20000, 200)
    b = block_from_bytes(d)
    base = assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, 20))
    t21 = list(base)
    t21[-1] = 21  # EOB: 21 bits (the table gets a hole)
    steps = default_length_codes(base[:-1] + [20])[1]
    c21 = (base[0], steps[:-1] + [steps[-1][:-1] + "100"])
    assert lengths_from_codes(c21) == t21
    used = set(b.symbols)
    # a table with its top symbols at length 0 (EOB among them): only groups without EOB and without them use it
    top = [s for s in range(b.alpha - 1, 0, -1)]
    k = 1
    while top[k] not in used and k < 10:
        k += 1
    t0 = deep_lengths(b.alpha - k, 20) + [0] * k
    steps0 = default_length_codes(t0[:b.alpha - k])[1]
    last = t0[b.alpha - k - 1]
    steps0 += [("11" * (last - 1)) + "110"] + ["0"] * (k - 1)
    c0 = (t0[0], steps0)
    assert lengths_from_codes(c0) == t0
    ng = (len(b.symbols) + G_SIZE - 1) // G_SIZE
    owned = [all(t0[s] for s in b.symbols[g * G_SIZE:(g + 1) * G_SIZE]) for g in range(ng)]
    sel = [1 if ok and rng.random() < 0.7 else 0 for ok in owned]
    blk = b.copy(lengths=[t21, t0], selectors=sel, length_codes=[c21, c0])
    out.append(Case("A3-len21-len0", write(Stream(9, [blk])), 0, d))
    # a table of zeros only (start value 0) that no selector picks
    z0 = (0, ["0"] * b.alpha)
    blk = b.copy(lengths=[base, [0] * b.alpha], selectors=[0] * ng, length_codes=[default_length_codes(base), z0])
    out.append(Case("A3-all-zero-table-unused", write(Stream(9, [blk])), 0, d))
    # an incomplete code: used only on owned codewords (valid), then hitting its hole (E_DATA after block 1)
    d0 = _rand_bytes(rng, 5000, 50)
    b0 = block_from_bytes(d0)
    inc = list(base)
    i_long = max(range(b.alpha), key=lambda s: (inc[s], s))
    inc[i_long] += 0 if inc[i_long] == 20 else 1
    if kraft(inc) == 1 << 21:
        j = min(range(b.alpha), key=lambda s: inc[s])
        inc[j] += 1
    assert kraft(inc) < 1 << 21
    blk = b.copy(lengths=[inc, inc])
    out.append(Case("A4-incomplete-owned", write(Stream(9, [b0, blk])), 0, d0 + d, multi=True))
    sym = list(b.symbols)
    sym[len(sym) // 2] = -1  # the hole, in the middle of the block
    blk = b.copy(lengths=[inc, inc], symbols=sym)
    out.append(Case("A4-incomplete-hole", write(Stream(9, [b0, blk])), E_DATA, d0, multi=True))
    # over-subscribed: a table that is used, and the same table as a second one no selector picks
    over = list(base)
    j = max(range(b.alpha), key=lambda s: (over[s], -s))
    over[j] -= 1
    assert kraft(over) > 1 << 21
    out.append(Case("A5-oversubscribed-used", write(Stream(9, [b0, b.copy(lengths=[over, base])])), E_DATA, d0, multi=True))
    out.append(Case("A5-oversubscribed-unpicked", write(Stream(9, [b0, b.copy(lengths=[base, over])])), E_DATA, d0,
                    multi=True))
    return out


def _eob_start(b, level=9):
    """bit offset of EOB's code inside a one-block stream of b"""
    w = _Bits()
    w.put(0, 32)
    _write_block(w, b.copy(symbols=b.symbols[:-1]))
    return w.nbits()


def family_b(oracle):
    """truncation inside the EOB code: EOB codes of 9-20 bits with zero tails, at all 8 bit alignments, in tables
    whose max_len is at most 12 and above 12; every byte cut that falls inside EOB"""
    rng = np.random.default_rng(202)
    out = []
    d = _rand_bytes(rng, 3000, 40)
    b = block_from_bytes(d)
    base = oracle.bzip2_code_lengths(np.bincount(b.symbols, minlength=b.alpha).tolist(), 8)[0]
    eob = b.alpha - 1
    for lb in (9, 10, 11, 12, 13, 20):
        for high in (False, True):
            if high and lb >= 13:
                continue  # (max_len is above 12 already)
            t = list(base)
            t[eob] = lb
            if high:  # one rare data symbol at 14 bits: max_len 14, EOB still alone at its length
                x = min((s for s in range(1, eob)), key=lambda s: (b.symbols.count(s), s))
                t[x] = 14
            assert kraft(t) <= 1 << 21
            code = canonical_codes(t)[eob]
            tz = (code & -code).bit_length() - 1 if code else lb
            assert tz >= 1, "EOB without a zero tail"
            for pad in range(8):
                blk = b.copy(lengths=[t, t])
                e0 = _eob_start(blk)
                extra = (pad - e0) % 8
                blk = blk.copy(selectors=blk.selectors + [blk.selectors[-1]] * extra)
                e = _eob_start(blk)
                assert e % 8 == pad
                st = Stream(9, [blk])
                fill_crcs(st, oracle)
                z = write(st)
                for cut in range(e // 8, (e + lb + 7) // 8):
                    missing = e + lb - 8 * cut
                    if missing <= 0 or cut * 8 <= e:
                        ok = False
                    else:
                        ok = missing <= tz and lb <= 12
                    out.append(Case("B-eob%d-%s-al%d-cut%d" % (lb, "max14" if high else "max%d" % lb, pad, cut),
                                    z[:cut], E_DATA, d if ok else b""))
    # the last 12 bytes of a normal multi-block stream
    d = _rand_bytes(rng, 250000, 30)
    import bz2
    z = bz2.compress(d, 1)
    for cut in range(len(z) - 12, len(z)):
        out.append(Case("B-tail-cut%d" % (len(z) - cut), z[:cut], E_DATA, None, multi=True))
    return out


def _eob_at(data_fn, pos, rng, tries=200):
    """a block (true BWT) whose EOB sits at position `pos` of its 50-symbol group"""
    for k in range(tries):
        d = data_fn(k)
        b = block_from_bytes(d)
        if (len(b.symbols) - 1) % G_SIZE == pos:
            return d, b
    raise AssertionError("no block with EOB at %d" % pos)


def family_c(oracle):
    """selectors and groups: 2-6 tables that change every group, over 600 groups; n_selectors as needed, more
    (up to 32767) and one too few; EOB at group positions 0, 1, 48, 49"""
    rng = np.random.default_rng(303)
    out = []
    base_d = _rand_bytes(rng, 36000, 120)
    for nt in (2, 3, 4, 5, 6):
        d = base_d[:34000 + 400 * nt]
        b = block_from_bytes(d)
        tabs = [assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, 9 + 2 * t), rng) for t in range(nt)]
        blk = with_selectors(b, nt, rng, tabs)
        assert len(blk.selectors) > 600
        out.append(Case("C-tables%d" % nt, write(Stream(9, [blk])), 0, d))
        if nt in (2, 6):
            more = blk.copy(selectors=blk.selectors + [int(x) for x in rng.integers(0, nt, 32767 - len(blk.selectors))])
            out.append(Case("C-tables%d-nsel32767" % nt, write(Stream(9, [more])), 0, d))
            more = blk.copy(selectors=blk.selectors + [int(x) for x in rng.integers(0, nt, 300)])
            out.append(Case("C-tables%d-nsel+300" % nt, write(Stream(9, [more])), 0, d))
            few = blk.copy(n_selectors=len(blk.selectors) - 1)
            d0 = base_d[:777]
            out.append(Case("C-tables%d-nsel-1" % nt, write(Stream(9, [block_from_bytes(d0), few])), E_DATA, d0,
                            multi=True))
    for pos in (0, 1, 48, 49):
        d, b = _eob_at(lambda k: base_d[:20000 + 3 * k + pos * 7], pos, rng)
        tabs = [assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, 12), rng) for _ in range(3)]
        out.append(Case("C-eob-at-%d" % pos, write(Stream(9, [with_selectors(b, 3, rng, tabs)])), 0, d))
    return out


def symbols_of(items, n_in_use):
    """symbols from ("lit", rank) / ("run", length) items, with EOB"""
    out = []
    for kind, v in items:
        out += zle_digits(v) if kind == "run" else [v + 1]
    return out + [n_in_use + 1]


def _plain_block(sym, n_in_use, orig_ptr=0, **kw):
    in_use = list(range(97, 97 + n_in_use))
    lens = code_lengths(sym, n_in_use + 2, 17)
    return Block(sym, [lens, lens], [0] * ((len(sym) + G_SIZE - 1) // G_SIZE), in_use, orig_ptr, **kw)


def family_d(oracle):
    """zero runs: digits across symbol 512k, runs ending at nblock_max - 1 / nblock_max, a literal ending at
    nblock_max, 19-21 digits, a run right before EOB"""
    rng = np.random.default_rng(404)
    out = []
    K = 20
    lit = lambda: ("lit", int(rng.integers(1, K)))
    # level 1: runs whose digits straddle symbols 512 k (k = 1..), literals in between
    items, nsym, ntt = [], 0, 0
    k = 1
    while ntt < 95000:
        run = int(rng.integers(3, 1 << int(rng.integers(3, 11))))
        nd = len(zle_digits(run))
        start = 512 * k - int(rng.integers(1, nd)) if nd > 1 else 512 * k
        while nsym < start:
            items.append(lit())
            nsym += 1
            ntt += 1
        if ntt + run > 99000:
            break
        items.append(("run", run))
        nsym += nd
        ntt += run
        items.append(lit())
        nsym += 1
        ntt += 1
        k += 1
    blk = _plain_block(symbols_of(items, K), K, orig_ptr=int(rng.integers(0, ntt)))
    out.append(Case("D-straddle-512k", _stream(oracle, [blk], 1), 0))
    # the end of a level-1 block: tt length after a run = 99 999 (valid) / 100 000 (error); a literal at 100 000
    head = [lit() for _ in range(60000)]
    for name, tail, status in (("run-to-nmax-1", [("run", 40000 - 1)], 0), ("run-to-nmax", [("run", 40000)], E_DATA),
                               ("lit-to-nmax", [("run", 39999), lit()], 0),
                               ("lit-past-nmax", [("run", 40000), lit()], E_DATA)):
        first = _plain_block(symbols_of([lit() for _ in range(3000)], K), K, orig_ptr=5)
        blk = _plain_block(symbols_of(head + tail, K), K, orig_ptr=12345)
        out.append(Case("D-" + name, _stream(oracle, [first, blk], 1), status, multi=True))
    # digit counts: 19 (valid at level 9), 20 and 21 (the run overflows any block)
    for nd, status in ((19, 0), (20, E_DATA), (21, E_DATA)):
        run = (1 << nd) - 1  # nd RUNA digits
        first = _plain_block(symbols_of([lit() for _ in range(2000)], K), K, orig_ptr=7)
        blk = _plain_block(symbols_of([lit() for _ in range(300)] + [("run", run), lit()], K), K, orig_ptr=100)
        out.append(Case("D-digits%d" % nd, _stream(oracle, [first, blk], 9), status, multi=True, cap=64 << 20))
    # a run directly before EOB, inside a level-9 block
    blk = _plain_block(symbols_of([lit() for _ in range(5000)] + [("run", 777)], K), K, orig_ptr=4000)
    out.append(Case("D-run-before-eob", _stream(oracle, [blk], 9), 0))
    return out


def _column_case(oracle, name, L, orig, randomised=False, level=9, status=0):
    b = block_from_column(L, orig, randomised=randomised)
    if status == 0 and rle1_ends_in_count(walk_output(L, orig, randomised)):
        return None  # (the walk would end inside a 4-byte run: the decoder reads a count from beyond the block)
    return Case(name, _stream(oracle, [b], level), status, cap=256 << 20)


def _fill(spec, n):
    return spec + [n - sum(spec)]


def family_e(oracle):
    """last columns that are not a BWT: orig_ptr on a fixed point, a 2-cycle, a cycle of n/2, a long cycle with
    few sample slots (stretches of 8 and of 10 rows of 7031 slots between them: above kSegCap, the second above
    0xFFFF), mixed cycle lengths; each also with the randomisation bit set.  CRCs filled: status 0."""
    out = []
    specs = [
        ("n1-fixed", 1, [1]), ("n2-2cycle", 2, [2]), ("n3-fixed", 3, [1, 2]), ("n129-2cycle", 129, [2, 127]),
        ("n1000-fixed", 1000, [1, 999]), ("n4096-half", 4096, [2048, 2048]), ("n70000-2cycle", 70000, [2, 69998]),
        ("n300001-fixed", 300001, [1, 150000, 150000]), ("n900000-half", 900000, [450000, 450000]),
        ("n900000-2cycle", 900000, [2, 899998]), ("n900000-fixed", 900000, [1, 1, 899998]),
        ("n899968-rows8", 899968, ("rows", 8)), ("n899968-rows10", 899968, ("rows", 10)),
        ("n65536-rows2", 65536, ("rows", 2)),
        ("n500000-mixed", 500000, _fill([123457, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597,
                                         2584, 4181, 6765, 10946, 17711, 28657, 46368, 75025], 500000)),
        ("n100000-mixed-small", 100000, _fill([7] + [3] * 100 + [2] * 100 + [1] * 40, 100000)),
    ]
    for i, (name, n, spec) in enumerate(specs):
        for rnd in (False, True):
            for attempt in range(4):  # (a walk that ends inside a run: one slot less on the last cycle)
                m = n - attempt
                sp = spec if isinstance(spec, tuple) or attempt == 0 else spec[:-1] + [spec[-1] - attempt]
                if isinstance(sp, tuple) and attempt:
                    break
                L, orig = last_column_with_cycles(m, sp, 500 + i)
                if not isinstance(sp, tuple):
                    assert len(cycle_of(lf_map(L), orig)) == sp[0], name
                c = _column_case(oracle, "E-%s%s" % (name, "-rand" if rnd else ""), L, orig, rnd)
                if c is not None:
                    out.append(c)
                    break
            assert c is not None, name
    return out


def family_f(oracle):
    """header edges: orig_ptr at 0, n-1, n, 10 + 100000 * level and one above; alphabets of 3 and 258; a flagged
    but empty 16-bit group; in-use bytes that never occur; level 1 against 100 000 and 100 001 bytes"""
    rng = np.random.default_rng(606)
    out = []
    n = 5000
    L = _rand_bytes(rng, n, 256)
    L = bytes(np.frombuffer(L, np.uint8) | 1)
    for name, op, status in (("orig0", 0, 0), ("orig-n-1", n - 1, 0), ("orig-n", n, E_DATA),
                             ("orig-10+900000", 10 + 900000, E_DATA), ("orig-10+900001", 10 + 900001, E_DATA)):
        b = block_from_column(L, op)
        if status == 0 and rle1_ends_in_count(walk_output(L, op)):
            b.orig_ptr = op = 1
        first = _plain_block(symbols_of([("lit", 1 + i % 5) for i in range(400)], 6), 6, orig_ptr=3)
        out.append(Case("F-" + name, _stream(oracle, [first, b]), status, multi=True))
    out.append(Case("F-alpha3", _stream(oracle, [block_from_column(bytes([200, 200, 200]), 1)]), 0))
    L256 = bytes(rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), 40)))
    out.append(Case("F-alpha258", _stream(oracle, [block_from_column(L256, 77)]), 0))
    out.append(Case("F-alpha258-bwt", write(Stream(9, [block_from_bytes(L256)])), 0, bytes(L256)))
    d = bytes(rng.choice(np.frombuffer(b"abcdefgh", np.uint8), 8000))
    bb = block_from_bytes(d)
    g16 = sum(1 << (15 - i) for i in range(16) if any(16 * i <= v < 16 * i + 16 for v in bb.in_use))
    out.append(Case("F-empty-group16", write(Stream(9, [bb.copy(groups16=g16 | (1 << 15) | 1)])), 0, d))
    extra = sorted(set(bb.in_use) | {0, 17, 98 + 128, 255})
    L = np.frombuffer(bytes(rng.choice(np.frombuffer(b"abcdefgh", np.uint8), 6000)), np.uint8)
    out.append(Case("F-unused-in-use", _stream(oracle, [block_from_column(L.tobytes(), 11, in_use=extra)]), 0))
    for name, n, status in (("level1-100000", 100000, 0), ("level1-100001", 100001, E_DATA)):
        L = rng.integers(0, 256, n, dtype=np.uint8)
        L[-1], L[-2] = 3, 4  # a literal at the end (a run there would fail one byte earlier)
        b = block_from_column(L.tobytes(), 0)
        out.append(Case("F-" + name, _stream(oracle, [b], 1), status, cap=64 << 20))
    return out


def family_g(oracle):
    """mixtures: one stream of 300 small blocks drawn from the families' kinds, valid CRCs; three streams"""
    rng = np.random.default_rng(707)
    blocks = []
    for i in range(300):
        kind = i % 6
        if kind == 0:  # long codes over a true BWT
            d = _rand_bytes(rng, int(rng.integers(300, 3000)))
            b = block_from_bytes(d)
            ml = int(rng.integers(11, 21))
            t = assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, ml), rng)
            b = b.copy(lengths=[t, t])
        elif kind == 1:  # several tables, changing every group
            d = _rand_bytes(rng, int(rng.integers(1000, 4000)), int(rng.integers(2, 60)))
            b = block_from_bytes(d)
            nt = int(rng.integers(2, 7))
            b = with_selectors(b, nt, rng, [assign_by_use(b.symbols, b.alpha, deep_lengths(b.alpha, min(15, b.alpha - 1)), rng)
                                            for _ in range(nt)])
        elif kind == 2:  # zero runs
            K = 10
            items = []
            for _ in range(int(rng.integers(5, 40))):
                items += [("lit", int(rng.integers(1, K))) for _ in range(int(rng.integers(1, 20)))]
                items.append(("run", int(rng.integers(1, 300))))
            items.append(("lit", 3))
            b = _plain_block(symbols_of(items, K), K, orig_ptr=0)
        elif kind == 3:  # a column that is not a BWT, cycles of mixed length, sometimes randomised
            n = int(rng.integers(10, 5000))
            a = int(rng.integers(1, n // 3 + 1))
            L, op = last_column_with_cycles(n, [a, n - a], int(rng.integers(1 << 30)))
            rnd = bool(rng.integers(0, 2))
            if rle1_ends_in_count(walk_output(L, op, rnd)):
                continue
            b = block_from_column(L, op, randomised=rnd)
        elif kind == 4:  # tiny alphabets and header edges
            n = int(rng.integers(1, 300))
            L = rng.integers(0, int(rng.integers(1, 4)), n, dtype=np.uint8) + 40
            op = int(rng.integers(0, n))
            if rle1_ends_in_count(walk_output(L.tobytes(), op)):
                continue
            b = block_from_column(L.tobytes(), op)
        else:  # plain data, more selectors than needed
            d = _rand_bytes(rng, int(rng.integers(1, 2000)), 256)
            b = block_from_bytes(d)
            b = b.copy(selectors=b.selectors + [0] * int(rng.integers(0, 100)))
        got, status = oracle.decode(write(Stream(9, [b.copy(crc=0)])), 1 << 20)
        if status in (0, E_DATA):  # (not a walk that ends inside a run, not a block that expands past 1 MB)
            blocks.append(b.copy(crc=oracle.crc32_bzip2(got)))
    assert len(blocks) > 250
    big = write(Stream(9, blocks))
    out = [Case("G-300-blocks", big, 0, multi=True, cap=64 << 20)]
    s2 = Stream(1, [_plain_block(symbols_of([("lit", 1), ("run", 5)] * 100, 4), 4, orig_ptr=9)])
    fill_crcs(s2, oracle)
    three = write([parse(big)[0], s2, Stream(5, blocks_from_bytes(_rand_bytes(rng, 30000, 7), 5))])
    out.append(Case("G-three-streams", three, 0, multi=True, cap=64 << 20))
    return out


# ---------------------------------------------------------------------------- families h and i: stage D4
# The last decode stage (the RLE1 undo and the block CRC) is fed IMAGES: what the walk yields, chosen byte by byte,
# wrapped into a block with the image's true BWT.  The expected bytes are rle1_undo's, never a decoder's.
#
# The tiling of the stage, each constant where rust-compression_amd/csrc/k_dec.hip has it:
SUB = 64              # k_dec_rle_sub: image bytes per sub-tile (`p = sub * 64u`)
WAVE = 64 * SUB       # k_dec_rle_expand: one lane per sub-tile, 64 sub-tiles (4 096 image bytes) per wave
GROUP = 4 * WAVE      # k_dec_rle_expand: four waves (16 384 image bytes) per workgroup (`blockIdx.x * 4u + w`)
CHAIN = 1024          # k_dec_rle_chain: threads per block; each folds K = ceil(nsub / 1024) sub-tiles
EXP_STAGE = 8192      # kExpStage: a wave stages its output in LDS when total + shift <= 8192
PIECE = 16            # k_dec_crc: bytes per piece, aligned in memory
TILE_PIECES = 256     # k_dec_crc: pieces per tile (one per thread)
SLICE_PIECES = 4096   # k_dec_crc: pieces per workgroup (16 tiles)
NO_COUNT = -100       # the oracle's answer to a block that ends behind four equal bytes, at any capacity


def share_k(n):
    """sub-tiles per thread of k_dec_rle_chain for an image of n bytes"""
    nsub = (n + SUB - 1) // SUB
    return (nsub + CHAIN - 1) // CHAIN


def rle1_parse(image):
    """(image as uint8 array, mask of the bytes that are counts, True when the image ends behind four equal bytes
    with no count).  The state machine of decoder.rs:555-577, run by run: inside a run of equal bytes that starts
    fresh every fifth byte is a count, and a run of 5 k + 4 bytes takes the byte behind it as its count."""
    x = np.frombuffer(bytes(image), np.uint8)
    n = len(x)
    is_count = np.zeros(n, bool)
    if n == 0:
        return x, is_count, False
    brk = np.flatnonzero(x[1:] != x[:-1]) + 1
    starts = np.concatenate([[0], brk])
    ends = np.concatenate([brk, [n]])
    long_ = ends - starts >= 4  # (a run whose first byte was eaten as a count only gets shorter)
    eaten, pending = -1, False
    for s, e in zip(starts[long_].tolist(), ends[long_].tolist()):
        if s == eaten:
            s += 1
        if e - s < 4:
            continue
        is_count[s + 4:e:5] = True
        if (e - s) % 5 == 4:
            if e < n:
                is_count[e] = True
                eaten = e
            else:
                pending = True
    return x, is_count, pending


def rle1_undo(image):
    """(bytes, ends_in_count): the plain RLE1 undo of an image; ends_in_count is True when the image ends behind
    four equal bytes (the count is missing: the bytes are then those in front of it)"""
    x, is_count, pending = rle1_parse(image)
    reps = np.where(is_count, x, 1).astype(np.int64)
    vals = x.copy()
    idx = np.flatnonzero(is_count)
    vals[idx] = x[idx - 1]
    return np.repeat(vals, reps).tobytes(), pending


def rle1_states(x, is_count):
    """per image byte: the entering state in the kernel's terms (0 fresh, 1..3 that many equal bytes in front,
    4 this byte is a count)"""
    n = len(x)
    fresh = np.ones(n, bool)
    fresh[1:] = ((x[1:] != x[:-1]) & ~is_count[1:]) | is_count[:-1]
    start = np.maximum.accumulate(np.where(fresh, np.arange(n), 0))
    e = (np.arange(n) - start) % 5
    assert np.array_equal(e == 4, is_count)
    return e


def block_from_image(image, crc=None, flip=0):
    """a block whose walk yields `image`: its true BWT, as blocks_from_bytes makes it, without the RLE1 encoder in
    front.  The CRC is that of rle1_undo(image) (`flip` is xored into it)."""
    from oracle import oracle
    image = bytes(image)
    sa = oracle.bwt(image)
    sym, freq, orig, n_in_use = oracle.mtf_zle(image, sa)
    in_use = sorted(set(image))
    assert len(in_use) == n_in_use
    lens = oracle.bzip2_code_lengths(freq[:n_in_use + 2], 17)[0]
    if crc is None:
        crc = oracle.crc32_bzip2(rle1_undo(image)[0])
    return Block(sym, [lens, lens], [0] * ((len(sym) + G_SIZE - 1) // G_SIZE), in_use, orig, crc=crc ^ flip)


# ---- a model of the three-step undo and of the CRC geometry, for the mutants of tests/test_bzforge.py ----------
RLE_MUTANTS = ("exit ignores nxt", "exit for cnt==4 dropped", "e=4 run byte from X[p]",
               "count equal to run byte extends the run", "K share rounded down", "staging test uses <",
               "flush drops tail bytes", "flush drops head bytes")
CRC_MUTANTS = ("leading lo bytes not zeroed", "ragged branch for a full last piece", "last-tile cover ends at piece edge",
               "initial value uses R")
FILL = 0xA5  # what the model's output memory holds where nothing was written


def _rle_steps(X, n, last, cnt, mut, emit):
    """64 steps of the state machine over the rows of X (sub-tiles) for any number of state columns; returns
    (out sizes, last, cnt) and, with emit, the per-byte (repeat, value) arrays of column 0"""
    nsub = X.shape[0]
    p0 = np.arange(nsub) * SUB
    out = np.zeros(last.shape, np.int64)
    reps = np.zeros((nsub, SUB), np.int64)
    vals = np.zeros((nsub, SUB), np.uint8)
    for k in range(SUB):
        valid = (p0 + k < n)[:, None]
        b = X[:, k].astype(np.int64)[:, None]
        is4 = cnt == 4
        if mut == "count equal to run byte extends the run":
            is4 = is4 & (b != last)
            lit_at_4 = (cnt == 4) & (b == last)
        eq = (b == last) & ~is4
        if emit:
            reps[:, k] = np.where(valid, np.where(is4, b, 1), 0)[:, 0]
            vals[:, k] = np.where(is4, last, b)[:, 0].astype(np.uint8)
        out += np.where(valid, np.where(is4, b, 1), 0)
        nl = np.where(is4, 0x100, np.where(eq, last, b))
        nc = np.where(is4, 0, np.where(eq, cnt + 1, 1))
        if mut == "count equal to run byte extends the run":
            nc = np.where(lit_at_4, 4, nc)
        last = np.where(valid, nl, last)
        cnt = np.where(valid, nc, cnt)
    return out, last, cnt, reps, vals


def tiled_undo(image, phase=0, mut=None):
    """(bytes, None | NO_COUNT, per wave True = staged): the undo as stage D4 tiles it -- tabulate every sub-tile
    for five entering states, compose along the block in 1024 shares, replay every sub-tile, flush staged waves as
    dwords and end bytes.  `phase` is the address of the block's first output byte mod 4; `mut` one of
    RLE_MUTANTS.  Memory nothing writes holds FILL."""
    x = np.frombuffer(bytes(image), np.uint8)
    n = len(x)
    nsub = (n + SUB - 1) // SUB
    xp = np.concatenate([x, np.zeros(nsub * SUB + 1 - n, np.uint8)])
    X = xp[:nsub * SUB].reshape(nsub, SUB)
    p0 = np.arange(nsub) * SUB
    # tabulate (k_dec_rle_sub)
    b0 = X[:, 0].astype(np.int64)
    last = np.stack([np.full(nsub, 0x100), b0, b0, b0, np.full(nsub, 0x100)], 1)
    cnt = np.tile(np.arange(5), (nsub, 1))
    t_out, last, cnt, _, _ = _rle_steps(X, n, last, cnt, mut, False)
    nxt = np.where(p0 + SUB < n, xp[np.minimum(p0 + SUB, len(xp) - 1)].astype(np.int64), 0x200)[:, None]
    if mut == "exit ignores nxt":
        t_ex = np.where(cnt == 4, 4, cnt)
    elif mut == "exit for cnt==4 dropped":
        t_ex = np.where(last == nxt, cnt, 0)
    else:
        t_ex = np.where(cnt == 4, 4, np.where(last == nxt, cnt, 0))
    t_ex = np.minimum(t_ex, 4)
    # compose (k_dec_rle_chain): every thread folds its share for the five states, thread 0 links them
    K = nsub // CHAIN if mut == "K share rounded down" else (nsub + CHAIN - 1) // CHAIN
    j = np.arange(CHAIN)
    s0 = j * K
    s1 = np.minimum(s0 + K, nsub)
    e = np.tile(np.arange(5), (CHAIN, 1))
    off = np.zeros((CHAIN, 5), np.int64)
    for t in range(K):
        s = s0 + t
        ok = (s < s1)[:, None]
        sc = np.minimum(s, nsub - 1)[:, None]
        off = off + np.where(ok, t_out[sc, e], 0)
        e = np.where(ok, t_ex[sc, e], e)
    in_e = np.zeros(CHAIN, np.int64)
    in_off = np.zeros(CHAIN, np.int64)
    ce, co = 0, 0
    for t in range(CHAIN):
        in_e[t], in_off[t] = ce, co
        co += int(off[t, ce])
        ce = int(e[t, ce])
    out_len = co
    if ce == 4:
        return b"", NO_COUNT, []
    sub_e = np.zeros(nsub, np.int64)
    soff = np.zeros(nsub + 1, np.int64)
    soff[nsub] = out_len
    ce, co = in_e.copy(), in_off.copy()
    for t in range(K):
        s = s0 + t
        ok = s < s1
        sc = np.minimum(s, nsub - 1)
        sub_e[sc[ok]] = ce[ok]
        soff[sc[ok]] = co[ok]
        co = co + np.where(ok, t_out[sc, ce], 0)
        ce = np.where(ok, t_ex[sc, ce], ce)
    # replay (k_dec_rle_expand), 64 waves at a time
    out = np.full(out_len + 8, FILL, np.uint8)
    staged_log = []
    prev = np.concatenate([[0], xp[p0[1:] - 1]]).astype(np.int64) if nsub > 1 else np.zeros(1, np.int64)
    run4 = b0 if mut == "e=4 run byte from X[p]" else prev
    r_last = np.where(sub_e == 0, 0x100, np.where(sub_e == 4, run4, b0))[:, None]
    r_cnt = sub_e[:, None]
    step = 64 * 64
    for c0 in range(0, nsub, step):
        c1 = min(c0 + step, nsub)
        _, _, _, reps, vals = _rle_steps(X[c0:c1], n - c0 * SUB, r_last[c0:c1], r_cnt[c0:c1], mut, True)
        o_in = np.cumsum(reps, 1) - reps
        subs = np.arange(c0, c1)
        wave0 = (subs // 64) * 64
        base = soff[wave0]
        total = soff[np.minimum(wave0 + 64, nsub)] - base
        shift = (phase + base) & 3
        lim = EXP_STAGE - 1 if mut == "staging test uses <" else EXP_STAGE
        staged = total + shift <= lim
        staged_log += staged[::64].tolist()
        # position of every emitted byte inside its wave's output, then its fate
        keep = reps.ravel() > 0
        rp = reps.ravel()[keep]
        w_pos = np.repeat((soff[subs][:, None] - base[:, None] + o_in).ravel()[keep], rp)
        w_pos = w_pos + (np.arange(len(w_pos)) - np.repeat(np.cumsum(rp) - rp, rp))
        rows = np.repeat(np.repeat(np.arange(c1 - c0), SUB)[keep], rp)
        v = np.repeat(vals.ravel()[keep], rp)
        st, sh, tot, bs = staged[rows], shift[rows], total[rows], base[rows]
        sp = w_pos + sh  # byte index in the staging buffer
        first, lastb = sh, sh + tot
        dw0, dw1 = (first + 3) // 4, lastb // 4
        ok = np.ones(len(v), bool)
        ok &= ~st | ((sp < EXP_STAGE + 8) & (sp < lastb))  # (the flush copies [first, lastb) only)
        if mut == "flush drops tail bytes":
            ok &= ~(st & (dw0 <= dw1) & (sp >= dw1 * 4))
        if mut == "flush drops head bytes":
            ok &= ~(st & (dw0 <= dw1) & (sp < dw0 * 4))
        d = bs + w_pos
        ok &= (d >= 0) & (d < len(out))
        out[d[ok]] = v[ok]
    return out[:out_len].tobytes(), None, staged_log


_CRC_TAB = []


def _crc_tab():
    if not _CRC_TAB:
        t = []
        for i in range(256):
            c = i << 24
            for _ in range(8):
                c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
            t.append(c)
        _CRC_TAB.append(np.array(t, np.uint64))
    return _CRC_TAB[0]


def _gf_mul(a, b):
    """a * b in GF(2)[x] / 0x104C11DB7 (numpy uint64 arrays or ints that hold 32 bits)"""
    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    r = np.zeros(np.broadcast(a, b).shape, np.uint64)
    M = np.uint64(0xFFFFFFFF)
    for i in range(31, -1, -1):
        r = ((r << np.uint64(1)) & M) ^ np.where(r & np.uint64(0x80000000), np.uint64(0x04C11DB7), np.uint64(0))
        r = r ^ np.where((b >> np.uint64(i)) & np.uint64(1), a, np.uint64(0))
    return r


_XP = {}


def _xpow_bytes(nbytes):
    """x^(8 nbytes) mod P; nbytes is taken mod 2^64 as the kernel's u64 would be"""
    if not _XP:
        xp2 = [0x100]
        for _ in range(63):
            xp2.append(int(_gf_mul(xp2[-1], xp2[-1])))
        xp16 = [1]
        for _ in range(255):
            xp16.append(int(_gf_mul(xp16[-1], xp2[4])))
        _XP["xp2"], _XP["xp16"] = xp2, np.array(xp16, np.uint64)
    nbytes &= (1 << 64) - 1
    r, k = 1, 0
    while nbytes:
        if nbytes & 1:
            r = int(_gf_mul(r, _XP["xp2"][k]))
        nbytes >>= 1
        k += 1
    return r


def crc_model(mem, A, ln, mut=None):
    """the CRC of mem[A:A + ln] as k_dec_crc folds it: aligned 16-byte pieces from (A & ~15) on, 256-piece tiles,
    4096-piece slices.  `mem` is a uint8 array whose index 0 stands at a 16-byte aligned address and which has 16
    spare bytes at its end; `mut` one of CRC_MUTANTS."""
    tab = _crc_tab()
    _xpow_bytes(0)
    xp16 = _XP["xp16"]
    a0 = A & ~15
    R = A - a0 + ln
    npieces = (R + 15) // 16
    total = 0
    for sl in range(max(1, (npieces + SLICE_PIECES - 1) // SLICE_PIECES)):
        p0 = sl * SLICE_PIECES
        s_tile = []
        for tile in range(16):
            i = p0 + tile * TILE_PIECES + np.arange(TILE_PIECES, dtype=np.int64)
            i = i[i < npieces]
            if not len(i):
                s_tile.append(0)
                continue
            by = mem[a0 + i[0] * 16:a0 + (i[-1] + 1) * 16].reshape(len(i), 16).astype(np.uint64)
            pbeg = i * 16
            pend = np.minimum(pbeg + 16, R)
            lo = np.where(i == 0, 0 if mut == "leading lo bytes not zeroed" else A - a0, 0)
            hi = pend - pbeg
            c = np.zeros(len(i), np.uint64)
            for k in range(16):
                b = np.where(k >= lo, by[:, k], np.uint64(0))
                nc = tab[((c >> np.uint64(24)) ^ b).astype(np.int64)] ^ ((c << np.uint64(8)) & np.uint64(0xFFFFFFFF))
                c = np.where(k < hi, nc, c)
            last = min(p0 + tile * TILE_PIECES + TILE_PIECES - 1, npieces - 1)
            if last == npieces - 1 and ((R & 15) or mut == "ragged branch for a full last piece"):
                c2 = _gf_mul(_gf_mul(c, xp16[np.clip(last - 1 - i, 0, 255)]), _xpow_bytes(R & 15))
            else:
                c2 = _gf_mul(c, xp16[last - i])
            c = np.where(pend == R, c, c2)
            s_tile.append(int(np.bitwise_xor.reduce(c)))
        acc, end_piece = 0, 0
        for tile in range(16):
            first = p0 + tile * TILE_PIECES
            if first >= npieces:
                break
            lastp = min(first + TILE_PIECES - 1, npieces - 1)
            cover_end = R if lastp == npieces - 1 and mut != "last-tile cover ends at piece edge" else (lastp + 1) * 16
            acc = int(_gf_mul(acc, _xpow_bytes(cover_end - first * 16))) ^ s_tile[tile]
            end_piece = cover_end
        if npieces:
            acc = int(_gf_mul(acc, _xpow_bytes(R - end_piece)))
        if sl == 0:
            acc ^= int(_gf_mul(0xFFFFFFFF, _xpow_bytes(R if mut == "initial value uses R" else ln)))
        total ^= acc
    return total ^ 0xFFFFFFFF


# ---- targets ----------------------------------------------------------------------------------------------------------
H_EDGES = ("sub", "wave", "group", "share2", "share14")
H_COUNTS = (0, 1, 3, 4, 251, 252, 255)
H_SELF_V = (0, 1, 4, 5, 255)
H_SELF_N = tuple(n for n in list(range(1, 12)) + [63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385, 70001]
                 if n % 5 != 4)  # (n = 5 k + 4 ends behind four equal bytes: no count)
I_PIECES = (1, 2, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)


def _required_h():
    r = set()
    for edge in H_EDGES:
        r |= {"H edge=%s e=0" % edge, "H edge=%s e=4" % edge}
        for e in (1, 2, 3):
            r |= {"H edge=%s e=%d goes on" % (edge, e), "H edge=%s e=%d breaks" % (edge, e)}
    for at in ("", " at sub edge"):
        r |= {"H count=%d%s" % (c, at) for c in H_COUNTS}
        r |= {"H count==run byte" + at, "H byte after count equals run byte" + at}
    r |= {"H self v=%d n=%d" % (v, n) for v in H_SELF_V for n in H_SELF_N}
    r |= {"H period5 n<64", "H period5 n>=4096", "H sub out>=3300"}
    r |= {"H end n%64=0", "H end n%64=1", "H end n%64=63", "H end n=1", "H end count=0", "H end count=255",
          "H end equal=1", "H end equal=2", "H end equal=3"}
    r |= {"H stage total+shift=%d shift=%d" % (t, s) for t in (8191, 8192, 8193) for s in range(4)}
    r |= {"H seam %s shift=%d" % (k, s) for k in ("staged|direct", "direct|staged") for s in range(4)}
    r |= {"H total<4 shift=%d" % s for s in (1, 2, 3)}
    # the one-dword branch of the flush (dw0 > dw1) needs shift + total < 4: shift 3 never takes it
    r |= {"H one-dword flush shift=1", "H one-dword flush shift=2"}
    r |= {"H no count only", "H no count middle", "H no count last"}
    return r


def _required_i():
    r = {"I a=%d r=%d" % (a, q) for a in range(16) for q in range(16)}
    r |= {"I pieces=%d last=%s a=%d" % (p, l, a) for p in I_PIECES for l in ("full", "ragged") for a in (0, 1, 15)}
    r.discard("I pieces=1 last=ragged a=15")  # (R = 15 + len >= 16: one piece behind 15 bytes is a full one)
    r |= {"I wrong crc pieces=1", "I wrong crc ragged tile seam", "I wrong crc slice seam"}
    return r


REQUIRED = {"h": _required_h(), "i": _required_i()}


def _hits_h_image(image, phase):
    """targets one block's image reaches, its first output byte at an address = phase (mod 4)"""
    h = set()
    x, is_count, pending = rle1_parse(image)
    n = len(x)
    e = rle1_states(x, is_count)
    reps = np.where(is_count, x, 1).astype(np.int64)
    cpad = np.concatenate([is_count, np.zeros(8, bool)])
    K = share_k(n)
    P = np.arange(SUB, n, SUB)
    if len(P):
        full = (e[P] == 0) & cpad[P + 4]  # four equal bytes and their count begin at the edge
        kinds = {"sub": P % WAVE != 0, "wave": (P % WAVE == 0) & (P % GROUP != 0), "group": P % GROUP == 0,
                 "share2": (P % (2 * SUB) == 0) & (K == 2), "share14": (P % (14 * SUB) == 0) & (K == 14)}
        what = {"e=0": full, "e=4": is_count[P]}
        for c in (1, 2, 3):
            what["e=%d goes on" % c] = (e[P] == c) & cpad[P + 4 - c]
            what["e=%d breaks" % c] = full & (x[P] != x[P - 1]) & ~is_count[P - 1] & (e[P - 1] == c - 1)
        for kn, km in kinds.items():
            for wn, wm in what.items():
                if np.any(km & wm):
                    h.add("H edge=%s %s" % (kn, wn))
    ci = np.flatnonzero(is_count)
    xpad = np.concatenate([x.astype(np.int64), np.full(8, -1)])
    for at, sel in (("", ci), (" at sub edge", ci[ci % SUB == 0])):
        for c in set(x[sel].tolist()) & set(H_COUNTS):
            h.add("H count=%d%s" % (c, at))
        if np.any(x[sel] == x[sel - 1]):
            h.add("H count==run byte" + at)
        if np.any((xpad[sel + 1] == x[sel - 1]) & cpad[sel + 5]):
            h.add("H byte after count equals run byte" + at)
    if n and np.all(x == x[0]) and int(x[0]) in H_SELF_V and n in H_SELF_N:
        h.add("H self v=%d n=%d" % (x[0], n))
    if n >= 10 and n % 5 == 0 and np.array_equal(x, np.tile(x[:5], n // 5)) and len(set(x[:4].tolist())) == 1 \
            and x[4] != x[0]:
        h.add("H period5 n<64" if n < 64 else "H period5 n>=4096" if n >= 4096 else "H period5")
    outpos = np.concatenate([[0], np.cumsum(reps)])
    subs = np.arange(0, n, SUB)
    if np.any(outpos[np.minimum(subs + SUB, n)] - outpos[subs] >= 3300):
        h.add("H sub out>=3300")
    if not pending:
        if n % 64 in (0, 1, 63):
            h.add("H end n%%64=%d" % (n % 64))
        if n == 1:
            h.add("H end n=1")
        if is_count[-1] and int(x[-1]) in (0, 255):
            h.add("H end count=%d" % x[-1])
        if not is_count[-1] and 1 <= e[-1] + 1 <= 3:
            h.add("H end equal=%d" % (e[-1] + 1))
    # waves of k_dec_rle_expand
    w0 = np.arange(0, n, WAVE)
    base = outpos[w0]
    total = outpos[np.minimum(w0 + WAVE, n)] - base
    shift = (phase + base) & 3
    staged = total + shift <= EXP_STAGE
    for t, s, sg in zip(total.tolist(), shift.tolist(), staged.tolist()):
        if t + s in (8191, 8192, 8193):
            h.add("H stage total+shift=%d shift=%d" % (t + s, s))
        if 0 < t < 4 and s:
            h.add("H total<4 shift=%d" % s)
        if 0 < t and s and t + s < 4:
            h.add("H one-dword flush shift=%d" % s)
    for w in range(1, len(w0)):
        if staged[w - 1] != staged[w]:
            h.add("H seam %s shift=%d" % ("staged|direct" if staged[w - 1] else "direct|staged", shift[w]))
    return h, pending, int(outpos[-1])


def hits(case, k=0):
    """the named targets a case of family h or i reaches, recomputed from its images with the tiling constants
    above; k is the address of the stream's first output byte mod 16"""
    h = set()
    pos = k
    fam = case.name[0]
    nblk = len(case.images)
    for bi, image in enumerate(case.images):
        if fam == "H":
            hh, pending, ln = _hits_h_image(image, pos & 3)
            if pending:
                h.add("H no count " + ("only" if nblk == 1 else "last" if bi == nblk - 1 else "middle"))
                break
            h |= hh
        else:
            ln = len(rle1_undo(image)[0])
            a = pos & 15
            R = a + ln
            npieces = (R + 15) // 16
            ragged = bool(R & 15)
            if ln <= 48:
                h.add("I a=%d r=%d" % (a, R & 15))
            if npieces in I_PIECES and a in (0, 1, 15):
                h.add("I pieces=%d last=%s a=%d" % (npieces, "ragged" if ragged else "full", a))
            if case.flips and case.flips[bi]:
                if npieces == 1:
                    h.add("I wrong crc pieces=1")
                if npieces == TILE_PIECES + 1 and ragged:
                    h.add("I wrong crc ragged tile seam")
                if npieces == SLICE_PIECES + 1:
                    h.add("I wrong crc slice seam")
                break
        pos += ln
    return h & REQUIRED[fam.lower()]


# ---- images -------------------------------------------------------------------------------------------------------------
def norun(rng, n):
    """n bytes, no two neighbours equal"""
    if n == 0:
        return np.zeros(0, np.uint8)
    return (np.cumsum(1 + rng.integers(0, 254, n)) % 256).astype(np.uint8)


def _other(rng, *avoid):
    while True:
        v = int(rng.integers(0, 256))
        if v not in avoid:
            return v


def plant(x, P, e, breaks, count, rng):
    """write a group v v v v count into x so that position P falls behind e of its equal bytes (e = 4: on the
    count); with `breaks`, e bytes of another value u stand in front of P and the group begins at P"""
    if breaks:
        s = P - e
        u = _other(rng, int(x[s - 1]))
        x[s:P] = u
        g = P
    else:
        g = P - e
        u = int(x[g - 1])
    v = _other(rng, u)
    x[g:g + 4] = v
    x[g + 4] = v if count is None else count


_EDGE_VARIANTS = [(0, False), (1, False), (2, False), (3, False), (1, True), (2, True), (3, True), (4, False)]


def image_with_total(rng, total, n_lit):
    """an image whose undo has exactly `total` bytes: about n_lit literals without runs, then groups of count 255
    with changing run bytes, then one group or a few literals for the rest"""
    n_lit = min(n_lit, total)
    rest = total - n_lit
    if 0 < rest < 4:
        n_lit, rest = total, 0
    parts = [norun(rng, n_lit)]
    prev = int(parts[0][-1]) if n_lit else -1
    while rest:
        take = min(rest, 259)
        if rest - take in (1, 2, 3):
            take -= 4
        v = _other(rng, prev)
        parts.append(np.array([v, v, v, v, take - 4], np.uint8))
        prev = -1  # (behind a count everything is fresh)
        rest -= take
    return np.concatenate(parts).tobytes()


def _img_case(name, images, status=0, flips=None, cut=None, **kw):
    """a case from block images: expected bytes from rle1_undo of the blocks in front of `cut` (all of them when
    None)"""
    blocks = [block_from_image(im, flip=(flips[i] if flips else 0)) for i, im in enumerate(images)]
    z = write(Stream(9, blocks))
    data = b"".join(rle1_undo(im)[0] for im in (images if cut is None else images[:cut]))
    c = Case(name, z, status, data, multi=len(images) > 1, **kw)
    c.images, c.flips = [bytes(im) for im in images], flips
    c.no_oracle = False
    return c


_MEMO = {}


def family_h(oracle):
    """the RLE1 undo at its tile seams (stage D4): run groups at chosen phases against sub-tile, wave, workgroup
    and thread-share edges, the count values and a count equal to its run byte, self-similar images, image ends,
    waves on both sides of the staging threshold at every dword phase, and blocks that end behind four equal bytes.
    Expected bytes come from rle1_undo."""
    if "h" in _MEMO:
        return _MEMO["h"]
    rng = np.random.default_rng(808)
    out = []
    counts = list(H_COUNTS) + [None]  # None: the count equals the run byte
    # sub-tile, wave and workgroup edges: one block per variant, 16 384 + 200 bytes
    images = []
    for vi, (e, brk) in enumerate(_EDGE_VARIANTS):
        x = norun(rng, GROUP + 200)
        for j, P in enumerate((GROUP, WAVE, 3 * WAVE, SUB, 7 * SUB, WAVE + SUB, GROUP - SUB, GROUP + SUB)):
            plant(x, P, e, brk, counts[(vi + j) % len(counts)], rng)
        images.append(x)
    out.append(_img_case("H-edges-sub-wave-group", images))
    # thread shares of two sub-tiles (65 537..131 072 image bytes) and of fourteen (899 981)
    for name, n in (("share2", 70000), ("share14", 899981)):
        x = norun(rng, n)
        K = share_k(n)
        assert K == (2 if name == "share2" else 14)
        edges = [K * SUB * j for j in range(1, n // (K * SUB))]
        picks = [edges[i * (len(edges) - 1) // 23] for i in range(24)]  # the first, the last, and between
        for i, P in enumerate(picks):
            e, brk = _EDGE_VARIANTS[i % 8]
            plant(x, P, e, brk, counts[(i // 8 + i) % len(counts)], rng)
        out.append(_img_case("H-edges-%s" % name, [x], cap=8 << 20))
    # counts: every value, a count equal to its run byte, a fresh run behind a count; each also with the count
    # as the first byte of a sub-tile
    x = norun(rng, 40 * SUB)
    P = SUB
    for at_edge in (False, True):
        for c in counts:
            plant(x, P if at_edge else P + 17, 4, False, c, rng)
            P += 2 * SUB
        g = P - 4 if at_edge else P + 9   # a a a a 00 a a a a 02
        a = _other(rng, int(x[g - 1]), int(x[g + 10]), 0, 2)
        x[g:g + 10] = [a, a, a, a, 0, a, a, a, a, 2]
        P += 2 * SUB
    out.append(_img_case("H-counts", [x]))
    # self-similar images: the parse has period 5 against tiles of 64
    for v in H_SELF_V:
        out.append(_img_case("H-self-%d" % v, [bytes([v]) * n for n in H_SELF_N], cap=16 << 20))
    out.append(_img_case("H-period5", [bytes([97, 97, 97, 97, 3]) * 3, bytes([0, 0, 0, 0, 255]) * 1000,
                                       bytes([7, 7, 7, 7, 0]) * 13, bytes([4, 4, 4, 4, 5]) * 900]))
    # image ends
    ends = [norun(rng, 128), norun(rng, 65), norun(rng, 63), norun(rng, 1)]
    for tail in ([9, 9, 9, 9, 0], [9, 9, 9, 9, 255], [9], [9, 9], [9, 9, 9]):
        b = norun(rng, 100)
        b[-1] = 8
        ends.append(np.concatenate([b, np.array(tail, np.uint8)]))
    out.append(_img_case("H-ends", ends))
    # staging: one-wave blocks on both sides of the threshold at every phase; fillers of 1-3 bytes set the phase
    images, pos = [], 0

    def at_phase(s):
        nonlocal pos
        f = (s - pos) % 4
        if f:
            images.append(norun(rng, f))
            pos += f

    def add(im):
        nonlocal pos
        images.append(im)
        pos += len(rle1_undo(im)[0])

    for s in range(4):
        for t in (8191, 8192, 8193):
            at_phase(s)
            add(image_with_total(rng, t - s, 3900))
    for s in range(4):  # a staged wave, a wave of count-255 groups (direct), a staged one
        at_phase(s)
        v = _other(rng)
        mid = np.tile(np.array([v, v, v, v, 255], np.uint8), 819)
        add(np.concatenate([norun(rng, WAVE - 1), [_other(rng, v)], mid, [_other(rng, v)], norun(rng, 1000)]).astype(np.uint8))
    for s in (1, 2, 3):  # a last wave of one to three bytes, and whole blocks that small
        at_phase(s)
        add(norun(rng, WAVE + s))
        for t in (1, 2, 3):
            at_phase(s)
            add(norun(rng, t))
    out.append(_img_case("H-staging", images))
    # four equal bytes and no count: DataError, the blocks in front intact, nothing of that block.  The oracle,
    # like the reference, reads on around the closed pointer chain and answers -100 at any capacity, so these
    # cases are not compared with it (no_oracle).
    good = [norun(rng, 300), norun(rng, 77)]
    bad = np.concatenate([norun(rng, 200), np.array([5, 6, 6, 6, 6], np.uint8)])
    for name, imgs, cut in (("only", [bad], 0), ("middle", [good[0], bad, good[1]], 1), ("last", [good[0], bad], 1)):
        c = _img_case("H-no-count-%s" % name, imgs, status=E_DATA, cut=cut)
        c.no_oracle = True
        c.multi = len(imgs) > 1
        out.append(c)
    # 899 981 bytes of ff: fourteen sub-tiles per thread, every sub-tile near its largest output (46.6 MB)
    out.append(_img_case("H-ff-899981", [b"\xff" * 899981], cap=64 << 20))
    _MEMO["h"] = out
    return out


def _euler_circuit(k):
    """a closed walk over the complete directed graph on k nodes with loops that takes every edge once"""
    nxt = {a: list(range(k)) for a in range(k)}
    stack, walk = [0], []
    while stack:
        a = stack[-1]
        if nxt[a]:
            stack.append(nxt[a].pop())
        else:
            walk.append(stack.pop())
    return walk[::-1]


def family_i(oracle):
    """the block CRC at every geometry of k_dec_crc: all 256 pairs of (address of the first byte, end) mod 16 on
    blocks of 1-48 bytes, piece counts around the tile (256) and slice (4096) seams with a full and a ragged last
    piece at alignments 0, 1 and 15, and a wrong stored CRC at three of these"""
    if "i" in _MEMO:
        return _MEMO["i"]
    rng = np.random.default_rng(909)
    out = []
    walk = _euler_circuit(16)
    assert len(walk) == 257 and walk[0] == 0
    images = []
    for a, r in zip(walk, walk[1:]):
        ln = (r - a) % 16 + 16 * int(rng.integers(0, 3))
        images.append(image_with_total(rng, ln or 16 * int(rng.integers(1, 4)), 6))
    out.append(_img_case("I-grid", images))
    for a in (0, 1, 15):
        images, pos = [], 0
        for p in I_PIECES:
            for ragged in (False, True):
                if p == 1 and ragged and a == 15:
                    continue
                f = (a - pos) % 16
                if f:
                    images.append(image_with_total(rng, f, 16))
                    pos += f
                R = 16 * p - (int(rng.integers(1, 16 - (a if p == 1 else 0))) if ragged else 0)
                images.append(image_with_total(rng, R - a, 100))
                pos += R - a
        out.append(_img_case("I-pieces-a%d" % a, images))
    for name, a, R in (("one-piece", 3, 9), ("ragged-tile-seam", 5, 16 * 256 + 7), ("slice-seam", 15, 16 * 4096 + 16)):
        images = [image_with_total(rng, 16 + a, 16), image_with_total(rng, R - a, 100), norun(rng, 40)]
        out.append(_img_case("I-wrong-crc-%s" % name, images, status=E_DATA, flips=[0, 1 << int(rng.integers(0, 32)), 0],
                             cut=2))
    _MEMO["i"] = out
    return out


FAMILIES = ("a", "b", "c", "d", "e", "f", "g", "h", "i")


def all_cases(oracle, families=FAMILIES):
    out = []
    for f in families:
        out += globals()["family_" + f](oracle)
    return out
