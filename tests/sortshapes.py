"""Blocks placed where the round driver of the rotation sort (run_bwt_once, rust-compression_amd/csrc/k_bwt.hip) picks
another set of kernels (CPU only: Python, numpy; the oracle only where a test compares orders).

After the init the driver reads two counts per round -- m, the rotations of the batch whose first h symbols are not
unique, and mx, the most of them in one block -- and chooses from them: the walk form (m * 4 >= total), the survivor
form (below that; inside LDS, k_surv_local, when also m * 8 < total and no segment of an earlier round overflowed), the
period round, link rounds behind it, and the end (m == 0, or the depth reaches the block length with equal rotations
left).  Each case here is a generator name with its arguments; `build(case)` rebuilds the bytes, `profile(block, hs)`
computes m(h), the largest group G(h) and the group sizes in sorted order with plain prefix doubling in numpy -- neither
the product nor the oracle's sort --, `hits(case)` recomputes from the profile which targets the bytes reach, and
`REQUIRED` is the set the committed cases must cover.  The figures are committed as tests/golden/sort_shapes.json
(no block bytes); `python tests/sortshapes.py --regen` rewrites it.

How the properties are stated.  The depth a round compares at is h = 2c << step, c the symbols per key the GPU picked
(KeyInfo::chars: 4 for a block of more than 128 symbols that uses more than 1024 byte pairs, up to 8 otherwise).  m is
monotone in h, so a property "lo <= m(h) < hi for every h in a..b" is checked at the two ends and holds whatever c is.
The list geometry (which groups start in which tile of 8192 list entries: `segments`) is checked at every depth of
DEPTHS.  Only the exact list lengths (8192 k - 1, 8192 k, 8192 k + 1) hold at one depth alone -- every construction
loses one rotation per symbol of depth at the end of each repeat --: they are stated at h = 8, and `hits` checks that
the block has c = 4 by the rule above.

The period round's pass count and whether link rounds pay follow from tables only the GPU builds; for those `hits`
checks what the generator can promise (the smallest distance at which a fifth of the block agrees with itself; the
unordered share at the depths the triggers look at) and the GPU test reads the form itself off the trace.
"""
import hashlib
import json
import os
import random
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "sort_shapes.json")
TRACE_SAMPLE = os.path.join(HERE, "golden", "sort_trace_sample.txt")

TILE = 8192        # list entries per tile (bzgpu.h kSortTile)
LOC_CAP = 2 * TILE  # entries of one segment of k_surv_local (kLocCap)
LOC_LOOK = LOC_CAP + 64  # positions k_surv_local looks at for a group start
DEPTHS = (8, 16, 32, 64)
DEEP = 2048
L1 = 100000 - 19   # block limit of level 1

EXACT = tuple(TILE * k + d for k in (1, 2) for d in (-1, 0, 1))

# (the segment's group count decides the LDS pass count, its length whether the second half of the registers is in use:
# all four combinations; the period round by when it is entered and by what decides its pass count)
REQUIRED = frozenset(
    ["S1 walk carried", "S2 walk later", "S3 list<tile", "S3 straddle", "S3 empty tile",
     "S3 groups<=128 seg<=8192", "S3 groups<=128 seg>8192", "S3 groups>128 seg<=8192", "S3 groups>128 seg>8192",
     "S4 group>cap", "S4 alignment", "S5 no LDS attempt",
     "S6 at once, distances>=1024", "S6 at once, distance<1024", "S6 later, distances>=1024", "S6 later, short period cut",
     "S7 copies of copies", "S7 nine copies", "S8 cyclic period", "S9 unordered block, tail=0",
     "S9 unordered block, tail=1", "S9 unordered block, tail=2", "S9 unordered block, tail=3", "S9 alphabets 2|256",
     "S9 group start out of reach"] +
    ["S3 list=%d" % x for x in EXACT])


# ------------------------------------------------------------------------------------------------------- generators
def filler(seed, n, lo=0, k=200):
    """n random bytes over the k values lo..lo+k-1, every odd position different from the even one before it: unique at
    depth 8 for k = 200 in any block this file builds (two of 140 000 rotations share eight such bytes with probability
    4e-9), and never four equal bytes in a row, even where two pieces meet (RLE1 leaves it alone)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, k, n, dtype=np.int64)
    odd = np.arange(1, n, 2)
    x[odd] = (x[odd - 1] + 1 + rng.integers(0, k - 1, odd.size)) % k
    return ((x + lo) % 256).astype(np.uint8).tobytes()


def para(seed, k, alpha=b"abcdefgh "):
    rng = random.Random(seed)
    return bytes(rng.choice(alpha) for _ in range(k))


def runs(seed, nfill, lo, *rl):
    """filler over lo..lo+199, then runs of rl[0] bytes (lo+200), rl[1] bytes (lo+201), ..: a run of R equal bytes is
    one group of R - h + 1 rotations at depth h"""
    return filler(seed, nfill, lo) + b"".join(bytes([(lo + 200 + i) % 256]) * r for i, r in enumerate(rl))


def pairs(seed, nfill, lc, ncopy, *rl):
    """filler, a chunk of lc filler bytes ncopy times with a fresh byte behind each copy (groups of ncopy rotations:
    lc - h + 1 of them at depth h), then runs as in `runs`.  The filler and the chunk use the values 0..199, the
    separators and the runs 200 and up: the runs' groups sort behind all the small groups."""
    chunk = filler(seed + 1000, lc)
    body = b"".join(chunk + bytes([250 - i]) for i in range(ncopy))
    return filler(seed, nfill) + body + b"".join(bytes([200 + i]) * r for i, r in enumerate(rl))


def golden(name, n):
    """the first n bytes of a file of tests/golden (sample1.ref: libbzip2's text sample, all 256 byte values in use)"""
    with open(os.path.join(HERE, "golden", name), "rb") as f:
        return f.read()[:n]


def repeat(seed, plen, nrep, nfill):
    """a paragraph of plen letters cut to nrep bytes of its repetition, then filler"""
    return (para(seed, plen) * (nrep // plen + 1))[:nrep] + filler(seed, nfill)


def ugh(seed):
    """a short period cut by changed bytes (test_gpu_parity.py: "ugh\\n" x 30 000 of libbzip2's sample3)"""
    rng = random.Random(seed)
    u = bytearray(b"ugh\n" * 12000)
    for pos in range(700, len(u), 1900):
        u[pos] = (u[pos] + (1 if (pos // 1900) % 3 else 251)) & 255
    for pos in (10000, 20000, 30000):
        u[pos] = ord("#")
        u[pos + 1204] = ord("#")
    st = bytes(rng.choice(bytes(range(33, 97))) for _ in range(5000))
    return bytes(u[:40000]) + st + bytes(u[40000:48000])


def _touched(rng, b, every):
    out = bytearray(b)
    for pos in range(rng.randrange(every), len(out), every):
        out[pos] = out[pos] ^ (1 + rng.randrange(7))
    return bytes(out)


def copies(seed, kind, n):
    """touched copies (test_gpu_parity.py, test_link_rounds_on_copies_of_copies): kind 0 a stretch that repeats inside
    itself, four times, a byte changed every 4 KiB (groups of 2 to 8); kind 1 nine copies of one stretch"""
    rng = random.Random(seed)
    alpha = bytes(range(33, 97))

    def stretch(k):
        return bytes(rng.choice(alpha) for _ in range(k))

    inner = stretch(9000)
    unit = inner + stretch(3000) + _touched(rng, inner, 2048) + stretch(1500)
    if kind == 0:
        return b"".join(_touched(rng, unit, 4096) for _ in range(4))[:n]
    return (_touched(rng, inner * 9, 4096) + stretch(100))[:n]


def cyclic(seed, plen, reps):
    return para(seed, plen) * reps


def batch(seed, kind, tail):
    """an input of level-1 blocks (no run of four equal bytes, so RLE1 cuts it every L1 bytes).  kind 0: fourteen filler
    blocks round one block that is a paragraph repeated (every rotation unordered), then `tail` more bytes: sixteen
    blocks.  kind 1: three filler blocks over 256 values, then "ab" x `tail`: a cyclic period over two symbols.  kind 2:
    fourteen filler blocks round a block "abab..a": two groups of half the block each."""
    if kind == 0:
        p = filler(seed + 50, 4096, 0, 9)
        deep = (p * (L1 // 4096 + 1))[:L1]
        b = [filler(seed + i, L1) for i in range(15)]
        b[7] = deep
        return b"".join(b) + filler(seed + 99, tail)
    if kind == 2:
        b = [filler(seed + i, L1) for i in range(15)]
        b[7] = (b"ab" * L1)[:L1]
        return b"".join(b)
    return b"".join(filler(seed + i, L1, 0, 256) for i in range(3)) + b"ab" * tail


GENS = {"filler": filler, "runs": runs, "pairs": pairs, "golden": golden, "repeat": repeat, "ugh": ugh, "copies": copies,
        "cyclic": cyclic, "batch": batch}


def build(case):
    return GENS[case["gen"]](*case["args"])


def blocks_of(case, data=None):
    """the blocks the sort sees: the bytes themselves, or for a batch case their level-1 blocks"""
    data = build(case) if data is None else data
    if case["gen"] != "batch":
        return [data]
    return [data[i:i + L1] for i in range(0, len(data), L1)]


# --------------------------------------------------------------------------------------------------------- profile
class Profile:
    """ranks of the cyclic rotations of one block by their first h symbols, by prefix doubling: the rank at depth
    a + b is the rank of the pair (rank at depth a, rank at depth b of the rotation a places on)"""

    def __init__(self, block):
        self.b = np.frombuffer(bytes(block), dtype=np.uint8)
        self.n = len(self.b)
        self._r = {1: self._dense(self.b.astype(np.int64), np.zeros(self.n, dtype=np.int64))}

    def _dense(self, first, second):
        """dense ranks 0.. of the pairs, in lexicographic order"""
        order = np.lexsort((second, first))
        f, s = first[order], second[order]
        new = np.ones(self.n, dtype=np.int64)
        new[1:] = (f[1:] != f[:-1]) | (s[1:] != s[:-1])
        r = np.empty(self.n, dtype=np.int64)
        r[order] = np.cumsum(new) - 1
        return r

    def ranks(self, h):
        if h not in self._r:
            p = 1 << (h.bit_length() - 1)
            if p == h:
                a = b = h // 2
            else:
                a, b = p, h - p
            ra, rb = self.ranks(a), self.ranks(b)
            self._r[h] = self._dense(ra, np.roll(rb, -(a % self.n)))
        return self._r[h]

    def sizes(self, h):
        """sizes of the groups of equal h-prefixes, in sorted order"""
        return np.bincount(self.ranks(h))

    def groups(self, h):
        """sizes of the groups of more than one rotation, in sorted order: the survivor list of a round at depth h"""
        s = self.sizes(h)
        return s[s > 1]

    def m(self, h):
        return int(self.groups(h).sum())

    def G(self, h):
        return int(self.sizes(h).max())

    def order(self):
        """the rotations in sorted order; equal rotations (a cyclic period) by their start"""
        h = 1
        while h < self.n:
            h *= 2
        return np.argsort(self.ranks(h), kind="stable")

    def full_ranks(self):
        h = 1
        while h < self.n:
            h *= 2
        return self.ranks(h)


_CACHE = {}


def _profile_of(block):
    """(the batch cases share fifteen of their sixteen blocks)"""
    key = hashlib.sha256(block).digest()
    if key not in _CACHE:
        if len(_CACHE) >= 20:
            _CACHE.clear()
        _CACHE[key] = Profile(block)
    return _CACHE[key]


def profile(block, hs):
    """{h: {"m": rotations whose h-symbol prefix is not unique, "G": the largest group of equal h-prefixes, "groups": the
    sizes of the groups of more than one rotation, in sorted order}} of one block"""
    p = _profile_of(bytes(block))
    return {h: {"m": p.m(h), "G": p.G(h), "groups": p.groups(h).tolist()} for h in hs}


def order_matches(p, sa):
    """`sa` (rotation starts, the oracle's) is the profile's order wherever rotations differ"""
    sa = np.asarray(sa, dtype=np.int64)
    if len(sa) != p.n or not np.array_equal(np.sort(sa), np.arange(p.n)):
        return False
    r = p.full_ranks()[sa]
    return bool(np.all(r[1:] >= r[:-1]))


def segments(groups):
    """k_surv_local's view of a survivor list whose groups have these sizes, in order: per tile of the list (a
    workgroup each) None where no group starts inside, "lost" where no group start lies within LOC_LOOK entries of
    the tile's first or of the next tile's first, else (first entry, entries, groups) of the segment -- the groups
    that START inside the tile; more than LOC_CAP entries do not fit."""
    groups = np.asarray(groups, dtype=np.int64)
    cnt = int(groups.sum())
    starts = np.concatenate((np.cumsum(groups) - groups, [cnt]))  # (the list's end stands in for a start behind it)

    def first(p0):
        if p0 >= cnt:
            return cnt
        i = int(np.searchsorted(starts, p0))
        if i == len(groups):  # (the list's end is seen only by a step of 64 entries that begins inside the reach)
            return cnt if cnt - p0 <= LOC_LOOK - 64 else None
        return int(starts[i]) if starts[i] - p0 < LOC_LOOK else None

    out = []
    for t0 in range(0, cnt, TILE):
        s0, s1 = first(t0), first(t0 + TILE)
        if s0 is None or s1 is None:
            out.append("lost")
        elif s1 <= s0:
            out.append(None)
        else:
            out.append((s0, s1 - s0, int(np.searchsorted(starts, s1) - np.searchsorted(starts, s0))))
    return out


def fits(segs):
    return all(s is None or (s != "lost" and s[1] <= LOC_CAP) for s in segs)


def key_chars(block):
    """symbols per key of the init, by k_key_params' rule: 30 // bits-per-symbol of them (4 at eight bits, 8 at most), or,
    when the block uses at most 1024 of its byte pairs and that is more, 2 * (30 // bits-per-pair).  A round's depth is
    twice that, shifted by its step."""
    b = np.frombuffer(block, dtype=np.uint8).astype(np.int64)
    bits = max(1, int(len(np.unique(b)) - 1).bit_length())
    c = 4 if bits >= 8 else min(8, 30 // bits)
    pbits = max(1, int(len(np.unique(b * 256 + np.roll(b, -1))) - 1).bit_length())
    if pbits <= 10 and min(8, 2 * (30 // pbits)) > c:
        c = min(8, 2 * (30 // pbits))
    return c


def agreement(block, lo, hi):
    """the smallest distance p in lo..hi-1 at which at least a fifth of the block equals itself p places on, or 0"""
    b = np.frombuffer(block, dtype=np.uint8)
    for p in range(lo, hi):
        if int(np.count_nonzero(b[p:] == b[:-p])) * 5 >= len(b):
            return p
    return 0


# ---------------------------------------------------------------------------------------------------------- targets
def hits(case, data=None):
    """the targets this case's bytes reach, from the profile alone; also the figures per depth"""
    data = build(case) if data is None else data
    fam = case["family"]
    h = set()
    blks = blocks_of(case, data)
    profs = [_profile_of(b) for b in blks]
    total, max_n = sum(p.n for p in profs), max(p.n for p in profs)
    depths = (8, 16) if fam == "S9" else DEPTHS + (DEEP,)
    fig = {str(d): {"m": sum(p.m(d) for p in profs), "mx": max(p.m(d) for p in profs), "G": max(p.G(d) for p in profs)}
           for d in depths}
    if fam == "S9":
        m8, mx8 = fig["8"]["m"], fig["8"]["mx"]
        if case["args"][1] == 0:
            deep = [p for p in profs if p.m(16) * 64 >= p.n * 63]
            # the batch in survivor form with an LDS attempt at any first depth, while one block's list spans 13 tiles
            if len(deep) == 1 and m8 * 8 < total and mx8 == m8 and fig["16"]["mx"] > 12 * TILE:
                h.add("S9 unordered block, tail=%d" % (len(blks[-1]) % L1))
        if case["args"][1] == 2:
            # (k_surv_local finds no group start within LOC_LOOK entries of a tile's first, at the batch's depth or the block's)
            if m8 * 8 < total and all("lost" in segments(p.groups(d)) for p in profs if p.m(8) for d in (8, 16)):
                h.add("S9 group start out of reach")
        if case["args"][1] == 1:
            last = profs[-1]
            if len(np.unique(last.b)) == 2 and last.m(2 * last.n) == last.n and last.n < 20000 and \
                    all(len(np.unique(p.b)) == 256 for p in profs[:-1]):
                h.add("S9 alphabets 2|256")
        return h & REQUIRED, fig
    p, n = profs[0], profs[0].n
    m = {d: p.m(d) for d in depths}
    G = {d: p.G(d) for d in depths}
    quiet = m[8] * 64 < n * 63  # (no period round at once, whatever the first depth)
    no_period = quiet and m[8] * 4 < n * 3  # (nor later: m is monotone)
    if fam == "S1" and p.m(2 * key_chars(data)) * 4 >= n and quiet:  # (at the depth the init reaches on this block)
        h.add("S1 walk carried")
    if fam == "S2" and m[DEEP] * 4 >= n and no_period:
        h.add("S2 walk later")
    if fam in ("S3", "S4") and no_period:
        segs = {d: segments(p.groups(d)) for d in DEPTHS}
        lds = all(m[d] * 8 < n for d in DEPTHS)  # (the driver tries the LDS form at every depth 8..64)
        ok = {d: fits(segs[d]) for d in DEPTHS}
        real = {d: [s for s in segs[d] if s not in (None, "lost")] for d in DEPTHS}
        if fam == "S3" and lds and all(ok.values()):
            def every(f):
                return all(f(d) for d in DEPTHS)
            if every(lambda d: 0 < m[d] < TILE):
                h.add("S3 list<tile")
            if m[8] in EXACT and key_chars(data) == 4:
                h.add("S3 list=%d" % m[8])
            if every(lambda d: any(s[0] // TILE != (s[0] + s[1] - 1) // TILE and s[2] > 1 for s in real[d])):
                h.add("S3 straddle")  # (a segment of several groups that ends behind its tile: its last group lies across the edge)
            if every(lambda d: None in segs[d]):
                h.add("S3 empty tile")
            for small in (True, False):
                for short in (True, False):
                    if every(lambda d: any((s[2] <= 128) == small and (s[1] <= TILE) == short for s in real[d])):
                        h.add("S3 groups%s128 seg%s8192" % ("<=" if small else ">", "<=" if short else ">"))
        if fam == "S4" and m[8] * 8 < n and not ok[8]:
            if G[64] > LOC_CAP:  # (G is monotone too: larger than a segment at every depth 8..64)
                h.add("S4 group>cap")
            elif G[8] <= LOC_CAP:
                h.add("S4 alignment")
    if fam == "S5" and m[8] * 4 < n and m[DEEP] * 8 >= n:
        h.add("S5 no LDS attempt")
    if fam == "S6":
        when = "at once" if m[16] * 64 >= n * 63 else ("later" if quiet and m[32] * 4 >= n * 3 else None)
        d = agreement(data, 1, 4200)
        what = "distances>=1024" if d >= 1024 else ("distance<1024" if d > 64 else ("short period cut" if 0 < d <= 16 else None))
        if when and what:
            h.add("S6 %s, %s" % (when, what))
    if fam == "S7" and m[32] * 4 >= n * 3 and p.m(2 * n) == 0:  # (a period round by round 2, and no equal rotations)
        h.add("S7 copies of copies" if case["args"][1] == 0 else "S7 nine copies")
    if fam == "S8" and n < 20000 and p.m(2 * n) == n:
        h.add("S8 cyclic period")
    return h & REQUIRED, fig


# ------------------------------------------------------------------------------------------------------------ trace
_ROUND = re.compile(r"^bz2_mi355x: sort round (\d+) \(h = (\d+)\): (\d+) of (\d+) rotations unordered, at most (\d+) in one "
                    r"block \(block (\d+); of (\d+)\): (period round|link round|survivor form|walk form)$")
_PASSES = {"one pass over the keys": 1, "two passes over the keys": 2, "three passes over thirty-bit keys": 3}


def parse_trace(text):
    """the BZ_BWT_TRACE lines of one process as a list of sorts, each a list of rounds {"round", "h", "m", "total", "mx",
    "max_n", "form": walk | survivor | period | link}; a survivor round also has "lds": None (no attempt), "done" or
    "did not fit"; a period round "passes": 1, 2 or 3.  A sort starts at every round 1.  Lines of other traces and the
    period round's per-block lines are passed over; a `sort round` line that does not parse raises ValueError."""
    sorts = []
    for line in text.splitlines():
        s = line.strip()
        if "sort round" in s:
            mt = _ROUND.match(s)
            if not mt:
                raise ValueError("sort round line not understood: %r" % line)
            r = {"round": int(mt.group(1)), "h": int(mt.group(2)), "m": int(mt.group(3)), "total": int(mt.group(4)),
                 "mx": int(mt.group(5)), "max_n": int(mt.group(7)), "form": mt.group(8).split()[0]}
            if r["form"] == "survivor":
                r["lds"] = None
            if r["round"] == 1:
                sorts.append([])
            if not sorts or r["round"] != len(sorts[-1]) + 1:
                raise ValueError("sort round out of sequence: %r" % line)
            sorts[-1].append(r)
        elif s.startswith("survivor round inside LDS:"):
            if not sorts or sorts[-1][-1]["form"] != "survivor" or sorts[-1][-1]["lds"] is not None:
                raise ValueError("LDS line without its survivor round: %r" % line)
            rest = s.split(":", 1)[1].strip()
            if rest == "done":
                sorts[-1][-1]["lds"] = "done"
            elif rest.startswith("a segment did not fit"):
                sorts[-1][-1]["lds"] = "did not fit"
            else:
                raise ValueError("LDS line not understood: %r" % line)
        elif s.startswith("period round:"):
            rest = s.split(":", 1)[1].strip()
            n = next((v for k, v in _PASSES.items() if rest.startswith(k)), None)
            if n is None or not sorts or sorts[-1][-1]["form"] != "period" or "passes" in sorts[-1][-1]:
                raise ValueError("period round line not understood: %r" % line)
            sorts[-1][-1]["passes"] = n
    return sorts


def forms(rounds):
    """the names of the forms one sort's rounds took (the vocabulary of FORMS).  Read off the sequence: a survivor round
    without an LDS line is "list too long" when m * 8 >= total and "sticky" otherwise (an earlier round's segment did not
    fit); a link round paid when the round behind it was given at most three quarters of what it was given, or when the
    sort ends behind it (the depth has not moved, so nothing was left); the sort ends by depth when its last round is a
    doubling round whose doubled depth reaches the largest block."""
    out = set()
    for i, r in enumerate(rounds):
        f = r["form"]
        if f == "walk":
            out.add("walk round 1" if r["round"] == 1 else "walk later")
        elif f == "survivor":
            if r["lds"] is None:
                out.add("survivor global, list too long" if r["m"] * 8 >= r["total"] else "survivor global, sticky")
            else:
                out.add("survivor LDS " + r["lds"])
        elif f == "period":
            out.add("period at once" if r["round"] == 1 else "period later")
            out.add("period %d pass" % r["passes"])
        else:
            nxt = rounds[i + 1]["m"] if i + 1 < len(rounds) else 0
            out.add("link paid" if (r["m"] - nxt) * 4 >= r["m"] else "link did not pay")
    if rounds and rounds[-1]["form"] in ("walk", "survivor") and 2 * rounds[-1]["h"] >= rounds[-1]["max_n"]:
        out.add("end by depth")
    return out


FORMS = frozenset(["walk round 1", "walk later", "survivor global, list too long", "survivor global, sticky",
                   "survivor LDS done", "survivor LDS did not fit", "period at once", "period later", "period 1 pass",
                   "period 2 pass", "period 3 pass", "link paid", "link did not pay", "end by depth"])
PERIOD = ("period at once", "period later")
LINK = ("link paid", "link did not pay")


def check_sequence(case, rounds):
    """what a case asks of the ORDER of its rounds (AssertionError when it is not so)"""
    seq = case.get("sequence")
    kinds = [(r["form"], r.get("lds")) for r in rounds]
    if seq == "all LDS":  # every round of the sort: survivor form, inside LDS, done
        assert rounds and all(k == ("survivor", "done") for k in kinds), kinds
    elif seq == "overflow once":  # "did not fit" once, then survivor rounds without an LDS line although m * 8 < total
        assert kinds[0] == ("survivor", "did not fit") and len(kinds) > 1, kinds
        assert all(k == ("survivor", None) for k in kinds[1:]), kinds
        assert all(r["m"] * 8 < r["total"] for r in rounds), rounds
    elif seq == "no attempt first":
        assert kinds[0] == ("survivor", None) and rounds[0]["m"] * 8 >= rounds[0]["total"], rounds[0]
    elif seq == "links to the end":  # the sort ends behind a link round, with nothing left
        assert kinds[-1][0] == "link" and 2 * rounds[-1]["h"] < rounds[-1]["max_n"], rounds
    elif seq == "one link":  # one link round that does not pay, doubling rounds behind it that a link round could have taken
        at = [i for i, k in enumerate(kinds) if k[0] == "link"]
        assert len(at) == 1 and at[0] + 1 < len(rounds), kinds
        assert any(r["m"] * 256 >= r["total"] for r in rounds[at[0] + 2:]), rounds
    elif seq == "equal rotations":  # nothing is ever ordered, and the doubling runs until the depth reaches the block
        assert rounds and all(r["m"] == r["max_n"] for r in rounds), rounds
    else:
        assert seq is None, seq


# ------------------------------------------------------------------------------------------------------------ cases
def _seek_run(gen, args, want):
    """the last argument (a run length) moved until m(8) == want: m grows by one with the run"""
    args = list(args)
    for _ in range(6):
        got = Profile(GENS[gen](*args)).m(8)
        if got == want:
            return args
        args[-1] += want - got
    raise RuntimeError("no run length gives a list of %d entries" % want)


def candidates():
    c = []

    def add(fam, gen, args, why, forms=(), absent=(), sequence=None):
        c.append({"family": fam, "gen": gen, "args": list(args), "why": why, "forms": list(forms), "absent": list(absent),
                  "sequence": sequence})

    lds = dict(forms=["survivor LDS done"], absent=["survivor LDS did not fit", "survivor global, sticky"], sequence="all LDS")
    over = dict(forms=["survivor LDS did not fit", "survivor global, sticky"], absent=["survivor LDS done"],
                sequence="overflow once")

    add("S1", "golden", ("sample1.ref", 100000), "text: two fifths unordered behind the init",
        forms=["walk round 1"], absent=PERIOD + LINK)
    add("S2", "repeat", (5, 4096, 40000, 58000), "a paragraph ten times and filler: two fifths unordered at any depth",
        forms=["walk round 1", "walk later"], absent=PERIOD + LINK)
    add("S3", "runs", (11, 90000, 0, 3000), "one group, a list shorter than a tile", **lds)
    add("S3", "runs", (12, 88000, 0, 10000), "one group of 10 000: nothing starts in the list's second tile", **lds)
    add("S3", "pairs", (14, 83000, 3000, 2, 5000), "pairs, then a group of 5000 across the edge of the first tile", **lds)
    for want in EXACT:
        nfill = (98000 if want < 10000 else 140000) - want - 200
        add("S3", "pairs", _seek_run("pairs", (20 + want % 7, nfill, (want - 150) // 2 + 7, 2, 160), want),
            "a list of %d entries at depth 8" % want, **lds)
    add("S4", "runs", (31, 123000, 0, 17000), "one group larger than a segment", **over)
    add("S4", "pairs", (32, 121000, 1000, 2, 15000), "2000 entries in pairs in front of a group of 15 000 in one tile", **over)
    add("S5", "runs", (41, 80000, 0, 18000), "between an eighth and a quarter unordered",
        forms=["survivor global, list too long"], absent=["survivor LDS did not fit", "survivor global, sticky"],
        sequence="no attempt first")
    add("S6", "repeat", (51, 4096, 40001, 0), "a paragraph of 4096 repeated: period round at once, distances >= 1024",
        forms=["period at once", "period 1 pass"])
    add("S6", "repeat", (52, 300, 40001, 0), "a paragraph of 300 repeated: a distance below 1024",
        forms=["period at once", "period 2 pass"])
    add("S6", "repeat", (53, 4096, 64000, 16000), "four fifths a paragraph repeated: the period round in round 2",
        forms=["walk round 1", "period later", "period 1 pass"], absent=["period at once"])
    add("S6", "ugh", (54,), "a period of 4 cut by changed bytes: thirty-bit keys",
        forms=["walk round 1", "period later", "period 3 pass"], absent=["period at once"])
    add("S7", "copies", (606, 0, 99000), "copies of copies: link rounds that pay until nothing is left",
        forms=["link paid"], absent=["link did not pay"], sequence="links to the end")
    add("S7", "copies", (606, 1, 82000), "nine copies: groups beyond the link rounds' reach",
        forms=["link did not pay", "walk later"], absent=["link paid"], sequence="one link")
    add("S8", "cyclic", (71, 1000, 19), "a cyclic period: equal rotations to the end",
        forms=["end by depth"], sequence="equal rotations")
    for t in (0, 1, 2, 3):
        add("S9", "batch", (81, 0, t), "one unordered block among filler blocks, and a last block of %d bytes" % t,
            forms=["survivor LDS done", "period later"], absent=["survivor LDS did not fit", "period at once"])
    add("S9", "batch", (82, 1, 5000), "a cyclic period over two symbols beside blocks of 256",
        forms=["survivor LDS done"], absent=PERIOD)
    add("S9", "batch", (81, 2, 0), "two groups of 50 000 in one block of the batch: no group start within reach of a tile",
        forms=["survivor LDS did not fit", "period later"], absent=["survivor LDS done", "period at once"])
    return c


def search(log=print):
    cases = candidates()
    for c in cases:
        data = build(c)
        got, fig = hits(c, data)
        c["targets"] = sorted(got)
        c["sha256"] = hashlib.sha256(data).hexdigest()
        c["n"] = len(data)
        c["figures"] = fig
        log(case_id(c), len(data), c["targets"], {k: v for k, v in fig.items() if k in ("8", "64", "2048")})
    return cases


def load():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def case_id(c):
    return "%s-%s(%s)" % (c["family"], c["gen"], ",".join(str(x) for x in c["args"]))


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/sortshapes.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    sys.path.insert(0, ROOT)
    cases = search()
    got = set().union(*(c["targets"] for c in cases))
    missing = sorted(REQUIRED - got)
    with open(FIXTURE, "w") as f:
        json.dump({"about": "tests/sortshapes.py --regen: blocks at the shapes where the rotation sort's round driver "
                            "branches, with the figures of the numpy profile", "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases, %d targets, missing: %s" % (len(cases), len(got), missing or "none"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
