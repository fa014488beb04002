"""One-stream Deflate encoder inputs placed at the PART SEAMS (CPU only: Python, numpy, the oracle).

A segment longer than a part is encoded in several launch sequences (df_encode_parts / df_encode_core in
rust-compression_amd/csrc/deflate_engine.hip, k_df_part_keep / k_df_part_tail in csrc/k_deflate.hip).  A seam hands on which
blocks are final, the step of the lazy parse at which the next part resumes, the literals of that step already out
(`skip`), the bits of a shared byte (`bit0`, `carry_byte`), 32 KiB of history, `decompress_len` and the container's sums.
The cases here put an input at every branch of that hand-over; DESIGN_deflate.md, "Parts at their seams", has the rule.

A case is a list of pieces (generator, arguments, action) fed with Flush / Finish (or one piece under Action::Run through
the zlib / gzip wrappers), an optional dictionary, and the kinds it is encoded as.  `build_pieces(case)` rebuilds the
bytes; `seams(case, oracle)` is the SEAM MODEL: from the oracle's blocks and LZSS codes alone it says where every part of
every segment starts, how many bytes it keeps, its `skip`, the bits it hands on and the types of the blocks on either
side; `hits(case, oracle)` recomputes the targets a case hits from that model; `REQUIRED` is the set the committed cases
must cover.  tests/golden/df_seams.json holds parameters, digests and the model's results, never bytes;
`python tests/dfseams.py --regen` rewrites it.  The library is never an input of the model.

Families:
  K  the keep rule of k_df_part_keep, `bstart[k] + guard <= n`: a block start 16 below the threshold (the nearest a plain
     input comes), and 1 below, on and 1 above it (a Flush carry of 65 520 / 65 519 / 65 518 trigram-free bytes moves the
     block starts of the next segment there; these are also the multi-part segments with dl0 > 0)
  E  ends: a segment of exactly PART + GUARD bytes (no seam), one byte more (one seam), the shortest last part the rule
     allows (GUARD + 1 - 65 535 bytes), a last part of exactly PART + GUARD bytes
  Z  the step: skip 0, 1 and 2, and for skip 1 and 2 a case where the fresh parse from the block start differs from the
     parse that went on (a part that resumed at the block instead of at the step writes another stream)
  B  the shared byte: every count of bits handed on, a stored first block at every bit0 (its header pads from a phase
     the host supplied), fixed and dynamic first blocks at bit0 != 0, a stored first block behind 1 and 2 literals that
     are already out, a stored, a fixed and a dynamic last kept block
  H  history at a part's first position: distance 32 768 (the first byte of the history; taken; and at the second and
     third position, where the lazy searches of the part's first step find it), 32 769 (not taken), a
     match of 258, a candidate just beyond / just inside the 255 chain entries the search looks at, and a short
     flushed segment over a dictionary (the history is the dictionary's tail and fewer than 32 768 stream bytes)
  M  many: two and three seams in a segment, a part that starts and ends inside a step, two multi-part segments with a
     Flush between them, a multi-part segment under Action::Run through ZlibEncoder and GZipEncoder

A FIXED last kept block takes forging: a kept block that is neither the first behind a Flush nor the stream's last holds
at least 65 535 - 257 bytes, so at least 254 codes, and is written fixed only if its symbol counts sit on the fixed
code's own lengths so closely that a dynamic header (some 400 bits) costs more than it saves.  `fixed_block` builds one:
6 048 codes, every literal / length symbol with the count its fixed code length implies, all 30 distance codes about
equally often (`B-last-fixed`: fixed 64 7xx bits against some 70 more for dynamic).
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

import dfshapes as D
import lzhshapes as LZ

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "df_seams.json")
TRACE_SAMPLE = os.path.join(HERE, "golden", "df_seams_trace.txt")

# ------------------------------------------------------------------------------------------------------- constants
PART = 1 << 20            # df_part_bytes() in deflate_engine.hip with BZ_DF_PART_MIB=1, its smallest value
GUARD = 0x10000 + 1024    # kPartGuard in deflate_engine.hip
WIN, MAX_MATCH = 0x8000, 258   # kWin, the longest match (k_deflate.h)
BLOCK = D.BLOCK_MAX       # kBlockMax: bytes of a block
CHAIN = 255               # candidates one search looks at (slidedict.rs: pos_count)
RUN, FLUSH, FINISH = 0, 1, 2
BANK = 3 * 85 ** 3        # bytes of dfshapes.counter

SHORTEST_LAST = GUARD + 1 - BLOCK   # a seam needs n > PART + GUARD, and bcut <= pos + PART + BLOCK


def _required():
    req = {"K plain: last kept starts 16 below", "K start at threshold-1 kept", "K start at threshold kept",
           "K start at threshold+1 left out", "K multi-part with dl0>0"}
    req |= {"E n=PART+GUARD no seam", "E n=PART+GUARD+1 one seam", "E shortest last part", "E last part=PART+GUARD"}
    req |= {"Z skip=0", "Z skip=1", "Z skip=2", "Z skip=1 fresh parse differs", "Z skip=2 fresh parse differs"}
    req |= {"B end_bits=%d" % b for b in range(8)} | {"B first stored bit0=%d" % b for b in range(8)}
    req |= {"B first fixed bit0!=0", "B first dynamic bit0!=0", "B first stored skip=1", "B first stored skip=2",
            "B last kept stored", "B last kept fixed", "B last kept dynamic"}
    req |= {"H dist 32768 taken", "H dist 32769 not taken", "H match 258 at part start", "H beyond chain not found",
            "H inside chain found", "H dist 32768 taken at position 1", "H dist 32768 taken at position 2", "H dict oldest visible byte taken", "H dict one byte further not taken"}
    req |= {"M two seams", "M three seams", "M part starts and ends with skip>0", "M flush between multi-part segments",
            "M run zlib", "M run gzip"}
    return frozenset(req)


REQUIRED = _required()


# ------------------------------------------------------------------------------------------------------- generators
def filler(n, start=0):
    """n bytes without a repeated trigram: dfshapes.counter, and behind its 1.8 MB a second bank with two of the three
    byte classes exchanged (its trigrams have class patterns the first bank never shows)"""
    out = bytearray()
    while n:
        bank, off = divmod(start, BANK)
        assert bank < 2
        k = min(n, BANK - off)
        c = np.frombuffer(D.counter(k, off), dtype=np.uint8).astype(np.int16)
        if bank:
            c = np.where(c > 170, c - 85, np.where(c > 85, c + 85, c))
        out += c.astype(np.uint8).tobytes()
        n -= k
        start += k
    return bytes(out)


LAZY_BACK, LAZY_DA, LAZY_DC = 2000, 41, 6000   # (S and its source stand at different phases of the filler)
CHAIN_T, CHAIN_Y = b"\0\0\1", bytes(range(2, 10))
SPICE, SPICE_BACK = 500, 100


def gen_script(ops, dict_=b""):
    """ops in order, each appending to the text so far:
    fill(to, shift)   filler up to length `to`, taken from filler position len + shift, with a match of 3 every 500 bytes
    noise(seed, n), zeros(n), copy(dist, L)   (L bytes from `dist` back), dict(off, L)   (L bytes of the dictionary
                      from `off` in front of its end)
    lazy(at, skip, L, differ, shift[, far, da])   a block start at `at` inside a step of the lazy parse: the step starts `skip`
                      bytes in front of it with a match of 3 (S), the match taken, of L bytes, starts at `at`
                      (source B, planted 2 000 bytes earlier).  differ: a candidate 3 - skip bytes behind `at` is one
                      byte longer than B's match -- the step cannot look there any more, a fresh parse from `at` does.
                      far: B stands exactly 32 768 bytes in front of `at`, the furthest the search at the part's
                      second or third position may reach; da: S is taken da bytes further back
    fixedblock(seed)  a block of 65 535 bytes that is written fixed (fixed_block)
    chain(at, k, shift)   at `at` a trigram with k nearer occurrences (each good for 5 bytes, and for 4 and 3 at the
                      next two positions) and one further back that is good for 11"""
    o = bytearray()

    def fill(to, shift):
        assert to >= len(o), (to, len(o))
        lo = len(o)
        o.extend(filler(to - lo, lo + shift))
        # a match of 3 every SPICE bytes: a block of literals alone is written dynamic WITHOUT a distance code by the
        # reference (dfshapes: the quirk), and zlib refuses that; with these every stream here inflates.  They stand
        # clear of every multiple of 65 535, so the blocks are cut as if all codes were literals
        for m in range(lo - lo % SPICE + SPICE // 2, to - 3, SPICE):
            if m >= max(lo, SPICE_BACK):
                o[m:m + 3] = o[m - SPICE_BACK:m - SPICE_BACK + 3]
    for op in ops:
        k = op[0]
        if k == "fill":
            fill(op[1], op[2])
        elif k == "noise":
            o.extend(np.random.RandomState(op[1]).bytes(op[2]))
        elif k == "zeros":
            o.extend(bytes(op[1]))
        elif k == "copy":
            for _ in range(op[2]):
                o.append(o[-op[1]])
        elif k == "dict":
            o.extend(dict_[len(dict_) - op[1]:len(dict_) - op[1] + op[2]])
        elif k == "lazy":
            _, at, skip, L, differ, shift = op[:6]
            far = len(op) > 6 and op[6]   # B exactly 32 768 in front of `at`: the window's edge for the lazy search there
            assert not (far and differ)
            plant = at - WIN if far else at - skip - LAZY_BACK
            fill(plant, shift)
            a, c = plant - LAZY_DA - (op[7] if len(op) > 7 else 0), plant - LAZY_DC
            S, tail = bytes(o[a:a + 3]), bytes(o[c:c + L + 1])
            if o[a + 3] == tail[0]:
                raise ValueError("the match of 3 would go on")
            if differ:
                cut = L - (3 - skip)
                o.extend(S[skip:] + tail[:cut] + bytes([tail[cut] ^ 0x80]))
            else:
                o.extend(S[skip:] + tail)
            if far:   # (S's first source is out of the window by then: a second one)
                fill(plant + 3000, shift)
                o.extend(S)
            fill(at - skip, shift)
            o.extend(S + tail)
        elif k == "chain":
            _, at, nk, shift = op
            far = CHAIN_T + CHAIN_Y
            fill(at - 8 - 7 * nk - len(far) - 4, shift)
            o.extend(far)
            fill(len(o) + 4, shift)
            for i in range(nk):
                o.extend(CHAIN_T + CHAIN_Y[:2] + bytes([10 + i // 200, 10 + i % 200]))
            fill(at, shift)
            o.extend(far)
        elif k == "fixedblock":
            o.extend(fixed_block(bytes(o[-(WIN + 200):]), op[1]))
        else:
            raise ValueError(k)
    return bytes(o)


FIXED_G = 48   # a symbol whose fixed code has l bits occurs FIXED_G * 2^(13 - l) / 32 times: 24, 12 or 48


def fixed_block(hist, seed):
    """A whole block of exactly 65 535 bytes behind the history `hist` that the cost rule
    writes FIXED: its symbol counts sit on the lengths of the fixed code -- every literal below 144 occurs 24 times,
    every one from 144 up 12 times, every length code of 7 bits 48 times and of 8 bits 24 times, every distance code
    about 42 times -- so a dynamic code saves next to nothing and its header (some 400 bits) is not earned.  Matches are
    planted with dfshapes.Builder (fresh sources, literals that make no old trigram); distances 1 .. 4 are periods."""
    b = D.Builder(seed)
    for v in hist:
        b._push(v, 1)
    h0 = len(b.out)
    r = D.Rng(seed + 11)
    g = FIXED_G
    pool = [v for v in range(144) for _ in range(g // 2)] + [v for v in range(144, 256) for _ in range(g // 4)]
    r.shuffle(pool)
    lens = []
    for c in range(29):
        hi = D._LBASE[c] + (1 << D._LEXT[c]) - 1 if c < 28 else 258
        lens += [[c, min(hi, 258 if c == 28 else 257)] for _ in range(g if c < 23 else g // 2)]
    # lengths give way inside their codes, the longest codes first, until the block has exactly BLOCK bytes
    over = len(pool) + sum(x[1] for x in lens) - BLOCK
    for x in sorted(lens, key=lambda x: -x[0]):
        cut = min(over, x[1] - D._LBASE[x[0]])
        x[1] -= cut
        over -= cut
    assert over == 0
    # distance codes, 42 of each at most: 1 .. 4 are periods; the longest matches take the smallest code that holds them
    quota = [42] * 30
    lens.sort(key=lambda x: -x[1])
    plan = []
    per = [x for i, x in enumerate(lens) if i % 8 == 3][:4 * 39]   # (156 matches of all lengths for distances 1 .. 4)
    perset = set(id(x) for x in per)
    for i, x in enumerate(per):
        plan.append([x, i % 4])
    for x in lens:
        if id(x) in perset:
            continue
        c = next(c for c in range(4, 30) if quota[c] and D.dist_lo(c) >= x[1] + 2)
        quota[c] -= 1
        plan.append([x, c])
    r.shuffle(plan)
    for i, (x, c) in enumerate(plan):
        left = len(plan) - i
        k = min(len(pool), max(1, (len(pool) - 200) // left)) if pool else 0
        if k:
            b.lits([pool.pop() for _ in range(k)])
        L = x[1]
        if c < 4:
            period = [pool.pop() for _ in range(min(c + 1, len(pool)))] or [1]
            b.plant(L, c + 1, period + list(range(256)))
        else:
            for attempt in range(12):
                try:
                    b.ref_code(L, c)
                    break
                except ValueError:
                    pass
                try:   # (a source that another match copied already: the nearest copy is found first and is as long)
                    b.ref_code(L, c, fresh=False)
                    break
                except ValueError:   # (the few sources of a short distance all begin badly: one more literal moves them)
                    b.lits([pool.pop()])
            else:
                raise ValueError("no source at distance code %d" % c)
    if pool:
        b.lits(pool)
    out = bytes(b.out[h0:])
    if len(out) != BLOCK:
        raise ValueError("the forged block has %d bytes" % len(out))
    return out


def gen_noise(seed, n):
    return np.random.RandomState(seed).bytes(n)


GENS = {"script": gen_script, "filler": lambda n, start=0: filler(n, start), "noise": gen_noise, "text": D.gen_text}

_built = {}


def build_dict(case):
    d = case.get("dict")
    return GENS[d[0]](*d[1]) if d else b""


def build_pieces(case):
    """-> [(bytes, action)]"""
    key = json.dumps([case.get("dict"), case["pieces"]])
    if key not in _built:
        if len(_built) > 3:
            _built.clear()
        dict_ = build_dict(case)
        out = []
        for gen, args, act in case["pieces"]:
            out.append((gen_script(args, dict_) if gen == "script" else GENS[gen](*args), act))
        _built[key] = out
    return _built[key]


def digest(case):
    h = hashlib.sha256(build_dict(case))
    for data, act in build_pieces(case):
        h.update(b"|%d|%d|" % (len(data), act))
        h.update(data)
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------- the seam model
# named faults of the MODEL; tests/test_dfseams.py shows that each one changes the seams of some committed case.
# (Bit counts taken without the flushed segment's bits are not among them: every flushed piece here is shifted until its
# Flush pads nothing -- only such a stream inflates -- and then that fault changes no count modulo 8.)
FAULTS = ("lt_for_le", "guard_0x10000", "skip_ignored", "carry_not_subtracted", "last_part_lt", "keep_by_block_end",
          "threshold_from_segment_start", "skip_added", "bits_at_last_kept_block")


class Facts:
    """what the oracle says of one case: per segment the bytes, the 32 KiB in front, the blocks
    (tokens, decompress_len at the close, type, bits), the stream length in front and behind, the LZSS codes and
    their start positions"""
    pass


def facts(case, oracle):
    f = Facts()
    f.dict = build_dict(case)
    f.segs = []
    e = oracle.DeflateEncoder(f.dict)
    hist = f.dict[-(WIN + 8):]
    nb0 = 0
    for data, act in build_pieces(case):
        s = Facts()
        s.data, s.act, s.hist = data, act, hist
        s.out0 = len(e.output())
        # (a piece under Action::Run is one piece through a wrapper: its seams are those of the whole input)
        e.feed(data, FINISH if act == RUN else act)
        allb = e.blocks()
        s.blocks = [tuple(int(x) for x in b) for b in allb[nb0:]]
        nb0 = len(allb)
        s.out1 = len(e.output())
        assert (8 * s.out0 + sum(b[3] for b in s.blocks) + 7) // 8 == s.out1, "a block's bits do not hold its padding"
        s.toks = oracle.lzss_tokens_raw(data, hist[-WIN:])
        s.tstart = np.concatenate([[0], np.cumsum(np.where(s.toks[:, 0] > 0, s.toks[:, 0], 1).astype(np.int64))])
        assert int(s.tstart[-1]) == len(data) and len(s.toks) == sum(b[0] for b in s.blocks)
        f.segs.append(s)
        hist = (hist + data)[-(WIN + 8):]
    f.stream = e.output()
    return f


def _provable_step_start(toks, t):
    """code t is the first of a step: t is the segment's first code, or the code in front is a reference (a step ends
    with its reference), or codes t-1, t, t+1 are all literals (a step is [0..2 literals] reference or one literal:
    were literal t-1 one of a step's leading literals, t or t+1 would be that step's reference)"""
    if t == 0 or toks[t - 1, 0] != 0:
        return True
    return t + 1 < len(toks) and toks[t - 1, 0] == 0 and toks[t, 0] == 0 and toks[t + 1, 0] == 0


def step_of(s, bcut):
    """-> (skip, steps): the step of the lazy parse that holds the code at bcut, from the restatement of the step in
    tests/lzhshapes.py (window 0x8000, longest match 258) started at a provable step start in front of bcut; its codes
    are asserted equal to the oracle's from there to bcut.  The oracle's codes carry no step boundaries."""
    toks, tstart = s.toks, s.tstart
    ti = int(np.searchsorted(tstart, bcut))
    assert int(tstart[ti]) == bcut, "a block does not start at a code"
    t = ti
    while not _provable_step_start(toks, t):
        t -= 1
    p0 = int(tstart[t])
    lo = p0 - (WIN + 1)
    hi = min(len(s.data), bcut + 1024)
    front = s.hist[lo:] if lo < 0 else b""
    buf = front + s.data[max(lo, 0):hi]
    off = len(front) if lo < 0 else -lo   # buffer index = position + off
    steps = LZ.naive_steps(buf, WIN, MAX_MATCH, start=p0 + off, stop=bcut + off + 1)
    want = [("ref", int(l), int(p)) if l else ("sym", int(p)) for l, p in toks[t:t + len(LZ.steps_tokens(buf, steps))]]
    assert LZ.steps_tokens(buf, steps) == want, "the restated step does not give the oracle's codes"
    p, li = steps[-1][0] - off, steps[-1][1]
    assert p <= bcut <= p + li
    return bcut - p, steps


def seams(case, oracle, fault=None, f=None):
    """-> [[segment, pos_k, kept bytes = pos_{k+1} - pos_k, skip, end_bits, type of the last kept block, type of the
    first block of part k + 1, blocks kept]] for every part that is not its segment's last, then
    [segment, pos_last, n - pos_last, 0, 0, -1, -1, blocks of the last part] for every multi-part segment"""
    f = f or facts(case, oracle)
    guard = 0x10000 if fault == "guard_0x10000" else GUARD
    rows, carry = [], 0
    for si, s in enumerate(f.segs):
        n = len(s.data)
        starts, bitpos, p = [], [], 0
        bit = 8 * s.out0
        for i, (ntok, nbytes, btype, bits) in enumerate(s.blocks):
            starts.append(p)
            bitpos.append(bit)
            # the `bytes` of a block is decompress_len at its close: behind a Flush the first block's holds the carry
            p += nbytes - (carry if i == 0 and fault != "carry_not_subtracted" else 0)
            bit += bits
        assert fault or p == n
        starts.append(p)
        if s.blocks:
            carry = s.blocks[-1][1]
        pos, first, k = 0, 0, 0
        while (n - pos >= PART + guard) if fault == "last_part_lt" else (n - pos > PART + guard):
            thr = (k + 1) * PART if fault == "threshold_from_segment_start" else pos + PART
            if fault == "keep_by_block_end":
                keep = [j for j in range(len(s.blocks)) if starts[j + 1] <= thr]
            elif fault == "lt_for_le":
                keep = [j for j in range(len(s.blocks)) if starts[j] < thr]
            else:
                keep = [j for j in range(len(s.blocks)) if starts[j] <= thr]
            j = keep[-1]
            bcut = starts[j + 1]
            try:
                skip = step_of(s, bcut)[0]
            except (AssertionError, IndexError):
                if not fault:
                    raise
                skip = 0   # (a faulty rule may put bcut where no code starts: its rows stay well formed)
            nxt = bcut - skip
            if fault == "skip_ignored":
                nxt = bcut
            elif fault == "skip_added":
                nxt = bcut + skip
            eb = bitpos[j if fault == "bits_at_last_kept_block" else j + 1] & 7
            rows.append([si, pos, nxt - pos, skip, eb, s.blocks[j][2], s.blocks[j + 1][2], j + 1 - first])
            pos, first, k = nxt, j + 1, k + 1
        if k:
            rows.append([si, pos, n - pos, 0, 0, -1, -1, len(s.blocks) - first])
    return rows


# ------------------------------------------------------------------------------------------------------------- hits
def _tok_at(s, q):
    t = int(np.searchsorted(s.tstart, q))
    if t >= len(s.toks) or int(s.tstart[t]) != q:
        return None
    return int(s.toks[t, 0]), int(s.toks[t, 1])


def hits(case, oracle, f=None):
    """-> (the required targets this case hits, the model's rows, the oracle's facts)"""
    f = f or facts(case, oracle)
    rows = seams(case, oracle, f=f)
    h = set()
    carry = 0
    for si, s in enumerate(f.segs):
        n = len(s.data)
        mine = [r for r in rows if r[0] == si]
        nseam = max(len(mine) - 1, 0)
        if n == PART + GUARD and not mine:
            h.add("E n=PART+GUARD no seam")
        if n == PART + GUARD + 1 and nseam == 1:
            h.add("E n=PART+GUARD+1 one seam")
        if nseam == 2:
            h.add("M two seams")
        if nseam == 3:
            h.add("M three seams")
        if mine:
            last = mine[-1]
            if last[2] == SHORTEST_LAST:
                h.add("E shortest last part")
            if last[2] == PART + GUARD:
                h.add("E last part=PART+GUARD")
            if carry:
                h.add("K multi-part with dl0>0")
            if si and len([r for r in rows if r[0] == si - 1]) > 1 and f.segs[si - 1].act == FLUSH:
                h.add("M flush between multi-part segments")
            if s.act == RUN:
                h |= {"M run zlib", "M run gzip"} & {"M run %s" % {1: "zlib", 2: "gzip"}[k] for k in case["kinds"] if k}
        # block starts of this segment
        starts, p = [], 0
        for i, b in enumerate(s.blocks):
            starts.append(p)
            p += b[1] - (carry if i == 0 else 0)
        first = 0
        for r in mine[:-1]:
            _, pos, kept, skip, eb, t_last, t_first, nkept = r
            bcut = pos + kept + skip
            j = starts.index(bcut)
            rel_last, rel_cut = starts[j - 1] - (pos + PART), bcut - (pos + PART)
            if rel_last == -16 and carry == 0 and pos == 0:
                h.add("K plain: last kept starts 16 below")
            if rel_last == -1:
                h.add("K start at threshold-1 kept")
            if rel_last == 0:
                h.add("K start at threshold kept")
            if rel_cut == 1:
                h.add("K start at threshold+1 left out")
            h.add("Z skip=%d" % skip)
            h.add("B end_bits=%d" % eb)
            h.add("B last kept %s" % ("stored", "fixed", "dynamic")[t_last])
            if t_first == 0:
                h.add("B first stored bit0=%d" % eb)
                if skip:
                    h.add("B first stored skip=%d" % skip)
            elif eb:
                h.add("B first %s bit0!=0" % ("fixed" if t_first == 1 else "dynamic"))
            if skip:
                # the fresh parse from bcut against the parse that went on
                full = (s.hist + s.data[:bcut])[-WIN:]
                fresh = oracle.lzss_tokens_raw(s.data[bcut:bcut + 1500], full)
                ti = int(np.searchsorted(s.tstart, bcut))
                m = int(np.searchsorted(np.cumsum(np.where(fresh[:, 0] > 0, fresh[:, 0], 1)), 600))
                if not np.array_equal(fresh[:m], s.toks[ti:ti + m]):
                    h.add("Z skip=%d fresh parse differs" % skip)
                if pos and [x for x in mine if x[1] + x[2] == pos and x[3]]:
                    h.add("M part starts and ends with skip>0")
            # history at the next part's first position
            q = pos + kept
            hd = s.hist + s.data[:q + 600]
            o = len(s.hist)
            tok = _tok_at(s, q)
            if tok and tok[0] and tok[1] + 1 == WIN and q >= WIN:
                h.add("H dist 32768 taken")
            tok2 = _tok_at(s, bcut)
            if skip and tok2 and tok2[0] and tok2[1] + 1 == WIN:   # (found by the lazy search of the part's first step)
                h.add("H dist 32768 taken at position %d" % skip)
            if tok and not tok[0] and q > WIN and hd[o + q:o + q + 8] == hd[o + q - WIN - 1:o + q - WIN - 1 + 8]:
                h.add("H dist 32769 not taken")
            if tok and tok[0] == MAX_MATCH:
                h.add("H match 258 at part start")
            if tok and q >= WIN:
                T = hd[o + q:o + q + 3]
                occ, at = [], hd.find(T, o + q - WIN)
                while 0 <= at < o + q:
                    occ.append(at)
                    at = hd.find(T, at + 1)

                def mlen(x):
                    ln = 0
                    while ln < MAX_MATCH and hd[x + ln] == hd[o + q + ln]:
                        ln += 1
                    return ln
                if len(occ) > CHAIN:
                    near = max(mlen(x) for x in occ[-CHAIN:])
                    if mlen(occ[-CHAIN - 1]) > near and tok[0] == near:
                        h.add("H beyond chain not found")
                if len(occ) == CHAIN:
                    near = max(mlen(x) for x in occ[1:])
                    if mlen(occ[0]) > near and tok[0] == mlen(occ[0]):
                        h.add("H inside chain found")
        # a multi-part segment over a dictionary and fewer than 32 768 stream bytes
        prior = sum(len(x.data) for x in f.segs[:si])
        if mine and f.dict and 0 < prior < WIN and len(f.dict) + prior > WIN:
            tok = _tok_at(s, 0)
            src = len(s.hist) - WIN
            if tok and tok[0] and tok[1] + 1 == WIN:
                h.add("H dict oldest visible byte taken")
            if tok and not tok[0] and s.hist[src - 1:src + 7] == s.data[:8]:
                h.add("H dict one byte further not taken")
        if s.blocks:
            carry = s.blocks[-1][1]
    return h & REQUIRED, rows, f


# ------------------------------------------------------------------------------------------------------ the streams
def streams(case, oracle, f):
    """what the oracle writes: per kind [length, SHA-256] of the one-shot stream (one Finish piece), per piece of a
    flushed case the bytes the Inflater yields at that piece, per kind the wrapper's bytes under Action::Run"""
    pieces = build_pieces(case)
    dict_ = f.dict
    out = {}

    def rec(b):
        return [len(b), hashlib.sha256(b).hexdigest()]
    if len(pieces) == 1 and pieces[0][1] == FINISH:
        for k in case["kinds"]:
            out["kind%d" % k] = rec(oracle.deflate_encode(pieces[0][0], k, dict_))
    elif pieces[0][1] == RUN:
        for k in case["kinds"]:
            out["run%d" % k] = rec(oracle.WrapperEncoder(k, dict_).encode_iter(pieces[0][0], RUN))
    else:
        e = oracle.DeflateEncoder(dict_)
        got, done = [], 0
        for data, act in pieces:
            e.feed(data, act)
            o = e.output()
            got.append(rec(o[done:]))
            done = len(o)
        out["pieces"] = got
    return out


def block_counts(f):
    """[blocks, stored, fixed, dynamic] over all segments"""
    t = [b[2] for s in f.segs for b in s.blocks]
    return [len(t), t.count(0), t.count(1), t.count(2)]


# ----------------------------------------------------------------------------------------------------------- search
B17 = 17 * BLOCK   # with trigram-free filler in front, the first block left out of part 0 starts here
N1 = PART + GUARD + 1


def _case(name, family, pieces, kinds=(0, 1, 2), dict_=None):
    c = {"name": name, "family": family, "kinds": list(kinds), "pieces": pieces}
    if dict_:
        c["dict"] = dict_
    return c


def _one(ops):
    return [["script", ops, FINISH]]


def candidates():
    """every case the search proposes, in order; search() keeps those that add a target"""
    yield _case("K-plain", "K", _one([["fill", N1, 0]]))
    # (a Flush pads to the next byte and writes no marker: the stream inflates only where that padding is empty, so the
    # filler of every flushed piece is shifted until it is)
    for fl in (65520, 65519, 65518):
        for shift in range(64):
            yield _case("K-flush%d" % fl, "K", [["script", [["fill", fl, shift]], FLUSH],
                                               ["script", [["fill", N1, fl + shift]], FINISH]], kinds=(0,))
    yield _case("E-guard", "E", _one([["fill", PART + GUARD, 0]]))
    yield _case("E-last-full", "E", _one([["fill", B17 + PART + GUARD, 0]]))
    for skip in (1, 2):
        for differ in (1, 0):
            for L in (12, 13, 20, 33):
                yield _case("Z-skip%d-%s-L%d" % (skip, "differ" if differ else "same", L), "Z",
                            _one([["lazy", B17, skip, L, differ, 0], ["fill", N1, 0]]))
    # B: the phase of the shared byte is steered by where the filler in front starts
    for shift in range(0, 48):
        yield _case("B-stored-shift%d" % shift, "B", _one([["fill", B17, shift], ["noise", 7, BLOCK], ["fill", B17 + BLOCK + 1100, shift]]))
    for shift in range(0, 6):
        yield _case("B-fixed-shift%d" % shift, "B", _one([["fill", B17, shift], ["zeros", N1 - B17]]))
    for skip in (1, 2):
        for L in (5, 8):
            yield _case("B-stored-skip%d-L%d" % (skip, L), "B",
                        _one([["lazy", B17, skip, L, 0, 0], ["noise", 9, BLOCK - 64], ["fill", B17 + BLOCK + 1100, 0]]))
    yield _case("B-last-stored", "B", _one([["fill", 16 * BLOCK, 0], ["noise", 11, BLOCK], ["fill", N1 + BLOCK, 0]]))
    for seed in range(1, 9):
        yield _case("B-last-fixed", "B", _one([["fill", 16 * BLOCK, 0], ["fixedblock", seed], ["fill", N1, 0]]))
    yield _case("H-32768", "H", _one([["fill", B17, 0], ["copy", WIN, 20], ["fill", N1, 0]]))
    for skip in (1, 2):
        for da in range(12):   # (S from another place until the step comes out as designed)
            yield _case("H-32768-lazy%d" % skip, "H", _one([["lazy", B17, skip, 20, 0, 0, 1, da], ["fill", N1, 0]]))
    yield _case("H-32769", "H", _one([["fill", B17, 0], ["copy", WIN + 1, 20], ["fill", N1, 0]]))
    yield _case("H-258", "H", _one([["fill", B17, 0], ["copy", 5000, 258], ["fill", N1, 0]]))
    yield _case("H-chain255", "H", _one([["chain", B17, CHAIN, 0], ["fill", N1, 0]]))
    yield _case("H-chain254", "H", _one([["chain", B17, CHAIN - 1, 0], ["fill", N1, 0]]))
    for back in (0, 1):
        for shift in range(64):
            yield _case("H-dict-%d" % back, "H",
                        [["script", [["fill", 1000, shift]], FLUSH],
                         ["script", [["dict", WIN - 1000 + back, 24], ["fill", N1 + 64, 2000]], FINISH]],
                        kinds=(0,), dict_=["noise", [5, 40000]])
    yield _case("M-two", "M", _one([["fill", B17 + PART + GUARD + 1, 0]]))
    yield _case("M-three", "M", _one([["fill", 34 * BLOCK + PART + GUARD + 1, 0]]))
    yield _case("M-skip-both", "M", _one([["lazy", B17, 2, 12, 1, 0], ["lazy", 34 * BLOCK, 1, 13, 1, 0],
                                          ["fill", 34 * BLOCK + N1, 0]]))
    for shift in range(64):
        yield _case("M-flush-two", "M", [["script", [["fill", N1, shift]], FLUSH],
                                         ["script", [["fill", N1 + 5, N1 + shift]], FINISH]], kinds=(0,))
    yield _case("M-run", "M", [["script", [["fill", N1 + 40000, 0]], RUN]], kinds=(1, 2))


def record(case, oracle):
    f = facts(case, oracle)
    if any(s.act == FLUSH and sum(b[3] for b in s.blocks) % 8 for s in f.segs):
        raise ValueError("the Flush pads")
    got, rows, f = hits(case, oracle, f)
    case["targets"] = sorted(got)
    case["sha256"] = digest(case)
    case["bytes"] = sum(len(s.data) for s in f.segs)
    case["seams"] = rows
    case["streams"] = streams(case, oracle, f)
    case["blocks"] = block_counts(f)
    return got


def search(oracle, log=print):
    cases, have = [], set()
    for case in candidates():
        if any(c["name"] == case["name"] for c in cases):
            continue   # (the same case with another shift)
        try:
            got = record(case, oracle)
        except (ValueError, AssertionError) as e:
            log("dropped %s: %r" % (case["name"], e))
            continue
        if not got - have:
            continue
        have |= got
        cases.append(case)
    kept = []
    for i, case in enumerate(cases):
        others = set().union(*([set(x["targets"]) for x in kept] + [set(x["targets"]) for x in cases[i + 1:]] + [set()]))
        if set(case["targets"]) - others:
            kept.append(case)
    return kept


def runs_after(case):
    """the cases that also run with BZ_DF_CUTS=after (the block chain behind the marking kernel): every case that hits a
    target of family K, Z or B, whatever family it was built for -- that is every case with a seam"""
    return any(t[:2] in ("K ", "Z ", "B ") for t in case["targets"])


def load():
    with open(FIXTURE) as fh:
        return json.load(fh)


def case_id(c):
    return c["name"]


# ------------------------------------------------------------------------------------------------------- the trace
_TRACE = re.compile(r"deflate part (\d+): input \[(\d+), \+(\d+)\) of (\d+), kept (\d+) bytes of it, (\d+) stream bytes, "
                    r"(\d+) bits handed on, (\d+) blocks")


def parse_trace(text):
    """the BZ_DF_TRACE lines of df_encode_parts -> [(part, pos, len, n, kept, stream bytes, bits handed on, blocks)];
    a line that names a deflate part and does not parse is an error"""
    out = []
    for line in text.splitlines():
        if "deflate part" not in line:
            continue
        m = _TRACE.search(line)
        if not m:
            raise ValueError("unreadable trace line: %r" % line)
        out.append(tuple(int(x) for x in m.groups()))
    return out


def trace_calls(parts):
    """split parsed lines into calls (a call's parts count from 0) -> [[(pos, kept, bits, blocks), ...]]"""
    calls = []
    for k, pos, ln, n, kept, sb, bits, nb in parts:
        if k == 0:
            calls.append([])
        calls[-1].append((pos, kept, bits, nb))
    return calls


def model_calls(case):
    """the recorded seams in the trace's form, one call per multi-part segment"""
    calls = {}
    for si, pos, kept, skip, eb, tl, tf, nb in case["seams"]:
        calls.setdefault(si, []).append((pos, kept, eb, nb))
    return [calls[k] for k in sorted(calls)]


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/dfseams.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    sys.path.insert(0, ROOT)
    from oracle import oracle
    cases = search(oracle)
    got = set().union(*(c["targets"] for c in cases))
    missing = sorted(REQUIRED - got)
    with open(FIXTURE, "w") as fh:
        json.dump({"about": "tests/dfseams.py --regen: one-stream Deflate encoder inputs at the part seams (parameters, "
                            "digests and the seam model's results only)",
                   "part": PART, "guard": GUARD, "cases": cases}, fh, separators=(",", ":"))
        fh.write("\n")
    print("%d cases, %d targets, %d bytes in all, missing: %s" % (len(cases), len(got), sum(c["bytes"] for c in cases),
                                                                   missing or "none"))
    for c in cases:
        print("  %-28s %8d bytes  %s" % (c["name"], c["bytes"], ", ".join(c["targets"])))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
