"""Encoder inputs placed at the block shapes where the encode kernels branch (CPU only: Python, numpy, the oracle).

Each case is a small dict -- a generator name, its seed and lengths -- plus the oracle's per-block figures for the
bytes it builds and the targets it was chosen to hit.  `build(case)` rebuilds the bytes; `hits(case, oracle)`
recomputes from the oracle which targets the bytes really hit; `REQUIRED` is the set the committed cases must cover.
Exact targets come from searches over seeds and lengths, too slow to repeat in every run, so their results are
committed as tests/golden/enc_shapes.json; `python tests/encshapes.py --regen` rewrites it.

The switches (rust-compression_amd/csrc):
  A  table count from mtf_count (<200/600/1200/2400): k_huff.hip k_huffman and huff_group_num
  B  selector count ceil(mtf_count/50), the last short group, 256-group sweep steps and 2816-group trips
  C  the MTF rank kernel's two instances by alphabet (kMtfSmallAlpha = 96) and by batch size (kMtfSubBlocks = 16);
     512-symbol chunks in 32-chunk groups
  D  zero runs of MTF ranks against the 8192-symbol tiles of the ZLE stage
  E  sort tiles (8192 symbols) and the RLE1 block limit 100000*level-19
  F  the table kernel's two forms by batch size (kTabPipeBlocks = 320) and length-limited tables
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "enc_shapes.json")

FIG = ("nblock", "mtf_count", "in_use_count", "group_num", "n_selectors", "max_len", "lm_tables")
TILE = 8192  # ZLE and sort tiles (bzgpu.h kSortTile)
G = 50  # symbols per selector group

# ---------------------------------------------------------------------------------------------------------- targets
A_MTF = (199, 200, 599, 600, 1199, 1200, 2399, 2400)
A_USE = (4, 60, 96, 97, 256)
B_SEL = (1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 2816, 2817, 5632, 5633)
C_USE = (1, 2, 3, 48, 49, 95, 96, 97, 98, 128, 129, 255, 256)
C_NBLOCK = (511, 512, 513, 1023, 1024, 1025, 16383, 16384, 16385, 32767, 32768, 32769)
D_RUNS = tuple(sorted({1, 2, 3} | {(1 << j) + d for j in range(2, 15) for d in (-2, -1, 0, 1)}))
E_RUNS = (4, 100, 255)  # (RLE1 writes each as 5 bytes: 4 of them and a count)
LEVELS = (1, 2, 9)


def limit(level):
    return 100000 * level - 19


def _required():
    req = set()
    for m in A_MTF:
        for u in A_USE:
            if u < m:  # (256 symbols in use make at least ~256 non-zero ranks: mtf_count < 256 is out of reach)
                req.add("A mtf=%d in_use=%d" % (m, u))
    for m in (1199, 1200, 2399, 2400):  # the smallest alphabet that reaches 5 and 6 tables (one symbol makes no ranks)
        req.add("A mtf=%d in_use=2" % m)
    for s in B_SEL:
        req |= {"B mtf=%d" % (G * s), "B mtf=%d" % (G * s + 1)}
    req |= {"B last=1", "B last=49", "B max_selectors"}
    for u in C_USE:
        req |= {"C in_use=%d" % u, "C batch17 in_use=%d" % u}
    req |= {"C nblock=%d" % n for n in C_NBLOCK}
    req.add("C batch17 96|97")
    for r in D_RUNS:
        req |= {"D run=%d ends" % r, "D run=%d starts" % r}
        if r > 1:
            req.add("D run=%d crosses" % r)
    req |= {"D run>tile", "D run>2tiles", "D run@eob"}
    for lv in LEVELS:
        for d in (-1, 0, 1, 4):
            req.add("E level=%d len=L%+d" % (lv, d))
        for rl in E_RUNS:
            for rel in ("ends", "crosses", "starts"):
                req.add("E level=%d run=%d %s" % (lv, rl, rel))
    # (a table count below 6 means mtf_count < 2400, and a Huffman tree deeper than 17 needs a total weight of at least
    # Fibonacci(20) = 6765: the length-limited path is reachable at 6 tables only)
    req |= {"F 321 blocks", "F lm group_num=6", "F group cost>=840"}
    return frozenset(req)


REQUIRED = _required()


# ------------------------------------------------------------------------------------------------------- generators
def norun(seed, n, k, base=0):
    """n bytes over the k values base..base+k-1 (mod 256), all k of them in the first min(n, k) bytes, and no two
    neighbours of an aligned pair equal, nor the last two: no run of 4 equal bytes anywhere, even where two such
    pieces meet, so RLE1 leaves them alone and in_use is exactly k (n >= k)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, k, n, dtype=np.int64)
    if k > 1:
        h = min(n, k)
        x[:h] = rng.permutation(k)[:h]
        # odd positions: differ from the even one before them
        odd = np.arange(1, n, 2)
        odd = odd[odd >= h]
        x[odd] = (x[odd - 1] + 1 + rng.integers(0, k - 1, odd.size)) % k
        if n >= 2 and x[n - 1] == x[n - 2]:
            x[n - 1] = (x[n - 2] + 1) % k
    else:
        x[:] = 0
    return ((x + base) % 256).astype(np.uint8).tobytes()


def mono(byte, n):
    """in_use = 1: n runs of 255 bytes 0xfb (RLE1 cuts runs at 4 + 251 and writes each as fb fb fb fb fb), or for
    byte 0 the four zero bytes 0 0 0 0 (RLE1: 0 0 0 0 0) -- the count byte is the run's own byte"""
    return b"\xfb" * 255 * n if byte == 0xFB else b"\0" * 4


def zrun(seed, p, N):
    """p bytes below 0xf0, then (f0 f1)*N.  The prefix's rotations sort first; the f0 rotations put f1*(N-1) then
    the prefix's last byte into the last column, the f1 rotations f0*N: zero runs of N-2 ranks from p+1 and of
    N-1 ranks from p+N+1 to the block's end."""
    return norun(seed, p, 0xF0) + b"\xf0\xf1" * N


def cutrun(seed, level, start, rl):
    """a run of rl bytes 0xfa whose RLE1 image (5 bytes) starts at RLE1 position `start`, in norun bytes < 0xc8"""
    return norun(seed, start, 200) + b"\xfa" * rl + norun(seed + 1, 40, 200)


def batch(seed, parts, level=1):
    """one block per k in parts: norun(k) of exactly limit(level) bytes, or for k = 1 (last only) mono(0xfb, 10000)"""
    L = limit(level)
    return b"".join(mono(0xFB, 10000) if k == 1 else norun(seed + i, L, k, base=7 * i) for i, k in enumerate(parts))


def textmix(seed, n):
    """n bytes of corpus text, then random bytes up to the level-9 block limit: the text's tables take the
    length-limited path (max_len 17), and groups of the random part cost up to about 50 x 17 bits under them"""
    import corpus
    return corpus.chapter(seed, n) + norun(seed, limit(9) - n, 256)


GENS = {"norun": norun, "mono": mono, "zrun": zrun, "cutrun": cutrun, "batch": batch, "textmix": textmix}


def build(case):
    return GENS[case["gen"]](*case["args"])


# --------------------------------------------------------------------------------------------------------- figures
def figures(oracle, data, level):
    stream, st = oracle.encode(data, level, with_stats=True)
    return stream, [{k: int(b[k]) for k in FIG} for b in st]


def zero_runs(oracle, block):
    """maximal runs of MTF rank 0 in the block's last column, as (start, end) with end exclusive.  A rank is 0
    exactly when the symbol equals the one before it (position 0: when it is the smallest symbol in use)."""
    b = np.frombuffer(block, dtype=np.uint8)
    sa = np.asarray(oracle.bwt(block), dtype=np.int64)
    L = b[(sa - 1) % len(b)]
    z = np.empty(len(b), dtype=bool)
    z[0] = L[0] == b.min()
    z[1:] = L[1:] == L[:-1]
    d = np.diff(np.concatenate(([0], z.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def run_relations(start, end):
    """how the zero run [start, end) lies against the tile edges: 'ends' (its last rank is a tile's last),
    'starts' (its first is a tile's first), 'crosses' (an edge lies strictly inside it)"""
    rel = set()
    if end % TILE == 0:
        rel.add("ends")
    if start % TILE == 0 and start:
        rel.add("starts")
    if (end - 1) // TILE * TILE > start:
        rel.add("crosses")
    return rel


def max_group_cost(stream):
    """the largest cost in bits of a full 50-symbol group under a 17-bit table of the stream's own (final) tables:
    k_huff_sweep sums such costs in 10-bit fields, and 50 x 17 = 850 is the most there can be"""
    import bzforge
    best = 0
    for b in bzforge.parse(stream)[0].blocks:
        sym = np.asarray(b.symbols)
        full = len(sym) // G
        for lens in b.lengths:
            if max(lens) == 17 and full:
                best = max(best, int(np.asarray(lens)[sym[:full * G]].reshape(full, G).sum(axis=1).max()))
    return best


def hits(case, oracle, data=None):
    """the targets this case's bytes hit, recomputed from the oracle; also returns the stream and the figures"""
    data = build(case) if data is None else data
    fam, level = case["family"], case["level"]
    stream, fig = figures(oracle, data, level)
    h = set()
    f0 = fig[0] if fig else None
    if fam == "A" and len(fig) == 1:
        h.add("A mtf=%d in_use=%d" % (f0["mtf_count"], f0["in_use_count"]))
    elif fam == "B" and len(fig) == 1:
        m = f0["mtf_count"]
        h.add("B mtf=%d" % m)
        if m % G in (1, 49):
            h.add("B last=%d" % (m % G))
        if level == 9 and f0["nblock"] >= limit(9) and f0["in_use_count"] == 256 and f0["n_selectors"] > 17900:
            h.add("B max_selectors")
    elif fam == "C":
        if len(fig) <= 16:
            for b in fig:
                h |= {"C in_use=%d" % b["in_use_count"], "C nblock=%d" % b["nblock"]}
        if len(fig) == 17 and level == 1:
            use = [b["in_use_count"] for b in fig]
            h |= {"C batch17 in_use=%d" % u for u in use}
            if any({use[i], use[i + 1]} == {96, 97} for i in range(16)):
                h.add("C batch17 96|97")
    elif fam == "D" and len(fig) == 1:
        n = len(data)
        for s, e in zero_runs(oracle, data):
            for rel in run_relations(s, e):
                h.add("D run=%d %s" % (e - s, rel))
            if e - s > TILE and (s // TILE) != ((e - 1) // TILE):
                h.add("D run>tile")
            if e - s > 2 * TILE:
                h.add("D run>2tiles")
            if e == n and e - s > 1:
                h.add("D run@eob")
    elif fam == "E":
        L = limit(level)
        if case["gen"] == "norun" and len(data) - L in (-1, 0, 1, 4):
            d = len(data) - L
            if [b["nblock"] for b in fig] == ([L + d] if d <= 0 else [L, d]):
                h.add("E level=%d len=L%+d" % (level, d))
        elif case["gen"] == "cutrun":
            _, _, start, rl = case["args"]
            rel = {L - 5: "ends", L - 2: "crosses", L: "starts"}.get(start)
            # the run's RLE1 image is data[start:start+5] of the RLE1 output; the prefix keeps RLE1 the identity
            if rel and len(fig) == 2:
                h.add("E level=%d run=%d %s" % (level, rl, rel))
    elif fam == "F":
        if len(fig) == 321 and level == 1:
            h.add("F 321 blocks")
        for b in fig:
            if b["lm_tables"] > 0:
                h.add("F lm group_num=%d" % b["group_num"])
        if max_group_cost(stream) >= 840:
            h.add("F group cost>=840")
    return h & REQUIRED, stream, fig


# ---------------------------------------------------------------------------------------------------------- search
def _seek(oracle, make, level, target, n0, key="mtf_count", tries=60):
    """the smallest-effort n near n0 with figure `key` of the one block of make(n) equal to target, or None"""
    n, seen = max(1, n0), {}
    for _ in range(tries):
        if n in seen:
            break
        fig = figures(oracle, make(n), level)[1]
        v = fig[0][key] if len(fig) == 1 else -1
        seen[n] = v
        if v == target:
            return n
        step = round((target - v) * n / max(v, 1))
        step = (1 if target > v else -1) if step == 0 else step
        if abs(step) > 1 and any(abs(m - (n + step)) <= 1 for m in seen):
            step = 1 if target > v else -1
        n = max(1, n + step)
    for d in range(1, 40):  # a plain scan round the closest probe
        best = min(seen, key=lambda m: abs(seen[m] - target))
        for m in (best + d, best - d):
            if m > 0 and m not in seen:
                fig = figures(oracle, make(m), level)[1]
                seen[m] = fig[0][key] if len(fig) == 1 else -1
                if seen[m] == target:
                    return m
    return None


def search(oracle, log=print):
    cases = []

    def add(fam, gen, args, level, why):
        cases.append({"family": fam, "gen": gen, "args": list(args), "level": level, "why": why})

    # A: table count x alphabet
    for u in A_USE + (2,):
        for m in A_MTF:
            if ("A mtf=%d in_use=%d" % (m, u)) not in REQUIRED:
                continue
            for seed in range(1, 40):
                n = _seek(oracle, lambda n: norun(seed, max(n, u), u), 9, m, m)
                if n is not None:
                    add("A", "norun", (seed, max(n, u), u), 9, "A mtf=%d in_use=%d" % (m, u))
                    break
            else:
                log("A miss", m, u)
    # B: selector counts, last groups of 1 and 49, the largest selector count of a level-9 random block
    for m in sorted({G * s + d for s in B_SEL for d in (0, 1)} | {G * 256 + 49}):
        k = 256 if m > 600 else 40
        for seed in range(1, 40):
            n = _seek(oracle, lambda n: norun(seed, max(n, k), k), 9, m, m)
            if n is not None:
                add("B", "norun", (seed, max(n, k), k), 9, "B mtf=%d" % m)
                break
        else:
            log("B miss", m)
    add("B", "norun", (7, limit(9), 256), 9, "B max_selectors")
    # C: alphabets alone (single blocks of about 20000 symbols), chunk edges, one 17-block level-1 batch
    for i, u in enumerate(C_USE):
        if u == 1:
            add("C", "mono", (0xFB, 80), 9, "C in_use=1")
            add("C", "mono", (0x00, 1), 9, "C in_use=1 (zeros)")
        else:
            add("C", "norun", (100 + i, 20000, u, 3 * i), 9, "C in_use=%d" % u)
    for i, n in enumerate(C_NBLOCK):
        add("C", "norun", (200 + i, n, (96, 97, 256, 3)[i % 4]), 9, "C nblock=%d" % n)
    add("C", "batch", (300, (2, 3, 48, 49, 95, 96, 97, 98, 128, 129, 255, 256, 97, 96, 4, 60, 1)), 1, "C batch17")
    # D: zero runs at tile edges.  zrun(p, N): a run of N-2 from p+1, a run of N-1 from p+N+1 to the end
    for r in D_RUNS:
        N, T = r + 2, TILE * ((r + 17) // TILE + 1)  # (an edge far enough in for the run to end there after a prefix)
        add("D", "zrun", (r, T - 1 - r, N), 9, "D run=%d ends" % r)  # [p+1, p+1+r) ends at T
        add("D", "zrun", (r, T - 1, N), 9, "D run=%d starts" % r)  # starts at T
        if r > 1:
            add("D", "zrun", (r, T - 1 - r // 2, N), 9, "D run=%d crosses" % r)
    add("D", "zrun", (1, 3 * TILE - 20000, 20000), 9, "D run>2tiles")
    # E: block limit at levels 1, 2, 9 (plain bytes; a run ending at, crossing, starting at the cut)
    for lv in LEVELS:
        L = limit(lv)
        for d in (-1, 0, 1, 4):
            add("E", "norun", (400 + lv, L + d, 256), lv, "E level=%d len=L%+d" % (lv, d))
        for rl in E_RUNS:
            for start in (L - 5, L - 2, L):
                add("E", "cutrun", (500 + lv, lv, start, rl), lv, "E level=%d run=%d" % (lv, rl))
    # F: 321 level-1 blocks; length-limited tables and groups made only of 17-bit symbols
    add("F", "batch", (600, tuple((4, 60, 97, 256, 2)[i % 5] for i in range(321))), 1, "F 321 blocks")
    for seed in range(0, 12):
        c = {"family": "F", "gen": "textmix", "args": [seed, 880000], "level": 9}
        if {"F lm group_num=6", "F group cost>=840"} <= hits(c, oracle)[0]:
            add("F", "textmix", c["args"], 9, "F lm + costly group")
            break
    else:
        log("F miss")
    # the figures, the stream's digest and the targets hit, per case
    for c in cases:
        h, stream, fig = hits(c, oracle)
        c["targets"] = sorted(h)
        c["sha256"] = hashlib.sha256(stream).hexdigest()
        c["blocks"] = fig if len(fig) <= 32 else None
    return cases


def load():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def case_id(c):
    a = ",".join(str(x) if not isinstance(x, list) else "x%d" % len(x) for x in c["args"])
    return "%s-%s(%s)-l%d" % (c["family"], c["gen"], a, c["level"])


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/encshapes.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    from oracle import oracle
    cases = search(oracle)
    got = set().union(*(c["targets"] for c in cases))
    missing = sorted(REQUIRED - got)
    with open(FIXTURE, "w") as f:
        json.dump({"about": "tests/encshapes.py --regen: encoder inputs at the block shapes where the encode "
                            "kernels branch, with the oracle's figures", "cases": cases}, f, separators=(",", ":"))
        f.write("\n")
    print("%d cases, %d targets, missing: %s" % (len(cases), len(got), missing or "none"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
