#!/usr/bin/env python3
"""CPU census of the run heads of the BWT last column (the sizing behind the MTF stage on heads, k_mtf.hip "M0",
DESIGN.md section 4).  A head is position 0 of the column, or a position whose byte differs from the one in front of
it; only heads need the MTF list, every other position has rank 0.  Uses the oracle (test infrastructure): RLE1 blocks,
rotation order, L[i] = block[sa[i] - 1].

  tools/head_census.py [blocks per corpus, default 2] [corpus names ...]

Per corpus: symbols in use, heads / positions, and the heads per 512-position chunk (median, p90, max) -- the reason why
skipping repeats inside a rank kernel that owns 512 POSITIONS per lane would not collect the gain."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import corpus
from oracle import oracle

CHUNK = 512


def columns(raw, nblocks):
    rle, be, _, _ = oracle.rle1_blocks(raw, 9)
    b0 = 0
    for e in be[:nblocks]:
        blk = rle[b0:e]
        b0 = e
        sa = np.array(oracle.bwt(blk), dtype=np.int64)
        yield np.frombuffer(blk, dtype=np.uint8)[sa - 1]  # (sa = 0 reads the block's last byte)


def main(argv):
    nblocks = int(argv[1]) if len(argv) > 1 else 2
    names = argv[2:] or ["text"] + [m for m in ("mix", "logs", "binary", "dna", "random") if m in corpus.MATRIX] + ["t2"]
    nbytes = (nblocks * 900000 * 5) // 4 + (1 << 20)
    print("%-8s %-14s %-10s %s" % ("corpus", "symbols in use", "heads / n", "heads per %d positions: median, p90, max" % CHUNK))
    for name in names:
        if name == "text":
            raw = corpus.chapter(0, nbytes)
        elif name == "t2":
            raw = corpus.stress_t2(nbytes)
        else:
            raw = corpus.matrix_corpus(name, nbytes).tobytes()
        use, heads, total, per = [], 0, 0, []
        for L in columns(raw, nblocks):
            h = np.ones(len(L), dtype=bool)
            h[1:] = L[1:] != L[:-1]
            use.append(len(np.unique(L)))
            heads += int(h.sum())
            total += len(L)
            k = len(L) // CHUNK * CHUNK
            per.append(h[:k].reshape(-1, CHUNK).sum(axis=1))
        per = np.concatenate(per)
        print("%-8s %-14s %-10.3f %d, %d, %d" % (name, "-".join(str(u) for u in sorted(set(use))), heads / total,
                                                  np.median(per), np.percentile(per, 90), per.max()))


if __name__ == "__main__":
    main(sys.argv)
