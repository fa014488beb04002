"""The digit counts of the rotation sort's init, taken from the pack pass (k_bwt.hip: counts_from_pack).

A block in the pair form with 10-bit codes has key(j) = code(j) << 20 | code(j + 2) << 10 | code(j + 4), positions cyclic,
code(i) = rank of the pair (T[i], T[i+1]) among the pairs the block uses.  j -> j + 2 -> j + 4 (mod n) are bijections of the
positions, so each of the three 10-bit digit histograms over all rotations is the histogram of code(0 .. n-1) -- which
k_pack_text has in registers.  A wrong count misplaces a scatter, so the identity is restated here with numpy, the key
built the long way round (three gathers, shifts, masks) and the counts taken from the key's digits.

No GPU: this checks the argument, the GPU tests check the kernels (test_gpu_init_packed.py).
"""
import random

import numpy as np
import pytest

from test_gpu_pair_keys import make_block


def pair_codes(block):
    """code(i), i < n: the dense, order-preserving code of the pair (T[i], T[i+1 mod n])"""
    t = np.frombuffer(block, dtype=np.uint8).astype(np.uint32)
    pr = t * 256 + np.roll(t, -1)
    used = np.unique(pr)
    assert len(used) <= 1024
    return np.searchsorted(used, pr).astype(np.uint32)


def keys(block):
    """key(j) of every rotation, from the codes at j, j + 2, j + 4 (cyclic)"""
    code = pair_codes(block)
    n = len(code)
    j = np.arange(n)
    return (code[j] << 20) | (code[(j + 2) % n] << 10) | code[(j + 4) % n]


def check(block):
    code = pair_codes(block)
    want = np.bincount(code, minlength=1024)
    assert int(want.sum()) == len(block)  # (what a.count[lb] must end up as)
    k = keys(block)
    for shift in (0, 10, 20):
        got = np.bincount((k >> shift) & 1023, minlength=1024)
        assert np.array_equal(got, want), (len(block), shift)
    # and the digit bases the scatter uses: one exclusive scan serves all three digit positions
    assert np.array_equal(np.cumsum(want) - want, np.searchsorted(np.sort(k & 1023), np.arange(1024)))


@pytest.mark.parametrize("n", [1, 2, 5, 6, 7, 15, 16, 17])
def test_short_blocks(n):
    rng = random.Random(n)
    check(bytes(rng.sample(range(256), n)))        # distinct symbols: every key wraps
    check(bytes(rng.choice(b"ab") for _ in range(n)))  # and a block with repeated pairs


def test_text_like_block():
    check(make_block(36, 720, 20000, 11))


def test_ten_bit_codes():
    block = make_block(40, 1024, 20000, 12)  # codes up to 1023
    assert int(pair_codes(block).max()) == 1023
    check(block)


def test_wrap_pair_occurs_nowhere_else():
    body = make_block(12, 100, 3000, 77)
    free = [v for v in range(256) if v not in set(body)]
    block = bytes([free[1]]) + body + bytes([free[0]])
    t = np.frombuffer(block, dtype=np.uint8).astype(np.uint32)
    pr = t * 256 + np.roll(t, -1)
    assert int(np.sum(pr == pr[-1])) == 1  # the pair (T[n-1], T[0]) is counted once, at position n - 1
    check(block)
