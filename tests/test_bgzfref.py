"""CPU checks of tests/bgzfref.py, the expected BGZF file that the GPU tests compare with: Python's gzip and zlib read every
file it builds, the BSIZE chain walks from 0 to the end, the EOF marker is the standard one, and both arms of the strict
rule are taken -- on QUIRK (fixed) and on its twin over the symbols 144 and up (stored)."""
import gzip
import random
import zlib

import pytest

import bgzfref
from test_gpu_deflate_batch import QUIRK

QUIRK_HI = bytes(b for i in range(32) for j in range(32) for b in (144 + i, 176 + j))  # QUIRK over 9-bit literals


def seeded(seed):
    r = random.Random(seed)
    alpha = r.choice([4, 8, 16, 64, 256])
    n = r.choice([5, 40, 300, 1000, 5000])
    b = r.choice([1, 7, 16, 17, 100, 999, 4096, 4097, 65279, 65280, 0])
    if b == 1:
        n = min(n, 40)
    base = r.randrange(0, 257 - alpha)
    return bytes(base + r.randrange(alpha) for _ in range(n)), b


def test_marker_is_the_standard_one(oracle):
    assert len(bgzfref.EOF) == 28
    assert bgzfref.EOF == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert gzip.decompress(bgzfref.EOF) == b""
    assert bgzfref.build(oracle, b"") == (bgzfref.EOF, [0], [])
    assert bgzfref.build(oracle, b"", eof=False) == (b"", [0], [])
    # the marker is what the builder makes of an empty chunk: a fixed block of the end-of-block code alone
    assert bgzfref.wrap(b"", oracle.deflate_encode(b"", 0)) == bgzfref.EOF


def test_seeded_sweep_decodes_with_gzip(oracle):
    replaced = 0
    arms = set()
    for seed in range(120):
        data, b = seeded(seed)
        for eof in (True, False):
            file, offs, kinds = bgzfref.build(oracle, data, b, eof)
            assert gzip.decompress(file) == data, seed             # every case: none is skipped
            assert len(offs) == bgzfref.block_count(len(data), b) + 1 == len(kinds) + 1
            assert bgzfref.walk(file) == offs[:-1] + ([offs[-1]] if eof else [])
            assert file[offs[-1]:] == (bgzfref.EOF if eof else b"")
            assert len(file) <= bgzfref.bound(len(data), b, eof)
        replaced += sum(1 for _, rep in kinds if rep)
        arms |= {bt for bt, rep in kinds if rep}
    assert replaced >= 20           # the rule is no corner case
    assert arms <= {0, 1}


def test_members_decode_one_by_one(oracle):
    data = (QUIRK + QUIRK_HI + b"the quick brown fox " * 200 + bytes(range(256)) * 3) * 2
    b = 2048
    file, offs, kinds = bgzfref.build(oracle, data, b)
    for k in range(len(kinds)):
        member = file[offs[k]:offs[k + 1]]
        assert zlib.decompress(member[18:-8], -15) == data[k * b:(k + 1) * b]
        assert zlib.decompress(member, 31) == data[k * b:(k + 1) * b]
    assert [kd for kd in kinds[:2]] == [(1, True), (0, True)]


def test_both_arms_of_the_strict_rule(oracle):
    assert len(QUIRK) == len(QUIRK_HI) == 2048
    for x in (QUIRK, QUIRK_HI):
        ref = oracle.deflate_encode(x, 0)
        assert (ref[0] >> 1) & 3 == 2 and bgzfref.literals_only(oracle, x)
    assert bgzfref.fixed_bits(QUIRK) == 16393 and 8 * len(QUIRK) + 34 == 16418
    d, btype, rep = bgzfref.body(oracle, QUIRK)
    assert (btype, rep) == (1, True) and len(d) == (1 + 16393 + 7) // 8 and d[0] & 7 == 3
    assert bgzfref.fixed_bits(QUIRK_HI) == 2 + 9 * 2048 + 7
    d, btype, rep = bgzfref.body(oracle, QUIRK_HI)
    assert (btype, rep) == (0, True) and d == b"\x01\x00\x08\xff\xf7" + QUIRK_HI
    for x in (QUIRK, QUIRK_HI):
        assert zlib.decompress(bgzfref.body(oracle, x)[0], -15) == x
    # a block with a match keeps the oracle's bytes, whatever its type
    for x in (b"a" * 700, b"abcabcabc" * 50, bytes(range(256)) * 2):
        assert bgzfref.body(oracle, x) == (oracle.deflate_encode(x, 0), (oracle.deflate_encode(x, 0)[0] >> 1) & 3, False)


def test_zlib_refuses_the_unreplaced_stream(oracle):
    with pytest.raises(zlib.error):
        zlib.decompress(oracle.deflate_encode(QUIRK, 0), -15)
    with pytest.raises(zlib.error):
        zlib.decompress(oracle.deflate_encode(QUIRK_HI, 0), -15)


def test_fixed_body_is_zlibs_fixed_block():
    r = random.Random(1)
    for n in (0, 1, 2, 7, 8, 9, 300):
        x = bytes(r.randrange(256) for _ in range(n))
        assert zlib.decompress(bgzfref.fixed_body(x), -15) == x
        assert len(bgzfref.fixed_body(x)) == (1 + bgzfref.fixed_bits(x) + 7) // 8
