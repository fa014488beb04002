"""CPU-side checks of batched Deflate / zlib encoding with a preset dictionary (df_encode_batch_dict,
df_gpu_encode_batch_device_dict): the exported symbols, the parameter errors that never reach a device, the loud failure
without a GPU, the rule that an input of at most 0xFFFF bytes is one block WITH a dictionary too -- against the oracle's
block list --, and the window cases of tests/test_gpu_deflate_batch_dict.py pinned to the oracle's LZSS codes, so that
the GPU comparisons there are known to tell a right window rule from a wrong one."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("df_gpu_encode_batch_device_dict", "df_encode_batch_dict")
WIN = 32768


def rnd_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def words(seed, n, vocab=7):
    """word text; texts of the same `vocab` share their 300 words"""
    r = random.Random(vocab)
    w = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(1, 9))) for _ in range(300)]
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += r.choice(w) + b" "
    return bytes(out[:n])


# ---- the window cases: (dictionary, input) pairs, shared with the GPU tests
KEY = b"0123456789ABCDEF"


def distance_limit_cases():
    """[(dict, input, has a reference to the key)]: the key lies 32 768 bytes in front of the input's first byte"""
    d = KEY + rnd_bytes(11, WIN - len(KEY))
    far = KEY + rnd_bytes(12, 40000 - len(KEY))
    return [(d, KEY + b"!", True), (d, b"\xf1" + KEY + b"!", False), (d, b"\xf1\xf2" + KEY + b"!", False), (far, KEY + b"!", False)]


TAIL_CASE = (b"xyzqab", b"cabcabc")  # literal c, then length 6 at distance 3: the match starts in the window's last two bytes


def _occ(idx):
    return b"abc" + bytes([0x80 + idx // 32, 0xA0 + idx % 32])


def budget_case(k, m):
    """k own occurrences of `abc` in front of the input's final abcDEFGH, m in the dictionary in front of those, and behind
    them all the dictionary's abcDEFGH: candidate k + m + 1 of the chain"""
    d = b"abcDEFGH" + b"-" * 8 + b"".join(_occ(256 + j) for j in range(m))
    x = b"".join(_occ(i) for i in range(k)) + b"abcDEFGH"
    return d, x


BUDGET = [((0, 254), True), ((100, 154), True), ((254, 0), True), ((0, 255), False), ((100, 155), False), ((255, 0), False)]


def tail_equal_case():
    d = words(31, 40000)
    return d, d[-20000:]


def long_input_case():
    """40 000 bytes: a piece of the dictionary at the input's start (in the window), and again at 37 000, where both the
    dictionary and the first copy lie more than 32 768 bytes back"""
    seg = rnd_bytes(41, 1000)
    base = words(42, WIN)
    d = base[:20000] + seg + base[21000:]
    x = seg + rnd_bytes(43, 36000) + seg + rnd_bytes(44, 2000)
    assert len(d) == WIN and len(x) == 40000
    return d, x


def refs(tokens):
    return [t for t in tokens if t[0] == "ref"]


# ---- the interface
def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "bz2_mi355x.h")) as f:
        header = f.read()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.EXPORTS
        assert getattr(L, name) is not None


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off = (C.c_uint64 * 1)()
    ln = (C.c_uint64 * 1)()
    a = (C.c_uint64 * 1)(0)
    # the host form
    assert L.df_encode_batch_dict(2, 0, ins, lens, 1, b"dict", 4, C.byref(out), off, ln) == pkg.BZ_E_PARAM   # gzip has no with_dict
    assert L.df_encode_batch_dict(2, 0, None, None, 0, b"dict", 4, C.byref(out), None, None) == pkg.BZ_E_PARAM
    for kind in (0, 1):
        assert L.df_encode_batch_dict(kind, 0, ins, lens, 1, None, 4, C.byref(out), off, ln) == pkg.BZ_E_PARAM  # a length without a pointer
    for kind in (3, -1):
        assert L.df_encode_batch_dict(kind, 0, ins, lens, 1, b"dict", 4, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch_dict(0, 0, ins, lens, 1, b"dict", 4, None, off, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch_dict(0, 0, None, lens, 1, b"dict", 4, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    for kind, d, n in ((0, b"dict", 4), (1, b"dict", 4), (2, None, 0), (1, None, 0), (1, b"dict", 0)):
        assert L.df_encode_batch_dict(kind, 0, None, None, 0, d, n, C.byref(out), None, None) == pkg.BZ_OK   # count == 0
        assert bool(out)
        L.bz_free(out)
    # the device form: no engine ...
    assert L.df_gpu_encode_batch_device_dict(None, 0, None, a, a, 1, b"dict", 4, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_encode_batch_device_dict(None, 0, None, a, a, 0, None, 0, None, 0, a, a) == pkg.BZ_E_PARAM
    # ... and the dictionary's own errors, which are answered before the engine is looked at (any non-null handle does)
    handle = C.create_string_buffer(4096)
    assert L.df_gpu_encode_batch_device_dict(handle, 2, None, a, a, 1, b"dict", 4, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_encode_batch_device_dict(handle, 2, None, a, a, 0, b"dict", 4, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_encode_batch_device_dict(handle, 1, None, a, a, 1, None, 4, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_encode_batch_device_dict(handle, 1, None, a, a, 0, b"dict", 4, None, 0, a, a) == pkg.BZ_OK   # count == 0
    assert L.df_gpu_encode_batch_device_dict(handle, 2, None, a, a, 0, None, 0, None, 0, a, a) == pkg.BZ_OK


def test_python_refuses_gzip_with_a_dictionary(pkg):
    with pytest.raises(ValueError):
        pkg.deflate_compress_batch([b"x"], pkg.GZIP, dict_=b"dict")
    with pytest.raises(ValueError):
        pkg.deflate_compress_batch([b"x"], 3, dict_=b"dict")
    with pytest.raises(ValueError):
        pkg.deflate_compress_batch([], pkg.GZIP, dict_=b"dict")
    assert pkg.deflate_compress_batch([], pkg.GZIP, dict_=b"") == []   # an empty dictionary is none
    assert pkg.deflate_compress_batch([], pkg.ZLIB, dict_=b"dict") == []


def test_batch_with_a_dictionary_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    for kind in (pkg.DEFLATE, pkg.ZLIB):
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_compress_batch([b"x"], kind, dict_=b"dict")
        assert ei.value.kind == "NoGpu"


# ---- routing: what takes the batch path
@pytest.mark.parametrize("dlen", [1, 2, 3, 258, 32767, 32768, 40000, 70000])
def test_one_block_up_to_0xFFFF_bytes_with_a_dictionary(oracle, dlen):
    """InflaterInner::with_dict starts with decompress_len 0: the dictionary is history, not output"""
    d = words(dlen, dlen)
    for n, blocks in ((0, 1), (1, 1), (2, 1), (3, 1), (65534, 1), (65535, 1), (65536, 2), (65537, 2)):
        for data in (rnd_bytes(n, n), b"a" * n, words(n + 1, n)):
            e = oracle.DeflateEncoder(d)
            e.feed(data, oracle.ACTION_FINISH)
            assert len(e.blocks()) == blocks, (dlen, n)


# ---- the window cases, in the oracle's LZSS codes
def test_distance_limit_is_32768(oracle):
    for d, x, found in distance_limit_cases():
        r = refs(oracle.lzss_tokens(x, d))
        assert r == ([("ref", 16, WIN - 1)] if found else []), (len(d), len(x))   # (pos = distance - 1)
    d, x, _ = distance_limit_cases()[0]
    assert oracle.lzss_tokens(x, d) == [("ref", 16, WIN - 1), ("sym", ord("!"))]


def test_match_from_the_windows_last_two_bytes(oracle):
    d, x = TAIL_CASE
    assert oracle.lzss_tokens(x, d) == [("sym", ord("c")), ("ref", 6, 2)]
    assert refs(oracle.lzss_tokens(x)) == [("ref", 4, 2)]   # without the dictionary: c a b, then cabc


@pytest.mark.parametrize("km,found", BUDGET)
def test_candidate_budget_counts_own_and_dictionary_candidates_together(oracle, km, found):
    d, x = budget_case(*km)
    last = refs(oracle.lzss_tokens(x, d))[-1]
    assert (last[1] == 8) == found, last   # (not found: the lazy step finds bcDEFGH, length 7, through its own short chain)


def test_input_equal_to_the_dictionarys_tail(oracle):
    d, x = tail_equal_case()
    t = oracle.lzss_tokens(x, d)
    assert all(tok == ("ref", 258, len(x) - 1) for tok in t[:-1]) and len(t) == -(-len(x) // 258)


def test_long_input_leaves_the_window(oracle):
    d, x = long_input_case()
    t = oracle.lzss_tokens(x, d)
    assert t[0][:2] == ("ref", 258) and t[0][2] == WIN - 20000 - 1
    covered = sum(tok[1] for tok in refs(t))
    # the first copy only (the second one sees neither the dictionary nor the first), and the chance trigrams of 38 000
    # random bytes: some tens of length-3 references.  A second copy that matched would add 1 000.
    assert 1000 <= covered < 1500, covered
