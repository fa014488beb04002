"""CPU-side checks of the batched Deflate interface (df_encode_batch, df_gpu_encode_batch_device): the exported symbols,
the bound, the parameter errors that never reach a device, the loud failure without a GPU, and the rule that says which
inputs are certain to be one block -- against the oracle's block list."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW = ("df_encode_batch_bound", "df_gpu_encode_batch_device", "df_gpu_last_batch_stats", "df_encode_batch")


def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "bz2_mi355x.h")) as f:
        header = f.read()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.EXPORTS
        assert getattr(L, name) is not None


def test_batch_bound_is_the_sum_of_the_rounded_bounds(pkg):
    L = pkg.lib()
    lens = [0, 1, 15, 16, 4097, 65534, 65535, 65536, 65537, 5000000]
    want = sum((L.df_encode_bound(n) + 3) & ~3 for n in lens)
    assert pkg.deflate_encode_batch_bound(lens) == want
    assert pkg.deflate_encode_batch_bound([]) == 0
    assert pkg.deflate_encode_batch_bound([0]) == (L.df_encode_bound(0) + 3) & ~3


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off = (C.c_uint64 * 1)()
    ln = (C.c_uint64 * 1)()
    for kind in (3, -1):
        assert L.df_encode_batch(kind, 0, ins, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch(0, 0, None, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch(0, 0, ins, None, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch(0, 0, ins, lens, 1, C.byref(out), None, ln) == pkg.BZ_E_PARAM
    assert L.df_encode_batch(0, 0, ins, lens, 1, C.byref(out), off, None) == pkg.BZ_E_PARAM
    assert L.df_encode_batch(0, 0, ins, lens, 1, None, off, ln) == pkg.BZ_E_PARAM
    # no inputs: nothing to do and no device touched, an empty buffer that bz_free takes
    for kind in (0, 1, 2):
        assert L.df_encode_batch(kind, 0, None, None, 0, C.byref(out), None, None) == pkg.BZ_OK
        assert bool(out)
        L.bz_free(out)
    assert pkg.deflate_compress_batch([]) == []
    # the device entry points without an engine, and with one null array
    a = (C.c_uint64 * 1)(0)
    assert L.df_gpu_encode_batch_device(None, 0, None, a, a, 1, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_batch_stats(None, a) == pkg.BZ_E_PARAM
    with pytest.raises(ValueError):
        pkg.deflate_compress_batch([b"x"], kind=3)


def test_batch_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    for kind in (pkg.DEFLATE, pkg.ZLIB, pkg.GZIP):
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_compress_batch([b"x"], kind)
        assert ei.value.kind == "NoGpu"


@pytest.mark.parametrize("n,blocks", [(0, 1), (1, 1), (65534, 1), (65535, 1), (65536, 2), (65537, 2)])
def test_one_block_up_to_0xFFFF_bytes(oracle, n, blocks):
    """what the routing rests on: an input of at most 0xFFFF bytes is one block, whatever it holds"""
    import random
    rnd = random.Random(n)
    for data in (bytes(rnd.getrandbits(8) for _ in range(n)), b"a" * n, (b"lorem ipsum dolor sit amet " * (n // 27 + 1))[:n]):
        e = oracle.DeflateEncoder()
        e.feed(data, oracle.ACTION_FINISH)
        assert len(e.blocks()) == blocks
