"""CPU-side checks of the batch encode interface (bz_encode_batch, bz_gpu_encode_batch_device): the bound, the
parameter errors that never reach a device, the loud failure without a GPU, and the rule that says which inputs are
certain to be one block -- against the oracle's RLE1 and block cuts."""
import ctypes as C

import pytest


def one_block_bound(level):
    """largest n with 5 * (n / 4) + n % 4 <= 100000 * level - 19"""
    limit = 100000 * level - 19
    n = 4 * (limit // 5) + min(3, limit % 5)
    assert 5 * (n // 4) + n % 4 <= limit < 5 * ((n + 1) // 4) + (n + 1) % 4
    return n


def worst_case(n):
    """runs of four bytes, two values in turn, and what is left of n as single bytes: RLE1 makes five of every four"""
    out = bytearray()
    for i in range(n // 4):
        out += bytes([0x41 + i % 2]) * 4
    return bytes(out + bytes([0x61, 0x62, 0x63][:n % 4]))


def test_batch_bound_is_the_sum_of_the_rounded_bounds(pkg):
    L = pkg.lib()
    lens = [0, 1, 15, 16, 4097, 99981, 719984, 719985, 5000000]
    want = sum((L.bz_encode_bound(n) + 3) & ~3 for n in lens)
    assert pkg.encode_batch_bound(lens) == want
    assert pkg.encode_batch_bound([]) == 0
    assert pkg.encode_batch_bound([0]) == (L.bz_encode_bound(0) + 3) & ~3 >= 16


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off = (C.c_uint64 * 1)()
    ln = (C.c_uint64 * 1)()
    for level in (0, 10, -1):
        assert L.bz_encode_batch(level, 0, ins, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.bz_encode_batch(9, 0, None, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.bz_encode_batch(9, 0, ins, None, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.bz_encode_batch(9, 0, ins, lens, 1, C.byref(out), None, ln) == pkg.BZ_E_PARAM
    assert L.bz_encode_batch(9, 0, ins, lens, 1, None, off, ln) == pkg.BZ_E_PARAM
    # no inputs: nothing to do, an empty buffer that bz_free takes
    assert L.bz_encode_batch(9, 0, None, None, 0, C.byref(out), None, None) == pkg.BZ_OK
    assert bool(out)
    L.bz_free(out)
    # the device entry point without an engine
    a = (C.c_uint64 * 1)(0)
    assert L.bz_gpu_encode_batch_device(None, 9, None, a, a, 1, None, 0, a, a) == pkg.BZ_E_PARAM
    assert L.bz_gpu_last_batch_stats(None, a) == pkg.BZ_E_PARAM
    with pytest.raises(ValueError):
        pkg.compress_batch([b"x"], level=0)


def test_batch_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.compress_batch([b"x"])
    assert ei.value.kind == "NoGpu"


@pytest.mark.parametrize("level", [1, 2])
def test_one_block_bound_is_tight(oracle, level):
    """at the bound the worst-case input is one block of exactly 100000 * level - 19 or a little less; one byte more
    and the oracle cuts it in two"""
    n = one_block_bound(level)
    assert {1: 79985, 2: 159985}[level] == n
    _, block_end, in_end, _ = oracle.rle1_blocks(worst_case(n), level)
    assert len(block_end) == 1 and in_end == [n]
    assert block_end[0] == 5 * (n // 4) + n % 4 <= 100000 * level - 19
    _, block_end, in_end, _ = oracle.rle1_blocks(worst_case(n + 1), level)
    assert len(block_end) == 2 and in_end[-1] == n + 1


def test_one_block_bound_at_level_9():
    """179 996 runs of four and one odd byte: an image of exactly 899 981 bytes"""
    assert one_block_bound(9) == 719985
