"""CPU-side checks of the BGZF writer's interface (section 7 of include/bz2_mi355x.h): the exported symbols, bound and block
count, the parameter errors that never reach a device, the empty input (the marker, no device) and the loud failure
without a GPU."""
import ctypes as C
import os
import re

import pytest

import bgzfref
from conftest import ROOT

NEW = ("df_bgzf_block_count", "df_bgzf_bound", "df_gpu_bgzf_encode_device", "df_gpu_last_bgzf_stats", "df_bgzf_encode_buffer")
B = 65280


def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "bz2_mi355x.h")) as f:
        header = f.read()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.EXPORTS
        assert getattr(L, name) is not None
    assert re.search(r"#define\s+DF_BGZF_BLOCK\s+65280u", header)
    for name in ("bgzf_compress", "bgzf_bound", "bgzf_block_count"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert pkg.BGZF_BLOCK == B
    assert len(pkg.GpuEngine.BGZF_STATS) == 8


@pytest.mark.parametrize("b", [0, B, 1, 7, 4096, 65279])
def test_bound_and_count(pkg, b):
    bb = b or B
    for n, count in ((0, 0), (1, 1), (bb - 1, 1 if bb > 1 else 0), (bb, 1), (bb + 1, 2), (3 * bb, 3), (3 * bb + 1, 4)):
        assert pkg.bgzf_block_count(n, b) == count == bgzfref.block_count(n, b)
        for eof in (False, True):
            assert pkg.bgzf_bound(n, b, eof) == n + 31 * count + (28 if eof else 0) == bgzfref.bound(n, b, eof)
    assert pkg.bgzf_block_count(1 << 40, b) == ((1 << 40) + bb - 1) // bb   # a size_t, not 32 bits


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(7)
    off = (C.c_uint64 * 4)()
    assert L.df_bgzf_encode_buffer(0, b"x", 1, B + 1, 1, C.byref(out), C.byref(n), off) == pkg.BZ_E_PARAM
    assert L.df_bgzf_encode_buffer(0, None, 1, 0, 1, C.byref(out), C.byref(n), off) == pkg.BZ_E_PARAM
    assert L.df_bgzf_encode_buffer(0, b"x", 1, 0, 1, None, C.byref(n), off) == pkg.BZ_E_PARAM
    assert L.df_bgzf_encode_buffer(0, b"x", 1, 0, 1, C.byref(out), None, off) == pkg.BZ_E_PARAM
    assert not bool(out)
    # the device form without an engine, without out_len
    a = C.c_uint64(0)
    assert L.df_gpu_bgzf_encode_device(None, None, 0, 0, 1, None, 0, C.byref(a), None) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_bgzf_stats(None, off) == pkg.BZ_E_PARAM
    for bad in (B + 1, -1, 1 << 20):
        with pytest.raises(ValueError):
            pkg.bgzf_compress(b"x", block_bytes=bad)
        with pytest.raises(ValueError):
            pkg.bgzf_bound(1, bad)
        with pytest.raises(ValueError):
            pkg.bgzf_block_count(1, bad)


def test_empty_input_is_the_marker_and_touches_no_device(pkg):
    L = pkg.lib()
    for device in (0, 99):   # (a device that does not exist: nobody asks)
        assert pkg.bgzf_compress(b"", device=device) == bgzfref.EOF
        assert pkg.bgzf_compress(b"", eof=False, device=device) == b""
        assert pkg.bgzf_compress(b"", 7, device=device, offsets=True) == (bgzfref.EOF, [0])
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(7)
    assert L.df_bgzf_encode_buffer(0, None, 0, 0, 0, C.byref(out), C.byref(n), None) == pkg.BZ_OK
    assert bool(out) and n.value == 0
    L.bz_free(out)


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.bgzf_compress(b"x")
    assert ei.value.kind == "NoGpu"
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    assert L.df_bgzf_encode_buffer(0, b"x", 1, 0, 1, C.byref(out), C.byref(n), None) == pkg.BZ_E_NOGPU
    assert L.df_bgzf_encode_buffer(0, b"x", 1, B + 1, 1, C.byref(out), C.byref(n), None) == pkg.BZ_E_PARAM   # parameters first
