"""CPU-side checks of the BGZF reader's interface (section 8 of include/bz2_mi355x.h): the exported symbols, the parameter
errors of all five C calls that never reach a device, the empty input and the empty range (no device), and the loud failure
of a read without a GPU while the index still answers."""
import ctypes as C
import os
import re

import pytest

import bgzfforge as F
from conftest import ROOT

NEW = ("df_bgzf_index_buffer", "df_gpu_bgzf_index_device", "df_gpu_bgzf_read_device", "df_gpu_last_bgzf_read_stats", "df_bgzf_read_buffer")
U64P = C.POINTER(C.c_uint64)


def test_header_symbols_are_exported(pkg):
    with open(os.path.join(ROOT, "include", "bz2_mi355x.h")) as f:
        header = f.read()
    L = pkg.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in pkg.EXPORTS
        assert getattr(L, name) is not None
    assert "8. READING BGZF" in header
    for name in ("bgzf_index", "bgzf_decompress", "bgzf_read", "BgzfIndex"):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    for name in ("bgzf_index_device", "bgzf_read_device", "bgzf_read_stats"):
        assert callable(getattr(pkg.GpuEngine, name))
    assert len(pkg.GpuEngine.BGZF_READ_STATS) == 8
    assert issubclass(pkg.BgzfError, pkg.CompressionError)


def test_the_wrappers_name_the_calls():
    base = os.path.join(ROOT, "rust-compression_amd")
    hpp = open(os.path.join(base, "host", "compression.hpp")).read()
    for name in ("bgzf_index", "bgzf_read", "bgzf_decompress"):
        assert re.search(r"\b%s\s*\(" % name, hpp), name
    ffi = open(os.path.join(base, "rust_shim", "src", "ffi.rs")).read()
    for name in ("df_bgzf_index_buffer", "df_bgzf_read_buffer"):
        assert re.search(r"pub fn %s\(" % name, ffi), name
    rs = open(os.path.join(base, "rust_shim", "src", "mi355x.rs")).read()
    for name in ("bgzf_index", "bgzf_read", "bgzf_decode"):
        assert re.search(r"pub fn %s\b" % name, rs), name


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    pc, pu = U64P(), U64P()
    n = C.c_size_t(7)
    v = C.c_int32(7)
    # 1. the host index
    assert L.df_bgzf_index_buffer(None, 1, C.byref(pc), C.byref(pu), C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_bgzf_index_buffer(b"x", 1, None, C.byref(pu), C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_bgzf_index_buffer(b"x", 1, C.byref(pc), None, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_bgzf_index_buffer(b"x", 1, C.byref(pc), C.byref(pu), None, C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_bgzf_index_buffer(b"x", 1, C.byref(pc), C.byref(pu), C.byref(n), None) == pkg.BZ_E_PARAM
    assert not pc and not pu
    # 2. the device index and 3. the device read without an engine; 4. the statistics
    a = (C.c_uint64 * 4)()
    o = C.c_uint64(0)
    assert L.df_gpu_bgzf_index_device(None, None, 0, a, a, 3, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_gpu_bgzf_read_device(None, None, 0, a, a, 0, 0, 1, None, 0, C.byref(o), C.byref(v)) == pkg.BZ_E_PARAM
    s8 = (C.c_uint64 * 8)()
    assert L.df_gpu_last_bgzf_read_stats(None, s8) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_bgzf_read_stats(None, None) == pkg.BZ_E_PARAM
    # 5. the host read
    out = C.POINTER(C.c_uint8)()
    assert L.df_bgzf_read_buffer(0, b"x", 1, 0, 1, None, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_bgzf_read_buffer(0, b"x", 1, 0, 1, C.byref(out), None) == pkg.BZ_E_PARAM
    assert L.df_bgzf_read_buffer(0, None, 1, 0, 1, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert not out
    with pytest.raises(ValueError):
        pkg.bgzf_read(b"", -1, 1)
    with pytest.raises(ValueError):
        pkg.bgzf_read(b"", 0, -1)
    with pytest.raises(TypeError):
        pkg.bgzf_read(b"", 0, 1, index=[0])


def test_an_empty_input_and_an_empty_range_touch_no_device(pkg):
    L = pkg.lib()
    f = F.clean_files()["one_block"]
    for device in (0, 99):   # (a device that does not exist: nobody asks)
        assert pkg.bgzf_decompress(b"", device=device) == b""
        assert pkg.bgzf_read(b"", 5, 10, device=device) == b""
        assert pkg.bgzf_read(f.file, 0, 0, device=device) == b""
        assert pkg.bgzf_read(f.file, len(f.data), 9, device=device) == b""          # ustart = total
        assert pkg.bgzf_read(f.file, len(f.data) + 5, 9, device=device) == b""
        assert pkg.bgzf_decompress(F.clean_files()["marker_alone"].file, device=device) == b""
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(7)
    assert L.df_bgzf_read_buffer(0, None, 0, 0, 1, C.byref(out), C.byref(n)) == pkg.BZ_OK
    assert bool(out) and n.value == 0
    L.bz_free(out)
    ix = pkg.bgzf_index(b"")
    assert (ix.coff, ix.uoff, ix.blocks, ix.total, ix.verdict) == ([0], [0], 0, 0, pkg.BZ_OK)


def test_a_fault_in_front_of_an_empty_range_needs_no_device(pkg):
    """the chain's verdict is known on the host: a file whose first block is no block has no bytes to decode"""
    for device in (0, 99):
        with pytest.raises(pkg.BgzfError) as ei:
            pkg.bgzf_decompress(b"not a BGZF file at all", device=device)
        assert ei.value.kind == "DataError" and ei.value.partial == b""
        with pytest.raises(pkg.BgzfError) as ei:
            pkg.bgzf_decompress(F.HEAD[:10], device=device)
        assert ei.value.kind == "UnexpectedEof" and ei.value.partial == b""


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    f = F.clean_files()["one_block"]
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.bgzf_read(f.file, 0, 10)
    assert ei.value.kind == "NoGpu"
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.bgzf_decompress(f.file)
    assert ei.value.kind == "NoGpu"
    assert pkg.bgzf_index(f.file).blocks == 1                                   # the index still answers
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    assert L.df_bgzf_read_buffer(0, f.file, len(f.file), 0, 10, C.byref(out), C.byref(n)) == pkg.BZ_E_NOGPU
    assert L.df_bgzf_read_buffer(0, None, 5, 0, 10, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM   # parameters first
