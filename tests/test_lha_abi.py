"""CPU-side checks of the LHA reader's ABI (include/bz2_mi355x.h section 11): the symbols are exported, the member table
needs no GPU, parameter errors of the read calls come back before any device is touched, and without a GPU the host form
fails loudly (there is no CPU path)."""
import ctypes as C

import pytest

import lhaforge as F

NAMES = ("bz_lha_index_buffer", "bz_gpu_lha_read_device", "bz_gpu_last_lha_read_stats", "bz_lha_read_buffer")


@pytest.fixture(scope="module")
def arch():
    return {a.name: a for a in F.archives()}["M_methods"]


def _device(pkg, g, d_in, n, idx, sel, nsel, prefill=0x20, d_out=None, cap=0, nmembers=None):
    k = max(nsel, 1)
    off, ln, v = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_int32 * k)()
    a_sel = None if sel is None else (C.c_size_t * max(len(sel), 1))(*sel)
    return pkg.lib().bz_gpu_lha_read_device(g, d_in, n, idx._records, len(idx) if nmembers is None else nmembers, a_sel, nsel, prefill, d_out,
                                            cap, off, ln, v)


def _host(pkg, data, sel, nsel, prefill=0x20, out_null=False):
    k = max(nsel, 1)
    off, ln, v = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_int32 * k)()
    out, fault = C.POINTER(C.c_uint8)(), C.c_int32(0)
    a_sel = None if sel is None else (C.c_size_t * max(len(sel), 1))(*sel)
    rc = pkg.lib().bz_lha_read_buffer(0, data, len(data), a_sel, nsel, prefill, None if out_null else C.byref(out), off, ln, v, C.byref(fault))
    if out:
        pkg.lib().bz_free(out)
    return rc


def test_exports(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in pkg.EXPORTS, n
    for n in ("lha_index", "lha_extract", "LhaArchive", "LhaIndex", "LhaMember"):
        assert hasattr(pkg, n), n
    assert hasattr(pkg.GpuEngine, "lha_read_device") and hasattr(pkg.GpuEngine, "lha_read_stats")
    assert len(pkg.GpuEngine.LHA_READ_STATS) == 8


def test_the_table_needs_no_gpu(pkg, arch):
    idx = pkg.lha_index(arch.data)
    assert idx.fault == pkg.BZ_OK and len(idx) == 16
    assert [m.method for m in idx][:5] == [b"-lh0-", b"-lh4-", b"-lhd-", b"-lh5-", b"-lh1-"]
    assert idx[3].name == idx[13].name == b"same.txt" and idx[2].directory == b"sub\xff"
    a = pkg.LhaArchive(arch.data)          # creating one does not touch the device
    assert len(a.members) == 16


def test_read_device_parameter_errors_touch_no_device(pkg, arch):
    idx = pkg.lha_index(arch.data)
    n = len(arch.data)
    fake = C.create_string_buffer(64)      # (never looked into: every check below comes first)
    g, d_in = C.addressof(fake), 0x1000
    assert _device(pkg, None, d_in, n, idx, None, 16) == pkg.BZ_E_PARAM                    # a null engine
    assert _device(pkg, g, d_in + 4, n, idx, None, 16) == pkg.BZ_E_PARAM                   # a misaligned d_in
    assert _device(pkg, g, d_in, n, idx, None, 16, d_out=0x2008, cap=1 << 20) == pkg.BZ_E_PARAM   # a misaligned d_out
    assert _device(pkg, g, d_in, n, idx, [3, 1], 2) == pkg.BZ_E_PARAM                      # a selection out of order
    assert _device(pkg, g, d_in, n, idx, [1, 1], 2) == pkg.BZ_E_PARAM
    assert _device(pkg, g, d_in, n, idx, [1, 16], 2) == pkg.BZ_E_PARAM                     # ... out of range
    assert _device(pkg, g, d_in, n, idx, None, 15) == pkg.BZ_E_PARAM                       # all members: nsel is their count
    assert _device(pkg, g, d_in, n, idx, None, 16, prefill=-2) == pkg.BZ_E_PARAM
    assert _device(pkg, g, d_in, n, idx, None, 16, prefill=256) == pkg.BZ_E_PARAM
    assert _device(pkg, g, d_in, idx[5].header_off, idx, [5], 1) == pkg.BZ_E_PARAM         # a record whose span leaves the archive
    assert _device(pkg, g, d_in, n, idx, [], 0) == pkg.BZ_OK                               # nsel == 0: nothing touched
    assert pkg.lib().bz_gpu_last_lha_read_stats(None, (C.c_uint64 * 8)()) == pkg.BZ_E_PARAM
    k = 1
    off, ln, v = (C.c_uint64 * k)(), (C.c_uint64 * k)(), (C.c_int32 * k)()
    sel = (C.c_size_t * 1)(0)
    assert pkg.lib().bz_gpu_lha_read_device(g, d_in, n, idx._records, 16, sel, 1, 0x20, None, 0, None, ln, v) == pkg.BZ_E_PARAM
    assert pkg.lib().bz_gpu_lha_read_device(g, d_in, n, None, 16, sel, 1, 0x20, None, 0, off, ln, v) == pkg.BZ_E_PARAM


def test_read_buffer_parameter_errors_touch_no_device(pkg, arch):
    d = arch.data
    assert _host(pkg, d, None, 16, out_null=True) == pkg.BZ_E_PARAM
    assert _host(pkg, d, None, 16, prefill=-2) == pkg.BZ_E_PARAM
    assert _host(pkg, d, None, 16, prefill=256) == pkg.BZ_E_PARAM
    assert _host(pkg, d, None, 15) == pkg.BZ_E_PARAM
    assert _host(pkg, d, [2, 1], 2) == pkg.BZ_E_PARAM
    assert _host(pkg, d, [16], 1) == pkg.BZ_E_PARAM
    assert _host(pkg, d, [], 0) == pkg.BZ_OK                 # nothing selected: an empty buffer, no device
    assert _host(pkg, b"", None, 0) == pkg.BZ_OK             # an archive without members
    assert pkg.lha_extract(b"\0") == []
    with pytest.raises(KeyError):
        pkg.lha_extract(d, ["no such member"])
    with pytest.raises(IndexError):
        pkg.lha_extract(d, [16])
    with pytest.raises(ValueError):
        pkg.lha_extract(d, prefill=300)


def test_fails_loudly_without_gpu(pkg, arch):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _host(pkg, arch.data, None, 16) == pkg.BZ_E_NOGPU
    assert _host(pkg, arch.data, [2], 1) == pkg.BZ_E_NOGPU   # (even a directory: the call has no CPU path)
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lha_extract(arch.data)
    assert ei.value.kind == "NoGpu"
    with pytest.raises(pkg.CompressionError):
        pkg.LhaArchive(arch.data).read("same.txt")
