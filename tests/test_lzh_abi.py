"""CPU-side checks of the LZHUF decode ABI (include/bz2_mi355x.h section 9): the symbols are exported, parameter errors come
back before any device is touched, and without a GPU the calls fail loudly (there is no CPU path)."""
import ctypes as C

import pytest

NAMES = ("bz_gpu_lzh_decode_batch_device", "bz_gpu_last_lzh_decode_stats", "bz_lzh_decode_batch", "bz_lzh_decode_buffer")
NO_LEN = 0xFFFFFFFFFFFFFFFF


def _batch(pkg, method, prefill, datas, ins_null=False):
    L = pkg.lib()
    k = len(datas)
    ins = (C.c_char_p * max(k, 1))(*datas)
    lens = (C.c_size_t * max(k, 1))(*[len(d) for d in datas])
    off, ln, v = (C.c_uint64 * max(k, 1))(), (C.c_uint64 * max(k, 1))(), (C.c_int32 * max(k, 1))()
    out = C.POINTER(C.c_uint8)()
    rc = L.bz_lzh_decode_batch(method, prefill, 0, None if ins_null else ins, lens, None, k, C.byref(out), off, ln, v)
    if out:
        L.bz_free(out)
    return rc


def test_exports(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in pkg.EXPORTS, n
    assert [int(m) for m in pkg.LzhufMethod] == [4, 5, 6, 7]
    assert [(m.dictionary_bits, m.offset_bits) for m in pkg.LzhufMethod] == [(12, 4), (13, 4), (15, 5), (16, 5)]


@pytest.mark.parametrize("method,prefill", [(3, -1), (8, -1), (5, -2), (5, 256)])
def test_method_and_prefill_out_of_range(pkg, method, prefill):
    L = pkg.lib()
    assert _batch(pkg, method, prefill, [b"\x00\x00"]) == pkg.BZ_E_PARAM
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
    assert L.bz_lzh_decode_buffer(method, prefill, 0, b"\x00\x00", 2, NO_LEN, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_gpu_lzh_decode_batch_device(None, method, prefill, None, None, None, None, 0, None, 0, None, None, None) == pkg.BZ_E_PARAM
    with pytest.raises(ValueError):
        pkg.lzhuf_decompress(b"", method, prefill=prefill)
    with pytest.raises(ValueError):
        pkg.LzhufDecoder(method, prefill=prefill)


def test_null_arrays(pkg):
    L = pkg.lib()
    assert _batch(pkg, 5, -1, [b"\x00\x00"], ins_null=True) == pkg.BZ_E_PARAM
    lens = (C.c_size_t * 1)(2)
    ins = (C.c_char_p * 1)(b"\x00\x00")
    assert L.bz_lzh_decode_batch(5, -1, 0, ins, lens, None, 1, None, None, None, None) == pkg.BZ_E_PARAM
    out = C.POINTER(C.c_uint8)()
    assert L.bz_lzh_decode_batch(5, -1, 0, ins, lens, None, 1, C.byref(out), None, None, None) == pkg.BZ_E_PARAM
    n = C.c_size_t(0)
    assert L.bz_lzh_decode_buffer(5, -1, 0, None, 2, NO_LEN, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_lzh_decode_buffer(5, -1, 0, b"ab", 2, NO_LEN, None, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_gpu_last_lzh_decode_stats(None, (C.c_uint64 * 8)()) == pkg.BZ_E_PARAM
    assert L.bz_gpu_lzh_decode_batch_device(None, 5, -1, None, None, None, None, 0, None, 0, None, None, None) == pkg.BZ_E_PARAM


def test_count_zero_touches_no_device(pkg):
    assert _batch(pkg, 5, -1, []) == pkg.BZ_OK
    assert pkg.lzhuf_decompress_batch([], pkg.LzhufMethod.Lh7) == []


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _batch(pkg, 5, -1, [b"\x00\x00"]) == pkg.BZ_E_NOGPU
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lzhuf_decompress(b"\x00\x00", pkg.LzhufMethod.Lh5)
    assert ei.value.kind == "NoGpu"
    d = pkg.LzhufDecoder(pkg.LzhufMethod.Lh5)      # creating one does not touch the device
    with pytest.raises(pkg.CompressionError):
        d.decode_all(b"\x00\x00")
