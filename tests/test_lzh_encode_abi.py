"""CPU tests of the LZHUF encoder's boundary (include/bz2_mi355x.h section 10): parameter errors come back before any
device is touched, and bz_lzh_encode_batch_bound is at least the model's stream for every committed shape case, for noise
and for the worst case the format allows."""
import ctypes as C
import random

import pytest

import lzhref as R
import lzhshapes as S


def _arr(t, v):
    return (t * max(len(v), 1))(*v)


def test_parameter_errors_without_gpu(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    off, ln = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    n = C.c_size_t(0)
    ins = (C.c_char_p * 1)(b"abc")
    lens = (C.c_size_t * 1)(3)
    for method in (3, 8, 0, -1):
        assert L.bz_lzh_encode_batch(method, 0, ins, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
        assert L.bz_lzh_encode_buffer(method, 0, b"abc", 3, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_lzh_encode_batch(5, 0, ins, lens, 1, None, off, ln) == pkg.BZ_E_PARAM
    assert L.bz_lzh_encode_batch(5, 0, None, lens, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    assert L.bz_lzh_encode_batch(5, 0, ins, lens, 1, C.byref(out), None, ln) == pkg.BZ_E_PARAM
    assert L.bz_lzh_encode_buffer(5, 0, None, 3, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_lzh_encode_buffer(5, 0, b"abc", 3, None, C.byref(n)) == pkg.BZ_E_PARAM
    big = (C.c_size_t * 1)((1 << 30) + 1)  # (the length is refused before a byte is read)
    assert L.bz_lzh_encode_batch(5, 0, ins, big, 1, C.byref(out), off, ln) == pkg.BZ_E_PARAM
    # no engine: every device entry refuses
    s = (C.c_uint64 * 8)()
    assert L.bz_gpu_lzh_encode_batch_device(None, 5, None, off, ln, 1, None, 0, off, ln) == pkg.BZ_E_PARAM
    assert L.bz_gpu_last_lzh_encode_stats(None, s) == pkg.BZ_E_PARAM
    assert L.bz_gpu_lzh_debug_codes(None, 5, None, 0, None, 0, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.bz_gpu_lzh_debug_tables(None, 5, None, None, None, None, None, None) == pkg.BZ_E_PARAM
    # count == 0: an empty buffer, no device
    assert L.bz_lzh_encode_batch(5, 0, None, None, 0, C.byref(out), None, None) == pkg.BZ_OK
    L.bz_free(out)
    with pytest.raises(ValueError):
        pkg.lzhuf_compress(b"abc", 3)
    with pytest.raises(ValueError):
        pkg.LzhufEncoder(8)
    enc = pkg.LzhufEncoder(5)  # creating one does not touch the device; FLUSH is a parameter error
    enc.write(b"abc")
    with pytest.raises(pkg.CompressionError) as ei:
        enc.end(pkg.Action.FLUSH)
    assert ei.value.kind == "Param"


def test_without_gpu_the_host_calls_say_so(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lzhuf_compress(b"hello", 5)
    assert ei.value.kind == "NoGpu"
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lzhuf_compress_batch([b"hello", b""], 7)
    assert ei.value.kind == "NoGpu"


def test_bound_covers_the_model(pkg, oracle):
    assert pkg.lzhuf_encode_batch_bound([]) == 0 and pkg.lzhuf_encode_batch_bound([0]) == 0
    for c in S.load()["cases"]:
        data = S.build(c)
        for m in c["methods"]:
            assert pkg.lzhuf_encode_batch_bound([len(data)]) >= len(R.encode(data, m)), S.case_id(c)
    r = random.Random(7)
    for n in (1, 2, 3, 255, 256, 4096, 65535, 65536, 140000):
        noise = bytes(r.getrandbits(8) for _ in range(n))
        b = pkg.lzhuf_encode_batch_bound([n])
        assert b % 4 == 0 and b >= len(R.encode(noise, 7))
        assert pkg.lzhuf_encode_batch_bound([n, 0, n]) == 2 * b
    # the derivation (DESIGN_lzhuf.md section 8): 16 bits per byte and 1 084 bytes of header per 65 535 codes
    for n in (1, 65535, 65536, 1 << 30):
        assert pkg.lzhuf_encode_batch_bound([n]) == (2 * n + 1084 * -(-n // 65535) + 3) // 4 * 4
