"""CPU-side checks of the batch decode interface (bz_decode_batch, bz_gpu_decode_batch_device,
bz_gpu_last_decode_batch_stats): the parameter errors that never reach a device, the empty call, and the loud failure
without a GPU."""
import ctypes as C

import pytest


def test_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off = (C.c_uint64 * 1)()
    ln = (C.c_uint64 * 1)()
    vd = (C.c_int32 * 1)()
    assert L.bz_decode_batch(0, None, lens, 1, C.byref(out), off, ln, vd) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, ins, None, 1, C.byref(out), off, ln, vd) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, ins, lens, 1, C.byref(out), None, ln, vd) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, ins, lens, 1, C.byref(out), off, None, vd) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, ins, lens, 1, C.byref(out), off, ln, None) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, ins, lens, 1, None, off, ln, vd) == pkg.BZ_E_PARAM
    assert L.bz_decode_batch(0, None, None, 0, None, None, None, None) == pkg.BZ_E_PARAM
    # the device entry point without an engine, and the stats
    a = (C.c_uint64 * 1)(0)
    assert L.bz_gpu_decode_batch_device(None, None, a, a, 1, None, 0, a, a, vd) == pkg.BZ_E_PARAM
    assert L.bz_gpu_decode_batch_device(None, None, None, None, 0, None, 0, None, None, None) == pkg.BZ_E_PARAM
    assert L.bz_gpu_last_decode_batch_stats(None, a) == pkg.BZ_E_PARAM


def test_no_entries_is_an_empty_buffer_without_a_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    assert L.bz_decode_batch(0, None, None, 0, C.byref(out), None, None, None) == pkg.BZ_OK
    assert bool(out)
    L.bz_free(out)
    assert pkg.decompress_batch([]) == []


def test_batch_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.decompress_batch([b"x"])
    assert ei.value.kind == "NoGpu"
