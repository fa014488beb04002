"""CPU-side checks of the Deflate / zlib / gzip DECODE interface (df_gpu_decode_batch_device, df_decode_batch,
df_decode_buffer): the parameter errors that never reach a device, count == 0, the loud failure without a GPU, and the
Python classes, which are constructible without touching the device."""
import ctypes as C

import pytest


def arrays():
    return (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(0)


def test_device_entry_point_parameter_errors(pkg):
    L = pkg.lib()
    a, b, v = arrays()
    assert L.df_gpu_decode_batch_device(None, 0, None, a, a, 1, None, 0, b, b, v) == pkg.BZ_E_PARAM    # no engine
    assert L.df_gpu_decode_batch_device(None, 0, None, a, a, 0, None, 0, b, b, v) == pkg.BZ_E_PARAM    # ... also with count == 0
    assert L.df_gpu_last_decode_batch_stats(None, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_decode_batch_stats(None, None) == pkg.BZ_E_PARAM


def test_host_forms_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off, ln, v = arrays()
    for kind in (3, -1):
        assert L.df_decode_batch(kind, 0, ins, lens, 1, C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, None, lens, 1, C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, ins, None, 1, C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, ins, lens, 1, C.byref(out), None, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, ins, lens, 1, C.byref(out), off, None, v) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, ins, lens, 1, C.byref(out), off, ln, None) == pkg.BZ_E_PARAM
    assert L.df_decode_batch(0, 0, ins, lens, 1, None, off, ln, v) == pkg.BZ_E_PARAM
    null = (C.c_char_p * 1)(None)
    assert L.df_decode_batch(0, 0, null, lens, 1, C.byref(out), off, ln, v) == pkg.BZ_E_PARAM          # bytes announced, no pointer
    n = C.c_size_t(0)
    for kind in (3, -1):
        assert L.df_decode_buffer(kind, 0, b"x", 1, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer(0, 0, b"x", 1, None, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer(0, 0, b"x", 1, C.byref(out), None) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer(0, 0, None, 1, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    for kind in (3, -1):
        with pytest.raises(ValueError):
            pkg.deflate_decompress_batch([b"x"], kind=kind)
        with pytest.raises(ValueError):
            pkg.deflate_decompress(b"x", kind=kind)


def test_count_zero_touches_no_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    for kind in (0, 1, 2):
        assert L.df_decode_batch(kind, 0, None, None, 0, C.byref(out), None, None, None) == pkg.BZ_OK
        assert bool(out)        # an empty buffer that bz_free takes
        L.bz_free(out)
        assert pkg.deflate_decompress_batch([], kind) == []


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    for kind in (pkg.DEFLATE, pkg.ZLIB, pkg.GZIP):
        assert L.df_decode_buffer(kind, 0, b"\x03\x00", 2, C.byref(out), C.byref(n)) == pkg.BZ_E_NOGPU
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_decompress_batch([b"\x03\x00"], kind)
        assert ei.value.kind == "NoGpu"
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_decompress(b"\x03\x00", kind)
        assert ei.value.kind == "NoGpu"
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.Deflater().decode_all(b"\x03\x00")      # there is no CPU path behind the classes either
    assert ei.value.kind == "NoGpu"


def test_classes_are_constructible_without_a_device(pkg):
    for cls, kind in ((pkg.Deflater, pkg.DEFLATE), (pkg.ZlibDecoder, pkg.ZLIB), (pkg.GZipDecoder, pkg.GZIP)):
        d = cls()
        assert d.KIND == kind and callable(d.next) and callable(d.decode_all)
        assert cls.__name__ in pkg.__all__
    for name in ("df_gpu_decode_batch_device", "df_gpu_last_decode_batch_stats", "df_decode_batch", "df_decode_buffer"):
        assert name in pkg.EXPORTS
    assert len(pkg.GpuEngine.DEFLATE_DECODE_BATCH_STATS) == 8
