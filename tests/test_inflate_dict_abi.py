"""CPU-side checks of Deflate / zlib DECODING WITH A PRESET DICTIONARY (df_gpu_decode_batch_device_dict, df_decode_batch_dict,
df_decode_buffer_dict; include/bz2_mi355x.h section 5, clause (c)): the exports, the parameter errors that never reach a
device -- a dictionary's length without its bytes and gzip with a dictionary among them --, count == 0, the loud failure
without a GPU, and the Python classes, which are constructible without touching the device."""
import ctypes as C

import pytest

NAMES = ("df_gpu_decode_batch_device_dict", "df_decode_batch_dict", "df_decode_buffer_dict")
DICT = b"a preset dictionary"


def arrays():
    return (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(0), (C.c_int32 * 1)(0)


def test_exports(pkg):
    L = pkg.lib()
    for name in NAMES:
        assert name in pkg.EXPORTS
        assert getattr(L, name) is not None


def test_device_entry_point_parameter_errors(pkg):
    L = pkg.lib()
    a, b, v = arrays()
    for count in (1, 0):        # no engine
        assert L.df_gpu_decode_batch_device_dict(None, 0, None, a, a, count, DICT, len(DICT), None, 0, b, b, v) == pkg.BZ_E_PARAM
        assert L.df_gpu_decode_batch_device_dict(None, 0, None, a, a, count, None, 0, None, 0, b, b, v) == pkg.BZ_E_PARAM


def test_host_forms_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    ins = (C.c_char_p * 1)(b"x")
    lens = (C.c_size_t * 1)(1)
    off, ln, v = arrays()
    n = C.c_size_t(0)
    batch = lambda kind, i, l, d, dn, o, a, b, c: L.df_decode_batch_dict(kind, 0, i, l, 1, d, dn, o, a, b, c)
    for kind in (3, -1):
        assert batch(kind, ins, lens, DICT, len(DICT), C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
        assert L.df_decode_buffer_dict(kind, 0, b"x", 1, DICT, len(DICT), C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert batch(0, None, lens, DICT, len(DICT), C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert batch(0, ins, None, DICT, len(DICT), C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert batch(0, ins, lens, DICT, len(DICT), C.byref(out), None, ln, v) == pkg.BZ_E_PARAM
    assert batch(0, ins, lens, DICT, len(DICT), C.byref(out), off, None, v) == pkg.BZ_E_PARAM
    assert batch(0, ins, lens, DICT, len(DICT), C.byref(out), off, ln, None) == pkg.BZ_E_PARAM
    assert batch(0, ins, lens, DICT, len(DICT), None, off, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer_dict(0, 0, b"x", 1, DICT, len(DICT), None, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer_dict(0, 0, b"x", 1, DICT, len(DICT), C.byref(out), None) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer_dict(0, 0, None, 1, DICT, len(DICT), C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    for kind in (0, 1, 2):      # a length without the bytes
        assert batch(kind, ins, lens, None, 5, C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
        assert L.df_decode_buffer_dict(kind, 0, b"x", 1, None, 5, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
        assert L.df_decode_batch_dict(kind, 0, None, None, 0, None, 5, C.byref(out), None, None, None) == pkg.BZ_E_PARAM
    # gzip has no dictionary (GZipDecoder has no with_dict) -- also with nothing to decode
    assert batch(2, ins, lens, DICT, len(DICT), C.byref(out), off, ln, v) == pkg.BZ_E_PARAM
    assert L.df_decode_buffer_dict(2, 0, b"x", 1, DICT, len(DICT), C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_batch_dict(2, 0, None, None, 0, DICT, len(DICT), C.byref(out), None, None, None) == pkg.BZ_E_PARAM
    assert not bool(out)
    for fn in (lambda: pkg.deflate_decompress_batch([b"x"], pkg.GZIP, dict_=DICT), lambda: pkg.deflate_decompress(b"x", pkg.GZIP, dict_=DICT),
               lambda: pkg.deflate_decompress_batch([b"x"], 3, dict_=DICT), lambda: pkg.deflate_decompress(b"x", -1, dict_=DICT)):
        with pytest.raises(ValueError):
            fn()


def test_count_zero_touches_no_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    for kind in (0, 1):
        assert L.df_decode_batch_dict(kind, 0, None, None, 0, DICT, len(DICT), C.byref(out), None, None, None) == pkg.BZ_OK
        assert bool(out)        # an empty buffer that bz_free takes
        L.bz_free(out)
        assert pkg.deflate_decompress_batch([], kind, dict_=DICT) == []
    assert L.df_decode_batch_dict(2, 0, None, None, 0, None, 0, C.byref(out), None, None, None) == pkg.BZ_OK      # no dictionary: as ever
    L.bz_free(out)


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    for kind in (pkg.DEFLATE, pkg.ZLIB):
        assert L.df_decode_buffer_dict(kind, 0, b"\x03\x00", 2, DICT, len(DICT), C.byref(out), C.byref(n)) == pkg.BZ_E_NOGPU
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_decompress_batch([b"\x03\x00"], kind, dict_=DICT)
        assert ei.value.kind == "NoGpu"
        with pytest.raises(pkg.CompressionError) as ei:
            pkg.deflate_decompress(b"\x03\x00", kind, dict_=DICT)
        assert ei.value.kind == "NoGpu"
    for cls in (pkg.Deflater, pkg.ZlibDecoder):
        with pytest.raises(pkg.CompressionError) as ei:
            cls.with_dict(DICT).decode_all(b"\x03\x00")      # there is no CPU path behind the classes either
        assert ei.value.kind == "NoGpu"


def test_classes_are_constructible_without_a_device(pkg):
    for cls, kind in ((pkg.Deflater, pkg.DEFLATE), (pkg.ZlibDecoder, pkg.ZLIB)):
        for d in (cls.with_dict(DICT), cls.with_dict(bytearray(DICT), device=0), cls(dict_=DICT), cls(0, DICT), cls.with_dict(b"")):
            assert isinstance(d, cls) and d.KIND == kind and callable(d.next) and callable(d.decode_all)
    for cls in (pkg.GZipDecoder, pkg.MultiGZipDecoder):
        with pytest.raises(ValueError):
            cls(dict_=DICT)
        with pytest.raises(ValueError):
            cls.with_dict(DICT)
        assert cls(dict_=b"").KIND == pkg.GZIP      # an empty dictionary is no dictionary
