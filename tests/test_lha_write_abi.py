"""CPU-side checks of the LHA writer's ABI (include/bz2_mi355x.h section 12): the symbols are exported, the bound needs no GPU
and is the restatement's, every parameter error of the contract comes back before any device is touched, and without a GPU
the host form fails loudly (there is no CPU path)."""
import ctypes as C

import pytest

import lhawrite as W

NAMES = ("bz_lha_write_bound", "bz_gpu_lha_write_device", "bz_gpu_last_lha_write_stats", "bz_lha_write_buffer")
GIB = 1 << 30


def _entries(pkg, specs):
    """specs: (name, dir, is_dir)"""
    return pkg._lha_entries([pkg.LhaEntry(n, d, 1, 2, 3, isd) for n, d, isd in specs])


def _device(pkg, g, method, level, specs, lens, offs=None, d_in=0x1000, d_out=0x100000, cap=1 << 20, out_len=True, recs=True):
    k = len(specs)
    ents, keep = _entries(pkg, specs)
    if offs is None:
        offs, at = [], 0
        for n in lens:
            offs.append(at)
            at += (n + 15) & ~15
    a_off, a_len = (C.c_uint64 * max(k, 1))(*offs), (C.c_uint64 * max(k, 1))(*lens)
    n = C.c_size_t(0)
    return pkg.lib().bz_gpu_lha_write_device(g, method, level, d_in, a_off, a_len, ents if recs else None, k, d_out, cap,
                                             C.byref(n) if out_len else None, None)


def _host(pkg, method, level, specs, datas, out_null=False):
    k = len(specs)
    ents, keep = _entries(pkg, specs)
    ins = (C.c_char_p * max(k, 1))(*datas)
    lens = (C.c_size_t * max(k, 1))(*[len(d) for d in datas])
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
    rc = pkg.lib().bz_lha_write_buffer(method, level, 0, ins, lens, ents, k, None if out_null else C.byref(out), C.byref(n))
    got = C.string_at(out, n.value) if rc == pkg.BZ_OK else None
    if out:
        pkg.lib().bz_free(out)
    return rc, got


def test_exports(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in pkg.EXPORTS, n
    for n in ("LhaEntry", "lha_write_bound", "lha_compress", "LHA_STORED"):
        assert hasattr(pkg, n), n
    assert hasattr(pkg.GpuEngine, "lha_write_device") and hasattr(pkg.GpuEngine, "lha_write_stats")
    assert len(pkg.GpuEngine.LHA_WRITE_STATS) == 8
    assert C.sizeof(pkg._LhaEntryRec) == 40


def test_the_bound_is_the_restatements_and_needs_no_gpu(pkg):
    for c in W.load():
        ents = W.entries(c)
        es = [pkg.LhaEntry(e["name"], e["dir"], e["mtime"], e["attr"], e["os_id"], e["is_dir"]) for e, _ in ents]
        lens = [len(p) for _, p in ents]
        for level in c.get("levels", W.LEVELS):
            want = sum(W.header_size(level, e) + n for (e, _), n in zip(ents, lens)) + 1
            assert pkg.lha_write_bound(es, lens, level) == want, (c["name"], level)
            for method in c.get("methods", W.METHODS):          # it always suffices: the stored rule
                assert len(W.build(c, method, level)[0]) <= want
    assert pkg.lha_write_bound([], [], 2) == 1
    assert pkg.lha_write_bound(["n"], [5], 3) == 0 and pkg.lha_write_bound(["n"], [5], -1) == 0
    assert pkg.lha_write_bound([pkg.LhaEntry(b"n", b"d\xff")], [5], 0) == 0
    assert pkg.lha_write_bound([b"x" * 234], [5], 0) == 0 and pkg.lha_write_bound([b"x" * 233], [5], 0) == 24 + 233 + 5 + 1


def test_write_device_parameter_errors_touch_no_device(pkg):
    fake = C.create_string_buffer(64)      # (never looked into: every check below comes first)
    g = C.addressof(fake)
    P = pkg.BZ_E_PARAM
    one, ln = [(b"name", b"", False)], [100]
    assert _device(pkg, None, 5, 2, one, ln) == P                                   # a null engine
    assert _device(pkg, g, 5, 2, one, ln, out_len=False) == P
    assert _device(pkg, g, 5, 2, one, ln, d_out=None) == P
    assert _device(pkg, g, 5, 2, one, ln, recs=False) == P                          # a null array
    for method in (-1, 1, 2, 3, 8, 255):
        assert _device(pkg, g, method, 2, one, ln) == P, method
    for level in (-1, 3):
        assert _device(pkg, g, 5, level, one, ln) == P, level
    assert _device(pkg, g, 5, 2, one, ln, d_in=0x1008) == P                         # the encoder's: a misaligned d_in,
    assert _device(pkg, g, 5, 2, one * 2, ln * 2, offs=[0, 8]) == P                 # ... offset,
    assert _device(pkg, g, 5, 2, one * 2, ln * 2, offs=[0, 96]) == P                # ... ranges that overlap,
    assert _device(pkg, g, 5, 2, one * 2, ln * 2, offs=[112, 0]) == P               # ... or descend,
    assert _device(pkg, g, 5, 2, one, [GIB + 1]) == P                               # ... an input above 1 GiB
    assert _device(pkg, g, 0, 2, one, [(4 << 30) - 1]) == P                         # stored: a size field would reach 4 GiB - 1
    assert _device(pkg, g, 0, 1, [(b"x" * 300, b"", False)], [(4 << 30) - 1 - 303]) == P   # (level 1: the skip size)
    assert _device(pkg, g, 5, 2, one, ln, d_in=None) == P                           # bytes and no place they lie at
    assert _device(pkg, g, 5, 0, [(b"n", b"d\xff", False)], ln) == P                # level 0 has no place for a directory
    assert _device(pkg, g, 5, 0, [(b"x" * 234, b"", False)], ln) == P               # H > 255
    assert _device(pkg, g, 5, 1, [(b"x" * 65533, b"", False)], ln) == P             # an extended header above 65 535
    assert _device(pkg, g, 5, 2, [(b"n", b"d" * 65533, False)], ln) == P
    assert _device(pkg, g, 5, 2, [(b"x" * 40000, b"d" * 25499, False)], ln) == P    # T above 65 535
    assert _device(pkg, g, 5, 2, [(b"dir", b"", True)], [1]) == P                   # a directory with bytes
    assert _device(pkg, g, 5, 2, one + [(b"dir", b"", True)], [100, 16]) == P
    assert pkg.lib().bz_gpu_last_lha_write_stats(None, (C.c_uint64 * 8)()) == P
    assert pkg.lib().bz_gpu_last_lha_write_stats(g, None) == P


def test_write_buffer_parameter_errors_touch_no_device(pkg):
    P = pkg.BZ_E_PARAM
    one, d = [(b"name", b"", False)], [b"hello"]
    assert _host(pkg, 5, 2, one, d, out_null=True)[0] == P
    assert _host(pkg, 9, 2, one, d)[0] == P and _host(pkg, 1, 2, one, d)[0] == P
    assert _host(pkg, 5, 3, one, d)[0] == P
    assert _host(pkg, 5, 0, [(b"n", b"d\xff", False)], d)[0] == P
    assert _host(pkg, 0, 0, [(b"x" * 234, b"", False)], d)[0] == P
    assert _host(pkg, 5, 1, [(b"dir", b"", True)], d)[0] == P
    assert _host(pkg, 5, 2, [], []) == (pkg.BZ_OK, b"\0")        # no members: the end byte alone, no device
    assert _host(pkg, 0, 0, [], []) == (pkg.BZ_OK, b"\0")
    assert pkg.lha_compress([]) == b"\0"
    with pytest.raises(ValueError):
        pkg.lha_compress([("a", b"x")], method=3)
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lha_compress([(pkg.LhaEntry(b"a", b"d\xff"), b"x")], level=0)
    assert ei.value.code == P


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    one = [(b"name", b"", False)]
    assert _host(pkg, 5, 2, one, [b"hello"])[0] == pkg.BZ_E_NOGPU
    assert _host(pkg, 0, 0, one, [b"hello"])[0] == pkg.BZ_E_NOGPU           # (even stored: the call has no CPU path)
    assert _host(pkg, 5, 1, [(b"dir", b"", True)], [b""])[0] == pkg.BZ_E_NOGPU
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.lha_compress([("a.txt", b"hello")])
    assert ei.value.kind == "NoGpu"
