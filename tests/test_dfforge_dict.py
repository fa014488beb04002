"""The forged streams of tests/dfforge_dict.py against Python's zlib with the same dictionary, before any GPU sees them:
zlib.decompressobj(wbits, zdict=dict) is the arbiter of the body (include/bz2_mi355x.h section 5, clause (c)); where the
header rules are the reference's and differ from zlib's, the case says what zlib does and that is pinned too.  No GPU."""
import zlib

import pytest

import dfforge as F
import dfforge_dict as D


def zlib_says(c):
    """(bytes handed out, eof, raised): the stream fed byte by byte, so that the bytes in front of a fault come out"""
    d = zlib.decompressobj(F.WBITS[c.kind], zdict=c.dict)
    out = bytearray()
    try:
        for k in range(0, len(c.stream), 64):
            out += d.decompress(c.stream[k:k + 64])
    except zlib.error:
        return bytes(out), False, True
    return bytes(out), d.eof, False


def check(c):
    out, eof, raised = zlib_says(c)
    if c.zlib == "ignores the dictionary":
        assert c.verdict == F.E_DATA and (out, eof, raised) == (c.zlib_data, True, False), c
    elif c.verdict == F.OK:
        assert (out, eof, raised) == (c.data, True, False), c
    elif c.verdict == F.E_DATA or c.zlib == "raises":
        assert raised and c.data.startswith(out), c         # (zlib may hold back the last bytes in front of the fault)
    else:
        assert not raised and not eof and c.data.startswith(out), c


@pytest.mark.parametrize("n", D.DICT_LEN)
def test_copy_cases(n):
    cases = D.copy_cases(n)
    W = min(n, 32768)
    for c in cases + [D.as_zlib(c) for c in cases]:
        check(c)
    names = {c.name for c in cases}
    assert "dict%d_p0_l3_d%d" % (n, W) in names                                     # d = p + W is accepted
    far = [c for c in cases if c.verdict == F.E_DATA]
    assert all(c.name.endswith("_d%d" % (int(c.name.split("_p")[1].split("_")[0]) + W + 1)) for c in far)
    assert len(far) >= 2 * len(D.PREFIX) if W <= 258 else len(far) == (2 if W == 32767 else 0)      # d = p + W + 1 is refused
    if W >= 258:
        assert {"dict%d_p60_l64_d64" % n, "dict%d_p1_l258_d258" % n, "dict%d_p1_l258_d3" % n, "dict%d_chain" % n} <= names
        assert sum(c.verdict == F.OK for c in cases) >= 150
    # the window is the last 32 768 bytes: the same streams decode alike with those bytes alone as the dictionary
    for c in cases[::7]:
        d = zlib.decompressobj(-15, zdict=D.window(c.dict))
        if c.verdict == F.OK:
            assert d.decompress(c.stream) == c.data and d.eof


@pytest.mark.parametrize("n", D.DICT_LEN)
def test_zlib_cases(n):
    cases = D.zlib_cases(n)
    for c in cases:
        check(c)
    by = {c.name.split("_", 1)[1]: c for c in cases}
    assert by["right_dictid"].verdict == F.OK and by["right_dictid"].stream[1] & 0x20
    assert by["right_dictid"].stream[2:6] == (zlib.adler32(D.dictionary(n)) & 0xFFFFFFFF).to_bytes(4, "big")      # of the WHOLE dictionary
    for name in ("wrong_dictid", "fdict_clear", "cm_7_six_bytes"):
        assert (by[name].verdict, by[name].data) == (F.E_DATA, b"")
    for k in (2, 3, 4, 5):
        assert (by["cut_%d" % k].verdict, by["cut_%d" % k].data) == (F.E_EOF, b"")
    assert by["cm_7_cut_4"].verdict == F.E_EOF and len(by["cm_7_cut_4"].stream) == 4
    assert by["wrong_adler"].verdict == F.E_DATA and by["wrong_adler"].data == by["right_dictid"].data
    # zlib's own streams carry the same header
    c = zlib.compressobj(6, zlib.DEFLATED, 15, zdict=D.dictionary(n))
    assert (c.compress(b"x") + c.flush())[2:6] == by["right_dictid"].stream[2:6]


@pytest.mark.parametrize("n", (100, 20000))
def test_split_cases(n):
    cases = D.split_cases(n)
    assert len(cases) == 5
    for c in cases:
        check(c)
        assert len(c.stream) >= 4096 and c.pieces == 2
    ok = [c for c in cases if c.verdict == F.OK]
    assert all(c.unresolved > 0 for c in ok[1:]) and cases[1].verdict == F.E_DATA and len(cases[1].data) > 1024
