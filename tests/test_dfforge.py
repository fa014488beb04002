"""The Deflate forge (tests/dfforge.py) pinned by an independent decoder, Python's zlib, before any GPU sees one of its
streams: every clean stream decodes to exactly the bytes the forge says, every malformed one makes zlib raise -- or, for
the truncations, leaves decompressobj().eof False -- and the bytes zlib hands out in front of the fault (fed byte by byte)
are the forge's prefix.  Where zlib cannot arbitrate the case says so in its note: FDICT set (zlib asks for a dictionary
instead of raising: pinned by the forge's own bookkeeping -- the FLG bit is set, FCHECK is right, no byte is yielded), a
stored block cut short (zlib yields the bytes that are there, the contract none of the block), and two faults that zlib
reports before it has handed out the literals in front of them."""
import zlib

import pytest

import dfforge as F


def zlib_partial(case):
    """(bytes handed out, the zlib.error or None, eof) with the stream fed one byte at a time"""
    d = zlib.decompressobj(F.WBITS[case.kind])
    out = bytearray()
    try:
        for i in range(len(case.stream)):
            out += d.decompress(case.stream[i:i + 1])
    except zlib.error as e:
        return bytes(out), e, d.eof
    return bytes(out), None, d.eof


CLEAN = F.clean_cases()
MALFORMED = F.malformed_cases() + [F.quirk_like()]


def test_the_lists_are_what_the_gpu_tests_expect():
    names = [c.name for c in CLEAN + MALFORMED]
    assert len(set(names)) == len(names)
    assert len(F.copy_grid()) == len(F.COPY_DIST) * len(F.COPY_LEN) == 112
    assert all(c.verdict == F.OK for c in CLEAN) and all(c.verdict in (F.E_DATA, F.E_EOF) for c in MALFORMED)
    assert {c.kind for c in CLEAN} == {F.RAW, F.ZLIB, F.GZIP}
    assert sum(c.verdict == F.E_DATA for c in MALFORMED) >= 40 and sum(c.verdict == F.E_EOF for c in MALFORMED) >= 6


@pytest.mark.parametrize("case", CLEAN, ids=lambda c: c.name)
def test_clean_streams_decode_to_the_forged_bytes(case):
    d = zlib.decompressobj(F.WBITS[case.kind])
    assert d.decompress(case.stream) == case.data
    assert d.eof
    out, err, eof = zlib_partial(case)
    assert err is None and eof and out == case.data


@pytest.mark.parametrize("case", MALFORMED, ids=lambda c: c.name)
def test_malformed_streams_are_malformed_for_zlib(case):
    out, err, eof = zlib_partial(case)
    if case.verdict == F.E_EOF:
        assert err is None and not eof
    elif case.name == "zlib_fdict":
        # zlib's answer is Z_NEED_DICT (2), not a data error: the forge's own bookkeeping pins this one
        assert err is not None and "Error 2" in str(err)
        assert case.stream[1] & 0x20 and int.from_bytes(case.stream[:2], "big") % 31 == 0 and case.data == b""
    else:
        assert err is not None and "Error -3" in str(err)
    if case.note:
        assert case.data.startswith(out) or out.startswith(case.data)
    else:
        assert out == case.data


def test_last_bit_positions():
    """the two streams whose final bit is bit 7 / bit 0 of the last byte really end there: with the padding bits all
    ones, clearing the last code's final bit makes the stream end one code later or not at all"""
    for c in F.table_shapes():
        if c.name.startswith("last_bit_at_"):
            want = int(c.name[-1])
            broken = bytearray(c.stream)
            broken[-1] ^= 1 << want      # (end-of-block is 0000000: its last bit is 0; now it is a 1)
            d = zlib.decompressobj(-15)
            try:
                d.decompress(bytes(broken))
                assert not d.eof
            except zlib.error:
                pass
            if want < 7:
                assert c.stream[-1] >> (want + 1) == 0xFF >> (want + 1)   # only padding above it


def test_cut_points():
    pts = F.cut_points(1000)
    assert pts[:64] == list(range(64)) and pts[-64:] == list(range(936, 1000)) and len(pts) == 64 + 64 + 32
    assert F.cut_points(100) == list(range(100))
