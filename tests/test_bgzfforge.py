"""The BGZF forge (tests/bgzfforge.py) pinned on the CPU before any GPU sees one of its files: every clean forged file
round-trips through Python's gzip.decompress, bgzfref.walk agrees with its offsets, its own chain() agrees with both, and
the faulty files carry the fault they are named after."""
import gzip
import struct
import zlib

import pytest

import bgzfforge as F
import bgzfref
import dfforge


def _files():
    out = dict(F.clean_files())
    out["phases"] = F.phase_file()
    out["nested"] = F.nested()[0]
    return out


@pytest.mark.parametrize("name", sorted(_files()))
def test_clean_files_round_trip(name):
    f = _files()[name]
    assert f.data == b"".join(f.chunks)
    assert (gzip.decompress(f.file) if f.file else b"") == f.data
    assert bgzfref.walk(f.file) == f.coff[:-1]
    assert F.chain(f.file) == (f.coff, f.uoff, F.OK)
    assert f.coff[-1] == len(f.file) and f.uoff[-1] == len(f.data)
    for k in range(f.count):
        assert zlib.decompress(f.blocks[k], 31) == f.chunks[k]
        assert struct.unpack_from("<H", f.blocks[k], 16)[0] + 1 == len(f.blocks[k])


def test_block_kinds():
    d = F.text(500, 3)
    assert (F.stored(d)[0] >> 1) & 3 == 0 and (F.fixed(d)[0] >> 1) & 3 == 1 and (F.dynamic(d)[0] >> 1) & 3 == 2
    for raw in (F.stored(d), F.fixed(d), F.dynamic(d), F.three_blocks(d)):
        assert zlib.decompress(raw, -15) == d
    t = F.three_blocks(d)
    o = zlib.decompressobj(-15)
    assert o.decompress(t) == d and o.eof


def test_phase_file_takes_every_phase():
    f = F.phase_file()
    assert {c % 4 for c in f.coff[:-1]} == {0, 1, 2, 3}
    assert {u % 16 for u in f.uoff[:-1]} == set(range(16))
    assert 20 <= f.count <= 64


def test_nested_file_holds_64_false_headers():
    f, inner = F.nested()
    assert f.count == 2 and inner.count == 64
    heads = [p for p in range(len(f.file) - 17) if f.file[p:p + 4] == b"\x1f\x8b\x08\x04" and f.file[p + 10:p + 16] == b"\x06\x00BC\x02\x00"]
    assert len(heads) == 64 + 2


def test_chain_faults_are_what_they_are_named():
    cases = F.chain_faults()
    assert len({c[0] for c in cases}) == len(cases)
    seen = set()
    for name, data, v, n, base in cases:
        coff, uoff, got = F.chain(data)
        assert got == v, name
        assert coff == base.coff[:n + 1] and uoff == base.uoff[:n + 1], name   # the clean prefix is still indexed
        seen.add(v)
        if v == F.OK:
            assert gzip.decompress(data) == base.data[:base.uoff[n]]
    assert seen == {F.OK, F.E_DATA, F.E_EOF}
    assert sum(1 for c in cases if c[0].startswith("header_byte_")) == 10   # ten bytes pinned by value, BSIZE's two by the chain


def test_forged_trailers():
    d = F.text(100, 9)
    raw = F.raw_deflate(d)
    good = F.block(raw, d)
    assert good == bgzfref.wrap(d, raw)
    bad_crc = F.block(raw, d, crc=zlib.crc32(d) ^ 1)
    with pytest.raises(Exception):
        gzip.decompress(bad_crc)
    bad_isize = F.block(raw, d, isize=len(d) + 1)
    with pytest.raises(Exception):
        gzip.decompress(bad_isize)


def test_dfforge_streams_wrap():
    c = [x for x in dfforge.clean_cases() if x.kind == dfforge.RAW][0]
    assert gzip.decompress(bgzfref.wrap(c.data, c.stream)) == c.data


def test_forged_clean_file_holds_every_clean_raw_stream_but_one():
    f, left_out = F.forged_clean_file()
    clean = [c for c in dfforge.clean_cases() if c.kind == dfforge.RAW]
    assert len(clean) == 160 and f.count == 159 and left_out == ["stored_65535"]
    assert len(next(c for c in clean if c.name == "stored_65535").stream) == 65540
    assert f.chunks == [c.data for c in clean if c.name != "stored_65535"] and len(f.data) == 494490
    assert gzip.decompress(f.file) == f.data
    assert F.chain(f.file) == (f.coff, f.uoff, F.OK)
    assert len(f.chunks[0]) >= 2 and len(f.chunks[-1]) >= 2          # a range can begin inside the first and end inside the last
