"""GPU tests of the BGZF reader (include/bz2_mi355x.h section 8, DESIGN_deflate.md "Reading BGZF"): df_gpu_bgzf_index_device,
df_gpu_bgzf_read_device, df_bgzf_read_buffer and their Python forms.

Expected bytes never come from the library: they are the plain chunks the forge (tests/bgzfforge.py) built a file from,
and gzip.decompress.  Every device read goes through the sizes-only call and through an output buffer filled with 0xEE with
64 spare bytes on both sides, placed at d_out phases 0, 1, 7 and 15 mod 16 (the range grid and the forged-stream list take
one phase per read, in turn): nothing outside the range's extent may change."""
import ctypes as C
import gzip
import itertools
import zlib

import pytest

import bgzfforge as F
import bgzfref
import dfforge
from conftest import product

pytestmark = pytest.mark.gpu

OK, E_DATA, E_EOF = 0, -1, -2
FILL = 0xEE
PHASES = (0, 1, 7, 15)
_turn = itertools.cycle(PHASES)


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()


def extent(uoff, ustart, ulen):
    return max(0, min(ustart + ulen, uoff[-1]) - ustart)


def read(eng, ptr, in_len, index, ustart, ulen, want, verdict=OK, phases=PHASES):
    """the range through the sizes-only call and the real one at each phase of d_out; index: (coff, uoff)"""
    import torch
    rlen = extent(index[1], ustart, ulen)
    assert eng.bgzf_read_device(ptr, in_len, index, ustart, ulen, None, 0) == (rlen, OK)
    for phase in phases:
        buf = torch.full((rlen + 160,), FILL, dtype=torch.uint8, device="cuda")
        off = 64 + (phase - (buf.data_ptr() + 64)) % 16
        n, v = eng.bgzf_read_device(ptr, in_len, index, ustart, ulen, buf.data_ptr() + off, rlen)
        torch.cuda.synchronize()
        host = buf.cpu().numpy().tobytes()
        assert host[:off] == bytes([FILL]) * off, "bytes in front of d_out were written"
        assert host[off + rlen:] == bytes([FILL]) * (160 - off), "bytes at or behind the range's extent were written"
        assert v == verdict, "verdict %d, expected %d" % (v, verdict)
        assert n == len(want) and (v != OK or n == rlen), (n, len(want), rlen)
        assert host[off:off + n] == want, "first difference at %d" % next((k for k, (a, b) in enumerate(zip(host[off:off + n], want)) if a != b), -1)


def whole(eng, f, file=None):
    """a clean file, whole: equal to the chunks, to gzip.decompress and to the members call on the same buffer"""
    import torch
    file = f.file if file is None else file
    t = on_device(file)
    ix = eng.bgzf_index_device(t.data_ptr(), len(file))
    assert (ix.coff, ix.uoff, ix.verdict) == (f.coff, f.uoff, OK)
    assert (gzip.decompress(file) if file else b"") == f.data
    read(eng, t.data_ptr(), len(file), (ix.coff, ix.uoff), 0, len(f.data) + 9, f.data)
    st = eng.bgzf_read_stats()
    nonempty = [k for k in range(f.count) if f.chunks[k]]
    touched = nonempty[-1] - nonempty[0] + 1 if nonempty else 0
    assert st[0] == st[1] == touched and st[2] == 0 and st[5] == st[6] == len(f.data)
    o = torch.full((len(f.data) + 64,), FILL, dtype=torch.uint8, device="cuda")
    n, v = eng.gzip_decode_members_device(t.data_ptr(), len(file), o.data_ptr(), len(f.data))
    assert (n, v) == (len(f.data), OK) and o.cpu().numpy().tobytes()[:n] == f.data


# ---- 1. the device index equals the host index
def _index_files():
    out = [(name, f.file) for name, f in sorted(F.clean_files().items())]
    out += [("phases", F.phase_file().file), ("nested", F.nested()[0].file)]
    out += [(name, data) for name, data, _, _, _ in F.chain_faults()] + F.bsize_spoilt()
    return out


@pytest.mark.parametrize("case", _index_files(), ids=lambda c: c[0])
def test_device_index_equals_host_index(eng, pkg, case):
    name, file = case
    t = on_device(file)
    ix = eng.bgzf_index_device(t.data_ptr(), len(file))
    assert (ix.coff, ix.uoff, ix.verdict) == F.chain(file)
    assert ix == pkg.bgzf_index(file)
    st = eng.bgzf_read_stats()
    heads = [p for p in range(len(file) - 17) if file[p:p + 4] == b"\x1f\x8b\x08\x04" and file[p + 10:p + 16] == b"\x06\x00BC\x02\x00"]
    assert st[3] == len(heads)


@pytest.mark.parametrize("at", range(4093, 4100))
def test_a_header_that_straddles_a_tile_edge(eng, at):
    first = F.text(at - 31, at)
    f = F.File([(bgzfref.wrap(first, F.stored(first)), first), (F.zblock(F.text(99, 1)), F.text(99, 1)), (bgzfref.EOF, b"")])
    assert f.coff[1] == at
    t = on_device(f.file)
    ix = eng.bgzf_index_device(t.data_ptr(), len(f.file))
    assert (ix.coff, ix.uoff, ix.verdict) == (f.coff, f.uoff, OK)
    assert eng.bgzf_read_stats()[3:5] == [3, 0]


def test_false_candidates_are_never_landed_on(eng):
    f, inner = F.nested()
    t = on_device(f.file)
    ix = eng.bgzf_index_device(t.data_ptr(), len(f.file))
    assert ix.blocks == 2 and ix.verdict == OK
    assert eng.bgzf_read_stats()[3:5] == [66, 64]
    whole(eng, f)


def test_the_chain_crosses_list_windows(eng, monkeypatch):
    monkeypatch.setenv("BZ_DF_BGZF_BATCH", "4")
    f = F.of_chunks([F.text(80 + 9 * k, k) for k in range(11)])
    whole(eng, f)
    assert eng.bgzf_read_stats()[7] == 6           # three groups of at most four blocks: decode and check each
    g, _ = F.nested()
    t = on_device(g.file)
    ix = eng.bgzf_index_device(t.data_ptr(), len(g.file))
    assert (ix.coff, ix.uoff, ix.verdict) == (g.coff, g.uoff, OK) and eng.bgzf_read_stats()[3:5] == [66, 64]


def test_cap_blocks_one_too_small(eng, pkg):
    f = F.clean_files()["forty_blocks"]
    t = on_device(f.file)
    L = pkg.lib()
    n, v = C.c_size_t(0), C.c_int32(0)
    coff, uoff = (C.c_uint64 * 42)(), (C.c_uint64 * 42)()
    assert L.df_gpu_bgzf_index_device(eng._h, t.data_ptr(), len(f.file), coff, uoff, 40, C.byref(n), C.byref(v)) == pkg.BZ_E_CAPACITY
    assert n.value == 41                            # forty blocks and the marker
    assert L.df_gpu_bgzf_index_device(eng._h, t.data_ptr(), len(f.file), None, None, 0, C.byref(n), C.byref(v)) == pkg.BZ_E_CAPACITY
    assert n.value == 41
    assert L.df_gpu_bgzf_index_device(eng._h, t.data_ptr(), len(f.file), coff, uoff, 41, C.byref(n), C.byref(v)) == pkg.BZ_OK
    assert list(coff) == f.coff and list(uoff) == f.uoff and v.value == OK
    with pytest.raises(pkg.CompressionError) as ei:
        eng.bgzf_index_device(t.data_ptr(), len(f.file), cap_blocks=40)
    assert ei.value.kind == "Capacity"
    assert L.df_gpu_bgzf_index_device(eng._h, t.data_ptr() + 1, 8, coff, uoff, 41, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM   # misaligned


# ---- 2. whole-file reads of clean files
def _kinds_file():
    a, b, c, d = F.text(700, 1), F.text(901, 2), F.text(1203, 3), F.text(2000, 4)
    return F.File([(bgzfref.wrap(a, F.stored(a)), a), (bgzfref.wrap(b, F.fixed(b)), b), (bgzfref.wrap(c, F.dynamic(c)), c),
                   (bgzfref.wrap(d, F.three_blocks(d)), d), (bgzfref.EOF, b"")])


def _forged_copies_file():
    pre = dfforge.text(300, 3)
    s1 = dfforge.Stream().fixed(final=True).lit(pre).match(100, len(pre)).lit(b"tail").eob()       # distance == position
    s2 = dfforge.Stream().fixed(final=True).lit(b"a").match(258, 1).lit(pre).lit(b"z").match(258, 1).eob()   # runs at both ends
    return F.File([(bgzfref.wrap(bytes(s.out), s.raw()), bytes(s.out)) for s in (s1, s2, s1)])


def _full_block_file():
    d = bytes(60000) + F.text(5536, 8)
    assert len(d) == 65536
    return F.File([(F.zblock(F.text(77, 1)), F.text(77, 1)), (F.zblock(d), d), (F.zblock(F.text(78, 2)), F.text(78, 2))])


CLEAN = {"kinds": _kinds_file, "forged_copies": _forged_copies_file, "isize_65536": _full_block_file, "phases": F.phase_file,
         "empty_in_the_middle": lambda: F.clean_files()["empty_in_the_middle"], "marker_alone": lambda: F.clean_files()["marker_alone"],
         "forty_blocks": lambda: F.clean_files()["forty_blocks"], "length_residues": lambda: F.clean_files()["length_residues"]}


@pytest.mark.parametrize("name", sorted(CLEAN))
def test_whole_file(eng, name):
    whole(eng, CLEAN[name]())


def test_every_clean_forged_stream_as_a_block(eng):
    """The decode loop is the one the entry and piece kernels run: its BGZF form sees the corpus they see -- every clean raw
    stream of dfforge.clean_cases() that fits a block (all but stored_65535), a block each; the expected bytes are the forge's.
    Whole, then as a range that begins inside the first block and ends inside the last: both edge blocks go through a slot."""
    f, left_out = F.forged_clean_file()
    assert left_out == ["stored_65535"] and f.count == 159
    whole(eng, f)
    s, e = 1, f.uoff[-1] - 1
    assert 0 < s < f.uoff[1] and f.uoff[-2] < e < f.uoff[-1]
    t = on_device(f.file)
    read(eng, t.data_ptr(), len(f.file), (f.coff, f.uoff), s, e - s, f.data[s:e], phases=(next(_turn),))
    assert eng.bgzf_read_stats()[1:3] == [f.count - 2, 2] == list(_counts(f.uoff, s, e - s))


@pytest.mark.parametrize("block_bytes", [4093, 65280])
def test_whole_file_of_the_writers_own_output(eng, pkg, block_bytes):
    data = F.text(block_bytes + 1000 if block_bytes == 65280 else 3 * block_bytes + 17, 6)
    file, offs = pkg.bgzf_compress(data, block_bytes, offsets=True)
    chunks = [data[a:a + block_bytes] for a in range(0, len(data), block_bytes)]
    f = F.File([(file[offs[k]:offs[k + 1]], chunks[k]) for k in range(len(chunks))] + [(file[offs[-1]:], b"")])
    assert f.file == file and gzip.decompress(file) == data
    whole(eng, f)


# ---- 3. range reads
@pytest.fixture(scope="module")
def twelve():
    f = F.of_chunks([F.text(300 + 173 * ((5 * k) % 12), 30 + k) for k in range(12)], level=9)
    return f, on_device(f.file)


def _counts(uoff, ustart, ulen):
    """(blocks written in place, edge blocks) of a range, from the index alone"""
    lo, hi = ustart, min(ustart + ulen, uoff[-1])
    if lo >= hi:
        return 0, 0
    ks = [k for k in range(len(uoff) - 1) if uoff[k] < hi and uoff[k + 1] > lo]
    ks = range(ks[0], ks[-1] + 1)
    edge = sum(1 for k in ks if uoff[k] < lo or uoff[k + 1] > hi)
    return len(ks) - edge, edge


def test_the_range_grid(eng, twelve):
    f, t = twelve
    total = len(f.data)
    marks = sorted({e + d for e in f.uoff for d in (-1, 0, 1) if 0 <= e + d <= total})
    ranges = set()
    for s in marks:
        nxt = [e for e in f.uoff if e > s]
        for e in {s + 1, total} | {x + d for x in nxt[:1] for d in (-1, 0, 1)} | {x + 1 for x in nxt[4:5]}:
            if s < e <= total:
                ranges.add((s, e - s))
    ranges |= {(f.uoff[3] + 20, 50), (f.uoff[4], f.uoff[5] - f.uoff[4]), (f.uoff[2] + 9, f.uoff[6] + 5 - f.uoff[2] - 9)}
    ranges |= {(5, 0), (total, 7), (total - 1, 7), (total + 5, 7), (f.uoff[10] + 3, 1 << 40)}
    assert len(ranges) > 150
    for s, n in sorted(ranges):
        read(eng, t.data_ptr(), len(f.file), (f.coff, f.uoff), s, n, f.data[s:s + n], phases=(next(_turn),))
        st = eng.bgzf_read_stats()
        if extent(f.uoff, s, n):
            assert (st[1], st[2]) == _counts(f.uoff, s, n), (s, n)
            assert st[0] == st[1] + st[2] and st[6] == extent(f.uoff, s, n)


def test_ranges_at_every_phase(eng, twelve):
    f, t = twelve
    for s, n in ((f.uoff[3] + 20, 50), (f.uoff[4], f.uoff[5] - f.uoff[4]), (f.uoff[2] + 9, f.uoff[7] - f.uoff[2] - 20), (0, len(f.data))):
        read(eng, t.data_ptr(), len(f.file), (f.coff, f.uoff), s, n, f.data[s:s + n])
    assert _counts(f.uoff, f.uoff[2] + 9, f.uoff[7] - f.uoff[2] - 20) == (3, 2)      # cuts the first and the last of five blocks


def test_an_edge_block_whose_matches_reach_in_front_of_the_range(eng):
    chunk = (b"abcdefghij" * 40) + F.text(300, 2) + (b"0123456789" * 40)
    f = F.of_chunks([F.text(100, 1), chunk, F.text(100, 3)], level=9)
    t = on_device(f.file)
    for s in (f.uoff[1] + 15, f.uoff[1] + 395, f.uoff[1] + 1000):
        read(eng, t.data_ptr(), len(f.file), (f.coff, f.uoff), s, 80, f.data[s:s + 80])
        assert eng.bgzf_read_stats()[1:3] == [0, 1]


def test_a_rebased_index(eng, twelve):
    f, t = twelve
    base = f.coff[5] & ~15
    assert 0 < base
    ix = ([c - base for c in f.coff[5:]], f.uoff[5:])
    for s, n in ((f.uoff[5], 1 << 40), (f.uoff[6] + 11, f.uoff[9] - f.uoff[6])):
        read(eng, t.data_ptr() + base, len(f.file) - base, ix, s, n, f.data[s:s + n])
    with pytest.raises(product().CompressionError) as ei:          # in front of the index's first block
        eng.bgzf_read_device(t.data_ptr() + base, len(f.file) - base, ix, f.uoff[5] - 1, 9, None, 0)
    assert ei.value.kind == "Param"


def test_the_writers_offsets_as_the_index(eng, pkg):
    import torch
    B = 4093
    data = F.text(5 * B + 700, 12)
    src = on_device(data)
    dst = torch.zeros(pkg.bgzf_bound(len(data), B), dtype=torch.uint8, device="cuda")
    n, offs = eng.bgzf_encode_device(src.data_ptr(), len(data), dst.data_ptr(), dst.numel(), B, True, offsets=True)
    index = (offs, [min(k * B, len(data)) for k in range(len(offs))])
    assert len(offs) == 7 and gzip.decompress(dst.cpu().numpy().tobytes()[:n]) == data
    for s, m in ((0, len(data)), (B - 1, 2), (2 * B + 5, 3 * B), (len(data) - 3, 99)):
        read(eng, dst.data_ptr(), offs[-1], index, s, m, data[s:s + m])


def test_cap_one_short(eng, pkg, twelve):
    import torch
    f, t = twelve
    buf = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    L = pkg.lib()
    coff, uoff = (C.c_uint64 * 13)(*f.coff), (C.c_uint64 * 13)(*f.uoff)
    n, v = C.c_uint64(0), C.c_int32(0)
    rc = L.df_gpu_bgzf_read_device(eng._h, t.data_ptr(), len(f.file), coff, uoff, 12, 10, 1000, buf.data_ptr(), 999, C.byref(n), C.byref(v))
    torch.cuda.synchronize()
    assert rc == pkg.BZ_E_CAPACITY and n.value == 1000
    assert buf.cpu().numpy().tobytes() == bytes([FILL]) * 4096               # not one byte of d_out changed


# ---- 4. faults
def _seven(bad=None, at=(3,)):
    """seven blocks; `bad` = (block bytes, the ISIZE its trailer claims) replaces each block of `at`.  The index follows the
    file: coff from the blocks' lengths, uoff from the ISIZE fields."""
    chunks = [F.text(150 + 31 * k, 50 + k) for k in range(7)]
    blocks = [F.zblock(c) for c in chunks]
    sizes = [len(c) for c in chunks]
    for k in at if bad else ():
        blocks[k], sizes[k] = bad
    coff, uoff = [0], [0]
    for b, n in zip(blocks, sizes):
        coff.append(coff[-1] + len(b))
        uoff.append(uoff[-1] + n)
    return b"".join(blocks), (coff, uoff), chunks


def _bad_blocks():
    d = F.text(400, 77)
    raw = F.raw_deflate(d)
    out = {"wrong_crc": (F.block(raw, d, crc=zlib.crc32(d) ^ 0x100), len(d)),
           "isize_one_more": (F.block(raw, d, isize=len(d) + 1), len(d) + 1),
           "isize_one_less": (F.block(raw, d, isize=len(d) - 1), len(d) - 1),
           "one_byte_more_than_isize": (F.block(F.raw_deflate(d + b"x"), d), len(d)),
           "one_byte_fewer_than_isize": (F.block(F.raw_deflate(d[:-1]), d), len(d)),
           "two_spare_bytes": (F.block(raw + b"\0\0", d), len(d)),
           "stream_cut_by_bsize": (F.block(raw[:-3], d), len(d))}
    s = dfforge.Stream().fixed(final=True).lit(b"ab").match(3, 3, emit=False).lit(b"c").eob()   # one beyond the block's start
    out["distance_in_front_of_the_block"] = (F.block(s.raw(), b"ab" + b"?" * 4), 6)
    return out


@pytest.mark.parametrize("name", sorted(_bad_blocks()))
def test_a_fault_in_block_3_of_7(eng, name):
    file, index, chunks = _seven(_bad_blocks()[name])
    t = on_device(file)
    front = b"".join(chunks[:3])
    read(eng, t.data_ptr(), len(file), index, 0, 1 << 30, front, E_DATA)
    # the same fault in an edge block: the range ends, then starts, inside block 3
    read(eng, t.data_ptr(), len(file), index, 7, index[1][3] + 2 - 7, front[7:], E_DATA, phases=(1,))
    read(eng, t.data_ptr(), len(file), index, index[1][3] + 1, 1 << 30, b"", E_DATA, phases=(7,))
    # a fault in a block outside the range: the read is clean
    read(eng, t.data_ptr(), len(file), index, 5, index[1][3] - 5, front[5:], OK, phases=(15,))
    tail = b"".join(chunks[4:])
    read(eng, t.data_ptr(), len(file), index, index[1][4], 1 << 30, tail, OK, phases=(0,))


def test_every_malformed_stream_in_block_3(eng):
    cases = [c for c in dfforge.malformed_cases() if c.kind == dfforge.RAW]
    assert len(cases) >= 25
    for c in cases:
        file, index, chunks = _seven((F.block(c.stream, c.data), len(c.data)))
        t = on_device(file)
        read(eng, t.data_ptr(), len(file), index, 0, 1 << 30, b"".join(chunks[:3]), E_DATA, phases=(next(_turn),))


def test_an_index_that_disagrees_with_the_file(eng):
    file, (coff, uoff), chunks = _seven()
    t = on_device(file)
    front = b"".join(chunks[:3])
    u = list(uoff)
    u[4] += 1                                         # block 3's ISIZE is not uoff[4] - uoff[3]
    read(eng, t.data_ptr(), len(file), (coff, u), 0, 1 << 30, front, E_DATA)
    c = list(coff)
    c[3] += 1                                         # no header at coff[3]; block 2 is one byte longer than its BSIZE says:
    read(eng, t.data_ptr(), len(file), (c, uoff), 0, 1 << 30, b"".join(chunks[:2]), E_DATA)   # the lowest k, block 2, decides
    read(eng, t.data_ptr(), len(file), (c, uoff), uoff[3], 1 << 30, b"", E_DATA)              # block 3 alone: nothing in front
    read(eng, t.data_ptr(), len(file), (c, uoff), 0, uoff[2], b"".join(chunks[:2]), OK)       # blocks 0 and 1 are as they were


def test_the_lower_of_two_faulty_blocks_decides(eng):
    bad = _bad_blocks()["wrong_crc"]
    file, index, chunks = _seven(bad, at=(3, 5))
    t = on_device(file)
    read(eng, t.data_ptr(), len(file), index, 0, 1 << 30, b"".join(chunks[:3]), E_DATA)
    read(eng, t.data_ptr(), len(file), index, index[1][4], 1 << 30, chunks[4], E_DATA)


def test_parameter_errors_with_an_engine(eng, pkg):
    file, (coff, uoff), _ = _seven()
    t = on_device(file)
    P = pkg.CompressionError

    def param(*a):
        with pytest.raises(P) as ei:
            eng.bgzf_read_device(*a)
        assert ei.value.kind == "Param"
    c = list(coff)
    c[2], c[3] = c[3], c[2]
    param(t.data_ptr(), len(file), (c, uoff), 0, 10, None, 0)                       # unsorted
    u = list(uoff)
    u[2], u[3] = u[3], u[2]
    param(t.data_ptr(), len(file), (coff, u), 0, 10, None, 0)
    param(t.data_ptr(), len(file) - 1, (coff, uoff), 0, 10, None, 0)                # coff[count] > in_len
    param(t.data_ptr() + 4, len(file) - 4, ([x for x in coff[:2]], uoff[:2]), 0, 10, None, 0)   # d_in misaligned
    param(t.data_ptr(), len(file), (coff[:2], [0, 65537]), 0, 10, None, 0)          # a block longer than 65 536 bytes
    L = pkg.lib()
    n, v = C.c_uint64(0), C.c_int32(0)
    a = (C.c_uint64 * 8)(*coff)
    assert L.df_gpu_bgzf_read_device(eng._h, t.data_ptr(), len(file), a, a, 7, 0, 1, None, 0, None, C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_gpu_bgzf_read_device(eng._h, t.data_ptr(), len(file), a, a, 7, 0, 1, None, 0, C.byref(n), None) == pkg.BZ_E_PARAM
    assert L.df_gpu_bgzf_read_device(eng._h, t.data_ptr(), len(file), None, a, 7, 0, 1, None, 0, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM


# ---- 5. the host forms
@pytest.mark.parametrize("name", sorted(CLEAN))
def test_host_forms_on_clean_files(pkg, name):
    f = CLEAN[name]()
    assert pkg.bgzf_decompress(f.file) == f.data
    total = len(f.data)
    for s, n in ((0, total), (1, 10), (total // 3, total // 2), (max(total - 1, 0), 5), (f.uoff[f.count // 2], 1 << 40)):
        assert pkg.bgzf_read(f.file, s, n) == f.data[s:s + n], (s, n)
    assert pkg.bgzf_read(f.file, 0, None, index=pkg.bgzf_index(f.file)) == f.data


def test_host_read_of_one_block_out_of_forty(pkg):
    f = F.clean_files()["forty_blocks"]
    k = next(k for k in range(5, 40) if f.coff[k] % 2 == 1)
    assert pkg.bgzf_read(f.file, f.uoff[k], f.uoff[k + 1] - f.uoff[k]) == f.chunks[k]
    assert pkg.bgzf_read(f.file, f.uoff[k] + 3, 9) == f.chunks[k][3:12]


@pytest.mark.parametrize("name", sorted(_bad_blocks()))
def test_host_forms_on_faulty_blocks(pkg, name):
    bad = _bad_blocks()[name]
    file, (coff, uoff), chunks = _seven(bad)
    front = b"".join(chunks[:3])
    if F.chain(file) == (coff, uoff, OK):     # (the host form walks the file itself: a forged BSIZE or ISIZE moves its chain)
        with pytest.raises(pkg.BgzfError) as ei:
            pkg.bgzf_decompress(file)
        assert ei.value.kind == "DataError" and ei.value.partial == front
        assert pkg.bgzf_read(file, 3, uoff[3] - 3) == front[3:]
        with pytest.raises(pkg.BgzfError) as ei:
            pkg.bgzf_read(file, uoff[3] + 1, 5)
        assert ei.value.kind == "DataError" and ei.value.partial == b""


@pytest.mark.parametrize("case", F.chain_faults(), ids=lambda c: c[0])
def test_host_forms_on_every_verdict_of_the_chain(pkg, case):
    name, data, v, n, base = case
    good = base.data[:base.uoff[n]]
    if v == OK:
        assert pkg.bgzf_decompress(data) == good
        return
    with pytest.raises(pkg.BgzfError) as ei:
        pkg.bgzf_decompress(data)
    assert ei.value.kind == ("DataError" if v == E_DATA else "UnexpectedEof") and ei.value.partial == good
    assert pkg.bgzf_read(data, 10, len(good) - 10) == good[10:]              # a range in front of the fault is clean
    with pytest.raises(pkg.BgzfError) as ei:
        pkg.bgzf_read(data, 10, len(good))                                  # one byte behind the indexed blocks
    assert ei.value.partial == good[10:]
