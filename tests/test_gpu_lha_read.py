"""GPU tests of the LHA archive reader (include/bz2_mi355x.h section 11, DESIGN_lzhuf.md section 12).  The archives are those
of tests/lhaforge.py, which tests/test_lhaforge.py and tests/test_lha_index_host.py pin; every expected byte is one of the
forge's own plaintexts, every expected verdict and figure comes from what the forge wrote into the archive."""
import contextlib
import os

import pytest

import lhaforge as F
from conftest import product

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, 64
SWITCHES = ("BZ_LHA_CRC_PART_KIB", "BZ_LZH_SPLIT_KIB", "BZ_LZH_SPLIT_CAND_BYTES")
CORPUS = {c["name"]: c for c in F.load()}


@contextlib.contextmanager
def env(values):
    """the switches are read per call"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def slots(idx, sel, n):
    """the layout rule of section 11, restated: a member's slot is its original length when it can have bytes at all"""
    out, cursor, need = [], 0, 0
    for i in sel:
        m = idx[i]
        code = F.method_code(m.method)
        has = (code == F.STORED or 4 <= code <= 7) and m.data_off + m.packed_len <= n and not (code == F.STORED and m.packed_len != m.orig_len)
        s = m.orig_len if has else 0
        out.append(cursor)
        if s:
            need = cursor + s
        cursor += (s + 15) & ~15
    return out, need


def read_device(eng, data, sel=None, prefill=0x20, crc_faults=()):
    """-> [(bytes, verdict)] of one device call: d_in and d_out between guards of 64 bytes of 0xEE, sizes-only against the real
    call, capacity one byte short, the placement rule, nothing written outside the reported ranges.  crc_faults: positions in
    the selection whose only fault is the CRC (sizes-only computes none)."""
    import torch
    pkg = product()
    idx = pkg.lha_index(data)
    which = list(range(len(idx))) if sel is None else list(sel)
    t = torch.frombuffer(bytearray([FILL]) * GUARD + bytearray(data), dtype=torch.uint8).cuda()   # (ends with the archive's last byte)
    d_in = t.data_ptr() + GUARD
    assert d_in % 16 == 0
    s_off, s_len, s_ver = eng.lha_read_device(d_in, len(data), idx, None, 0, sel, prefill)
    place, cap = slots(idx, which, len(data))
    assert s_off == place
    o = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert o.data_ptr() % 16 == 0
    if cap:
        with pytest.raises(pkg.CompressionError) as ei:
            eng.lha_read_device(d_in, len(data), idx, o.data_ptr() + GUARD, cap - 1, sel, prefill)
        assert ei.value.code == pkg.BZ_E_CAPACITY
        torch.cuda.synchronize()
        assert bool((o == FILL).all())
    try:
        o_off, o_len, ver = eng.lha_read_device(d_in, len(data), idx, o.data_ptr() + GUARD, cap, sel, prefill)
    finally:
        torch.cuda.synchronize()
        host = o.cpu().numpy().tobytes()
    assert (o_off, o_len) == (s_off, s_len)
    assert [pkg.BZ_OK if k in crc_faults else v for k, v in enumerate(ver)] == s_ver
    assert host[:GUARD] == bytes([FILL]) * GUARD
    body, end = host[GUARD:], 0
    for a, n in zip(o_off, o_len):
        assert a % 16 == 0 and a >= end
        if n:   # (a member without bytes has a place and nothing at it)
            assert body[end:a] == bytes([FILL]) * (a - end)
            end = a + n
    assert end <= cap and body[end:] == bytes([FILL]) * (len(body) - end)
    return [(body[a:a + n], v) for a, n, v in zip(o_off, o_len, ver)]


def crc_positions(want):
    return {k for k, (b, v) in enumerate(want) if v == F.E_DATA and b}


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_every_archive_of_the_corpus(eng, name):
    a = F.build(CORPUS[name])
    for prefill in a.prefills:
        want = a.expect(prefill)
        with env(a.env):
            got = read_device(eng, a.data, None, prefill, crc_positions(want))
            stats = eng.lha_read_stats()
            split = eng.lzh_decode_split_stats()
        assert [v for _, v in got] == [v for _, v in want], (name, prefill)
        assert got == want, (name, prefill)
        assert stats[:7] == a.stats(prefill), (name, prefill)
        assert stats[7] >= 1 or not any(b for b, _ in want)
        if name == "S_split":
            assert split[0] == 1 and split[7] == 0


def test_the_default_part_size_and_a_small_one_agree(eng):
    a = F.build(CORPUS["C_default"])
    want = a.expect()
    for kib in ("4", "8", None):
        with env({} if kib is None else {"BZ_LHA_CRC_PART_KIB": kib}):
            assert read_device(eng, a.data) == want, kib


def test_subsets_of_the_methods_archive(eng):
    a = F.build(CORPUS["M_methods"])
    whole = read_device(eng, a.data)
    assert whole == a.expect()
    n = len(whole)
    for sel in [[i] for i in range(n)] + [[0, 1, 2, 3], [1, 5, 7, 8, 14], [2, 4, 15]]:
        assert read_device(eng, a.data, sel) == [whole[i] for i in sel], sel


def test_the_host_call_the_archive_object_and_names(eng):
    pkg = product()
    a = F.build(CORPUS["M_methods"])
    want = a.expect()
    assert pkg.lha_extract(a.data) == want
    arc = pkg.LhaArchive(a.data)
    assert arc.read_all() == want
    assert arc.read(7) == want[7] and arc.read(b"same.txt") == want[3]
    name = arc.members[5].name
    assert pkg.lha_extract(a.data, [name, 0, "same.txt"]) == [want[5], want[0], want[3]]
    bad = F.build(CORPUS["F_member_crc"])
    res = pkg.lha_extract(bad.data)
    assert res == bad.expect() and [v for _, v in res].count(pkg.BZ_E_DATA) == 2
    with pytest.raises(pkg.CompressionError):
        pkg.lha_extract(bad.data, check=True)
    cut = F.build(CORPUS["F_header_sum"])           # the members in front of the index's fault are read
    assert pkg.lha_extract(cut.data) == cut.expect() and pkg.lha_index(cut.data).fault[0] == pkg.BZ_E_DATA


def flip_member_crc(data, m):
    """one bit of the last byte of member m's header CRC flipped (levels 0 and 1: the header's byte sum put right again)"""
    d = bytearray(data)
    p = m.header_off
    at = p + 22 if m.level == 2 else p + 22 + d[p + 21] + 1
    d[at] ^= 0x10
    if m.level < 2:
        d[p + 1] = sum(d[p + 2:p + 2 + d[p]]) & 255
    return bytes(d)


def test_the_crc_of_every_member_through_a_mismatch(eng):
    pkg = product()
    a = F.build(CORPUS["C_parts"])
    want = a.expect()
    idx = pkg.lha_index(a.data)
    assert len(idx) == 2 * len(F.CRC_SIZES)
    with env(a.env):
        for k, m in enumerate(idx):
            assert m.level != 2 or F.index(a.data)[0][k]["name_len"] > 0
            d = flip_member_crc(a.data, m)
            assert pkg.lha_index(d).fault == pkg.BZ_OK
            got = read_device(eng, d, None, 0x20, {k})
            assert got == [(b, F.E_DATA if j == k else v) for j, (b, v) in enumerate(want)], k
            assert eng.lha_read_stats()[5] == 1


def test_the_split_member_on_both_paths(eng):
    a = F.build(CORPUS["S_split"])
    want = a.expect()
    with env(a.env):
        split = read_device(eng, a.data)
        st = eng.lzh_decode_split_stats()
    with env({"BZ_LZH_SPLIT_KIB": "0"}):
        one = read_device(eng, a.data)
        st0 = eng.lzh_decode_split_stats()
    assert split == one == want
    assert st[0] == 1 and st[2] >= 20 and st0[0] == 0


def test_round_trip_from_the_projects_encoder(eng):
    import corpus
    pkg = product()
    plains = [corpus.chapter(k, 16384) for k in range(64)]
    streams = pkg.lzhuf_compress_batch(plains, pkg.LzhufMethod.Lh5)
    arc = F.wrap(zip(plains, streams))
    assert pkg.lha_index(arc).fault == pkg.BZ_OK
    got = read_device(eng, arc)
    assert [v for _, v in got] == [pkg.BZ_OK] * 64
    assert [b for b, _ in got] == plains
    assert eng.lha_read_stats()[:7] == [64, 0, 0, 0, 0, 0, 64 * 16384]
