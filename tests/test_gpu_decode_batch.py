"""GPU tests of batched decoding (bz_gpu_decode_batch_device, bz_decode_batch): many independent entries in one call,
scanned by k_dec_scan_batch, Huffman-decoded inside their own byte ranges, chained by k_dec_chain_batch (one lane per
entry) and rebuilt together.  Every entry of every batch is compared with the oracle's decode of that entry ALONE:
same bytes, same verdict."""
import bz2
import functools
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, product, sample

pytestmark = pytest.mark.gpu

E_DATA, E_MAGIC_FIRST, E_MAGIC = -1, -4, -5
MAGIC = bytes.fromhex("314159265359")

_REF = {}


def ref(oracle, z):
    """the oracle's (bytes, verdict) for one entry, computed once per distinct entry"""
    if z not in _REF:
        _REF[z] = oracle.decode(z)
    return _REF[z]


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


@functools.lru_cache(None)
def trunc_stream():
    """the stream of test_gpu_decode.py::test_truncations.  Its comment says "two blocks"; sample1.ref is 98 696 bytes, so
    the slice is all of it and the stream holds ONE block.  It stays an entry as it is; two_blocks() below is the
    stream that does hold two, and every two-block case runs on that one."""
    d = sample(1)[:150000] + b"z" * 3000
    return d, bz2.compress(d, 1)


@functools.lru_cache(None)
def two_blocks():
    from bzforge import parse
    d = sample(2)[:150000] + b"z" * 3000
    z = bz2.compress(d, 1)
    assert len(parse(z)[0].blocks) == 2
    return d, z


def cut_list(z):
    return list(range(0, 60)) + [len(z) // 3, len(z) // 2, len(z) - 11, len(z) - 10, len(z) - 5, len(z) - 4,
                                 len(z) - 3, len(z) - 2, len(z) - 1]


class Dev:
    """entries packed at 4-byte-aligned offsets behind `lead` bytes of `fill`, with `fill` in every gap; the gaps cycle
    through the smallest legal ones: 0..3 bytes to the next multiple of 4, then 0 or 4 more (tight: never more)"""

    def __init__(self, entries, fill=0, lead=0, tight=False):
        import torch
        self.torch = torch
        self.entries = entries
        assert lead % 4 == 0
        self.off, buf = [], bytearray([fill]) * lead
        for i, x in enumerate(entries):
            self.off.append(len(buf))
            buf += x
            buf += bytes([fill]) * (-len(buf) % 4 + (0 if tight or i % 2 == 0 else 4))
        self.len = [len(x) for x in entries]
        self.host_in = bytes(buf)
        self.t = torch.frombuffer(buf if buf else bytearray(4), dtype=torch.uint8).cuda()

    def sizes(self, eng):
        return eng.decode_batch_device(self.t.data_ptr(), self.off, self.len, None, 0)

    def decode(self, eng, cap=None):
        """a sizes-only call, then the real one with exactly the capacity it asks for; the checks common to all tests;
        -> [(bytes, verdict)] per entry"""
        torch = self.torch
        s_off, s_len, _ = self.sizes(eng)
        need = max([a + n for a, n in zip(s_off, s_len)] + [0])
        cap = need if cap is None else cap
        self.o = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        o_off, o_len, verdicts = eng.decode_batch_device(self.t.data_ptr(), self.off, self.len, self.o.data_ptr(), cap)
        torch.cuda.synchronize()
        self.o_off, self.o_len, self.need = o_off, o_len, need
        host = self.o.cpu().numpy().tobytes()
        assert host[cap:] == b"\xee" * 64                     # nothing at or behind d_out + cap
        assert all(a % 16 == 0 for a in o_off)
        end = 0
        for a, n in sorted(zip(o_off, o_len)):                # ranges do not overlap
            assert a >= end or n == 0
            end = max(end, a + n)
        assert end <= cap
        assert o_off == s_off                                 # a sizes-only call assigns the same places
        for n, m, v in zip(o_len, s_len, verdicts):
            assert n == m or (n < m and v == E_DATA)
        return [(host[a:a + n], v) for a, n, v in zip(o_off, o_len, verdicts)]

    def check(self, eng, oracle):
        got = self.decode(eng)
        assert len(got) == len(self.entries)
        for i, (g, z) in enumerate(zip(got, self.entries)):
            w = ref(oracle, z)
            assert g[1] == w[1], "entry %d (%d bytes): verdict %d, oracle %d" % (i, len(z), g[1], w[1])
            assert g[0] == w[0], "entry %d (%d bytes): %d bytes, oracle %d" % (i, len(z), len(g[0]), len(w[0]))
        return got


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.GpuEngine(0, 8)
    yield e
    e.close()


def edge_entries():
    d2, z2 = two_blocks()
    ents = [bz2.compress(b"", lv) for lv in (1, 9)]
    ents += [bz2.compress(bytes(range(40, 40 + n)), 9) for n in (1, 2, 3, 4, 5)]
    ents += [bz2.compress(b"\xfa" * r, 5) for r in (255, 256, 259)]
    ents += [bz2.compress(bytes(range(256)), 9), bz2.compress(sample(1), 9), trunc_stream()[1], z2]
    ents += [golden("sample4.bz2"), golden("sample3.bz2")]
    return ents


_ERRORS = []


def error_entries(pkg):
    """every malformed entry is followed by a valid one whose payload starts differently"""
    if not _ERRORS:
        _ERRORS.append(_error_entries(pkg))
    return _ERRORS[0]


def _error_entries(pkg):
    z = pkg.compress(sample(1)[:60000], 9)
    d2, z2 = two_blocks()
    bad = [b"", b"BZh0", b"BZ", z + b"garbage!", z + b"\x00"]
    crc_bad = bytearray(z2)
    crc_bad[12] ^= 1                                          # the first block's stored CRC
    comb_bad = bytearray(z2)
    comb_bad[-3] ^= 1                                         # the combined CRC
    bad += [bytes(crc_bad), bytes(comb_bad)]
    z1 = trunc_stream()[1]
    bad += [z1[:c] for c in cut_list(z1)] + [z2[:c] for c in cut_list(z2)[60:]]
    ents, valid = [], {}
    for i, b in enumerate(bad):
        ents.append(b)
        payload = sample(2)[97 * i:97 * i + 200 + i]
        valid[len(ents)] = payload
        ents.append(bz2.compress(payload, 1 + i % 9))
    return ents, valid


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("lead", [0, 64])
def test_edge_entries(eng, oracle, fill, lead):
    ents = edge_entries()
    assert {len(e) % 4 for e in ents} == {0, 1, 2, 3}
    assert len(ents[0]) == 14 and ref(oracle, ents[0]) == (b"", 0)
    d2, z2 = two_blocks()
    assert ref(oracle, z2) == (d2, 0)
    got = Dev(ents, fill, lead).check(eng, oracle)
    assert all(v == 0 for _, v in got)
    assert got[-2][0] == golden("sample4.ref")               # two streams in one entry
    stats = eng.decode_batch_stats()
    assert stats[0] == len(ents) and stats[1] == 0
    assert eng.decode_stats()["streams"] == len(ents) + 1    # sums over the call: sample4 holds two


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("lead", [0, 64])
def test_errors_among_valid_neighbours(eng, oracle, pkg, fill, lead):
    ents, valid = error_entries(pkg)
    d2, z2 = two_blocks()
    got = Dev(ents, fill, lead).check(eng, oracle)
    for i, payload in valid.items():
        assert got[i] == (payload, 0), i
    assert got[0] == (b"", E_MAGIC_FIRST) and got[2] == (b"", E_MAGIC_FIRST) and got[4] == (b"", E_MAGIC_FIRST)
    assert got[6] == (sample(1)[:60000], E_MAGIC) and got[8] == (sample(1)[:60000], E_MAGIC)
    out, v = got[10]                                          # the bytes of block 1 only, then DataError
    assert v == E_DATA and 0 < len(out) < len(d2) and out == d2[:len(out)]
    assert got[12] == (d2, E_DATA)


def test_bit_flips(eng, oracle):
    rng = random.Random(43)
    z = bz2.compress(sample(2)[:120000], 1)
    ents = []
    for _ in range(60):
        bad = bytearray(z)
        bad[rng.randrange(len(z))] ^= 1 << rng.randrange(8)
        ents.append(bytes(bad))
    for p in range(4, 120):
        bad = bytearray(z)
        bad[p] ^= 0x08
        ents.append(bytes(bad))
    assert len(ents) == 176
    Dev(ents).check(eng, oracle)


def test_block_magic_across_a_seam(eng, oracle):
    """entry A ends with the first three bytes of the block magic, entry B (no gap) starts with the other three: the
    joined bytes hold a magic that belongs to neither"""
    d = sample(1)[:3000]
    z = bz2.compress(d, 9)
    a = z + b"\x00" * (-(len(z) + 3) % 4) + MAGIC[:3]
    b = MAGIC[3:] + b"9" + z[4:]
    assert len(a) % 4 == 0
    dev = Dev([a, b], tight=True)
    assert dev.off == [0, len(a)] and dev.host_in[len(a) - 3:len(a) + 3] == MAGIC
    assert ref(oracle, a) == (d, E_MAGIC) and ref(oracle, b) == (d, 0)
    assert dev.check(eng, oracle) == [(d, E_MAGIC), (d, 0)]


def test_irregular_entry_takes_the_one_stream_path(eng, oracle):
    d = sample(1)[:40000]
    odd = bytearray(bz2.compress(d, 9))
    assert odd[4:10] == MAGIC
    odd[5:10] = b"\x00\x01\x02\x03\x04"                      # only the first byte of the magic is compared
    ents = [bz2.compress(sample(2)[:5000], 9), bytes(odd), bz2.compress(sample(2)[5000:9000], 3)]
    dev = Dev(ents)
    got = dev.check(eng, oracle)
    assert got[1] == (d, 0)
    stats = eng.decode_batch_stats()
    assert stats[0] == 2 and stats[1] == 1
    assert dev.o_off[1] >= dev.o_off[0] + dev.o_len[0] and dev.o_off[1] >= dev.o_off[2] + dev.o_len[2]


def test_chain_on_the_device_and_on_the_host_agree(eng, oracle, monkeypatch):
    """The record chain's rules live in csrc/dec_chain.h once; k_dec_chain_batch (the batch path) and the host loop of
    decode_core (the one-stream path) both walk with them.  The same entries through both: at the default every entry is
    chained on the device; with a D1 workspace of ONE block every entry that holds two block magics or more is chained
    on the host.  Same bytes, lengths and verdicts -- the oracle's -- either way.  Offsets follow the path (a one-stream
    entry lies behind everything the batch path wrote): each run's are the running sum, rounded up to 16, of the lengths
    a sizes-only call reports, over the batch path's entries in call order and then the one-stream path's."""
    d2, z2 = two_blocks()
    three = z2 * 3
    digit, comb = bytearray(three), bytearray(three)
    assert digit[len(z2):len(z2) + 4] == b"BZh1"
    digit[len(z2) + 3] = ord("0")                             # the second stream's level digit
    comb[-3] ^= 1                                             # the last combined CRC
    main = [z2, three, bytes(digit), bytes(comb), three[:-1], three[:-5], three[:-11]]
    ents = []
    for i, z in enumerate(main):
        ents += [z, bz2.compress(sample(2)[97 * i:97 * i + 200 + i], 1)]
    ents.pop()                                                # a valid one-block neighbour BETWEEN each
    assert len(ents) == 13
    slow = list(range(0, 13, 2))                              # the entries with two magics or more

    def run(order):
        dev = Dev(ents)
        _, s_len, _ = dev.sizes(eng)
        got = dev.check(eng, oracle)
        want_off, end = [0] * len(ents), 0
        for i in order:
            want_off[i] = (end + 15) & ~15
            end = want_off[i] + s_len[i]
        assert dev.o_off == want_off
        return got, dev.o_len, eng.decode_batch_stats()

    got_a, len_a, stats_a = run(list(range(13)))
    assert stats_a[0] == 13 and stats_a[1] == 0
    monkeypatch.setenv("BZ_DEC_BATCH", "1")
    got_b, len_b, stats_b = run([i for i in range(13) if i not in slow] + slow)
    assert stats_b[1] == len(slow) > 0 and stats_b[0] == 13 - len(slow)
    assert got_a == got_b and len_a == len_b
    assert got_a[0] == (d2, 0) and got_a[2] == (d2 * 3, 0)
    assert got_a[4] == (d2, E_MAGIC) and got_a[6] == (d2 * 3, E_DATA)
    assert [v for _, v in got_a[8::2]] == [E_DATA] * 3 and [v for _, v in got_a[1::2]] == [0] * 6


def test_group_seams(eng, oracle, monkeypatch):
    """a workspace of three blocks: groups end where the next entry does not fit, and the entry of four blocks fits none"""
    monkeypatch.setenv("BZ_DEC_BATCH", "3")
    src = sample(2) + sample(1) + sample(2)
    blocks = [1, 1, 1, 2, 1, 3, 4, 1]
    datas = [src[1000 * i:1000 * i + 100000 * k - 50000] for i, k in enumerate(blocks)]
    ents = [bz2.compress(d, 1) for d in datas]
    got = Dev(ents).check(eng, oracle)
    assert got == [(d, 0) for d in datas]
    stats = eng.decode_batch_stats()
    assert stats[0] == 7 and stats[1] == 1 and stats[2] == sum(blocks) - 4 and stats[3] >= 4


def test_junk_entry_full_of_block_magics(eng, oracle, monkeypatch):
    """more candidates than the scan's first guess holds (its second attempt), and more than a group holds: the entry
    takes the one-stream path, its neighbours the batch path"""
    monkeypatch.setenv("BZ_DEC_BATCH", "8")
    d = sample(1)[:20000]
    junk = bz2.compress(d, 9) + b"BZh9" + (MAGIC + b"\x00\x11") * 1500
    ents = [bz2.compress(sample(2)[:3000], 9), junk, bz2.compress(sample(2)[3000:7000], 9)]
    got = Dev(ents).check(eng, oracle)
    assert got[1][0] == d and got[1][1] != 0 and got[0][1] == got[2][1] == 0
    stats = eng.decode_batch_stats()
    assert stats[0] == 2 and stats[1] == 1 and stats[3] == 2   # (no group reaches across the entry in the middle)
    assert eng.decode_stats()["candidates"] >= 1500


def test_many_tiny_entries(eng, oracle):
    datas = [bytes([65 + i % 26]) * (i + 1) for i in range(600)]
    ents = [bz2.compress(d, 1 + i % 9) for i, d in enumerate(datas)]
    got = Dev(ents).check(eng, oracle)
    assert got == [(d, 0) for d in datas]
    assert eng.decode_batch_stats()[:2] == [600, 0]


def test_sizes_only_and_capacity(eng, oracle, pkg):
    d2, z2 = two_blocks()
    crc_bad = bytearray(z2)
    crc_bad[12] ^= 1
    ents = [bz2.compress(sample(2)[:7000], 9), bytes(crc_bad), b"", bz2.compress(sample(2)[7000:9001], 2)]
    dev = Dev(ents)
    s_off, s_len, _ = dev.sizes(eng)
    got = dev.check(eng, oracle)                              # (compares the offsets and the lengths with the sizes-only call's)
    need = max(a + n for a, n in zip(s_off, s_len))
    assert dev.need == need
    assert s_len[1] == len(d2) > dev.o_len[1] and got[1][1] == E_DATA
    assert s_len[0] == dev.o_len[0] == 7000 and s_len[3] == dev.o_len[3] == 2001
    with pytest.raises(pkg.CompressionError) as ei:
        dev.decode(eng, cap=need - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def text(seed, n):
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(1, 199, size=n, dtype=np.int64)) % 199).astype(np.uint8).tobytes()


def edge_inputs():
    """the shapes of the batch encoder's edge test"""
    piece, seg = 4096, 16
    ins = [bytes(range(7, 7 + n)) for n in (0, 1, 2, 3, 4, 5, 15, 16, 17)]
    ins += [b"\xfa" * r for r in (4, 5, 254, 255, 256, 259, 510, 511)]
    ins += [text(1, piece - 2) + b"\xfb" * 7 + text(2, 100), text(3, piece - 3) + b"\xfb" * 300 + text(4, 50)]
    ins += [text(5, 5 * seg - 2) + b"\xfc" * 5 + text(6, 9), text(7, 37 * seg - 1) + b"\xfc" * 4 + text(8, 3)]
    ins += [rnd(n, n) for n in (4095, 4096, 4097)]
    ins += [text(9, 1000) + b"\xfd" * 4, text(10, piece - 4) + b"\xfd" * 4]
    ins += [bytes(range(256)), sample(1)]
    ins += [golden("fuzz_r6_%s.bin" % s) for s in ("links_2414", "links_880", "small_1522")]
    return ins


def test_round_trip_with_the_batch_encoder_on_the_device(eng, pkg):
    """encode_batch_device -> decode_batch_device -> encode_batch_device: each call takes the (buffer, offsets, lengths)
    of the one in front as they are"""
    import torch
    ins = edge_inputs()
    off, buf = [], bytearray()
    for x in ins:
        off.append(len(buf))
        buf += x
        buf += bytes(-len(buf) % 16 + 16)
    lens = [len(x) for x in ins]
    t_in = torch.frombuffer(buf, dtype=torch.uint8).cuda()
    ecap = pkg.encode_batch_bound(lens)
    t_z = torch.full((ecap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    z_off, z_len = eng.encode_batch_device(9, t_in.data_ptr(), off, lens, t_z.data_ptr(), ecap)
    s_off, s_len, _ = eng.decode_batch_device(t_z.data_ptr(), z_off, z_len, None, 0)
    cap = max(a + n for a, n in zip(s_off, s_len))
    t_d = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_off, d_len, verdicts = eng.decode_batch_device(t_z.data_ptr(), z_off, z_len, t_d.data_ptr(), cap)
    assert eng.decode_batch_stats()[:2] == [len(ins), 0]
    torch.cuda.synchronize()
    host = t_d.cpu().numpy().tobytes()
    assert host[cap:] == b"\xee" * 64
    assert verdicts == [0] * len(ins)
    for i, x in enumerate(ins):
        assert host[d_off[i]:d_off[i] + d_len[i]] == x, i
    t_z2 = torch.full((ecap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    z2_off, z2_len = eng.encode_batch_device(9, t_d.data_ptr(), d_off, d_len, t_z2.data_ptr(), ecap)
    torch.cuda.synchronize()
    first, second = t_z.cpu().numpy().tobytes(), t_z2.cpu().numpy().tobytes()
    assert z2_len == z_len
    for a, b, n in zip(z_off, z2_off, z_len):
        assert first[a:a + n] == second[b:b + n]


def test_parameter_errors(eng, oracle, pkg):
    ents = [bz2.compress(sample(2)[:1000], 9), bz2.compress(sample(2)[1000:3000], 9)]
    dev = Dev(ents)
    o = dev.torch.full((4096,), 0xEE, dtype=dev.torch.uint8, device="cuda")
    for off, ln in (([0, dev.off[1] + 2], dev.len),          # not a multiple of 4
                    ([0, dev.off[1] - 4], dev.len),          # the second entry begins inside the first
                    ([dev.off[1], dev.off[0]], dev.len)):    # out of order
        with pytest.raises(pkg.CompressionError) as ei:
            eng.decode_batch_device(dev.t.data_ptr(), off, ln, o.data_ptr(), 4096)
        assert ei.value.code == pkg.BZ_E_PARAM
    with pytest.raises(pkg.CompressionError) as ei:
        eng.decode_batch_device(dev.t.data_ptr() + 2, dev.off, dev.len, o.data_ptr(), 4096)
    assert ei.value.code == pkg.BZ_E_PARAM
    assert eng.decode_batch_device(dev.t.data_ptr(), [], [], o.data_ptr(), 4096) == ([], [], [])  # count == 0: BZ_OK
    dev.torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == b"\xee" * 4096       # none of these calls wrote anything
    assert [v for _, v in dev.check(eng, oracle)] == [0, 0]


def test_host_interface(pkg):
    ents, valid = error_entries(pkg)
    got = pkg.decompress_batch(ents)
    assert got == [pkg.decompress(e) for e in ents]
    for i, payload in valid.items():
        assert got[i] == (payload, 0)
    datas = [sample(1)[4000 * i:4000 * i + 1 + 977 * i] for i in range(18)] + [b"", b"\x00" * 300]
    assert pkg.decompress_batch(pkg.compress_batch(datas)) == [(d, 0) for d in datas]
    assert pkg.decompress_batch(pkg.compress_batch(datas)) == [(d, 0) for d in datas]   # (the cached engine)


def test_host_interface_one_stream_path(pkg):
    """an entry whose first block lacks its full magic, between plain ones and an empty one: its bytes lie behind the
    others' in the one buffer"""
    d = sample(1)[:40000]
    odd = bytearray(bz2.compress(d, 9))
    odd[5:10] = b"\x00\x01\x02\x03\x04"
    ents = [bz2.compress(sample(2)[:5000], 9), bytes(odd), b"", bz2.compress(sample(2)[5000:9000], 3), bytes(odd)]
    assert pkg.decompress_batch(ents) == [(sample(2)[:5000], 0), (d, 0), (b"", E_MAGIC_FIRST), (sample(2)[5000:9000], 0), (d, 0)]
