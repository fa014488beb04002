"""GPU tests of batched encoding (bz_gpu_encode_batch_device, bz_encode_batch): many inputs, one stream each, the
one-block inputs split by k_rle_batch (one workgroup per input, pieces of 4096 bytes, 16 bytes per lane) and encoded as
the blocks of one pipeline call.  Every stream is compared with the oracle's for that input alone, byte for byte."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, product, sample

pytestmark = pytest.mark.gpu

PIECE, SEG = 4096, 16


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def text(seed, n):
    """n bytes below 199, no two neighbours equal: RLE1 leaves them alone"""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.integers(1, 199, size=n, dtype=np.int64)) % 199).astype(np.uint8).tobytes()


def golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def worst_case(n):
    out = bytearray()
    for i in range(n // 4):
        out += bytes([0x41 + i % 2]) * 4
    return bytes(out + bytes([0x61, 0x62, 0x63][:n % 4]))


def one_block(n, level):
    return 5 * (n // 4) + n % 4 <= 100000 * level - 19


def edge_inputs():
    ins = [bytes(range(7, 7 + n)) for n in (0, 1, 2, 3, 4, 5, 15, 16, 17)]                 # distinct bytes
    ins += [b"\xfa" * r for r in (4, 5, 254, 255, 256, 259, 510, 511)]                      # the 255 cap and the chunk behind it
    ins += [text(1, PIECE - 2) + b"\xfb" * 7 + text(2, 100)]                                # a run across offset 4096
    ins += [text(3, PIECE - 3) + b"\xfb" * 300 + text(4, 50)]                               # ... with a count byte above 251 - 4
    ins += [text(5, 5 * SEG - 2) + b"\xfc" * 5 + text(6, 9)]                                # a run across a 16-byte lane edge
    ins += [text(7, 37 * SEG - 1) + b"\xfc" * 4 + text(8, 3)]                               # four bytes, one in front of the edge
    ins += [rnd(n, n) for n in (4095, 4096, 4097)]
    ins += [text(9, 1000) + b"\xfd" * 4, text(10, PIECE - 4) + b"\xfd" * 4]                 # ends in a run of exactly 4
    ins += [bytes(range(256))]
    ins += [sample(1)]
    ins += [golden("fuzz_r6_%s.bin" % s) for s in ("links_2414", "links_880", "small_1522")]
    return ins


class Dev:
    """inputs packed at 16-byte-aligned offsets behind `lead` bytes of `fill`, with `fill` in every gap"""

    def __init__(self, inputs, fill=0, lead=0):
        import torch
        self.torch = torch
        self.inputs = inputs
        self.off, buf = [], bytearray([fill]) * lead
        assert lead % 16 == 0
        for x in inputs:
            self.off.append(len(buf))
            buf += x
            buf += bytes([fill]) * (-len(buf) % 16 + 16)
        self.len = [len(x) for x in inputs]
        self.t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        self.cap = product().encode_batch_bound(self.len)
        self.o = torch.full((self.cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")

    def encode(self, eng, level, cap=None):
        o_off, o_len = eng.encode_batch_device(level, self.t.data_ptr(), self.off, self.len, self.o.data_ptr(),
                                               self.cap if cap is None else cap)
        self.torch.cuda.synchronize()
        host = self.o.cpu().numpy().tobytes()
        end = 0
        for a, n in zip(o_off, o_len):          # input order, multiples of 4 bytes, zeros in the gaps
            assert a % 4 == 0 and a == (end + 3) & ~3
            assert host[end:a] == bytes(a - end)
            end = a + n
        end = (end + 3) & ~3
        assert host[end:end + 8] == b"\xee" * 8  # nothing behind the last stream's slot
        return [host[a:a + n] for a, n in zip(o_off, o_len)]


@pytest.fixture(scope="module")
def eng8():
    e = product().GpuEngine(0, 8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def edge_expected(oracle):
    ins = edge_inputs()
    return ins, {level: [oracle.encode(x, level) for x in ins] for level in (1, 5, 9)}


@pytest.mark.parametrize("level", [1, 5, 9])
def test_edge_lengths(eng8, edge_expected, level):
    ins, want = edge_expected
    got = Dev(ins).encode(eng8, level)
    for i, (g, w) in enumerate(zip(got, want[level])):
        assert g == w, "input %d (%d bytes)" % (i, len(ins[i]))
    predicted = sum(one_block(len(x), level) for x in ins)   # level 1: sample1.ref and the fuzz fixtures are above 79 985
    assert predicted == (len(ins) - 4 if level == 1 else len(ins))
    assert eng8.batch_stats()[:2] == [predicted, len(ins) - predicted]
    if level == 9:
        assert got[0].hex() == "425a683917724538509000000000"  # the empty input: header and trailer, combined CRC 0


def test_inputs_do_not_see_each_other(eng8, oracle):
    """the byte in front of the first input and every gap hold `a`, and so do the inputs: a run that continued across an
    edge, or a byte read from outside, would change a count byte"""
    ins = [b"aaa", b"aaaa", b"aa", b"", b"aaaaa"]
    want = [oracle.encode(x, 9) for x in ins]
    got = Dev(ins, fill=0x61, lead=16).encode(eng8, 9)
    assert got == want
    assert Dev(ins[::-1], fill=0x61, lead=16).encode(eng8, 9) == want[::-1]


def test_more_inputs_than_the_workspace(oracle):
    ins = [sample(2)[7000 * i:7000 * i + 3000 + 3700 * i] for i in range(11)]   # 3 000 .. 40 000 bytes
    assert len(ins[0]) == 3000 and len(ins[-1]) == 40000
    eng = product().GpuEngine(0, 4)
    try:
        got = Dev(ins).encode(eng, 9)
        stats, blocks = eng.batch_stats(), eng.block_stats()
    finally:
        eng.close()
    assert stats == [11, 0, 11, 3]
    assert len(blocks) == 11
    for x, g, b in zip(ins, got, blocks):
        w, st = oracle.encode(x, 9, with_stats=True)
        assert g == w
        assert len(st) == 1
        assert (b["nblock"], b["block_crc"], b["orig_ptr"]) == (st[0]["nblock"], st[0]["block_crc"], st[0]["orig_ptr"])


_LEVEL1 = {}


def level1_expected(oracle, x):
    """(stream, block statistics) of the oracle at level 1, computed once per input"""
    if x not in _LEVEL1:
        _LEVEL1[x] = oracle.encode(x, 1, with_stats=True)
    return _LEVEL1[x]


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_bound_decides_the_path(eng8, oracle, where):
    """level 1: 79 985 worst-case bytes are one block for certain, 79 986 are not (the oracle makes two of them), and
    sample2.ref (all of its 212 340 bytes) is three"""
    fits, over, big = worst_case(79985), worst_case(79986), sample(2)
    small = [sample(1)[:5000], b"", text(1, 4097), b"\xfa" * 511]
    large = [over, big]
    ins = {"first": large + [fits] + small, "middle": small[:2] + [over, fits, big] + small[2:],
           "last": small + [fits] + large}[where]
    want = [level1_expected(oracle, x) for x in ins]
    assert len(want[ins.index(fits)][1]) == 1 and len(want[ins.index(over)][1]) == 2 and len(want[ins.index(big)][1]) >= 3
    got = Dev(ins).encode(eng8, 1)
    for i, (g, (w, _)) in enumerate(zip(got, want)):
        assert g == w, "input %d (%d bytes)" % (i, len(ins[i]))
    predicted = sum(one_block(len(x), 1) for x in ins)
    assert predicted == 5
    assert eng8.batch_stats()[:2] == [predicted, len(ins) - predicted]


def test_verify_on_gives_the_same_bytes(oracle):
    ins = [sample(1)[:30000], b"", rnd(3, 4097), b"\xfa" * 600 + text(4, 300), sample(1)[30000:50000]]
    want = [oracle.encode(x, 9) for x in ins]
    eng = product().GpuEngine(0, 8)
    try:
        plain = Dev(ins).encode(eng, 9)
        eng.set_verify(True)
        checked = Dev(ins).encode(eng, 9)
        vs = eng.verify_stats()
    finally:
        eng.close()
    assert plain == want and checked == want
    v = list(vs.values())
    assert v[0] == 4 and v[1] == 0   # four blocks (the empty input has none) checked, nothing redone


def test_round_trip_and_host_interface(pkg):
    datas = [sample(1)[4000 * i:4000 * i + 1 + 977 * i] for i in range(18)] + [b"", b"\x00" * 300]
    assert len(datas) == 20
    streams = pkg.compress_batch(datas)
    assert streams == [pkg.compress(d) for d in datas]
    back, rc = pkg.decompress(b"".join(streams))   # a multi-stream file
    assert rc == pkg.BZ_OK and back == b"".join(datas)
    assert pkg.compress_batch(datas) == streams      # the second call runs on the cached engine
    assert pkg.compress_batch([]) == []


def test_errors(eng8, pkg):
    import ctypes as C
    ins = [text(1, 1000), text(2, 2000)]
    d = Dev(ins)
    streams = d.encode(eng8, 9)
    need = sum((len(s) + 3) & ~3 for s in streams)
    assert d.encode(eng8, 9, cap=need) == streams
    with pytest.raises(pkg.CompressionError) as ei:
        d.encode(eng8, 9, cap=need - 4)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    for off, ln in (([0, 1008 + 8], d.len),          # not a multiple of 16
                    ([0, 992], d.len),               # the second input begins inside the first
                    ([d.off[1], d.off[0]], d.len)):  # out of order
        with pytest.raises(pkg.CompressionError) as ei:
            eng8.encode_batch_device(9, d.t.data_ptr(), off, ln, d.o.data_ptr(), d.cap)
        assert ei.value.code == pkg.BZ_E_PARAM
    with pytest.raises(pkg.CompressionError) as ei:
        eng8.encode_batch_device(0, d.t.data_ptr(), d.off, d.len, d.o.data_ptr(), d.cap)
    assert ei.value.code == pkg.BZ_E_PARAM
    a = (C.c_uint64 * 1)()
    assert pkg.lib().bz_gpu_encode_batch_device(eng8._h, 9, d.t.data_ptr(), None, a, 1, d.o.data_ptr(), d.cap, a, a) == pkg.BZ_E_PARAM
    assert eng8.encode_batch_device(9, d.t.data_ptr(), [], [], d.o.data_ptr(), d.cap) == ([], [])  # count == 0: BZ_OK
