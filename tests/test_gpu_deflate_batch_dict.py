"""GPU tests of batched Deflate / zlib encoding with a preset dictionary (df_gpu_encode_batch_device_dict,
df_encode_batch_dict): one dictionary for every input of a call, its last 32 768 bytes in the image in front of every slot.
Every stream is compared with the oracle's `::with_dict` stream for that input alone (oracle.deflate_encode(x, kind, dict_)),
byte for byte.  The window cases are pinned to the oracle's LZSS codes in tests/test_deflate_batch_dict_abi.py."""
import struct
import zlib

import pytest

from conftest import product
from test_deflate_batch_dict_abi import (BUDGET, TAIL_CASE, WIN, budget_case, distance_limit_cases, long_input_case, rnd_bytes,
                                         tail_equal_case, words)
from test_gpu_deflate_batch import Dev

pytestmark = pytest.mark.gpu

KINDS = (0, 1)  # raw and zlib: gzip has no dictionary
TILE = 4096


class WithDict:
    """the engine with `dict_` in every deflate_encode_batch_device call: the placement and fill checks of Dev.encode hold
    for the dictionary form as they stand"""

    def __init__(self, eng, dict_):
        self._eng, self._dict = eng, dict_

    def deflate_encode_batch_device(self, *args):
        return self._eng.deflate_encode_batch_device(*args, dict_=self._dict)


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def check(eng, oracle, ins, kind, d, want=None, **kw):
    want = [oracle.deflate_encode(x, kind, d) for x in ins] if want is None else want
    got = Dev(ins, **kw).encode(WithDict(eng, d), kind)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "kind %d dictionary %d input %d (%d bytes)" % (kind, len(d), i, len(ins[i]))
    if kind == 1 and d:
        head = b"\x78\xf9" + struct.pack(">I", zlib.adler32(d))   # FDICT, DICTID of the whole dictionary
        assert all(g[:6] == head for g in got)
    return got


def dictionary(n):
    return words(1000 + n, n)


# ---- 1. the edge grid
EDGE_N = [0, 1, 2, 3, 257, 258, 259, 260, 261, 262, 4095, 4096, 4097, 65534, 65535, 65536, 65537]
EDGE_INS = []
for _n in EDGE_N:
    EDGE_INS += [rnd_bytes(_n, _n), b"a" * _n, words(_n, _n)]


@pytest.fixture(scope="module")
def edge_expected(oracle):
    memo = {}

    def get(dlen, kind):
        if (dlen, kind) not in memo:
            memo[dlen, kind] = [oracle.deflate_encode(x, kind, dictionary(dlen)) for x in EDGE_INS]
        return memo[dlen, kind]
    return get


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dlen", [1, 32768, 40000])
def test_edge_grid(eng, oracle, edge_expected, dlen, kind):
    check(eng, oracle, EDGE_INS, kind, dictionary(dlen), edge_expected(dlen, kind))
    st = eng.deflate_batch_stats()
    assert st[:2] == [3 * (len(EDGE_N) - 2), 6]   # 65 536 and 65 537 bytes are two blocks: the one-input path
    btype = [(w[0] >> 1) & 3 for x, w in zip(EDGE_INS, edge_expected(dlen, 0)) if len(x) <= 0xFFFF]
    assert st[3:6] == [btype.count(0), btype.count(1), btype.count(2)]   # one block per batch-path input, as the oracle's


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dlen", [2, 3, 258, 4095, 4096, 4097, 32767])
def test_edge_dictionary_lengths(eng, oracle, dlen, kind):
    ins = []
    for n in (3, 4097):
        ins += [rnd_bytes(n, n), b"a" * n, words(n, n), dictionary(dlen)[-n:]]
    check(eng, oracle, ins, kind, dictionary(dlen))
    assert eng.deflate_batch_stats()[:3] == [len(ins), 0, 1]


# ---- 2. the window
@pytest.mark.parametrize("kind", KINDS)
def test_distance_limit(eng, oracle, kind):
    for d, x, _ in distance_limit_cases():
        check(eng, oracle, [x, x + x, b"", x], kind, d)


@pytest.mark.parametrize("kind", KINDS)
def test_match_from_the_windows_last_two_bytes(eng, oracle, kind):
    d, x = TAIL_CASE
    check(eng, oracle, [x, x[:3], x[:2], x[:1], x], kind, d)


@pytest.mark.parametrize("kind", KINDS)
def test_candidate_budget(eng, oracle, kind):
    for (k, m), _ in BUDGET:
        d, x = budget_case(k, m)
        check(eng, oracle, [x, x], kind, d)


@pytest.mark.parametrize("kind", KINDS)
def test_input_equal_to_the_dictionarys_tail(eng, oracle, kind):
    d, x = tail_equal_case()
    check(eng, oracle, [x, x[:TILE], x[1:], d[-WIN:], d[-WIN - 1:]], kind, d)


@pytest.mark.parametrize("kind", KINDS)
def test_long_input_leaves_the_window(eng, oracle, kind):
    d, x = long_input_case()
    check(eng, oracle, [x, x[:37999], x], kind, d)


# ---- 3. isolation
@pytest.mark.parametrize("kind", KINDS)
def test_inputs_see_the_dictionary_and_nothing_else(eng, oracle, kind):
    d = dictionary(WIN)
    ins = [d[-3000:], words(5, 5000), d[100:9000], b"", d[-1:], words(6, TILE)]
    want = [oracle.deflate_encode(x, kind, d) for x in ins]
    a = check(eng, oracle, ins, kind, d, want)
    # other neighbours: every input between two texts the dictionary does not hold
    other = [words(50 + i, 7000, vocab=9) for i in range(len(ins) + 1)]
    mixed = [other[0]]
    for x, o in zip(ins, other[1:]):
        mixed += [x, o]
    b = check(eng, oracle, mixed, kind, d)[1::2]
    # the caller's buffer holds the dictionary's text in front of and between the inputs
    c = check(eng, oracle, ins, kind, d, want, fill=d, lead=WIN)
    # the slot in front ends in the dictionary's text (what the window would hold if it were taken from the image)
    e = check(eng, oracle, [words(8, 1000) + d, ins[0], d[-TILE:], ins[1]], kind, d)
    assert a == b == c and [e[1], e[3]] == a[:2]


# ---- 4. sub-batch seams
def test_sub_batches(eng, oracle, monkeypatch):
    d = dictionary(WIN)
    ins = [words(70 + i, 100 + 2900 * i) for i in range(12)]   # 1 .. 8 input tiles, 8 window tiles each
    want = [oracle.deflate_encode(x, 1, d) for x in ins]

    def sub_batches(limit_tiles):
        k, tiles = 1, 0
        for x in ins:
            t = 8 + -(-len(x) // TILE)
            if tiles and tiles + t > limit_tiles:
                k, tiles = k + 1, 0
            tiles += t
        return k
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "0.0625")   # 16 tiles: every slot alone (the first input is always admitted)
    check(eng, oracle, ins, 1, d, want)
    assert eng.deflate_batch_stats()[:3] == [12, 0, 12] and sub_batches(16) == 12
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "0.25")
    check(eng, oracle, ins, 1, d, want)
    assert eng.deflate_batch_stats()[:3] == [12, 0, sub_batches(64)] and 1 < sub_batches(64) < 12
    monkeypatch.delenv("BZ_DF_BATCH_MIB")
    check(eng, oracle, ins, 1, d, want)
    assert eng.deflate_batch_stats()[:3] == [12, 0, 1]


# ---- 5. round trip on the device
@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_on_the_device(eng, oracle, pkg, kind):
    import torch
    d = dictionary(40000)
    ins = [d[-5000:], words(3, 20000), b"", b"a" * 700, rnd_bytes(4, 3000), d[-WIN:-WIN + 600] + words(9, 300), words(4, 65535), words(5, 70000)]
    dev = Dev(ins)
    o_off, o_len = eng.deflate_encode_batch_device(kind, dev.t.data_ptr(), dev.off, dev.len, dev.o.data_ptr(), dev.cap, dict_=d)
    cap = sum((len(x) + 15) & ~15 for x in ins) + 16
    back = torch.full((cap,), 0xEE, dtype=torch.uint8, device="cuda")
    b_off, b_len, verdicts = eng.deflate_decode_batch_device(kind, dev.o.data_ptr(), o_off, o_len, back.data_ptr(), cap, dict_=d)
    torch.cuda.synchronize()
    assert verdicts == [pkg.BZ_OK] * len(ins) and b_len == [len(x) for x in ins]
    host = back.cpu().numpy().tobytes()
    assert [host[a:a + n] for a, n in zip(b_off, b_len)] == ins
    streams = dev.o.cpu().numpy().tobytes()
    for x, a, n in zip(ins, o_off, o_len):
        z = zlib.decompressobj(-15 if kind == 0 else 15, zdict=d)
        assert z.decompress(streams[a:a + n]) + z.flush() == x and z.eof
        assert streams[a:a + n] == oracle.deflate_encode(x, kind, d)


# ---- 6. host to host
@pytest.mark.parametrize("kind", KINDS)
def test_host_form(eng, oracle, pkg, kind):
    d = dictionary(WIN + 1)
    datas = [d[4000 * i:4000 * i + 1 + 977 * i] for i in range(8)] + [b"", b"\x00" * 300, words(2, 70000), rnd_bytes(3, 5000)]
    streams = pkg.deflate_compress_batch(datas, kind, dict_=d)
    assert streams == check(eng, oracle, datas, kind, d)
    assert streams == [pkg.deflate_compress(x, kind, dict_=d) for x in datas]
    assert pkg.deflate_compress_batch(datas, kind, dict_=d) == streams   # the second call runs on the cached engine
    # an empty dictionary is no dictionary
    plain = pkg.deflate_compress_batch(datas, kind)
    assert pkg.deflate_compress_batch(datas, kind, dict_=b"") == plain == [oracle.deflate_encode(x, kind) for x in datas]
    assert Dev(datas).encode(WithDict(eng, b""), kind) == plain
    assert kind == 0 or all(s[:2] == b"\x78\xda" for s in plain)


def test_capacity(eng, oracle, pkg):
    d = dictionary(5000)
    dev = Dev([words(1, 1000), words(2, 2000)], lead=32)
    streams = dev.encode(WithDict(eng, d), 1)
    assert streams == [oracle.deflate_encode(x, 1, d) for x in (words(1, 1000), words(2, 2000))]
    need = sum((len(s) + 3) & ~3 for s in streams)
    assert dev.encode(WithDict(eng, d), 1, cap=need) == streams
    with pytest.raises(pkg.CompressionError) as ei:
        dev.encode(WithDict(eng, d), 1, cap=need - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    with pytest.raises(ValueError):
        eng.deflate_encode_batch_device(2, dev.t.data_ptr(), dev.off, dev.len, dev.o.data_ptr(), dev.cap, dict_=d)
