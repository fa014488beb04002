"""GPU tests of the BGZF writer (df_gpu_bgzf_encode_device, df_bgzf_encode_buffer; section 7 of the header): one contiguous
input cut into blocks of B bytes, each a gzip member of its own, side by side without padding, then the EOF marker.  Every
file is compared byte for byte with tests/bgzfref.py -- the oracle's one-block stream per chunk, the strict rule for
dynamic blocks without a match, zlib.crc32 -- in a buffer filled with 0xEE, of which nothing outside the file may change."""
import gzip
import random
import struct

import numpy as np
import pytest

import bgzfref
from conftest import product
from test_bgzfref import QUIRK, QUIRK_HI
from test_gpu_deflate_batch import rnd_bytes, words

pytestmark = pytest.mark.gpu

B = bgzfref.BLOCK
_expected = {}


def expected(oracle, data, b=0, eof=True):
    """bgzfref.build, made once per (data, b, eof) of the module"""
    key = (hash(data), len(data), b, eof)
    if key not in _expected:
        _expected[key] = bgzfref.build(oracle, data, b, eof)
    return _expected[key]


def text(seed, n):
    """n bytes of word text, quickly"""
    r = random.Random(seed)
    w = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(1, 9))) + b" " for _ in range(300)]
    idx = np.random.default_rng(seed).integers(0, len(w), size=n // 2 + 8)
    return b"".join(w[i] for i in idx)[:n]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


class Run:
    """one call: the input's last byte is the last byte of its tensor (16 bytes of 0xEE in front of it), the output buffer
    is 0xEE throughout and the file starts `shift` bytes into it"""

    def __init__(self, eng, data, b=0, eof=True, cap=None, shift=0, slack=64):
        import torch
        pkg = product()
        self.t = torch.frombuffer(bytearray(b"\xee" * 16 + data), dtype=torch.uint8).cuda()
        self.bound = pkg.bgzf_bound(len(data), b, eof)
        self.cap = self.bound if cap is None else cap
        self.o = torch.full((shift + max(self.cap, self.bound) + slack,), 0xEE, dtype=torch.uint8, device="cuda")
        self.error = None
        try:
            self.out_len, self.offs = eng.bgzf_encode_device(self.t.data_ptr() + 16, len(data), self.o.data_ptr() + shift, self.cap,
                                                             block_bytes=b, eof=eof, offsets=True)
        except pkg.CompressionError as e:
            self.error = e.code
            self.out_len, self.offs = 0, []
        torch.cuda.synchronize()
        host = self.o.cpu().numpy().tobytes()
        assert host[:shift] == b"\xee" * shift
        self.file = host[shift:shift + self.out_len]
        self.behind = host[shift + self.out_len:]
        self.behind_cap = host[shift + self.cap:]
        self.stats = eng.bgzf_stats()


def check(eng, oracle, data, b=0, eof=True, **kw):
    want, offs, kinds = expected(oracle, data, b, eof)
    r = Run(eng, data, b, eof, **kw)
    assert r.error is None
    assert r.out_len == len(want)
    assert r.file == want, "n %d B %d: first difference at %d" % (
        len(data), b, next((i for i, (x, y) in enumerate(zip(r.file, want)) if x != y), -1))
    assert r.behind == b"\xee" * len(r.behind)       # nothing at or behind d_out + out_len
    assert r.offs == offs
    bt = [k for k, _ in kinds]
    assert r.stats[0] == len(kinds) and r.stats[2:5] == [bt.count(0), bt.count(1), bt.count(2)]
    assert r.stats[6] == sum(1 for _, rep in kinds if rep) and r.stats[7] == len(want)
    return r


# ---- 1. edge lengths at the default B
EDGE_N = [0, 1, 65279, 65280, 65281, 130560, 130561]


@pytest.mark.parametrize("make", [rnd_bytes, lambda seed, n: b"a" * n, words], ids=["random", "run", "words"])
def test_edge_lengths(eng, oracle, make):
    whole = make(11, EDGE_N[-1])
    for n in EDGE_N:
        r = check(eng, oracle, whole[:n])
        assert r.stats[0] == (n + B - 1) // B and r.stats[1] == (1 if n else 0)
    assert check(eng, oracle, b"").file == bgzfref.EOF
    assert check(eng, oracle, b"", eof=False).file == b""


# ---- 2. cuts at any byte: nothing leaks across a cut
@pytest.mark.parametrize("b", [1, 7, 15, 16, 17, 4095, 4096, 4097, 65279])
def test_unaligned_cuts(eng, oracle, b):
    n = 40 if b == 1 else b * 7 // 2
    period = max(1, min(b - 2, 3001))
    base = words(b, period)
    data = (base * (n // period + 1))[:n]
    # a candidate, window or match that crossed a cut would find the text of the block in front and change the bytes
    r = check(eng, oracle, data, b)
    assert r.stats[0] == (n + b - 1) // b
    assert gzip.decompress(r.file) == data


# ---- 3. every block type in one call
def limited_chunk(seed):
    """2 048 bytes over a Zipf-like alphabet.  For the seeds used here the code length code of the oracle's block is 8 bits
    deep as a plain Huffman code (a seeded search on the CPU: the block's header gives the run-coded lengths, their counts the
    depth), one more than its limit of 7: candidates for the length-limited path"""
    r = random.Random(seed)
    ns = r.randint(20, 200)
    w = [1.0 / (k + 1) ** r.choice([1, 1.5, 2]) for k in range(ns)]
    syms = r.sample(range(256), ns)
    return bytes(r.choices(syms, w, k=2048))


def test_every_block_type(eng, oracle, pkg):
    import torch
    chunks = [rnd_bytes(1, 2048), b"a" * 2048, words(2, 2048), limited_chunk(452), QUIRK, QUIRK_HI, limited_chunk(1094), limited_chunk(1616),
              b"ab" * 1024, rnd_bytes(2, 700)]
    data = b"".join(chunks)
    want, offs, kinds = expected(oracle, data, 2048)
    assert [k for k in kinds[:6]] == [(0, False), (1, False), (2, False), (2, False), (1, True), (0, True)]
    limited = 0
    for x in chunks:                      # the same chunks through the one-input path, one by one: its limited tables
        t = torch.frombuffer(bytearray(x) + bytearray(16), dtype=torch.uint8).cuda()
        cap = pkg.deflate_bound(len(x))
        o = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        k = eng.deflate_encode_device(0, t.data_ptr(), len(x), o.data_ptr(), cap)
        assert bytes(o[:k].cpu().numpy()) == oracle.deflate_encode(x, 0)
        print("chunk of %d bytes: limited tables %d" % (len(x), eng.deflate_stats()["limited_tables"]))
        limited += eng.deflate_stats()["limited_tables"]
    r = check(eng, oracle, data, 2048)
    bt = [k for k, _ in kinds]
    assert r.stats[2:7] == [bt.count(0), bt.count(1), bt.count(2), limited, 2]
    assert min(r.stats[2:5]) >= 2 and limited >= 1
    for k in range(len(chunks)):          # zlib reads every member, QUIRK's included
        assert gzip.decompress(r.file[offs[k]:offs[k + 1]]) == chunks[k]


# ---- 4. sub-batch seams
def test_sub_batch_seams(eng, oracle, monkeypatch):
    data = text(4, 40 * B + 1000)
    r = check(eng, oracle, data)
    assert r.stats[:2] == [41, 1]
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "1")      # 16 slots of 16 tiles
    r1 = check(eng, oracle, data)
    assert r1.stats[:2] == [41, 3]
    assert r1.file == r.file and r1.offs == r.offs


# ---- 5. block offsets
@pytest.mark.parametrize("eof", [True, False])
def test_block_offsets(eng, oracle, eof):
    data = text(5, 5 * 4097 + 33) + rnd_bytes(5, 3 * 4097)
    r = check(eng, oracle, data, 4097, eof)
    count = (len(data) + 4096) // 4097
    assert len(r.offs) == count + 1 and r.offs[0] == 0
    for k in range(count):
        assert r.file[r.offs[k]:r.offs[k] + 4] == b"\x1f\x8b\x08\x04"
        assert r.offs[k + 1] - r.offs[k] == struct.unpack_from("<H", r.file, r.offs[k] + 16)[0] + 1
    if eof:
        assert r.file[r.offs[-1]:] == bgzfref.EOF
    else:
        assert r.offs[-1] == r.out_len == len(r.file)
    assert bgzfref.walk(r.file) == r.offs[:count] + ([r.offs[-1]] if eof else [])


# ---- 6. concatenation
def test_concatenation(eng, oracle):
    a, b = text(6, 100000), rnd_bytes(6, 3000) + text(7, 70000)
    fa = check(eng, oracle, a, eof=False).file
    fb = check(eng, oracle, b, eof=True).file
    assert gzip.decompress(fa + fb) == a + b
    assert bgzfref.walk(fa + fb)[-1] == len(fa) + len(fb) - 28


# ---- 7. capacity
def test_capacity_and_alignment(eng, oracle, pkg):
    data = text(8, 2 * B + 500) + rnd_bytes(8, 1000)
    want = expected(oracle, data)[0]
    assert len(want) < pkg.bgzf_bound(len(data))
    r = Run(eng, data, cap=len(want) - 1)
    assert r.error == pkg.BZ_E_CAPACITY
    assert r.behind_cap == b"\xee" * len(r.behind_cap)      # nothing at or behind d_out + cap
    assert check(eng, oracle, data, cap=len(want)).file == want
    for eof in (True, False):                               # the marker alone does not fit either
        w2 = expected(oracle, data, 0, eof)[0]
        r = Run(eng, data, eof=eof, cap=len(w2) - 1)
        assert r.error == pkg.BZ_E_CAPACITY and r.behind_cap == b"\xee" * len(r.behind_cap)
    for shift in (3, 1, 2):
        assert check(eng, oracle, data, shift=shift).file == want
    # parameters
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for args in ((t.data_ptr() + 4, 8, t.data_ptr(), 64, 0), (t.data_ptr(), 8, t.data_ptr() + 32, 32, B + 1), (None, 8, t.data_ptr(), 64, 0)):
        with pytest.raises(pkg.CompressionError) as ei:
            eng.bgzf_encode_device(args[0], args[1], args[2], args[3], block_bytes=args[4])
        assert ei.value.code == pkg.BZ_E_PARAM


# ---- 8. decoding back
def test_decoding_back(eng, oracle):
    import torch
    data = text(9, 3 * B + 77) + QUIRK + QUIRK_HI
    r = check(eng, oracle, data)
    count = len(r.offs) - 1
    z = torch.frombuffer(bytearray(r.file) + bytearray(16), dtype=torch.uint8).cuda()
    o = torch.full((len(data) + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    n, verdict = eng.gzip_decode_members_device(z.data_ptr(), len(r.file), o.data_ptr(), len(data))
    assert (n, verdict) == (len(data), 0)
    assert bytes(o[:n].cpu().numpy()) == data
    assert eng.gzip_decode_members_stats()[0] == count + 1
    assert gzip.decompress(r.file) == data


# ---- 9. host form
def test_host_form(eng, oracle, pkg):
    data = text(10, 2 * B + 5) + QUIRK
    for b, eof in ((0, True), (4097, False), (2048, True)):
        want, offs, _ = expected(oracle, data, b, eof)
        assert pkg.bgzf_compress(data, b, eof) == want
        assert pkg.bgzf_compress(data, b, eof, offsets=True) == (want, offs)
        r = check(eng, oracle, data, b, eof)
        assert (r.file, r.offs) == (want, offs)
