"""GPU tests of batched Deflate / zlib / gzip encoding (df_gpu_encode_batch_device, df_encode_batch): many inputs, one
stream each.  Inputs of at most 0xFFFF bytes are one block for certain and are encoded together from one image (every
input in a slot of whole 4096-position parse tiles); the others take the one-input path inside the same call.  Every
stream is compared with the oracle's for that input alone (oracle.deflate_encode), byte for byte."""
import random
import zlib

import numpy as np
import pytest

from conftest import product, sample
from test_oracle_deflate import VEC, expand

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)  # raw, zlib, gzip: the same numbers in the package and in the oracle
TILE = 4096


def rnd_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def words(seed, n):
    r = random.Random(seed)
    w = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(1, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(w) + b" "
    return bytes(out[:n])


def limited_input(seed):
    """the generator of test_gpu_deflate.py::test_length_limited_tables"""
    r = random.Random(seed)
    n = r.choice([300, 2000, 20000, 70000])
    return bytes((r.getrandbits(8) & r.getrandbits(8) & r.getrandbits(8)) for _ in range(n))


# the first of the seeds 0..199 whose input (n in {300, 2 000, 20 000}) takes the length-limited table path through
# df_gpu_encode_device, found on an MI355X with the one-input path (the oracle does not report that path)
LIMITED_SEED = 23

QUIRK = bytes(b for i in range(32) for j in range(32) for b in (i, 32 + j))  # 64 symbols, no trigram twice


class Dev:
    """inputs packed at 16-byte-aligned offsets behind `lead` bytes, the lead and every gap filled from `fill`
    (a byte, or a text that is repeated)"""

    def __init__(self, inputs, fill=0xEE, lead=0):
        import torch
        self.torch = torch
        assert lead % 16 == 0
        pat = bytes([fill]) if isinstance(fill, int) else fill
        stuff = lambda k: (pat * (k // len(pat) + 1))[:k]
        self.off, buf = [], bytearray(stuff(lead))
        for x in inputs:
            self.off.append(len(buf))
            buf += x
            buf += stuff(-len(buf) % 16 + 16)
        self.len = [len(x) for x in inputs]
        self.t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        self.cap = product().deflate_encode_batch_bound(self.len)
        self.o = torch.full((self.cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")

    def encode(self, eng, kind, cap=None):
        self.o.fill_(0xEE)
        o_off, o_len = eng.deflate_encode_batch_device(kind, self.t.data_ptr(), self.off, self.len, self.o.data_ptr(),
                                                       self.cap if cap is None else cap)
        self.torch.cuda.synchronize()
        host = self.o.cpu().numpy().tobytes()
        end = 0
        for a, n in zip(o_off, o_len):          # input order, multiples of 4 bytes, zeros in the gaps
            assert a % 4 == 0 and a == (end + 3) & ~3
            assert host[end:a] == bytes(a - end)
            end = a + n
        pad = (end + 3) & ~3
        assert host[end:pad] == bytes(pad - end)
        assert host[pad:] == b"\xee" * (len(host) - pad)  # nothing behind the last stream's slot
        return [host[a:a + n] for a, n in zip(o_off, o_len)]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def check(eng, oracle, ins, kind, want=None, **kw):
    want = [oracle.deflate_encode(x, kind) for x in ins] if want is None else want
    got = Dev(ins, **kw).encode(eng, kind)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "kind %d input %d (%d bytes)" % (kind, i, len(ins[i]))
    return got


# ---- 1. edge lengths
EDGE_N = [0, 1, 2, 3, 4, 5, 257, 258, 259, 260, 261, 262, 4095, 4096, 4097, 8191, 8192, 8193, 65534, 65535, 65536, 65537]


@pytest.fixture(scope="module")
def edge_expected(oracle):
    ins = []
    for n in EDGE_N:
        ins += [rnd_bytes(n, n), b"a" * n, words(n, n)]
    return ins, {k: [oracle.deflate_encode(x, k) for x in ins] for k in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_edge_lengths(eng, oracle, edge_expected, kind):
    ins, want = edge_expected
    got = check(eng, oracle, ins, kind, want[kind])
    st = eng.deflate_batch_stats()
    assert st[:2] == [3 * (len(EDGE_N) - 2), 6]   # 65 536 and 65 537 bytes are two blocks: the one-input path
    # one block per batch-path input; its BTYPE is in the oracle's raw stream
    btype = [(w[0] >> 1) & 3 for x, w in zip(ins, want[0]) if len(x) <= 0xFFFF]
    assert st[3:6] == [btype.count(0), btype.count(1), btype.count(2)]
    assert min(st[3:6]) >= 10                      # (random bytes are stored, runs of `a` fixed, word text dynamic)
    if kind == 0:
        assert got[0] == got[1] == got[2] == b"\x03\x00"  # the empty input: a fixed block


# ---- 2. inputs do not see each other
def test_inputs_do_not_see_each_other(eng, oracle):
    text = words(7, 5000)
    for kind in KINDS:
        check(eng, oracle, [text] * 6, kind, fill=text, lead=5008)
        ins = [b"abc" * k for k in (1, 2, 3, 5, 100, 1365, 1366, 0, 2731)]
        check(eng, oracle, ins, kind, fill=0x61, lead=16)
        check(eng, oracle, ins[::-1], kind, fill=0x61, lead=16)


# ---- 3. chains and window inside one input
def test_chains_stay_inside_an_input(eng, oracle):
    dna = bytes(random.Random(5).choice(b"ACGT") for _ in range(20000))
    check(eng, oracle, [dna] * 3, 0)   # full 255-candidate chains at the start of the second input if candidates leaked


@pytest.mark.parametrize("la", [32700, 33000])
def test_window_inside_an_input(eng, oracle, la):
    a = words(la, la)
    x = a + a[:2000]                     # a distance of 32 700 is inside the window, one of 33 000 is not
    assert len(x) <= 0xFFFF
    for kind in KINDS:
        check(eng, oracle, [x, x, a[:2000], x], kind)
    assert eng.deflate_batch_stats()[:2] == [4, 0]


def test_reference_vectors_in_one_call(eng, oracle):
    vs = [v for v in VEC["deflate"]] + [v for v in VEC["containers"] if "dict" not in v]
    vs += [v for v in VEC["lzss"] if "dict" not in v and v["name"] not in ("test_7", "test_11")]
    ins = [bytes(expand(v["input"])) for v in vs]
    assert len(ins) >= 10
    for kind in KINDS:
        got = check(eng, oracle, ins, kind)
        for v, g in zip(vs, got):
            if "kind" in v and {"zlib": 1, "gzip": 2}[v["kind"]] == kind:
                assert g == bytes(v["bytes"]), v["name"]    # the reference's own container bytes


# ---- 4. end of input
def test_end_of_input(eng, oracle):
    base = words(3, 3000)
    ins = [base + b"#" + base[100:100 + k] for k in (2, 3, 258, 259, 260)]
    # slots that end exactly on a tile, the next input's first bytes continuing the match
    for k in (1, 2, 3):
        body = words(10 + k, TILE * k - 300)
        body += body[500:800]
        assert len(body) == TILE * k
        ins += [body, body[800:1400]]
    for kind in KINDS:
        check(eng, oracle, ins, kind, fill=base)


# ---- 5. every block type in one call
def test_every_block_type(eng, oracle, pkg):
    import torch
    limited = limited_input(LIMITED_SEED)
    assert len(limited) <= 20000
    ins = [rnd_bytes(1, 3000), b"", b"ab", words(2, 9000), QUIRK, limited, b"a" * 700, rnd_bytes(2, 65535), words(4, 65535)]
    sums = dict(stored=0, fixed=0, dynamic=0, limited_tables=0, dynamic_without_distances=0)
    for x in ins:                       # the same inputs through the one-input path, one by one
        t = torch.frombuffer(bytearray(x) + bytearray(16), dtype=torch.uint8).cuda()
        cap = pkg.deflate_bound(len(x))
        o = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        k = eng.deflate_encode_device(0, t.data_ptr(), len(x), o.data_ptr(), cap)
        assert bytes(o[:k].cpu().numpy()) == oracle.deflate_encode(x, 0)
        st = eng.deflate_stats()
        assert st["blocks"] == 1
        for key in sums:
            sums[key] += st[key]
    for kind in KINDS:
        check(eng, oracle, ins, kind)
        st = eng.deflate_batch_stats()
        assert st[:3] == [len(ins), 0, 1]
        assert st[3:] == [sums["stored"], sums["fixed"], sums["dynamic"], sums["limited_tables"], sums["dynamic_without_distances"]]
    assert sums["stored"] >= 2 and sums["fixed"] >= 2 and sums["dynamic"] >= 3
    assert sums["dynamic_without_distances"] == 1
    assert sums["limited_tables"] >= 1


# ---- 6. image geometry
def test_slots_across_a_sort_chunk_edge(eng, oracle):
    ins = [words(20 + i, 60000) for i in range(10)]   # 15 tiles each: image position 524 288 lies inside the ninth
    check(eng, oracle, ins, 0)
    check(eng, oracle, ins, 2)
    assert eng.deflate_batch_stats()[:3] == [10, 0, 1]


def test_sub_batches(eng, oracle, monkeypatch):
    ins = [sample(2)[3000 * i:3000 * i + 29000 + 90 * i] for i in range(40)]   # eight tiles each
    want = [oracle.deflate_encode(x, 1) for x in ins]
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "0.25")   # 64 tiles: eight of these inputs
    check(eng, oracle, ins, 1, want)
    assert eng.deflate_batch_stats()[:3] == [40, 0, 5]
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "1")
    check(eng, oracle, ins, 1, want)
    assert eng.deflate_batch_stats()[:3] == [40, 0, 2]
    monkeypatch.delenv("BZ_DF_BATCH_MIB")
    check(eng, oracle, ins, 1, want)
    assert eng.deflate_batch_stats()[:3] == [40, 0, 1]


def test_small_and_large_interleaved(eng, oracle):
    s = sample(2)
    ins = [s[:70000], s[:100], b"", s[5000:5000 + 65536], s[100:9000], s[:200000], words(1, 4096), rnd_bytes(9, 66000), s[:1]]
    for kind in KINDS:
        check(eng, oracle, ins, kind)
        assert eng.deflate_batch_stats()[:3] == [5, 4, 4]   # (a run of neighbouring small inputs is a sub-batch)


def test_two_thousand_slices(eng, oracle):
    s = sample(1)
    r = random.Random(2000)
    ins = []
    for _ in range(2000):
        n = r.randint(1, 9000)
        a = r.randrange(0, len(s) - n)
        ins.append(s[a:a + n])
    check(eng, oracle, ins, 2)
    assert eng.deflate_batch_stats()[:3] == [2000, 0, 1]


# ---- 7. boundary
def test_boundary_and_errors(eng, oracle, pkg):
    import ctypes as C
    ins = [words(1, 1000), words(2, 2000)]
    d = Dev(ins, fill=0xEE, lead=32)
    streams = d.encode(eng, 1)
    assert streams == [oracle.deflate_encode(x, 1) for x in ins]
    need = sum((len(s) + 3) & ~3 for s in streams)
    assert d.encode(eng, 1, cap=need) == streams
    with pytest.raises(pkg.CompressionError) as ei:
        d.encode(eng, 1, cap=need - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    o0, o1 = d.off
    for off, ln in (([o0, o1 + 8], d.len),      # not a multiple of 16
                    ([o0, o0 + 992], d.len),    # the second input begins inside the first
                    ([o1, o0], d.len)):         # out of order
        with pytest.raises(pkg.CompressionError) as ei:
            eng.deflate_encode_batch_device(1, d.t.data_ptr(), off, ln, d.o.data_ptr(), d.cap)
        assert ei.value.code == pkg.BZ_E_PARAM
    with pytest.raises(pkg.CompressionError) as ei:
        eng.deflate_encode_batch_device(1, d.t.data_ptr() + 4, d.off, d.len, d.o.data_ptr(), d.cap)   # d_in misaligned
    assert ei.value.code == pkg.BZ_E_PARAM
    for kind in (3, -1):
        with pytest.raises(pkg.CompressionError) as ei:
            eng.deflate_encode_batch_device(kind, d.t.data_ptr(), d.off, d.len, d.o.data_ptr(), d.cap)
        assert ei.value.code == pkg.BZ_E_PARAM
    a = (C.c_uint64 * 1)()
    L = pkg.lib()
    assert L.df_gpu_encode_batch_device(eng._h, 1, d.t.data_ptr(), None, a, 1, d.o.data_ptr(), d.cap, a, a) == pkg.BZ_E_PARAM
    assert L.df_gpu_encode_batch_device(eng._h, 1, d.t.data_ptr(), a, a, 1, d.o.data_ptr(), d.cap, a, None) == pkg.BZ_E_PARAM
    assert eng.deflate_encode_batch_device(1, d.t.data_ptr(), [], [], d.o.data_ptr(), d.cap) == ([], [])  # count == 0: BZ_OK


# ---- 8. host form
def test_host_form(pkg, oracle):
    s = sample(1)
    datas = [s[4000 * i:4000 * i + 1 + 977 * i] for i in range(18)] + [b"", b"\x00" * 300, QUIRK, s[:70000], rnd_bytes(3, 5000)]
    for kind in KINDS:
        streams = pkg.deflate_compress_batch(datas, kind)
        assert streams == [pkg.deflate_compress(d, kind) for d in datas]
        assert streams == [oracle.deflate_encode(d, kind) for d in datas]
        assert pkg.deflate_compress_batch(datas, kind) == streams   # the second call runs on the cached engine
        if kind:
            for d, z in zip(datas, streams):
                if d is not QUIRK:   # (its HDIST = 0 block is what the reference writes and zlib rejects)
                    assert zlib.decompress(z, 15 if kind == 1 else 31) == d
    assert pkg.deflate_compress_batch([]) == []
