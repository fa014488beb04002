"""GPU tests of LZHUF ENCODING (bz_gpu_lzh_encode_batch_device, bz_lzh_encode_batch, bz_lzh_encode_buffer, the two debug
entries and the Python surface over them; include/bz2_mi355x.h section 10).  Every expected byte comes from the model
(tests/lzhref.py:encode through tests/lzhshapes.py), from oracle.lzss_tokens / oracle.make_tab_with_fn, or is the input
itself; the inputs are the shape cases of tests/lzhshapes.py, which tests/test_lzhshapes.py pins."""
import os
import random

import pytest

import lzhref as R
import lzhshapes as S
from conftest import product

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, 64
METHODS = (4, 5, 6, 7)


class Pack:
    """inputs at 16-byte-aligned offsets behind a 0xEE lead, 0xEE in the gaps; the output lies between two guards"""

    def __init__(self, datas, lead=16):
        import torch
        self.torch = torch
        buf = bytearray([FILL]) * lead
        self.off, self.len = [], [len(d) for d in datas]
        for i, d in enumerate(datas):
            buf += bytes([FILL]) * (-len(buf) % 16 + 16 * (i % 3))
            self.off.append(len(buf))
            buf += d
        self.t = torch.frombuffer(buf if buf else bytearray(1), dtype=torch.uint8).cuda()

    def encode(self, eng, method, cap=None):
        """[stream]; checks the placement rules and that nothing outside the streams' words was written"""
        torch = self.torch
        pkg = product()
        if cap is None:
            cap = pkg.lzhuf_encode_batch_bound(self.len)
        o = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert o.data_ptr() % 16 == 0
        try:
            o_off, o_len = eng.lzh_encode_batch_device(method, self.t.data_ptr(), self.off, self.len, o.data_ptr() + GUARD, cap)
        finally:
            torch.cuda.synchronize()
            host = o.cpu().numpy().tobytes()
        assert host[:GUARD] == bytes([FILL]) * GUARD
        body = host[GUARD:]
        end = 0
        for a, n in zip(o_off, o_len):
            assert a % 4 == 0 and a == (end + 3) & ~3          # input order, every offset a multiple of 4
            assert body[end:a] == bytes(a - end)               # zeros between the streams
            end = a + n
        pad = (end + 3) & ~3
        assert pad <= cap and body[end:pad] == bytes(pad - end)
        assert body[pad:] == bytes([FILL]) * (len(body) - pad)  # nothing behind the last stream, nothing behind cap
        self.out, self.o_off, self.o_len = o, o_off, o_len
        return [body[a:a + n] for a, n in zip(o_off, o_len)]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    """{method: [(case, data, tokens, block infos, stream)]} of the model, once"""
    out = {m: [] for m in METHODS}
    for c in S.load()["cases"]:
        data = S.build(c)
        for m in c["methods"]:
            toks, infos, stream = S.model(oracle, data, m)
            out[m].append((c, data, toks, infos, stream))
    return out


def model_stats(group, sub_batches):
    return [len(group), sub_batches, sum(len(g[3]) for g in group), sum(b["nlit"] for g in group for b in g[3]),
            sum(b["nref"] for g in group for b in g[3]), sum(len(g[1]) for g in group), sum(len(g[4]) for g in group),
            sum(1 for g in group for b in g[3] if b["lm"])]


def check(got, group):
    assert len(got) == len(group)
    for s, g in zip(got, group):
        assert s == g[4], "%s: %d bytes, expected %d" % (S.case_id(g[0]), len(s), len(g[4]))


# ---- 1. the corpus, per method, as entries of one device call
@pytest.mark.parametrize("method", METHODS)
def test_corpus_in_one_call(eng, corpus, method):
    group = corpus[method]
    check(Pack([g[1] for g in group]).encode(eng, method), group)
    assert eng.lzh_encode_stats() == model_stats(group, 1)


# ---- 2. the other call paths agree with the model (and so with the device call)
def test_host_calls_and_the_class(corpus):
    pkg = product()
    for method in (4, 7):
        group = corpus[method]
        assert pkg.lzhuf_compress_batch([g[1] for g in group], method) == [g[4] for g in group]
    small = [g for g in corpus[5] if len(g[1]) < 9000]
    for g in small[::3]:
        assert pkg.lzhuf_compress(g[1], 5) == g[4], S.case_id(g[0])
    for g in small[1::5]:
        assert pkg.LzhufEncoder(pkg.LzhufMethod.Lh5).encode_all(g[1]) == g[4]
        enc = pkg.LzhufEncoder(5)
        enc.write(g[1][:7])
        enc.end(pkg.Action.RUN)
        assert enc.read_all() == b""
        it, out = iter(g[1][7:]), bytearray()
        while True:
            b = enc.next(it, pkg.Action.FINISH)
            if b is None:
                break
            out.append(b)
        assert bytes(out) == g[4]
    assert pkg.lzhuf_compress(b"", 6) == b"" and pkg.lzhuf_compress_batch([], 6) == []


# ---- 3. layouts: shuffled order, several sub-batches, a far match across a sort-chunk seam of the image
def test_shuffled_and_in_several_sub_batches(eng, corpus, monkeypatch):
    group = list(corpus[7])
    random.Random(3).shuffle(group)
    check(Pack([g[1] for g in group]).encode(eng, 7), group)
    monkeypatch.setenv("BZ_DF_BATCH_MIB", "0.25")
    check(Pack([g[1] for g in group]).encode(eng, 7), group)
    st = eng.lzh_encode_stats()
    assert st[1] > 3 and st == model_stats(group, st[1])


def test_lh7_matches_across_a_sort_chunk_seam(eng, corpus, oracle):
    """118 slots of one tile put the far case at image position 483 328: its second half starts 960 bytes in front of the
    seam at 524 288, so the first positions of the second sort chunk have their only candidates 40 000 bytes back -- more
    than Deflate's 32 KiB of history in front of a chunk"""
    far = next(g for g in corpus[7] if S.case_id(g[0]) == "S-far40000")
    filler = S.gen_text(77, 4096)
    got = Pack([filler] * 118 + [far[1]]).encode(eng, 7)
    assert got[-1] == far[4] and got[0] == R.encode(filler, 7) and len(set(got[:118])) == 1
    assert any(t[0] == "ref" and t[2] >= 0x8000 for t in far[2])


def test_one_large_slot_composes_its_exit_tables(eng, oracle):
    """an input alone in its call, of more than 64 tiles: the tiles' exit tables are composed (two levels at 75 tiles, three
    above 4 096) where smaller slots are walked.  The larger one is held against its own bytes through the decoder."""
    import torch
    mid = S.gen_text(5, 75 * 4096 - 7)
    assert Pack([mid]).encode(eng, 6) == [R.encode(mid, 6)]
    big = (S.gen_text(6, 1 << 20) * 17)[:4100 * 4096 + 3]  # (repeats lie a MiB apart: outside every window)
    p = Pack([big])
    (stream,) = p.encode(eng, 5)
    assert eng.lzh_encode_stats()[:2] == [1, 1] and eng.lzh_encode_stats()[5] == len(big)
    back = torch.zeros((len(big) + 64,), dtype=torch.uint8, device="cuda")
    d_off, d_len, ver = eng.lzh_decode_batch_device(5, p.out.data_ptr() + GUARD, p.o_off, p.o_len, back.data_ptr(), len(big), [len(big)])
    torch.cuda.synchronize()
    assert (d_off, d_len, ver) == ([0], [len(big)], [0])
    assert back[:len(big)].cpu().numpy().tobytes() == big
    # the same bytes beside a second, tiny input: two slots, the serial walk -- the same stream
    assert Pack([big, b"x"]).encode(eng, 5)[0] == stream


# ---- 4. the parse alone
def test_parse_against_the_oracle(eng, corpus):
    import torch
    for method in METHODS:
        for c, data, toks, _, _ in corpus[method]:
            if c["family"] not in "LDZ" or not data:
                continue
            t = torch.frombuffer(bytearray(data) + bytearray(16), dtype=torch.uint8).cuda()
            codes = eng.lzh_debug_codes(method, t.data_ptr(), len(data))
            mine = [("sym", int(p)) if l == 0 else ("ref", int(l), int(p)) for l, p in codes]
            assert mine == toks, "%s lh%d" % (S.case_id(c), method)


# ---- 5. the table builder alone
def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def tables_case(eng, oracle, method, cf, pf):
    want = S.tables_of_counts(oracle, cf, pf, R.OFFSET_BITS[method])
    cl, pl, tl, hbits, flags, lm = eng.lzh_debug_tables(method, cf, pf)
    assert (cl, pl, tl, hbits) == want[:4]
    assert lm == (1 if want[4] else 0)
    return want, flags


def test_tables_against_the_oracle(eng, oracle):
    r = random.Random(11)
    for n, limited in ((17, False), (18, True), (19, True)):
        cf = [0] * 510
        for s, f in zip(r.sample(range(510), n), fib(n)):
            cf[s] = f
        want, flags = tables_case(eng, oracle, 5, cf, [0, 3, 0, 1] + [0] * 13)
        assert want[4] == limited and max(want[0]) == 16 and flags == 0
    # constant forms: c alone, p alone, t alone (256 symbols of one length), none of them
    one = [0] * 510
    one[65] = 9
    assert tables_case(eng, oracle, 4, one, [0] * 17)[1] == 3
    two = list(one)
    two[300] = 4
    assert tables_case(eng, oracle, 6, two, [0] * 12 + [4] + [0] * 4)[1] == 2
    flat = [1] * 256 + [0] * 254
    assert tables_case(eng, oracle, 7, flat, [1, 1, 2, 3, 5, 8, 13, 21, 34] + [0] * 8)[1] == 4
    # t-lengths of 7 and more (unary), every gap spelling, p-lengths to 16
    want, flags = tables_case(eng, oracle, 7, S.t_deep_counts(), fib(17))
    assert max(want[2]) >= 7 and max(want[1]) == 16 and flags == 0
    for seed in range(6):
        rr = random.Random(seed)
        cf = [rr.choice((0, 0, 0, 1, 2, 7, 40, 300)) for _ in range(510)]
        tables_case(eng, oracle, 5, cf, [rr.randrange(50) for _ in range(14)] + [0] * 3)


# ---- 6. encoder -> decoder -> encoder on the device, arrays handed over unchanged
def test_round_trip_on_the_device(eng, corpus):
    import torch
    group = corpus[6]
    p = Pack([g[1] for g in group])
    streams = p.encode(eng, 6)
    total = sum((len(g[1]) + 15) & ~15 for g in group)
    back = torch.full((total + 16,), FILL, dtype=torch.uint8, device="cuda")
    d_off, d_len, ver = eng.lzh_decode_batch_device(6, p.out.data_ptr() + GUARD, p.o_off, p.o_len, back.data_ptr(), total,
                                                    [len(g[1]) for g in group])
    torch.cuda.synchronize()
    host = back.cpu().numpy().tobytes()
    assert ver == [0] * len(group)
    assert [host[a:a + n] for a, n in zip(d_off, d_len)] == [g[1] for g in group]
    cap = product().lzhuf_encode_batch_bound(d_len)
    again = torch.zeros((cap + 16,), dtype=torch.uint8, device="cuda")
    e_off, e_len = eng.lzh_encode_batch_device(6, back.data_ptr(), d_off, d_len, again.data_ptr(), cap)
    torch.cuda.synchronize()
    host = again.cpu().numpy().tobytes()
    assert [host[a:a + n] for a, n in zip(e_off, e_len)] == streams


# ---- 7. capacity
def test_capacity_one_byte_short(eng, corpus):
    pkg = product()
    group = [g for g in corpus[5] if len(g[1]) < 9000]
    need = sum((len(g[4]) + 3) & ~3 for g in group)
    p = Pack([g[1] for g in group])
    check(p.encode(eng, 5, cap=need), group)
    with pytest.raises(pkg.CompressionError) as ei:
        p.encode(eng, 5, cap=need - 1)
    assert ei.value.kind == "Capacity"
    check(p.encode(eng, 5), group)  # (the engine is sound)
