"""GPU tests of LZHUF DECODING (bz_gpu_lzh_decode_batch_device, bz_lzh_decode_batch, bz_lzh_decode_buffer and the Python
surface over them; include/bz2_mi355x.h section 9): many streams in one call, one wave per stream.  Every expected value
comes from the plain-Python model (tests/lzhref.py) or is the data a stream was made from; the forged streams come from
tests/lzhforge.py, which tests/test_lzhforge.py pins."""
import random

import pytest

import lzhforge as F
import lzhref as R
from conftest import product, sample

pytestmark = pytest.mark.gpu

OK, E_DATA, E_EOF = 0, -1, -2
FILL, GUARD = 0xEE, 64
METHODS = (4, 5, 6, 7)


class Pack:
    """entries at 4-byte-aligned offsets behind a 0xEE lead, 0xEE in the gaps; the device buffer ends with the last entry's
    last byte.  The output lies between two guards of 64 bytes of 0xEE."""

    def __init__(self, entries, lead=16):
        import torch
        self.torch = torch
        buf = bytearray([FILL]) * lead
        self.off, self.len = [], [len(e) for e in entries]
        for i, e in enumerate(entries):
            buf += bytes([FILL]) * (-len(buf) % 4 + 4 * (i % 3))
            self.off.append(len(buf))
            buf += e
        self.t = torch.frombuffer(buf if buf else bytearray(1), dtype=torch.uint8).cuda()

    def sizes(self, eng, method, orig_len=None, prefill=-1):
        return eng.lzh_decode_batch_device(method, self.t.data_ptr(), self.off, self.len, None, 0, orig_len, prefill)

    def decode(self, eng, method, orig_len=None, prefill=-1):
        """[(bytes, verdict)]; checks the placement rules, sizes-only against the real call, and that nothing outside the
        reported ranges was written -- the guards in front of and behind d_out included"""
        torch = self.torch
        s_off, s_len, s_ver = self.sizes(eng, method, orig_len, prefill)
        assert eng.lzh_decode_stats()[7] == 1
        cap = max([a + n for a, n in zip(s_off, s_len)] + [0])
        o = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert o.data_ptr() % 16 == 0
        try:
            o_off, o_len, ver = eng.lzh_decode_batch_device(method, self.t.data_ptr(), self.off, self.len, o.data_ptr() + GUARD, cap,
                                                            orig_len, prefill)
        finally:
            torch.cuda.synchronize()
            host = o.cpu().numpy().tobytes()
        assert (o_off, o_len, ver) == (s_off, s_len, s_ver)
        assert host[:GUARD] == bytes([FILL]) * GUARD
        body = host[GUARD:]
        end = 0
        for a, n in zip(o_off, o_len):
            assert a % 16 == 0 and a == (end + 15) & ~15           # input order, every offset a multiple of 16
            assert body[end:a] == bytes([FILL]) * (a - end)        # the gaps keep their fill
            end = a + n
        assert end <= cap
        assert body[end:] == bytes([FILL]) * (len(body) - end)     # ... and so does everything behind the last entry
        return [(body[a:a + n], v) for a, n, v in zip(o_off, o_len, ver)]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """the forged corpus with the model's answer for every case, once: {(method, prefill): [(case, stream, Result)]}"""
    groups = {}
    for c in F.expand(F.load()):
        s = F.build(c)
        r = R.decode_full(s, c["method"], c.get("orig_len"), c.get("prefill", -1))
        groups.setdefault((c["method"], c.get("prefill", -1)), []).append((c, s, r))
    return groups


def check(got, want, names):
    assert len(got) == len(want)
    for g, r, name in zip(got, want, names):
        assert g[1] == r.verdict, "%s: verdict %d, expected %d" % (name, g[1], r.verdict)
        assert g[0] == bytes(r.out), "%s: %d bytes, expected %d" % (name, len(g[0]), len(r.out))


def model_stats(results, launches):
    clean = [r for r in results if r.verdict == OK]
    return [len(clean), len(results) - len(clean), sum(r.blocks for r in results), sum(r.literals for r in results),
            sum(r.matches for r in results), sum(len(r.out) for r in results), sum((r.bits + 7) // 8 for r in clean), launches]


# ---- 1. the forged corpus
@pytest.mark.parametrize("method", METHODS)
def test_forged_corpus_in_one_batch(eng, corpus, method):
    for (m, prefill), group in sorted(corpus.items()):
        if m != method:
            continue
        ol = [c.get("orig_len") for c, _, _ in group]
        got = Pack([s for _, s, _ in group]).decode(eng, method, ol if any(x is not None for x in ol) else None, prefill)
        check(got, [r for _, _, r in group], [F.case_id(c) for c, _, _ in group])
        assert eng.lzh_decode_stats() == model_stats([r for _, _, r in group], 2)


def test_forged_corpus_one_by_one(corpus):
    pkg = product()
    for (m, prefill), group in sorted(corpus.items()):
        for c, s, r in group:
            if c.get("k", 0) % 8 or len(r.out) > (1 << 20):     # (every eighth preamble: a host call per stream)
                continue
            got = pkg.lzhuf_decompress(s, m, c.get("orig_len"), prefill)
            assert got == (bytes(r.out), r.verdict), F.case_id(c)


def test_forged_corpus_through_the_class(corpus):
    pkg = product()
    for (m, prefill), group in sorted(corpus.items()):
        for c, s, r in group:
            if c.get("k", 0) or len(r.out) > (1 << 20):
                continue
            d = pkg.LzhufDecoder(pkg.LzhufMethod(m), orig_len=c.get("orig_len"), prefill=prefill)
            if r.verdict == OK:
                assert d.decode_all(s) == bytes(r.out), F.case_id(c)
            else:
                with pytest.raises(pkg.CompressionError) as ei:
                    d.decode_all(s)
                assert ei.value.code == r.verdict and ei.value.partial == bytes(r.out), F.case_id(c)
    d = pkg.LzhufDecoder(pkg.LzhufMethod.Lh5)
    it = iter(R.encode(b"abcabcabc", 5))
    assert bytes(iter(lambda: d.next(it), None)) == b"abcabcabc"


def test_truncations(eng):
    for m in (5, 7):
        cut = [s for mm, s in F.truncations() if mm == m]
        want = [R.decode_full(s, m) for s in cut]
        check(Pack(cut).decode(eng, m), want, ["cut at %d" % len(s) for s in cut])
        assert {r.verdict for r in want} == {OK, E_EOF}


# ---- 2. isolation
def test_mixed_verdicts_leave_the_neighbours_alone(eng, corpus):
    group = [x for x in corpus[(5, -1)] if x[0].get("k", 0) == 0 and x[0].get("orig_len") is None and len(x[2].out) < 70000]
    alone = {F.case_id(c): (bytes(r.out), r.verdict) for c, _, r in group}
    assert {v for _, v in alone.values()} == {OK, E_DATA, E_EOF}
    rng = random.Random(26)
    for _ in range(3):
        rng.shuffle(group)
        got = Pack([s for _, s, _ in group]).decode(eng, 5)
        for g, (c, _, _) in zip(got, group):
            assert g == alone[F.case_id(c)], F.case_id(c)


# ---- 3. the model encoder's streams
def _inputs():
    words = (b"lorem ipsum dolor sit amet consectetur adipiscing elit sed do eiusmod tempor " * 400)[:30000]
    return [words, b"\x55" * 70000, sample(1), random.Random(7).randbytes(70000)]


@pytest.fixture(scope="module")
def encoded():
    ins = _inputs()
    return ins, {m: [R.encode(x, m) for x in ins] for m in METHODS}


@pytest.mark.parametrize("method", METHODS)
def test_encoder_streams_decode_to_their_input(eng, encoded, method):
    ins, z = encoded
    got = Pack(z[method]).decode(eng, method)
    for g, x in zip(got, ins):
        assert g == (x, OK)
    st = eng.lzh_decode_stats()
    assert st[0] == len(ins) and st[1] == 0 and st[5] == sum(len(x) for x in ins) and st[6] == sum(len(s) for s in z[method])
    assert st[2] >= len(ins) + 1                                  # (70 000 random bytes are two blocks)
    got = Pack(z[method]).decode(eng, method, [len(x) for x in ins])
    for g, x in zip(got, ins):
        assert g == (x, OK)
    got = Pack(z[method]).decode(eng, method, [len(x) // 2 for x in ins])
    for g, x in zip(got, ins):
        assert g == (x[:len(x) // 2], OK)
    got = Pack(z[method]).decode(eng, method, [len(x) + 1 for x in ins])
    for g, x in zip(got, ins):
        assert g == (x, E_EOF)


def test_host_batch_equals_the_device_call(encoded):
    pkg = product()
    ins, z = encoded
    got = pkg.lzhuf_decompress_batch(z[6] + [b"", b"\x00\x01"], pkg.LzhufMethod.Lh6, [None] * len(ins) + [None, 5])
    assert got == [(x, OK) for x in ins] + [(b"", OK), (b"", E_EOF)]
    assert pkg.lzhuf_decompress_batch([], 5) == []


# ---- 4. capacity and parameter errors
def test_capacity_one_byte_short_leaves_the_output_untouched(eng, corpus):
    import torch
    pkg = product()
    (c, s, r), = [x for x in corpus[(7, -1)] if x[0]["name"] == "const_matches_max"]
    assert len(r.out) == 1 + 65535 * 256 and r.verdict == OK
    p = Pack([s])
    off, ln, ver = p.sizes(eng, 7)
    assert (off, ln, ver) == ([0], [len(r.out)], [OK])
    o = torch.full((len(r.out) + 64,), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.CompressionError) as ei:
        eng.lzh_decode_batch_device(7, p.t.data_ptr(), p.off, p.len, o.data_ptr(), len(r.out) - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    torch.cuda.synchronize()
    assert bool((o == FILL).all())
    eng.lzh_decode_batch_device(7, p.t.data_ptr(), p.off, p.len, o.data_ptr(), len(r.out))
    torch.cuda.synchronize()
    assert o[:len(r.out)].cpu().numpy().tobytes() == bytes(r.out) and bool((o[len(r.out):] == FILL).all())


def test_parameter_errors_on_the_device_call(eng):
    pkg = product()
    p = Pack([R.encode(b"abc", 5)])
    for method, prefill in ((3, -1), (8, -1), (5, -2), (5, 256)):
        with pytest.raises(pkg.CompressionError) as ei:
            eng.lzh_decode_batch_device(method, p.t.data_ptr(), p.off, p.len, None, 0, None, prefill)
        assert ei.value.code == pkg.BZ_E_PARAM
    with pytest.raises(pkg.CompressionError) as ei:
        eng.lzh_decode_batch_device(5, p.t.data_ptr(), [p.off[0] + 2], p.len, None, 0)
    assert ei.value.code == pkg.BZ_E_PARAM
    assert eng.lzh_decode_batch_device(5, p.t.data_ptr(), [], [], None, 0) == ([], [], [])
