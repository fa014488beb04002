"""GPU tests of ONE LARGE LZHUF STREAM ACROSS MANY WAVES (include/bz2_mi355x.h section 9 (g), DESIGN_lzhuf.md section 11).
The streams are those of tests/lzhsplit.py -- a few KB with blocks of 1 .. 2 000 codes, so that BZ_LZH_SPLIT_KIB of a
fraction of a KiB splits them and BZ_LZH_SPLIT_CAND_BYTES=1 lets every candidate through -- which tests/test_lzhsplit.py
pins.  Every expected byte, length, verdict and figure comes from the model (tests/lzhref.py); the same streams are also run
on the one-wave path (BZ_LZH_SPLIT_KIB=0) and must give the same."""
import contextlib
import ctypes as C
import os
import random

import pytest

import lzhref as R
import lzhsplit as S
from conftest import product

pytestmark = pytest.mark.gpu

OK, E_DATA, E_EOF = 0, -1, -2
FILL, GUARD = 0xEE, 64
SPLIT_ALL = {"BZ_LZH_SPLIT_KIB": "0.0625", "BZ_LZH_SPLIT_CAND_BYTES": "1"}  # entries of 64 bytes and more, any number of candidates
ONE_WAVE = {"BZ_LZH_SPLIT_KIB": "0"}


@contextlib.contextmanager
def env(values):
    """the switches are read per call"""
    old = {k: os.environ.get(k) for k in ("BZ_LZH_SPLIT_KIB", "BZ_LZH_SPLIT_CAND_BYTES")}
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

    def decode(self, eng, method, orig_len=None, prefill=-1):
        """-> ([(bytes, verdict)], stats, split stats): sizes-only against the real call, the placement rules, nothing written
        outside the reported ranges (the guards on both sides of d_out included), capacity one byte short"""
        torch = self.torch
        pkg = product()
        s_off, s_len, s_ver = eng.lzh_decode_batch_device(method, self.t.data_ptr(), self.off, self.len, None, 0, orig_len, prefill)
        s_stats, s_split = eng.lzh_decode_stats(), eng.lzh_decode_split_stats()
        cap = max([a + n for a, n in zip(s_off, s_len)] + [0])
        o = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        assert o.data_ptr() % 16 == 0
        if cap:
            with pytest.raises(pkg.CompressionError) as ei:
                eng.lzh_decode_batch_device(method, self.t.data_ptr(), self.off, self.len, o.data_ptr() + GUARD, cap - 1, orig_len, prefill)
            assert ei.value.code == pkg.BZ_E_CAPACITY
            torch.cuda.synchronize()
            assert bool((o == FILL).all())
        try:
            o_off, o_len, ver = eng.lzh_decode_batch_device(method, self.t.data_ptr(), self.off, self.len, o.data_ptr() + GUARD, cap,
                                                            orig_len, prefill)
        finally:
            torch.cuda.synchronize()
            host = o.cpu().numpy().tobytes()
        stats, split = eng.lzh_decode_stats(), eng.lzh_decode_split_stats()
        assert (o_off, o_len, ver) == (s_off, s_len, s_ver)
        assert stats[:7] == s_stats[:7] and split[:5] == s_split[:5] and split[7] == s_split[7]
        assert host[:GUARD] == bytes([FILL]) * GUARD
        body = host[GUARD:]
        end = 0
        for a, n in zip(o_off, o_len):
            assert a % 16 == 0 and a == (end + 15) & ~15
            assert body[end:a] == bytes([FILL]) * (a - end)
            end = a + n
        assert end <= cap
        assert body[end:] == bytes([FILL]) * (len(body) - end)
        return [(body[a:a + n], v) for a, n, v in zip(o_off, o_len, ver)], stats, split


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


@pytest.fixture(scope="module")
def groups():
    """{(method, prefill): [(case, the model's Result, the split model's over the TRUE starts)]}, once.  The split model over
    the true starts alone gives the chain, the pieces decoded again and the bytes the gather fills: false pieces never enter
    a chain, so they change none of these (the whole search in Python is tests/test_lzhsplit.py's)."""
    g = {}
    for c in S.cases():
        want = c.model()
        sp = S.decode(c.stream, c.method, c.orig_len, c.prefill, cands=c.starts)
        assert S.same(sp, want)
        g.setdefault((c.method, c.prefill), []).append((c, want, sp))
    return g


def model_stats(results):
    clean = [r for r in results if r.verdict == OK]
    return [len(clean), len(results) - len(clean), sum(r.blocks for r in results), sum(r.literals for r in results),
            sum(r.matches for r in results), sum(len(r.out) for r in results), sum((r.bits + 7) // 8 for r in clean)]


def check(got, want, names):
    assert len(got) == len(want)
    for g, r, name in zip(got, want, names):
        assert g[1] == r.verdict, "%s: verdict %d, expected %d" % (name, g[1], r.verdict)
        assert g[0] == bytes(r.out), "%s: %d bytes, expected %d" % (name, len(g[0]), len(r.out))


# ---- 0. the surface
def test_the_new_symbol_and_its_parameter_errors(eng):
    pkg = product()
    L = pkg.lib()
    assert L.bz_gpu_last_lzh_decode_split_stats(None, (C.c_uint64 * 8)()) == pkg.BZ_E_PARAM
    assert L.bz_gpu_last_lzh_decode_split_timings(None, (C.c_double * 6)()) == pkg.BZ_E_PARAM
    assert len(pkg.GpuEngine.LZH_DECODE_SPLIT_STATS) == 8 and len(eng.lzh_decode_split_stats()) == 8


# ---- 1. the forged cases: split, and on one wave
@pytest.mark.parametrize("key", sorted({(c.method, c.prefill) for c in S.cases()}))
def test_forged_cases_split_and_on_one_wave(eng, groups, key):
    method, prefill = key
    group = groups[key]
    names = [c.name for c, _, _ in group]
    ol = [c.orig_len for c, _, _ in group]
    ol = ol if any(x is not None for x in ol) else None
    p = Pack([c.stream for c, _, _ in group])
    with env(SPLIT_ALL):
        got, stats, split = p.decode(eng, method, ol, prefill)
    check(got, [w for _, w, _ in group], names)
    assert stats[:7] == model_stats([w for _, w, _ in group])
    stay = [sp for c, _, sp in group if not sp.fallback]
    assert split[0] == len(stay) and split[7] == len(group) - len(stay)
    assert split[2] == sum(sp.chain for sp in stay)
    assert split[1] >= sum(len([s for s in c.starts[1:] if S.header_end(c.stream, s, method) is not None])
                           for c, _, sp in group if not sp.fallback)
    assert split[3] >= sum(len(c.expect.get("images", ())) for c, _, sp in group if not sp.fallback)
    assert split[3] == split[1] + split[0] - split[2]              # every candidate's piece is in a chain or false
    assert split[4] == sum(sp.again for sp in stay)
    assert split[6] == sum(sp.filled for sp in stay)
    assert split[5] >= len([sp for sp in stay if len(sp.out)])
    with env(ONE_WAVE):
        one, stats1, split1 = p.decode(eng, method, ol, prefill)
    assert one == got and stats1[:7] == stats[:7] and stats1[7] == 2 and split1 == [0] * 8


def test_a_pointer_chain_over_ten_pieces_takes_several_jump_rounds(eng, groups):
    (c, want, sp), = [x for x in groups[(5, -1)] if x[0].name == "run_ten_blocks"]
    assert sp.depth == 9 and sp.chain == 10
    with env(SPLIT_ALL):
        got, _, split = Pack([c.stream]).decode(eng, 5)
    check(got, [want], [c.name])
    assert split[0] == 1 and split[2] == 10 and split[6] == sp.filled and split[5] >= 2


def test_host_call_and_class(groups):
    pkg = product()
    with env(SPLIT_ALL):
        for (m, prefill), group in sorted(groups.items()):
            for c, want, _ in group:
                assert pkg.lzhuf_decompress(c.stream, m, c.orig_len, prefill) == (bytes(want.out), want.verdict), c.name
                d = pkg.LzhufDecoder(pkg.LzhufMethod(m), orig_len=c.orig_len, prefill=prefill)
                if want.verdict == OK:
                    assert d.decode_all(c.stream) == bytes(want.out), c.name
                else:
                    with pytest.raises(pkg.CompressionError) as ei:
                        d.decode_all(c.stream)
                    assert ei.value.code == want.verdict and ei.value.partial == bytes(want.out), c.name


# ---- 2. every prefix of one multi-block stream
def test_every_prefix_of_a_multi_block_stream(eng):
    s, rows = S.prefix_results()
    full = bytes(R.decode_full(s, 5).out)
    p = Pack([s[:n] for n in range(len(s) + 1)])
    want_stats = [sum(1 for r in rows if r[1] == OK), sum(1 for r in rows if r[1] != OK), sum(r[3] for r in rows), sum(r[4] for r in rows),
                  sum(r[5] for r in rows), sum(r[0] for r in rows), sum((r[2] + 7) // 8 for r in rows if r[1] == OK)]
    _, starts = S.prefix_stream()
    short = (S.header_end(s, starts[1], 5) + 7) // 8               # prefixes shorter than this have one piece
    for switches in (SPLIT_ALL, ONE_WAVE):
        with env(switches):
            off, ln, ver = eng.lzh_decode_batch_device(5, p.t.data_ptr(), p.off, p.len, None, 0)
            assert (ln, ver) == ([r[0] for r in rows], [r[1] for r in rows])
            assert eng.lzh_decode_stats()[:7] == want_stats
            split = eng.lzh_decode_split_stats()
            # a prefix of 64 bytes or more stays split iff piece 0 stops: the second block's header lies whole inside it
            assert split == [0] * 8 if switches is ONE_WAVE else (split[0], split[7]) == (len(s) + 1 - short, short - 64)
    with env(SPLIT_ALL):  # the bytes of every fiftieth prefix and of those around the block starts
        pick = sorted(set(range(0, len(s) + 1, 50)) | {max(0, b // 8 + d) for b in starts for d in (-1, 0, 1, 2)} | {len(s)})
        got, _, _ = Pack([s[:n] for n in pick]).decode(eng, 5)
        assert got == [(full[:rows[n][0]], rows[n][1]) for n in pick]


# ---- 3. split and small entries in one batch; the candidate cap
def test_split_and_small_entries_shuffled(eng, groups):
    group = list(groups[(5, -1)])
    small = [R.encode(b"abcabcabc", 5), b"", R.encode(b"x" * 300, 5), b"\x00\x01"]
    rng = random.Random(29)
    with env({"BZ_LZH_SPLIT_KIB": "0.1", "BZ_LZH_SPLIT_CAND_BYTES": "1"}):  # (102 bytes: some cases split, some do not)
        for _ in range(3):
            entries = [(c.stream, c.orig_len, w) for c, w, _ in group] + [(s, None, R.decode_full(s, 5)) for s in small]
            rng.shuffle(entries)
            got, stats, split = Pack([e[0] for e in entries]).decode(eng, 5, [e[1] for e in entries])
            check(got, [e[2] for e in entries], ["entry %d" % i for i in range(len(entries))])
            assert stats[:7] == model_stats([e[2] for e in entries])
            assert 0 < split[0] < len(entries)
            assert split[0] + split[7] == len([e for e in entries if len(e[0]) >= 102])


def test_a_stream_over_the_candidate_cap_falls_back(eng):
    c = S.over_cap_stream()
    assert len(c.stream) >= 1024 and len(c.starts) > max(64, len(c.stream) // 1024)
    with env({"BZ_LZH_SPLIT_KIB": "1"}):  # (the default of 1 024 bytes per candidate)
        got, stats, split = Pack([c.stream]).decode(eng, c.method)
    check(got, [c.model()], [c.name])
    assert split[0] == 0 and split[7] == 1 and stats[7] == 2 + 1   # (the count pass of the search, then the two launches)
    with env({"BZ_LZH_SPLIT_KIB": "1", "BZ_LZH_SPLIT_CAND_BYTES": "8"}):
        got, _, split = Pack([c.stream]).decode(eng, c.method)
    check(got, [c.model()], [c.name])
    assert split[0] == 1 and split[7] == 0 and split[2] == len(c.starts)


# ---- 4. a real stream at the default threshold
@pytest.mark.parametrize("method", (5, 7))
def test_four_mib_from_the_encoder_at_the_default_threshold(eng, method):
    import torch
    import corpus
    pkg = product()
    data = corpus.corpus_bytes(4 << 20)
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = pkg.lzhuf_encode_batch_bound([len(data)])
    z = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    e_off, e_len = eng.lzh_encode_batch_device(method, src.data_ptr(), [0], [len(data)], z.data_ptr(), cap)
    assert e_len[0] >= 1 << 20
    out = torch.full((len(data) + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
    with env({}):
        off, ln, ver = eng.lzh_decode_batch_device(method, z.data_ptr(), e_off, e_len, out.data_ptr() + GUARD, len(data))
    torch.cuda.synchronize()
    assert (off, ln, ver) == ([0], [len(data)], [OK])
    assert bool((out[GUARD:GUARD + len(data)] == src).all())
    assert bool((out[:GUARD] == FILL).all()) and bool((out[GUARD + len(data):] == FILL).all())
    split, stats = eng.lzh_decode_split_stats(), eng.lzh_decode_stats()
    assert split[0] == 1 and split[7] == 0 and split[2] == stats[2] >= 2 and split[4] == 0
    assert stats[0] == 1 and stats[5] == len(data) and stats[6] == e_len[0]
