"""GPU tests of Deflate / zlib DECODING WITH A PRESET DICTIONARY (df_gpu_decode_batch_device_dict, df_decode_batch_dict,
df_decode_buffer_dict and the Python surface over them; include/bz2_mi355x.h section 5, clause (c)): the window is history
in front of position 0 of every entry's output, on the one-wave path and on the split path.

Expected values: for round trips the data the stream was made from; forged streams come from tests/dfforge_dict.py, which
tests/test_dfforge_dict.py pins against zlib.decompressobj(wbits, zdict=dict); for split entries also the same call on the
one-wave path.  One batch call per (dictionary, kind)."""
import ctypes as C
import random
import zlib

import pytest

import dfforge as F
import dfforge_dict as D
from conftest import product
from test_gpu_deflate_batch import words
from test_gpu_inflate_batch import Pack, run

pytestmark = pytest.mark.gpu

OK, E_DATA, E_EOF = 0, -1, -2
KINDS = (0, 1)
OWN_DICT = (1, 300, 32768, 40000)


class WithDict:
    """the engine with `dict_` in every deflate_decode_batch_device call: the placement and fill checks of Pack.decode hold
    with a dictionary as they are"""

    def __init__(self, eng, dict_):
        self._eng, self._dict = eng, dict_

    def deflate_decode_batch_device(self, *args):
        return self._eng.deflate_decode_batch_device(*args, dict_=self._dict)

    def __getattr__(self, name):
        return getattr(self._eng, name)


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def run_cases(eng, kind, cases):
    assert cases and all(c.kind == kind and c.dict == cases[0].dict for c in cases)
    return run(WithDict(eng, cases[0].dict), kind, [c.stream for c in cases], [(c.data, c.verdict) for c in cases])


# ---- 1. the forged corpus
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", D.DICT_LEN)
def test_forged_corpus(eng, n, kind):
    cases = D.copy_cases(n)
    if kind == 1:
        cases = [D.as_zlib(c) for c in cases] + [c for c in D.zlib_cases(n) if "other_dictionary" not in c.name]
    run_cases(eng, kind, cases)
    st = eng.deflate_decode_batch_stats()
    assert st[0] == sum(c.verdict == OK for c in cases) and st[0] + st[1] == len(cases)
    # the bits of an entry include the six header bytes: a clean stream is consumed whole
    assert st[6] >= sum(len(c.stream) for c in cases if c.verdict == OK)
    run_cases(eng, kind, cases[::-1])


@pytest.mark.parametrize("n", D.DICT_LEN)
def test_another_dictionary_of_the_same_length(eng, n):
    other = next(c for c in D.zlib_cases(n) if "other_dictionary" in c.name)
    run_cases(eng, 1, [other])                              # the DICTID tells it: BZ_E_DATA, no bytes
    cases = [c for c in D.copy_cases(n) if c.verdict == OK]
    want = [(zlib.decompressobj(-15, zdict=other.dict).decompress(c.stream), OK) for c in cases]
    assert any(w[0] != c.data for w, c in zip(want, cases))
    run(WithDict(eng, other.dict), 0, [c.stream for c in cases], want)      # kind 0 cannot: the bytes that dictionary gives


# ---- 2. the project's own streams
def own_inputs(d):
    return [b"", b"x", d[-300:], d[:5000], words(19, 65537), d * 3]


@pytest.fixture(scope="module")
def own(oracle):
    out = {}
    for n in OWN_DICT:
        d = words(100 + n, n)
        ins = own_inputs(d)
        streams = {k: [oracle.deflate_encode(x, k, d) for x in ins] for k in KINDS}
        for k in KINDS:     # (none of them is the reference's match-free dynamic block: zlib reads them all)
            for x, z in zip(ins, streams[k]):
                o = zlib.decompressobj(F.WBITS[k], zdict=d)
                assert o.decompress(z) == x and o.eof
        out[n] = (d, ins, streams)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", OWN_DICT)
def test_round_trip_of_own_streams(eng, pkg, own, n, kind):
    d, ins, streams = own[n]
    z = streams[kind]
    want = [(x, OK) for x in ins]
    run(WithDict(eng, d), kind, z, want)
    assert eng.deflate_decode_batch_stats()[5] == sum(len(x) for x in ins)
    assert pkg.deflate_decompress_batch(z, kind, dict_=d) == want
    assert pkg.deflate_decompress_batch(z, kind, dict_=bytearray(d)) == want
    for x, s in zip(ins, z):
        assert pkg.deflate_decompress(s, kind, dict_=d) == (x, OK)
    cls = (pkg.Deflater, pkg.ZlibDecoder)[kind]
    assert cls.with_dict(d).decode_all(z[3]) == ins[3]
    dec, it = cls(dict_=d), iter(z[2])
    got = []
    while True:
        b = dec.next(it)
        if b is None:
            break
        got.append(b)
    assert bytes(got) == ins[2]
    # the same streams without the dictionary: today's behaviour -- no entry sees a window it was not given
    got = Pack(z).decode(eng, kind)
    for i, ((g, v), x, s) in enumerate(zip(got, ins, z)):
        o = zlib.decompressobj(F.WBITS[kind])
        try:
            clean = o.decompress(s) == x and o.eof
        except zlib.error:
            clean = False
        assert kind == 0 or not clean
        assert v == (OK if clean else E_DATA), "entry %d without the dictionary: verdict %d" % (i, v)
        assert x.startswith(g) and (clean or kind == 0 or g == b"")
    if kind == 1 or n > 1:      # (the last 300 bytes of the dictionary: a match into it)
        assert got[2][1] == E_DATA
        with pytest.raises(pkg.CompressionError) as ei:
            cls().decode_all(z[2])
        assert ei.value.kind == "DataError"


# ---- 3. foreign streams
@pytest.mark.parametrize("wbits", (-15, 15))
@pytest.mark.parametrize("n", (300, 40000))
def test_foreign_streams(eng, n, wbits):
    d = words(200 + n, n)
    texts = [d[-200:] + words(7, 4097) + d[:300], words(8, 65537), d[len(d) // 2:] + d, b""]
    entries, want = [], []
    for t in texts:
        for level in (1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, wbits, zdict=d)
            h = len(t) // 2
            entries.append(c.compress(t[:h]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(t[h:]) + c.flush())
            want.append((t, OK))
    run(WithDict(eng, d), 0 if wbits < 0 else 1, entries, want)


# ---- 4. a dictionary that is never used changes nothing
def test_unused_dictionary(eng):
    cases = [c for c in F.clean_cases() if c.kind == 0]
    assert len(cases) >= 150
    run(WithDict(eng, F.text(300, 77)), 0, [c.stream for c in cases], [(c.data, OK) for c in cases])


# ---- 5. a mixed batch
def test_mixed_batch(eng, pkg):
    n = 258
    d = D.dictionary(n)
    for kind in KINDS:
        cases = D.copy_cases(n) if kind == 0 else [D.as_zlib(c) for c in D.copy_cases(n)] + D.zlib_cases(n)[:-1]
        clean = [c for c in cases if c.verdict == OK]
        entries = [(c.stream, (c.data, c.verdict), c.data) for c in cases]
        for c in clean[::9]:        # truncated: every cut of a few clean streams is BZ_E_EOF, with a prefix of the data
            entries += [(c.stream[:k], None, c.data) for k in sorted({len(c.stream) - 1, len(c.stream) // 2, 1})]
        random.Random(5).shuffle(entries)
        got = Pack([e for e, _, _ in entries]).decode(WithDict(eng, d), kind)
        alone = {}
        for (e, w, data), g in zip(entries, got):
            if w is not None:
                assert g == w
            else:
                assert g[1] == E_EOF and data.startswith(g[0])
                alone.setdefault(e, g)
        assert {v for _, v in got} == {OK, E_DATA, E_EOF}
        # ... and each entry alone gets what it got among the others
        few = list(alone.items())[:6]
        assert Pack([e for e, _ in few]).decode(WithDict(eng, d), kind) == [g for _, g in few]
    # count == 0 with a dictionary: BZ_OK, nothing touched
    assert eng.deflate_decode_batch_device(0, None, [], [], None, 0, dict_=d) == ([], [], [])
    # gzip has no dictionary
    p = Pack([b"\x1f\x8b"])
    with pytest.raises(ValueError):
        eng.deflate_decode_batch_device(2, p.t.data_ptr(), p.off, p.len, None, 0, dict_=d)
    a, b, v = (C.c_uint64 * 1)(p.off[0]), (C.c_uint64 * 1)(2), (C.c_int32 * 1)()
    assert pkg.lib().df_gpu_decode_batch_device_dict(eng._h, 2, p.t.data_ptr(), a, b, 1, d, len(d), None, 0, a, b, v) == pkg.BZ_E_PARAM
    assert pkg.lib().df_gpu_decode_batch_device_dict(eng._h, 0, p.t.data_ptr(), a, b, 1, None, 5, None, 0, a, b, v) == pkg.BZ_E_PARAM
    # dict_len == 0 is the call without a dictionary, whatever the pointer: FDICT stays BZ_E_DATA
    z = D.zlib_cases(n)[0]
    assert Pack([z.stream]).decode(WithDict(eng, b""), 1) == [(b"", E_DATA)]
    p = Pack([z.stream])
    a, b = (C.c_uint64 * 1)(p.off[0]), (C.c_uint64 * 1)(p.len[0])
    o, ln = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    assert pkg.lib().df_gpu_decode_batch_device_dict(eng._h, 1, p.t.data_ptr(), a, b, 1, d, 0, None, 0, o, ln, v) == pkg.BZ_OK
    assert (ln[0], v[0]) == (0, E_DATA)


# ---- 6. the split path
def split_run(eng, monkeypatch, kind, entries, want, dict_, piece=1, split=4):
    """the entries through the split path against `want` and against the one-wave path (tests/test_gpu_inflate_split.py's
    split_run, with the dictionary); returns (results, split stats)"""
    eng = WithDict(eng, dict_)
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", str(split))
    monkeypatch.setenv("BZ_DF_INF_PIECE_KIB", str(piece))
    got = Pack(entries).decode(eng, kind)
    st = eng.deflate_decode_split_stats()
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", "0")
    ref = Pack(entries).decode(eng, kind)
    assert eng.deflate_decode_split_stats() == [0] * 8
    assert len(got) == len(ref) == len(entries) == len(want)
    for i, (g, r, w) in enumerate(zip(got, ref, want)):
        assert g[1] == r[1] == w[1], "entry %d: verdict %d, the one-wave path says %d, expected %d" % (i, g[1], r[1], w[1])
        assert r[0] == w[0], "entry %d, one-wave path: %d bytes, expected %d" % (i, len(r[0]), len(w[0]))
        assert g[0] == w[0], "entry %d: %d bytes, expected %d (first difference at %d)" % (
            i, len(g[0]), len(w[0]), next((k for k, (a, b) in enumerate(zip(g[0], w[0])) if a != b), -1))
    print("split stats", st)
    return got, st


@pytest.mark.parametrize("flush", (zlib.Z_FULL_FLUSH, zlib.Z_SYNC_FLUSH), ids=("full", "sync"))
@pytest.mark.parametrize("kind", KINDS)
def test_split_zlib_made(eng, monkeypatch, kind, flush):
    """(a) about 64 KiB whose text is cut from the dictionary, flushed every 700 bytes (behind a sync flush the matches of
    LATER pieces still reach into the window)"""
    d = words(31, 32768)
    r = random.Random(9)
    text = b""
    while len(text) < 65536:
        at = r.randrange(len(d) - 400)
        text += d[at:at + r.randrange(40, 400)]
    c = zlib.compressobj(6, zlib.DEFLATED, F.WBITS[kind], zdict=d)
    z = b"".join(c.compress(text[at:at + 700]) + c.flush(flush) for at in range(0, len(text), 700)) + c.flush()
    assert len(z) >= 8192
    got, st = split_run(eng, monkeypatch, kind, [z], [(text, OK)], d)
    assert st[0] == 1 and st[2] > 1 and st[4] < len(text) / 2, st


@pytest.mark.parametrize("n", (100, 20000))
def test_split_forged(eng, monkeypatch, n):
    """(b) matches of a later piece that lie in front of the entry, (c) one byte too far there, (d) a straddle there"""
    cases = D.split_cases(n)
    ok = [c for c in cases if c.verdict == OK]
    bad = [c for c in cases if c.verdict != OK]
    assert len(ok) == 4 and len(bad) == 1 and bad[0].verdict == E_DATA
    got, st = split_run(eng, monkeypatch, 0, [c.stream for c in ok], [(c.data, OK) for c in ok], ok[0].dict)
    assert st[0] == len(ok) and st[2] == sum(c.pieces for c in ok) and st[3] == 0 and st[4] == 0, st
    # a window byte is its own root: only the bytes whose value lies in an earlier piece of the ENTRY are left to the gather
    assert st[5] == sum(c.unresolved for c in ok), st
    got, st = split_run(eng, monkeypatch, 0, [c.stream for c in cases], [(c.data, c.verdict) for c in cases], cases[0].dict)
    assert st[0] == len(cases) and st[2] == sum(c.pieces for c in cases), st
    # ... and in a zlib container, whose six header bytes move every piece
    z = [D.as_zlib(c) for c in cases]
    got, st = split_run(eng, monkeypatch, 1, [c.stream for c in z], [(c.data, c.verdict) for c in z], cases[0].dict)
    assert st[0] == len(cases) and st[2] >= len(cases), st
