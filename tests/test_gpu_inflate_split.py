"""GPU tests of the SPLIT path of Deflate / zlib / gzip decoding (include/bz2_mi355x.h section 5, DESIGN_deflate.md "One
large stream across many waves"): an entry of BZ_DF_INF_SPLIT_KIB or more is cut into pieces of BZ_DF_INF_PIECE_KIB, a search
finds a block header in every piece, one wave decodes from each and a chain keeps exactly the pieces that start where the
piece in front of them ended.  A split entry must get the bytes, the length and the verdict of the one-wave path.

Expected values: for clean streams the data the stream was made from, for forged streams the dfforge case, and for EVERY
stream the result of the same call with BZ_DF_INF_SPLIT_KIB=0: the one-wave path, pinned by tests/test_gpu_inflate_batch.py.
Every test asserts through deflate_decode_split_stats() that the split really happened -- [0] >= 1 entries split, [2] >= 2
pieces confirmed without repair, [4] (bytes of the serial tail) below half the output -- unless it says why not: a path that
always fell back would pass otherwise."""
import random
import zlib

import pytest

import dfforge as F
from conftest import product
from test_gpu_deflate_batch import rnd_bytes, words
from test_gpu_inflate_batch import FILL, Pack, run

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
OK, E_DATA, E_EOF = 0, -1, -2


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def split_run(eng, monkeypatch, kind, entries, want, piece, need_split=True, split=4):
    """the entries through the split path (threshold `split` KiB) against `want` ([(bytes, verdict)], None: whatever the
    one-wave path says) and against the one-wave path; returns (results, split stats)"""
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", str(split))
    monkeypatch.setenv("BZ_DF_INF_PIECE_KIB", str(piece))
    got = Pack(entries).decode(eng, kind)
    st = eng.deflate_decode_split_stats()
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", "0")
    ref = Pack(entries).decode(eng, kind)
    assert eng.deflate_decode_split_stats() == [0] * 8
    assert len(got) == len(ref) == len(entries)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g[1] == r[1], "entry %d: verdict %d, the one-wave path says %d" % (i, g[1], r[1])
        assert g[0] == r[0], "entry %d: %d bytes, the one-wave path has %d (first difference at %d)" % (
            i, len(g[0]), len(r[0]), next((k for k, (a, b) in enumerate(zip(g[0], r[0])) if a != b), -1))
    if want is not None:
        for i, (g, w) in enumerate(zip(got, want)):
            assert g[1] == w[1], "entry %d: verdict %d, expected %d" % (i, g[1], w[1])
            assert g[0] == w[0], "entry %d: %d bytes, expected %d" % (i, len(g[0]), len(w[0]))
    print("split stats", st)
    if need_split:
        big = sum(len(g[0]) for g, e in zip(got, entries) if len(e) >= split * 1024)
        assert st[0] >= 1 and st[2] >= 2 and st[4] < big / 2, st
    return got, st


def flushed(level, kind, text, step, **kw):
    """zlib's stream of `text`, flushed every `step` input bytes with sync and full flushes alternating"""
    c = zlib.compressobj(level, zlib.DEFLATED, F.WBITS[kind], **kw)
    z = b""
    for k, at in enumerate(range(0, len(text), step)):
        z += c.compress(text[at:at + step])
        if at + step < len(text):
            z += c.flush(zlib.Z_SYNC_FLUSH if k % 2 else zlib.Z_FULL_FLUSH)
    return z + c.flush()


def letters():
    """tables of a forged dynamic block: the lower-case letters, a blank, end-of-block, lengths 3 .. 10 and 258; distances
    1 .. 4 and 24577 .. 32768"""
    ll = F.balanced([ord(c) for c in "abcdefghijklmnopqrstuvwxyz "] + [256] + list(range(257, 265)) + [285], 286)
    dl = F.balanced([0, 1, 2, 3, 29], 30)
    return ll, dl


# ---- 1. the project's own streams
@pytest.fixture(scope="module")
def own(oracle):
    ins = [words(1, 400000), rnd_bytes(2, 300000)]
    e = oracle.DeflateEncoder()
    e.feed(ins[0], oracle.ACTION_FINISH)
    blocks = list(e.blocks())
    assert sum(1 for _, _, btype, _ in blocks if btype == 2) >= 6
    return ins, {k: [oracle.deflate_encode(x, k) for x in ins] for k in KINDS}


@pytest.mark.parametrize("piece", (4, 16))
@pytest.mark.parametrize("kind", KINDS)
def test_own_streams(eng, own, monkeypatch, kind, piece):
    ins, streams = own
    got, st = split_run(eng, monkeypatch, kind, streams[kind], [(x, OK) for x in ins], piece)
    # at least 6 dynamic blocks of the text and 5 stored blocks of the random bytes; the first of each is the first piece,
    # the last is final, and no two of the others start in the same piece (each is far longer than one)
    assert st[0] == 2 and st[1] >= (6 - 2) + (5 - 2)


# ---- 2. foreign streams
@pytest.fixture(scope="module")
def foreign():
    text = words(3, 120000)
    return text, {(level, kind): flushed(level, kind, text, 3000) for level in (0, 1, 6, 9) for kind in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_foreign_streams(eng, foreign, monkeypatch, kind):
    text, z = foreign
    entries = [z[(level, kind)] for level in (0, 1, 6, 9)]
    got, st = split_run(eng, monkeypatch, kind, entries, [(text, OK)] * 4, 1)
    assert st[0] == 4 and st[2] >= 4 * 10


# ---- 3. no candidates
def test_no_candidates(eng, monkeypatch):
    text = words(4, 100000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    z = c.compress(text) + c.flush()
    assert len(z) >= 8192
    # (fixed blocks are not searched for: the first piece decodes the whole stream, at the one-wave path's speed)
    got, st = split_run(eng, monkeypatch, 0, [z], [(text, OK)], 4, need_split=False)
    assert st[0] == 1 and st[2] == 1 and st[3] == 0 and st[4] == 0


# ---- 4. false candidates that validate
def decoys(n_decoys, piece=1024):
    """a true prefix of many blocks, then n_decoys stored blocks of exactly one piece each, every one with a decoy in its
    payload exactly at a piece start: a complete decodable non-final dynamic block, or a LEN / NLEN pair with zero bits in
    front and a stored block's header behind its payload -- candidates by every rule, and all of them false.  A piece reports its
    first candidate only, so the true block start behind the decoy (the next stored block's LEN) has none: the piece in
    front overshoots and has to be repaired, decoy after decoy.  Then true blocks again."""
    text = words(5, 90000)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    z = b""
    for at in range(0, len(text), 3000):
        z += c.compress(text[at:at + 3000]) + c.flush(zlib.Z_SYNC_FLUSH)          # (byte-aligned, no final block)
    ll, dl = letters()
    s = F.Stream().stored(F.text((-(len(z) + 5 + 100)) % piece, 3))               # the next block starts 100 bytes in front of a piece
    for k in range(n_decoys):
        assert s.w.n == 0 and (len(z) + len(s.w.out) + 100) % piece == 0
        payload = bytearray(F.text(piece - 5, 11 + k))
        if k % 2 == 0:
            d = F.Stream().dynamic(ll, dl).lit(b"a decoy block ").match(8, 4).eob().raw()
        else:
            d = b"\x00" + (5).to_bytes(2, "little") + (5 ^ 0xFFFF).to_bytes(2, "little") + b"decoy" + b"\x00\x00\x00\xff\xff"
        payload[95:95 + len(d)] = d
        s.stored(bytes(payload))
    s.dynamic(ll, dl).lit(b"the true stream goes on ").match(10, 3).eob()
    for k in range(3):
        s.stored(F.text(1500, 40 + k))
    s.fixed(final=True).lit(b"and ends").eob()
    return z + s.raw(), text + bytes(s.out)


def test_false_candidates(eng, monkeypatch):
    z, data = decoys(2)
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, OK)], 1)
    assert st[3] >= 1                                # a repair round
    z, data = decoys(7)
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, OK)], 1)
    assert st[3] == 4 and st[4] > 0                  # more than four false candidates in a row: the serial tail ran


# ---- 5. window chains
def test_window_chain_of_a_repeated_pattern(eng, monkeypatch):
    pat = rnd_bytes(6, 32000)                        # (zlib looks back 32 768 - 262 bytes at the most: a period it can reach)
    data = (pat * 33)[:1 << 20]
    c = zlib.compressobj(9, zlib.DEFLATED, -15)
    z = b""
    for at in range(0, len(data), 8192):
        z += c.compress(data[at:at + 8192]) + c.flush(zlib.Z_SYNC_FLUSH)
    z += c.flush()
    # (every piece's bytes are copies of the piece in front of it: the chain is as deep as there are pieces)
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, OK)], 1)
    assert st[5] > 0 and st[6] >= 3


def window_chain_forged():
    """(stream, data): a distance-1 run through 400 blocks, 40 pieces of stored bytes, and two far copies"""
    ll, dl = letters()
    s = F.Stream().dynamic(ll, dl).lit(b"z")
    marks = []
    for k in range(400):                             # a distance-1 run through 400 blocks (about 12 KiB of headers)
        s.match(258, 1).match(3 + k % 8, 1).eob()
        marks.append(s.w.bit_length)
        s.dynamic(ll, dl)
    s.match(9, 1).eob()
    assert marks[-1] - marks[0] >= 8 * 8 * 1024       # the run crosses at least 8 pieces of 1 KiB
    tail = rnd_bytes(7, 40000)
    s.stored(tail)                                   # 40 pieces of which 39 have no candidate
    s.dynamic(ll, dl).lit(b"far ").match(258, 32768).match(10, 32767).lit(b" away").eob()
    s.fixed(final=True).lit(b".").eob()
    return s.raw(), bytes(s.out)


def test_window_chain_forged(eng, monkeypatch):
    z, data = window_chain_forged()
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, OK)], 1)
    assert st[5] > 0 and st[6] >= 3


# ---- 6. malformed entries
def test_cuts_in_the_last_pieces(eng, foreign, monkeypatch):
    text, zs = foreign
    for level in (6, 0):                             # level 0: the cuts fall into stored payloads
        z = zs[(level, 1)]
        cuts = [len(z) - 3072 + c for c in F.cut_points(3072)]
        entries = [z[:c] for c in cuts]
        want = None
        if level == 6:
            want = [(zlib.decompressobj(15).decompress(e), E_EOF) for e in entries]
        got, st = split_run(eng, monkeypatch, 1, entries, want, 1)
        assert st[0] == len(cuts)
        for g in got:
            assert g[1] == E_EOF and text.startswith(g[0])


def test_flipped_bytes(eng, foreign, monkeypatch):
    text, zs = foreign
    z = zs[(6, 1)]
    r = random.Random(8)
    entries = []
    for _ in range(24):
        b = bytearray(z)
        b[r.randrange(len(z) // 3, 2 * len(z) // 3)] ^= 1 << r.randrange(8)
        entries.append(bytes(b))
    got, st = split_run(eng, monkeypatch, 1, entries, None, 1)
    # (whatever the damage does to the codes, Adler-32 sees it -- unless it hit a padding bit and did nothing)
    assert all(v != OK or d == text for d, v in got) and sum(v != OK for _, v in got) >= 12


def test_distance_in_front_of_the_entry(eng, monkeypatch):
    ll, dl = letters()
    s = F.Stream().stored(F.text(2100, 1))           # the first two pieces
    s.dynamic(ll, dl).lit(b"in the third piece ")
    data = bytes(s.out)
    s.match(10, 30000, emit=False)                   # 30 000 <= 32 768, but only 2 119 bytes lie in front
    s.lit(b"never").eob()
    s.stored(F.text(3000, 2)).fixed(final=True).lit(b"x").eob()
    z = s.raw(0xFF)
    assert len(z) >= 4096 and len(data) == 2119
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, E_DATA)], 1)
    assert st[2] >= 2


def test_wrong_trailers_and_junk(eng, foreign, monkeypatch):
    text, zs = foreign
    z1, z2 = zs[(6, 1)], zs[(9, 2)]
    junk = zs[(1, 0)]                                # valid block headers behind the final block
    flip = lambda z, at: z[:at] + bytes([z[at] ^ 0x10]) + z[at + 1:]
    got, st = split_run(eng, monkeypatch, 1, [flip(z1, len(z1) - 1), flip(z1, len(z1) - 4), z1 + junk], [(text, E_DATA), (text, E_DATA), (text, OK)], 1)
    got, st = split_run(eng, monkeypatch, 2, [flip(z2, len(z2) - 1), flip(z2, len(z2) - 8), z2 + junk], [(text, E_DATA), (text, E_DATA), (text, OK)], 1)
    got, st = split_run(eng, monkeypatch, 0, [zs[(6, 0)] + junk], [(text, OK)], 1)


# ---- 7. a mixed batch
def test_mixed_batch(eng, pkg, foreign, monkeypatch):
    text, zs = foreign
    small = [words(20 + i, 50 + 600 * i) for i in range(6)]
    other = words(9, 70000)
    bad = zs[(6, 1)][:len(zs[(6, 1)]) - 1500]
    entries = [zlib.compress(small[0]), zs[(6, 1)], zlib.compress(small[1]), zlib.compress(small[2], 1), bad, zlib.compress(small[3]),
               flushed(9, 1, other, 5000), zlib.compress(small[4]), zlib.compress(small[5], 9)]
    want = [(small[0], OK), (text, OK), (small[1], OK), (small[2], OK), (zlib.decompressobj(15).decompress(bad), E_EOF), (small[3], OK),
            (other, OK), (small[4], OK), (small[5], OK)]
    got, st = split_run(eng, monkeypatch, 1, entries, want, 4)
    assert st[0] == 3
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", "4")
    p = Pack(entries)
    assert p.decode(eng, 1) == got
    assert p.sizes_verdicts == [v for _, v in got]   # the sizes-only form (no trailer is wrong here)
    assert eng.deflate_decode_split_stats()[0] == 3
    s_off, s_len, _ = p.sizes(eng, 1)
    assert eng.deflate_decode_split_stats()[0] == 3 and eng.deflate_decode_split_stats()[5] == 0   # split, and nothing written
    need = max(a + n for a, n in zip(s_off, s_len))
    with pytest.raises(pkg.CompressionError) as ei:
        p.decode(eng, 1, cap=need - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    assert p.host == bytes([FILL]) * len(p.host)
    # the host forms and the classes go through the same core
    assert pkg.deflate_decompress_batch(entries, 1) == got
    assert pkg.deflate_decompress(entries[1], 1) == (text, OK)
    assert pkg.deflate_decompress(bad, 1) == got[4]
    for cls, kind in ((pkg.Deflater, 0), (pkg.ZlibDecoder, 1), (pkg.GZipDecoder, 2)):
        assert cls().decode_all(zs[(6, kind)]) == text
        cut = zs[(6, kind)][:-1500]
        with pytest.raises(pkg.CompressionError) as ei:
            cls().decode_all(cut)
        assert ei.value.kind == "UnexpectedEof" and ei.value.partial == zlib.decompressobj(F.WBITS[kind]).decompress(cut)


# ---- 8. the defaults
def test_defaults(eng, oracle, monkeypatch):
    monkeypatch.delenv("BZ_DF_INF_SPLIT_KIB", raising=False)
    monkeypatch.delenv("BZ_DF_INF_PIECE_KIB", raising=False)
    r = random.Random(10)
    vocab = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(1, 9))) for _ in range(3000)]
    text = b" ".join(r.choices(vocab, k=600000))
    z = zlib.compressobj(1, zlib.DEFLATED, -15)
    z = z.compress(text) + z.flush()
    assert 1.2 * (1 << 20) <= len(z) <= 2.5 * (1 << 20), len(z)
    got = run(eng, 0, [z], [(text, OK)])
    st = eng.deflate_decode_split_stats()
    print("split stats", st)
    assert st[0] == 1 and st[2] >= 2 and st[4] < len(text) / 2
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", "0")
    assert Pack([z]).decode(eng, 0) == got and eng.deflate_decode_split_stats() == [0] * 8
    monkeypatch.delenv("BZ_DF_INF_SPLIT_KIB")
    # the 200 000-byte entries of test_gpu_inflate_batch.py stay on the one-wave path
    ins = [words(200000, 200000), rnd_bytes(200001, 200000)]
    run(eng, 0, [oracle.deflate_encode(x, 0) for x in ins], [(x, OK) for x in ins])
    assert eng.deflate_decode_split_stats() == [0] * 8
    assert eng.deflate_decode_batch_stats()[7] == 2
