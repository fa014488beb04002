"""GPU tests of batched Deflate / zlib / gzip DECODING (df_gpu_decode_batch_device, df_decode_batch, df_decode_buffer and the
Python surface over them): many streams in one call, one wave per stream.  The expected value of every round trip is the
data the stream was made from; forged streams come from tests/dfforge.py, which tests/test_dfforge.py pins against Python's
zlib; the verdicts and prefixes of malformed streams are those of the contract in include/bz2_mi355x.h, section 5."""
import random
import zlib

import pytest

import dfforge as F
from conftest import product
from test_gpu_deflate_batch import QUIRK, Dev, rnd_bytes, words

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
OK, E_DATA, E_EOF = 0, -1, -2
FILL = 0xEE


class Pack:
    """entries at 4-byte-aligned offsets behind a 0xEE lead, 0xEE in the gaps (as Dev packs its inputs); the device
    buffer ends with the last entry's last byte"""

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

    def sizes(self, eng, kind):
        return eng.deflate_decode_batch_device(kind, self.t.data_ptr(), self.off, self.len, None, 0)

    def decode(self, eng, kind, cap=None):
        """[(bytes, verdict)]; checks the placement rules and that nothing outside the reported ranges was written"""
        torch = self.torch
        s_off, s_len, s_ver = self.sizes(eng, kind)
        need = max([a + n for a, n in zip(s_off, s_len)] + [0])
        cap = need if cap is None else cap
        o = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
        try:
            o_off, o_len, ver = eng.deflate_decode_batch_device(kind, self.t.data_ptr(), self.off, self.len, o.data_ptr(), cap)
        finally:
            torch.cuda.synchronize()
            self.host = o.cpu().numpy().tobytes()
        assert (o_off, o_len) == (s_off, s_len)
        self.sizes_verdicts = s_ver
        end = 0
        for a, n in zip(o_off, o_len):
            assert a % 16 == 0 and a == (end + 15) & ~15           # input order, every offset a multiple of 16
            assert self.host[end:a] == bytes([FILL]) * (a - end)   # the gaps keep their fill
            end = a + n
        assert end <= cap
        assert self.host[end:] == bytes([FILL]) * (len(self.host) - end)   # ... and so does everything behind the last entry
        return [(self.host[a:a + n], v) for a, n, v in zip(o_off, o_len, ver)]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def run(eng, kind, entries, want):
    got = Pack(entries).decode(eng, kind)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[1] == w[1], "entry %d: verdict %d, expected %d" % (i, g[1], w[1])
        assert g[0] == w[0], "entry %d: %d bytes, expected %d" % (i, len(g[0]), len(w[0]))
    return got


def run_cases(eng, kind, cases):
    return run(eng, kind, [c.stream for c in cases], [(c.data, c.verdict) for c in cases])


# ---- 1. the project's own streams
OWN_N = (0, 1, 2, 3, 4095, 4096, 4097, 65535, 65536, 65537, 200000)


@pytest.fixture(scope="module")
def own(oracle):
    ins = [words(n, n) for n in OWN_N] + [rnd_bytes(n + 1, n) for n in OWN_N] + [b"fixed", b"ab\x00\xffz"]
    for x in ins:       # none of them may be the reference's match-free dynamic block (malformed: see QUIRK below)
        e = oracle.DeflateEncoder()
        e.feed(x, oracle.ACTION_FINISH)
        for tokens, nbytes, btype, _ in e.blocks():
            assert not (btype == 2 and tokens >= nbytes), "a dynamic block without any match"
    return ins, {k: [oracle.deflate_encode(x, k) for x in ins] for k in KINDS}


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_of_own_streams(eng, own, kind):
    ins, streams = own
    run(eng, kind, streams[kind], [(x, OK) for x in ins])
    st = eng.deflate_decode_batch_stats()
    assert st[0] == len(ins) and st[1] == 0
    assert min(st[2:5]) > 0                                   # stored, fixed and dynamic blocks all occurred
    assert st[5] == sum(len(x) for x in ins)
    assert st[6] == sum(len(s) for s in streams[kind])
    assert st[7] == (2 if kind == 0 else 3)


# ---- 2. foreign streams
@pytest.mark.parametrize("kind", KINDS)
def test_foreign_streams(eng, kind):
    wbits = F.WBITS[kind]
    texts = [words(n, n) for n in (1, 4097, 65537, 200000)] + [rnd_bytes(5, 70000), b""]
    entries, want = [], []
    for t in texts:
        for level in (0, 1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, wbits)
            h = len(t) // 2
            z = c.compress(t[:h]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(t[h:]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(t[:99]) + c.flush()
            entries.append(z)
            want.append((t + t[:99], OK))
        c = zlib.compressobj(6, zlib.DEFLATED, wbits, 8, zlib.Z_FIXED)
        entries.append(c.compress(t) + c.flush())
        want.append((t, OK))
        c = zlib.compressobj(9, zlib.DEFLATED, wbits)
        entries.append(c.compress(t) + c.flush())
        want.append((t, OK))
    run(eng, kind, entries, want)


# ---- 3. the copy grid
def test_copy_grid(eng):
    cases = F.copy_grid() + F.copy_chains() + F.copy_residues()
    assert len(cases) >= 112 + 4 + 32
    run_cases(eng, 0, cases)
    run_cases(eng, 0, cases[::-1])


# ---- 4. table shapes
def test_table_shapes(eng):
    cases = F.table_shapes()
    names = {c.name for c in cases}
    for must in ("lengths_up_to_15", "single_literal_plus_eob", "one_distance_code_of_length_1", "hlit286_hdist30_hclen5",
                 "hlit286_hdist30_hclen19", "hclen4_all_zero", "run_across_hlit_16", "run_across_hlit_17", "run_across_hlit_18",
                 "stored_65535", "stored_empty", "last_bit_at_7", "last_bit_at_0"):
        assert must in names
    run_cases(eng, 0, cases)
    # the two last-bit streams as the LAST entry of the buffer: the device buffer ends with their last byte
    for c in cases:
        if c.name.startswith("last_bit_at_"):
            run_cases(eng, 0, [cases[0], c])


# ---- 5. containers
@pytest.mark.parametrize("kind", (1, 2))
def test_containers(eng, kind):
    cases = [c for c in F.containers() if c.kind == kind]
    assert len(cases) >= 19 and any(c.verdict != OK for c in cases)
    run_cases(eng, kind, cases)
    st = eng.deflate_decode_batch_stats()
    assert st[0] == sum(c.verdict == OK for c in cases) and st[0] + st[1] == len(cases)


# ---- 6. malformed entries between good ones
def test_malformed_entries_do_not_touch_their_neighbours(eng, oracle):
    text = words(6, 30000)
    z = zlib.compress(text, 6)
    good = [(zlib.compress(words(i, 50 + 777 * i), 1 + i % 9), words(i, 50 + 777 * i)) for i in range(7)]
    bad = []
    for c in F.malformed_cases():
        if c.kind == F.RAW:      # behind a zlib header (and without a trailer) the fault and the bytes in front of it are the same
            bad.append((b"\x78\x9c" + c.stream, c.data, c.verdict))
        elif c.kind == F.ZLIB:
            bad.append((c.stream, c.data, c.verdict))
    n_forged = len(bad)
    assert n_forged >= 30             # every raw Deflate class of the contract, and the zlib container classes
    for cut in F.cut_points(len(z)):
        d = zlib.decompressobj(15)
        bad.append((z[:cut], d.decompress(z[:cut]), E_EOF))
    assert len(bad) == n_forged + 160
    quirk = oracle.deflate_encode(QUIRK, 1)
    entries, want = [], []
    for i, (s, data, v) in enumerate(bad):
        entries += [s, good[i % 7][0]]
        want += [(data, v), (good[i % 7][1], OK)]
    entries += [quirk, good[0][0]]
    got = Pack(entries).decode(eng, 1)
    assert got[-1] == (good[0][1], OK)
    assert got[-2][1] in (E_DATA, E_EOF)                      # the reference's match-free dynamic block: malformed
    for i, (g, w) in enumerate(zip(got[:-2], want)):
        assert g[1] == w[1], "entry %d: verdict %d, expected %d" % (i, g[1], w[1])
        if i % 2 == 0 and i // 2 >= n_forged:                 # a cut: a prefix of the data; nothing for a cut in the header
            assert text.startswith(g[0])
            if len(entries[i]) < 2:
                assert g[0] == b""
        assert g[0] == w[0], "entry %d: %d bytes, expected %d" % (i, len(g[0]), len(w[0]))
    st = eng.deflate_decode_batch_stats()
    assert st[0] == len(bad) + 1 and st[1] == len(bad) + 1


@pytest.mark.parametrize("kind", (0, 2))
def test_malformed_raw_and_gzip(eng, kind):
    cases = [c for c in F.malformed_cases() if c.kind == kind]
    fine = [c for c in F.clean_cases() if c.kind == kind]
    assert len(fine) >= 8
    mixed = [c for i, bad in enumerate(cases) for c in (bad, fine[i % len(fine)])]   # every bad entry in front of a good one
    assert len(mixed) == 2 * len(cases) >= 12
    run_cases(eng, kind, mixed)


# ---- 7. the device chain: encoder -> decoder -> encoder
@pytest.mark.parametrize("count,kind", [(1, 0), (2, 1), (1000, 2)])
def test_device_chain(eng, pkg, oracle, count, kind):
    import torch
    r = random.Random(count)
    base = words(count, 70000)
    lens = [70000] if count == 1 else [0, 65536] if count == 2 else \
        [r.choice((0, 1, 5, 300, 2000, 4096, 9000)) for _ in range(count - 3)] + [70000, 65535, 65537]
    r.shuffle(lens)
    ins = [base[:n] if i % 2 else rnd_bytes(i, n) if n < 3000 else base[-n:] for i, n in enumerate(lens)]
    assert sum(lens) < 4 << 20 and max(lens) >= 65536
    for x in set(ins):  # as in test 1: none of them may be the reference's match-free dynamic block
        e = oracle.DeflateEncoder()
        e.feed(x, oracle.ACTION_FINISH)
        assert not any(btype == 2 and tokens >= nbytes for tokens, nbytes, btype, _ in e.blocks())
    d = Dev(ins)
    o_off, o_len = eng.deflate_encode_batch_device(kind, d.t.data_ptr(), d.off, d.len, d.o.data_ptr(), d.cap)
    torch.cuda.synchronize()
    first = d.o.cpu().numpy().tobytes()
    streams = [first[a:a + n] for a, n in zip(o_off, o_len)]
    # the encoder's (d_out, offsets, lengths) go in unchanged
    s_off, s_len, s_ver = eng.deflate_decode_batch_device(kind, d.o.data_ptr(), o_off, o_len, None, 0)
    cap = max(a + n for a, n in zip(s_off, s_len))
    back = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    b_off, b_len, ver = eng.deflate_decode_batch_device(kind, d.o.data_ptr(), o_off, o_len, back.data_ptr(), cap)
    torch.cuda.synchronize()
    assert ver == [OK] * count and b_len == lens and (b_off, b_len) == (s_off, s_len)
    host = back.cpu().numpy().tobytes()
    assert [host[a:a + n] for a, n in zip(b_off, b_len)] == ins
    # ... and the decoder's go back into the encoder
    again = torch.full((d.cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    a_off, a_len = eng.deflate_encode_batch_device(kind, back.data_ptr(), b_off, b_len, again.data_ptr(), d.cap)
    torch.cuda.synchronize()
    second = again.cpu().numpy().tobytes()
    assert (a_off, a_len) == (o_off, o_len)
    assert [second[a:a + n] for a, n in zip(a_off, a_len)] == streams


# ---- 8. sizes only, capacity, host forms, classes
def test_sizes_only_and_capacity(eng, pkg):
    cases = [c for c in F.containers() if c.kind == 2]
    p = Pack([c.stream for c in cases])
    got = p.decode(eng, 2)
    s_off, s_len, s_ver = p.sizes(eng, 2)
    assert eng.deflate_decode_batch_stats()[7] == 1
    for c, g, v in zip(cases, got, s_ver):
        trailer = c.name.startswith(("gzip_crc_bit", "gzip_isize"))
        assert v == (OK if trailer else g[1])                 # the sizes-only call does not look at CRC-32 and ISIZE
        assert g[1] == c.verdict and (not trailer or g[0] == c.data)
    need = max(a + n for a, n in zip(s_off, s_len))
    assert p.decode(eng, 2, cap=need) == got
    with pytest.raises(pkg.CompressionError) as ei:
        p.decode(eng, 2, cap=need - 1)
    assert ei.value.code == pkg.BZ_E_CAPACITY
    assert p.host == bytes([FILL]) * len(p.host)              # the output's fill is untouched
    # parameter errors of the device form
    o = p.torch.zeros(need + 64, dtype=p.torch.uint8, device="cuda")
    call = lambda kind, ptr, off, ln, optr=None: eng.deflate_decode_batch_device(kind, ptr, off, ln, o.data_ptr() if optr is None else optr, need)
    for args in ((3, p.t.data_ptr(), p.off, p.len), (-1, p.t.data_ptr(), p.off, p.len),
                 (2, p.t.data_ptr() + 4, p.off, p.len),                               # d_in misaligned
                 (2, p.t.data_ptr(), [p.off[0], p.off[1] + 2] + p.off[2:], p.len),    # an offset that is no multiple of 4
                 (2, p.t.data_ptr(), [p.off[1], p.off[0]] + p.off[2:], p.len),        # out of order
                 (2, p.t.data_ptr(), [p.off[0], p.off[0] + 4] + p.off[2:], p.len),    # overlap
                 (2, p.t.data_ptr(), p.off, p.len, o.data_ptr() + 8)):                # d_out misaligned
        with pytest.raises(pkg.CompressionError) as ei:
            call(*args)
        assert ei.value.code == pkg.BZ_E_PARAM
    assert eng.deflate_decode_batch_device(2, p.t.data_ptr(), [], [], o.data_ptr(), need) == ([], [], [])   # count == 0


def test_host_forms_equal_the_device_form(eng, pkg):
    for kind in KINDS:
        cases = [c for c in F.clean_cases() + F.malformed_cases() if c.kind == kind][:60]
        dev = Pack([c.stream for c in cases]).decode(eng, kind)
        assert pkg.deflate_decompress_batch([c.stream for c in cases], kind) == dev
        assert pkg.deflate_decompress_batch([c.stream for c in cases], kind) == dev    # the cached engine
        for c, g in list(zip(cases, dev))[::7]:
            assert pkg.deflate_decompress(c.stream, kind) == g == (c.data, c.verdict)


def test_python_classes(pkg):
    data = words(12, 5000)
    for cls, kind, wbits in ((pkg.Deflater, 0, -15), (pkg.ZlibDecoder, 1, 15), (pkg.GZipDecoder, 2, 31)):
        c = zlib.compressobj(6, zlib.DEFLATED, wbits)
        z = c.compress(data) + c.flush()
        assert cls().decode_all(z) == data
        assert bytes(pkg.decode(z, cls())) == data
        with pytest.raises(pkg.CompressionError) as ei:
            cls().decode_all(z[:len(z) // 2])
        assert ei.value.kind == "UnexpectedEof" and 0 < len(ei.value.partial) < len(data) and data.startswith(ei.value.partial)
        if kind == 0:
            continue
        broken = bytearray(z)
        broken[-1] ^= 0x40                                    # the trailer's last byte
        dec, got, it = cls(), bytearray(), iter(bytes(broken))
        with pytest.raises(pkg.CompressionError) as ei:
            while True:
                b = dec.next(it)
                assert b is not None
                got.append(b)
        assert ei.value.kind == "DataError" and ei.value.partial == data == bytes(got)   # all bytes were yielded first
        assert dec.next(it) is None
