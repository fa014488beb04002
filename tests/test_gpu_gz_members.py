"""GPU tests of "every member of a gzip file" (include/bz2_mi355x.h section 6, DESIGN_deflate.md "Every member of a gzip
file"): df_gpu_decode_members_device, df_decode_members_buffer, MultiGZipDecoder.

Expected values come from serial() below: the contract's loop, with zlib.decompressobj(31) per member, `unused_data` for the
member's end, lstrip(b"\\0") for the padding and `eof` false meaning BZ_E_EOF.  Where zlib raises it cannot say which bytes
lay in front of the fault, so the test names them: `forged` maps a member's position to its (bytes, verdict) -- a dfforge
Case, or a member whose trailer the test spoilt.  A position zlib raises at without such an entry is junk: no bytes,
BZ_E_DATA.  serial() never calls the library.

Members are built by hand (dfforge.gzip_wrap around zlib's raw stream); an FNAME of chosen length sets a member's length
to the byte.  Every file goes through the sizes-only call too, and the output buffer is filled with 0xEE: nothing at or
behind out_len may change."""
import random
import struct
import zlib

import pytest

import dfforge as F
from conftest import product
from test_gpu_deflate_batch import words

pytestmark = pytest.mark.gpu

OK, E_DATA, E_EOF = 0, -1, -2
FILL = 0xEE
HEAD = bytes([0x1F, 0x8B, 8])


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def serial(data, forged=None):
    out, pos = b"", 0
    while True:
        pos = len(data) - len(data[pos:].lstrip(b"\0"))
        if pos == len(data):
            return out, OK
        if forged and pos in forged:
            return out + forged[pos][0], forged[pos][1]
        d = zlib.decompressobj(31)
        try:
            out += d.decompress(data[pos:])
        except zlib.error:
            return out, E_DATA
        if not d.eof:
            return out, E_EOF
        pos = len(data) - len(d.unused_data)


def raw_of(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def member(data, level=6, **kw):
    return F.gzip_wrap(raw_of(data, level), data, **kw)


def member_of_length(data, total):
    """a member of exactly `total` bytes: an FNAME pads it"""
    base = len(member(data, name=b""))
    assert total >= base, (total, base)
    m = member(data, name=b"n" * (total - base))
    assert len(m) == total
    return m


def candidates(buf):
    return [p for p in range(len(buf) - 3) if buf[p:p + 3] == HEAD and not buf[p + 3] & 0xE0]


def decode(eng, data, want=None, trailer_fault=False):
    """the file through the sizes-only call and the real one; returns (bytes, verdict) and checks the fill behind them"""
    import torch
    t = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()   # (ends with the file's last byte)
    need, v0 = eng.gzip_decode_members_device(t.data_ptr(), len(data), None, 0)
    o = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda")
    n, v = eng.gzip_decode_members_device(t.data_ptr(), len(data), o.data_ptr(), need)
    torch.cuda.synchronize()
    host = o.cpu().numpy().tobytes()
    assert host[n:] == bytes([FILL]) * (need + 64 - n), "bytes at or behind out_len were written"
    if trailer_fault:        # (the sizes-only call does not look at trailers)
        assert n <= need and v0 in (OK, v)
    else:
        assert (need, v0) == (n, v), "sizes only: %r, the real call: %r" % ((need, v0), (n, v))
    got = host[:n], v
    if want is not None:
        assert got[1] == want[1], "verdict %d, expected %d" % (got[1], want[1])
        assert got[0] == want[0], "%d bytes, expected %d (first difference at %d)" % (
            len(got[0]), len(want[0]), next((k for k, (a, b) in enumerate(zip(got[0], want[0])) if a != b), -1))
    return got


TEXT = words(11, 40000)


def small(i, n=None):
    n = 50 + 37 * i if n is None else n
    return TEXT[100 * i:100 * i + n]


# ---- 1. shapes
def test_one_member_equals_the_one_member_decoder(eng, pkg):
    m = member(TEXT)
    got = decode(eng, m, (TEXT, OK))
    assert got == pkg.deflate_decompress(m, kind=2)
    st = eng.gzip_decode_members_stats()
    assert st[:4] == [1, 1, 0, 0] and st[6] == 1


def test_two_and_three_members(eng):
    a, b, c = small(1), small(2), small(3)
    f = member(a) + member(b, level=1)
    decode(eng, f, serial(f))
    assert serial(f) == (a + b, OK)
    f = member(a) + member(b"") + member(c, level=9)          # an empty one in the middle
    decode(eng, f, (a + c, OK))
    assert serial(f) == (a + c, OK)
    assert eng.gzip_decode_members_stats()[0] == 3


def bgzf_block(data):
    """a BGZF block: FEXTRA with the subfield B C, 2, BSIZE = block length - 1"""
    raw = raw_of(data)
    bsize = 12 + 6 + len(raw) + 8 - 1
    m = F.gzip_wrap(raw, data, extra=b"BC" + struct.pack("<HH", 2, bsize))
    assert len(m) == bsize + 1
    return m


def test_bgzf_file(eng):
    r = random.Random(5)
    parts = [TEXT[a:a + r.randint(0, 3000)] for a in (r.randint(0, 36000) for _ in range(1000))]
    f = b"".join(bgzf_block(p) for p in parts) + bgzf_block(b"")
    assert len(bgzf_block(b"")) == 28
    assert len(candidates(f)) == 1001
    decode(eng, f, (b"".join(parts), OK))
    st = eng.gzip_decode_members_stats()
    assert st[0] == 1001 and st[1] == 1001 and st[2] == 0 and st[3] == 0
    assert serial(f) == (b"".join(parts), OK)


def test_all_optional_header_fields(eng):
    kw = dict(extra=b"XY\x03\x00abc", name=b"file.txt", comment=b"a comment", hcrc=True, text=True)
    f = member(small(1), **kw) + member(small(2), **kw) + member(small(3))
    decode(eng, f, serial(f))
    assert serial(f) == (small(1) + small(2) + small(3), OK)


# ---- 2. where a start can hide
@pytest.mark.parametrize("edge", (64, 256, 1024, 4096, 65536))
def test_member_start_around_a_tile_or_wave_edge(eng, edge):
    second = member(small(4))
    for d in range(-4, 5):
        f = member_of_length(small(5, 20), edge + d) + second
        assert candidates(f) == [0, edge + d]
        decode(eng, f, (small(5, 20) + small(4), OK))
        assert eng.gzip_decode_members_stats()[:3] == [2, 2, 0]


def test_member_starts_at_every_residue_and_ends(eng):
    for r in range(4):
        first = member_of_length(small(6, 30), 80 + r)
        f = first + member(small(7)) + member(small(8))
        assert candidates(f)[1] % 4 == r
        decode(eng, f, (small(6, 30) + small(7) + small(8), OK))
    f = member(small(1)) + member(small(2))                     # the last member ends with the input's last byte
    decode(eng, f, (small(1) + small(2), OK))
    for k in range(1, 6):                                      # ... and is followed by 1..5 bytes: no header fits, or none is there
        g = f + b"\x1f\x8b\x08\x00\x00"[:k]
        decode(eng, g, serial(g))
        assert serial(g) == (small(1) + small(2), E_EOF)
        g = f + b"\xAB" * k
        decode(eng, g, (small(1) + small(2), E_DATA))


# ---- 3. zero padding
ZEROS = (1, 2, 3, 4, 5, 511, 10240)


def test_zero_padding(eng):
    a, b = member(small(1)), member(small(2))
    want = (small(1) + small(2), OK)
    for z in ZEROS:
        f = a + bytes(z) + b
        assert serial(f) == want
        decode(eng, f, want)
        assert eng.gzip_decode_members_stats()[4] == z
        f = a + b + bytes(z)
        decode(eng, f, want)
        assert eng.gzip_decode_members_stats()[4] == z
    f = bytes(7) + a + bytes(3) + b + bytes(9)
    decode(eng, f, want)
    assert eng.gzip_decode_members_stats()[4] == 19


def test_zeros_only_and_no_bytes(eng):
    for z in (1, 4, 63, 64, 65, 5000):
        decode(eng, bytes(z), (b"", OK))
        assert eng.gzip_decode_members_stats()[:2] == [0, 0]
    decode(eng, b"", (b"", OK))


# ---- 4. false candidates
def nested(k):
    """a stored-block member that holds k whole gzip members and three more bytes"""
    payload = b"".join(member(small(10 + i, 40)) for i in range(k)) + b"abc"
    m = member(payload, level=0)
    assert len(candidates(m)) == 1 + k
    return payload, m


@pytest.mark.parametrize("k,redecodes", ((1, 1), (2, 2), (3, 2), (8, 4), (9, 4)))
def test_members_inside_a_stored_block(eng, k, redecodes):
    payload, m = nested(k)
    f = member(small(1)) + m + member(small(2))
    want = (small(1) + payload + small(2), OK)
    assert serial(f) == want
    decode(eng, f, want)
    st = eng.gzip_decode_members_stats()
    assert st[0] == 3 and st[1] == 3 + k and st[2] == k and st[3] == redecodes, st


def test_header_bytes_inside_a_stored_block(eng):
    payload = (HEAD + b"\x00") * 5
    f = member(small(1)) + member(payload, level=0) + member(small(2))
    decode(eng, f, (small(1) + payload + small(2), OK))
    st = eng.gzip_decode_members_stats()
    assert st[2] == 5 and st[3] == 3, st


def test_false_candidate_inside_the_last_member(eng):
    payload, m = nested(2)
    f = member(small(1)) + m
    decode(eng, f, (small(1) + payload, OK))
    st = eng.gzip_decode_members_stats()
    assert st[0] == 2 and st[2] == 2 and st[3] == 2, st
    g = f + bytes(5)
    decode(eng, g, (small(1) + payload, OK))


# ---- 5. faults
def test_file_cut_inside_the_second_member(eng):
    d2 = TEXT[:6000]
    m1, m2, m3 = member(small(1)), member(d2, name=b"second"), member(small(3))
    head, body = 10 + 7, len(m2) - 8
    cuts = list(range(1, head + 1)) + [head + (body - head) * i // 17 for i in range(1, 17)] + list(range(body, len(m2)))
    for cut in cuts:
        f = m1 + m2[:cut]
        want = serial(f)
        assert want[1] == E_EOF and want[0][:len(small(1))] == small(1)
        decode(eng, f, want)
    assert serial(m1 + m2[:len(m2) - 1])[0] == small(1) + d2


def test_wrong_trailer_in_the_second_member(eng):
    d2 = small(2, 700)
    m1, m3 = member(small(1)), member(small(3))
    for kw in (dict(crc=F.crc32(d2) ^ 1), dict(isize=len(d2) + 1)):
        m2 = member(d2, **kw)
        f = m1 + m2 + m3
        want = serial(f, {len(m1): (d2, E_DATA)})
        assert want == (small(1) + d2, E_DATA)
        decode(eng, f, want, trailer_fault=True)
        assert eng.gzip_decode_members_stats()[0] == 2           # (member 3 was found, and is not decoded)


def trailer_is_wrong(m):
    """the member's only fault is its CRC-32 or ISIZE (zlib says which check failed): the one fault the sizes-only call,
    which does not look at trailers, cannot see"""
    try:
        zlib.decompressobj(31).decompress(m)
    except zlib.error as e:
        return "incorrect data check" in str(e) or "incorrect length check" in str(e)
    return False


def test_forged_second_member(eng):
    m1, m3 = member(small(1)), member(small(3))
    cases = [c for c in F.malformed_cases() if c.kind != F.ZLIB]      # (a zlib container's faults have no gzip form)
    assert len(cases) >= 30 and {c.verdict for c in cases} == {E_DATA, E_EOF}
    for c in cases:
        if c.kind == F.GZIP:
            m2 = c.stream
        elif c.verdict == E_EOF:     # the stream ends in the fault: nothing may follow it, not even a trailer
            m2 = F.gzip_wrap(c.stream, c.data)[:-8]
        else:
            m2 = F.gzip_wrap(c.stream, c.data)
        f = m1 + m2 + (m3 if c.verdict != E_EOF else b"")
        if not m2:                   # (an empty forged entry: the file simply ends behind member 1)
            decode(eng, f, (small(1), OK))
            continue
        want = serial(f, {len(m1): (c.data, c.verdict)})
        assert want == (small(1) + c.data, c.verdict), c.name
        try:
            decode(eng, f, want, trailer_fault=trailer_is_wrong(m2))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (c.name, e))


def test_junk_and_reserved_flag(eng):
    ms = [member(small(i)) for i in (1, 2, 3)]
    all3 = small(1) + small(2) + small(3)
    f = b"".join(ms) + b"junk"
    assert serial(f) == (all3, E_DATA)
    decode(eng, f, (all3, E_DATA))
    f = ms[0] + ms[1] + member(small(3), reserved=0x20)
    assert serial(f) == (small(1) + small(2), E_DATA)
    decode(eng, f, (small(1) + small(2), E_DATA))


def test_truncated_member_in_front_of_an_intact_one(eng):
    """the serial definition: the decoder runs on into member 3's bytes -- here it takes them for member 2's trailer"""
    d2 = small(2, 900)
    m1, m2, m3 = member(small(1)), member(d2), member(small(3))
    for keep in (8, 4):
        f = m1 + m2[:len(m2) - keep] + m3
        want = serial(f, {len(m1): (d2, E_DATA)})
        assert want == (small(1) + d2, E_DATA)
        decode(eng, f, want, trailer_fault=True)


# ---- 6. a split member among small ones
def test_split_member_among_small_ones(eng, monkeypatch):
    big = words(21, 1200000)
    mb = member(big, level=1)
    assert len(mb) >= 200 * 1024
    left = [small(i) for i in range(10)]
    right = [small(20 + i) for i in range(10)]
    front = b"".join(member(x) for x in left)
    if len(front) % 2 == 0:
        front = member_of_length(left[0], len(member(left[0], name=b"")) + 1) + b"".join(member(x) for x in left[1:])
    assert len(front) % 2 == 1                                   # the large member starts at an odd byte
    f = front + mb + b"".join(member(x) for x in right)
    want = (b"".join(left) + big + b"".join(right), OK)
    monkeypatch.setenv("BZ_DF_INF_SPLIT_KIB", "128")
    decode(eng, f, want)
    st = eng.gzip_decode_members_stats()
    assert st[0] == 21 and st[5] == 1, st
    assert eng.deflate_decode_split_stats()[0] == 1


# ---- 7. sub-batches
def test_sub_batches(eng, monkeypatch):
    payload, m = nested(9)
    parts = [small(i % 40, 30 + i) for i in range(200)]
    f = b"".join(member(p) for p in parts[:100]) + m + bytes(3) + b"".join(member(p) for p in parts[100:])
    want = (b"".join(parts[:100]) + payload + b"".join(parts[100:]), OK)
    got = decode(eng, f, want)
    whole = eng.gzip_decode_members_stats()
    assert whole[6] == 1
    monkeypatch.setenv("BZ_DF_GZ_BATCH", "64")
    assert decode(eng, f, want) == got
    st = eng.gzip_decode_members_stats()
    assert st[6] > whole[6] and st[:5] == whole[:5], (st, whole)
    g = f[:-1]                                                   # ... and a fault in the last sub-batch
    assert decode(eng, g) == serial(g)


def test_false_candidates_across_a_sub_batch_edge(eng, monkeypatch):
    """the extension of a member reaches over the end of its sub-batch (candidates in another window of the list), and
    once over the end of the list"""
    monkeypatch.setenv("BZ_DF_GZ_BATCH", "64")
    payload, m = nested(9)
    parts = [small(i % 40, 30 + i) for i in range(150)]
    for at in (60, 63, 120):                                     # false candidates 61..69, 64..72, 121..129: edges at 64 and 128
        f = b"".join(member(p) for p in parts[:at]) + m + b"".join(member(p) for p in parts[at:])
        want = (b"".join(parts[:at]) + payload + b"".join(parts[at:]), OK)
        assert serial(f) == want
        decode(eng, f, want)
        st = eng.gzip_decode_members_stats()
        assert st[:4] == [151, 160, 9, 4] and st[6] >= 3, st
    f = b"".join(member(p) for p in parts[:62]) + m               # ... and the last extension reaches the input's end
    decode(eng, f, (b"".join(parts[:62]) + payload, OK))
    assert eng.gzip_decode_members_stats()[:4] == [63, 72, 9, 4]


# ---- 8. capacity and parameters
def test_parameter_errors_with_an_engine(eng, pkg):
    """every one returns before any launch: the output keeps its fill"""
    import ctypes as C
    import torch
    L = pkg.lib()
    f = member(small(1))
    t = torch.frombuffer(bytearray(f) + bytearray(16), dtype=torch.uint8).cuda()
    o = torch.full((1024,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n, v = C.c_uint64(77), C.c_int32(77)
    call = L.df_gpu_decode_members_device
    assert call(eng._h, t.data_ptr() + 1, len(f), o.data_ptr(), 1024, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM      # a misaligned d_in
    assert call(eng._h, t.data_ptr(), 1 << 32, o.data_ptr(), 1024, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM         # 4 GiB
    assert call(eng._h, None, len(f), o.data_ptr(), 1024, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM                  # bytes announced, no pointer
    assert call(eng._h, t.data_ptr(), len(f), o.data_ptr(), 1024, None, C.byref(v)) == pkg.BZ_E_PARAM
    assert call(eng._h, t.data_ptr(), len(f), o.data_ptr(), 1024, C.byref(n), None) == pkg.BZ_E_PARAM
    torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == bytes([FILL]) * 1024
    assert call(eng._h, t.data_ptr(), len(f), o.data_ptr(), 1024, C.byref(n), C.byref(v)) == pkg.BZ_OK
    assert (n.value, v.value) == (len(small(1)), OK)


# ---- 8b. capacity
def test_capacity(eng, pkg):
    import torch
    f = member(small(1)) + member(small(2)) + member(small(3))
    t = torch.frombuffer(bytearray(f), dtype=torch.uint8).cuda()
    need, v = eng.gzip_decode_members_device(t.data_ptr(), len(f), None, 0)
    assert (need, v) == (len(small(1) + small(2) + small(3)), OK)
    o = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda")
    with pytest.raises(pkg.CompressionError) as ei:
        eng.gzip_decode_members_device(t.data_ptr(), len(f), o.data_ptr(), need - 1)
    assert ei.value.kind == "Capacity"
    torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == bytes([FILL]) * (need + 64)
    assert eng.gzip_decode_members_device(t.data_ptr(), len(f), o.data_ptr(), need) == (need, OK)
    torch.cuda.synchronize()
    assert o.cpu().numpy().tobytes() == small(1) + small(2) + small(3) + bytes([FILL]) * 64


# ---- 9. host forms and classes
def test_host_forms_and_classes(eng, pkg):
    payload, m = nested(3)
    f = member(small(1)) + bytes(6) + m + member(b"") + member(small(2))
    want = (small(1) + payload + small(2), OK)
    assert decode(eng, f, want) == pkg.gzip_decompress_members(f) == want
    assert pkg.MultiGZipDecoder().decode_all(f) == want[0]
    d = pkg.MultiGZipDecoder()
    it = iter(f)
    assert bytes(iter(lambda: d.next(it), None)) == want[0]
    bad = f + b"junk"
    assert pkg.gzip_decompress_members(bad) == (want[0], E_DATA)
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.MultiGZipDecoder().decode_all(bad)
    assert ei.value.kind == "DataError" and ei.value.partial == want[0]
    cut = f[:-3]
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.MultiGZipDecoder().decode_all(cut)
    assert ei.value.kind == "UnexpectedEof" and ei.value.partial == serial(cut)[0]
    # the one-member decoder is what it was: the first member, whatever follows
    assert pkg.GZipDecoder().decode_all(f) == small(1)
    assert pkg.deflate_decompress(f, kind=2) == (small(1), OK)
