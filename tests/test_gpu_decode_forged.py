"""GPU decode of forged streams (run with -m gpu on an MI355X): streams no encoder writes -- long, incomplete,
over-subscribed and zero-length codes, EOB cut inside its code, selectors that change table every group, zero runs
at the edges of a block and of the 512-symbol chunks, last columns that are not a BWT (cycles of unequal length,
randomised), header edges, and mixtures -- through bz_decode_buffer, the streaming bz_dec_* context and
bz_gpu_decode_device, each against the oracle's restatement of src/bzip2/decoder.rs: same bytes, same verdict.

Families h and i feed the last stage (the RLE1 undo and the block CRC, D4 of k_dec.hip) block images chosen byte by
byte -- run groups at chosen phases against its sub-tile, wave, workgroup and thread-share edges, waves on both sides
of the staging threshold at every dword phase, every (address, end) pair mod 16 of the CRC's pieces and its tile and
slice seams -- with the expected bytes from the forge's plain undo, also at every phase of the caller's pointer and
as entries of one batch call.

The streams come from tests/bzforge.py (the same cases tests/test_bzforge.py pins on the CPU).  Where the reference
panics on a malformed table (an over-subscribed one; a code hole hit: unreachable!()), the oracle's documented
deviation reports DataError, and so must the GPU."""
import random

import numpy as np
import pytest

import bzforge

pytestmark = pytest.mark.gpu

_CASES = {}


def cases(oracle, fam):
    if fam not in _CASES:
        _CASES[fam] = bzforge.all_cases(oracle, fam)
    return _CASES[fam]


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.GpuEngine(0, 16)
    yield e
    e.close()


def _streaming(pkg, z, seed):
    """BZip2Decoder fed in seeded uneven pieces -> (bytes, status)"""
    rng = random.Random(seed)
    dec = pkg.BZip2Decoder()
    got = bytearray()
    try:
        pos = 0
        while pos < len(z):
            step = rng.choice([1, 3, 97, 1000, 4096, 30000, 250000])
            dec.write(z[pos:pos + step])
            pos += step
            got += dec.read_available()
        got += dec.decode_all(b"")
    except pkg.BZip2Error as e:
        return bytes(got + e.partial), e.code
    return bytes(got), 0


def _device(eng, z, want_len):
    import torch
    tin = torch.frombuffer(bytearray(z) + bytearray(64), dtype=torch.uint8).cuda()
    size, _ = eng.decode_device(tin.data_ptr(), len(z), None, 0)
    cap = max(size, want_len)
    tout = torch.empty(cap + 64, dtype=torch.uint8, device="cuda")
    n, st = eng.decode_device(tin.data_ptr(), len(z), tout.data_ptr(), cap)
    return bytes(tout[:n].cpu().numpy()), st


def check(pkg, oracle, eng, c, monkeypatch, seed):
    if c.no_oracle:  # a block that ends behind four equal bytes: the oracle has no answer (status -100 at any cap),
        want = (c.data, c.status)  # the case carries the library's documented one
    else:
        want = oracle.decode(c.z, c.cap) if c.cap else oracle.decode(c.z)
        assert want[1] == c.status, (c.name, want[1])
        if c.data is not None:
            assert want[0] == c.data, c.name
    got = pkg.decompress(c.z)
    assert (got[1], len(got[0])) == (want[1], len(want[0])), ("decompress", c.name)
    assert got[0] == want[0], ("decompress", c.name)
    monkeypatch.setenv("BZ_DEC_CHUNK", "20000")  # blocks cross chunks
    got = _streaming(pkg, c.z, seed)
    monkeypatch.delenv("BZ_DEC_CHUNK")
    assert (got[1], len(got[0])) == (want[1], len(want[0])), ("BZip2Decoder", c.name)
    assert got[0] == want[0], ("BZip2Decoder", c.name)
    got = _device(eng, c.z, len(want[0]))
    assert (got[1], len(got[0])) == (want[1], len(want[0])), ("decode_device", c.name)
    assert got[0] == want[0], ("decode_device", c.name)
    if c.multi:
        monkeypatch.setenv("BZ_DEC_BATCH", "1")
        got = pkg.decompress(c.z)
        monkeypatch.delenv("BZ_DEC_BATCH")
        assert got == want, ("decompress, BZ_DEC_BATCH=1", c.name)


def _run(pkg, oracle, eng, monkeypatch, fam, only=None):
    cs = [c for c in cases(oracle, fam) if only is None or only(c)]
    assert cs
    for i, c in enumerate(cs):
        check(pkg, oracle, eng, c, monkeypatch, 1000 * ord(fam) + i)


def test_a_long_and_odd_codes(pkg, oracle, eng, monkeypatch):
    """codes of 11-21 bits used densely (one block of 120 000 symbols), lengths 0 and 21 from the delta coding,
    an incomplete code on its owned codewords and on its hole, over-subscribed tables used and unpicked"""
    _run(pkg, oracle, eng, monkeypatch, "a")


def test_b_truncation_inside_eob(pkg, oracle, eng, monkeypatch):
    """EOB codes of 9-20 bits at every bit alignment, cut at every byte inside the code; up to 12 bits the
    zero-padded peek still finds EOB (the block's bytes, then DataError), from 13 bits on the block fails"""
    _run(pkg, oracle, eng, monkeypatch, "b")


def test_c_selectors_and_groups(pkg, oracle, eng, monkeypatch):
    _run(pkg, oracle, eng, monkeypatch, "c")


def test_d_zero_runs(pkg, oracle, eng, monkeypatch):
    _run(pkg, oracle, eng, monkeypatch, "d")


def test_e_last_columns_that_are_not_a_bwt(pkg, oracle, eng, monkeypatch):
    """fixed points, 2-cycles, n/2 cycles, a long cycle with stretches of 56 000 and 70 000 slots between sample
    slots, mixed cycle lengths, each also randomised"""
    _run(pkg, oracle, eng, monkeypatch, "e")


def test_f_header_edges(pkg, oracle, eng, monkeypatch):
    _run(pkg, oracle, eng, monkeypatch, "f")


def test_g_mixtures(pkg, oracle, eng, monkeypatch):
    _run(pkg, oracle, eng, monkeypatch, "g")


LARGEST = "H-ff-899981"


def test_h_rle1_undo(pkg, oracle, eng, monkeypatch):
    """run groups at every phase against sub-tile, wave, workgroup and thread-share (K = 2, 14) edges, counts
    0..255 and equal to the run byte, self-similar images, image ends, waves at the staging threshold at every
    dword phase, staged beside direct waves, and blocks that end behind four equal bytes (DataError, the blocks in
    front intact): the bytes of bzforge.rle1_undo"""
    _run(pkg, oracle, eng, monkeypatch, "h", lambda c: c.name != LARGEST)


def test_h_rle1_undo_largest_block(pkg, oracle, eng, monkeypatch):
    """899 981 bytes of ff: fourteen sub-tiles per chain thread, every wave direct, 46.6 MB"""
    _run(pkg, oracle, eng, monkeypatch, "h", lambda c: c.name == LARGEST)


def test_i_block_crc(pkg, oracle, eng, monkeypatch):
    """all 256 (first byte, end) pairs mod 16, 1..8193 pieces with a full and a ragged last one at alignments 0, 1
    and 15, and a wrong stored CRC at one piece, a ragged tile seam and a slice seam"""
    _run(pkg, oracle, eng, monkeypatch, "i")


GUARD = 64
STAGE_TARGETS = ("H stage", "H seam", "H total<4", "H one-dword")


def test_output_pointer_phase(pkg, oracle, eng):
    """the multi-block streams of both families through decode_device with the output at base + k, k = 0..15: the
    same bytes, and 64 bytes on each side untouched (a flush that writes a dword too far shows there).  The dword
    phase of every wave and the piece alignment of every block move with k; the targets are recomputed for the k
    used."""
    import torch
    multi = [c for fam in "hi" for c in cases(oracle, fam) if c.multi]
    assert len(multi) >= 15
    seen = {k: set() for k in range(16)}
    for c in multi:
        tin = torch.frombuffer(bytearray(c.z) + bytearray(64), dtype=torch.uint8).cuda()
        n = len(c.data)
        size, _ = eng.decode_device(tin.data_ptr(), len(c.z), None, 0)
        cap = max(size, n)
        buf = torch.empty(GUARD + 16 + cap + GUARD, dtype=torch.uint8, device="cuda")
        base = buf.data_ptr()
        assert base % 16 == 0
        targets = c.name.startswith(("H-staging", "I-grid", "I-pieces"))
        for k in range(16):
            buf.fill_(0xEE)
            got_n, st = eng.decode_device(tin.data_ptr(), len(c.z), base + GUARD + k, cap)
            assert (got_n, st) == (n, c.status), (c.name, k)
            host = buf.cpu().numpy()
            assert host[GUARD + k:GUARD + k + n].tobytes() == c.data, (c.name, k)
            assert host[:GUARD + k].tobytes() == b"\xee" * (GUARD + k), (c.name, k, "bytes in front")
            if cap == n:
                assert host[GUARD + k + n:].tobytes() == b"\xee" * (len(host) - GUARD - k - n), (c.name, k, "bytes behind")
            assert host[GUARD + k + cap:].tobytes() == b"\xee" * (len(host) - GUARD - k - cap), (c.name, k, "behind cap")
            if targets:
                seen[k] |= bzforge.hits(c, k)
    grid = {t for t in bzforge.REQUIRED["i"] if t.startswith("I a=")}
    stage = {t for t in bzforge.REQUIRED["h"] if t.startswith(STAGE_TARGETS)}
    for k in range(16):
        assert grid <= seen[k], (k, sorted(grid - seen[k]))
    for k0 in range(0, 16, 4):  # the dword phase has period 4: any four pointers in a row reach every target
        got = set().union(*(seen[k] for k in range(k0, k0 + 4)))
        assert stage <= got, (k0, sorted(stage - got))


def test_batch_entries(pkg, oracle):
    """the small cases of both families as entries of one decompress_batch call, in seeded order, with empty and
    wrong-CRC entries between them: every entry gets its own bytes and verdict"""
    small = [c for fam in "hi" for c in cases(oracle, fam) if len(c.data) <= 300000 and len(c.z) <= 150000]
    assert len(small) >= 12 and any(c.no_oracle for c in small) and any(c.flips for c in small)
    ents = [(c.z, (c.data, c.status)) for c in small]
    good = next(c for c in small if c.name == "H-counts")
    bad = bytearray(good.z)
    bad[10 + 3] ^= 0x10  # the block CRC (behind "BZh9" and the 48-bit magic)
    ents += [(b"", (b"", -4)), (bytes(bad), (good.data, bzforge.E_DATA)), (b"", (b"", -4)), (good.z, (good.data, 0))]
    random.Random(4711).shuffle(ents)
    got = pkg.decompress_batch([z for z, _ in ents])
    assert len(got) == len(ents)
    for i, (g, (_, w)) in enumerate(zip(got, ents)):
        assert (g[1], len(g[0])) == (w[1], len(w[0])), i
        assert g[0] == w[0], i
