"""GPU decode of forged streams (run with -m gpu on an MI355X): streams no encoder writes -- long, incomplete,
over-subscribed and zero-length codes, EOB cut inside its code, selectors that change table every group, zero runs
at the edges of a block and of the 512-symbol chunks, last columns that are not a BWT (cycles of unequal length,
randomised), header edges, and mixtures -- through bz_decode_buffer, the streaming bz_dec_* context and
bz_gpu_decode_device, each against the oracle's restatement of src/bzip2/decoder.rs: same bytes, same verdict.

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


def _run(pkg, oracle, eng, monkeypatch, fam):
    cs = cases(oracle, fam)
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
