"""GPU tests of the RLE1 front end in one pass (k_rle_onepass, csrc/k_rle1.hip) at the sizes where it branches: tiles
of 4096 bytes, spans of eight tiles (32 768 bytes, one workgroup), segments of 16 bytes (one lane), sub-tiles of 256.
Level 1 (blocks of 99 981 image bytes), so that a few hundred KB hold several cuts.  Every case: the oracle's stream
byte for byte, the stream of the three-kernel front end (BZ_RLE_ONEPASS=0, a switch read once per process: a child
process), and the kernel profile says which form wrote the image.  BZ_RLE_ONEPASS_FAILTEST=1 (another child) makes
the host discard the one pass and redo the split with the three kernels: the same streams."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT, product

pytestmark = pytest.mark.gpu

SEG, SUB, TILE, SPAN = 16, 256, 4096, 32768
LEVEL = 1
LIMIT = 100000 * LEVEL - 19
RUN_LENGTHS = (3, 4, 5, 6, 254, 255, 256, 258, 259, 260, 510, 511, 769)
TEXT_LENGTHS = (1, 15, 16, 17, 255, 256, 4095, 4096, 4097, 32767, 32768, 32769, 65541)


def text(seed, n):
    """n bytes below 199, no two neighbours equal: RLE1 leaves them alone"""
    rng = np.random.default_rng(seed)
    return bytearray((np.cumsum(rng.integers(1, 199, size=n, dtype=np.int64)) % 199).astype(np.uint8).tobytes())


def put(buf, start, length, byte=0xFA):
    """a run of `length` bytes `byte` (>= 199: none of the text's) from `start`; the runs of a case never touch"""
    assert 0 <= start and start + length <= len(buf)
    assert all(b < 199 for b in buf[max(0, start - 1):start + length + 1]), "runs touch"
    buf[start:start + length] = bytes([byte]) * length
    return buf


def runs_at_edges(r):
    """a run of r bytes whose fourth byte falls one before, on and one behind a segment edge, a tile edge and a span
    edge (edge = first byte of the next unit; three edges of each kind, one per placement)"""
    buf = text(r, 4 * SPAN + 1000)
    edges = [5 * SEG + 7 * TILE + k * 2 * TILE for k in range(3)]   # segment edges that are no sub-tile edge
    edges += [TILE * t for t in (1, 3, 5)]                          # tile edges inside span 0
    edges += [SPAN * s for s in (1, 2, 3)]
    for i, e in enumerate(edges):
        put(buf, e + (i % 3 - 1) - 3, r)
    return bytes(buf)


def four_split(before, edge):
    """four equal bytes, `before` of them in front of the edge"""
    return bytes(put(text(before + edge, 2 * SPAN + 77), edge - before, 4))


def ends(kind):
    buf = text(11, 2 * SPAN + 1003)  # (1003: not a multiple of 16)
    n = len(buf)
    for r, t in ((5, 0), (300, 1)):  # a short run and one with a count above 251 - 4, at two edges of the kind
        if kind == "tile_end":
            put(buf, TILE * (2 + 3 * t) - r, r)
        elif kind == "span_end":
            put(buf, SPAN * (1 + t) - r, r)
        elif kind == "input_end":
            if t == 0:
                put(buf, n - r, r)
        elif kind == "tile_last_byte":
            put(buf, TILE * (2 + 3 * t) - 1, r)
    return bytes(buf)


def long_run(r):
    return b"\xfb" * r + bytes(text(r, 50000))


def alternating_tiles():
    """three spans whose tiles are in turn run-free and packed with runs of 4 to 6 bytes"""
    buf = text(5, 3 * SPAN)
    for t in range(1, 3 * SPAN // TILE, 2):
        p, k = t * TILE, 0
        while p + 6 <= (t + 1) * TILE:
            r = 4 + k % 3
            buf[p:p + r] = bytes([0xC8 + k % 2]) * r
            p += r
            k += 1
    return bytes(buf)


def cut_near_span_edge(delta):
    """the first block's cut at input byte 3 * SPAN + delta: k runs of four bytes (five in the image) in front of it
    put the image LIMIT bytes ahead of the input by exactly the distance to the span's edge"""
    k = LIMIT - (3 * SPAN + delta)
    buf = text(delta + 9, 4 * SPAN)
    for i in range(k):
        buf[100 + 4 * i:104 + 4 * i] = bytes([0xF0 + i % 2]) * 4
    assert 100 + 4 * k < 3 * SPAN - 100
    return bytes(buf)


def cases():
    c = {}
    for n in TEXT_LENGTHS:
        c["text_%d" % n] = lambda n=n: bytes(text(n, n))
    for r in RUN_LENGTHS:
        c["run_%d_at_edges" % r] = lambda r=r: runs_at_edges(r)
    for name, edge in (("tile", 3 * TILE), ("span", SPAN)):
        for before in (3, 2, 1):
            c["four_%d_%d_across_%s" % (before, 4 - before, name)] = lambda b=before, e=edge: four_split(b, e)
    for kind in ("tile_end", "span_end", "input_end", "tile_last_byte"):
        c["run_%s" % kind] = lambda k=kind: ends(k)
    for r in (10000, 40000, 70000):
        c["long_run_%d" % r] = lambda r=r: long_run(r)
    c["one_value_100000"] = lambda: b"\x41" * 100000
    c["runs_of_300"] = lambda: bytes(np.repeat((np.arange(1000) % 251).astype(np.uint8), 300).tobytes())
    c["alternating_tiles"] = alternating_tiles
    for delta in (-4, 0, 3):
        c["cut_%+d_of_span_edge" % delta] = lambda d=delta: cut_near_span_edge(d)
    return c


CASES = cases()


def _encode_all(names):
    """{case: (stream, launches of k_rle_onepass, launches of k_rle_scatter)} through one engine, in the given order"""
    import torch
    eng = product().GpuEngine(0, 16)
    out = {}
    try:
        for name in names:
            data = CASES[name]()
            t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            cap = (product().encode_bound(len(data)) + 16 + 15) & ~15
            o = torch.empty(cap, dtype=torch.uint8, device="cuda")
            eng.profile(True)  # (clears the counts)
            n = eng.encode_device(LEVEL, t.data_ptr(), len(data), o.data_ptr(), cap)
            kp = eng.kernel_profile()
            out[name] = (bytes(o[:n].cpu().numpy()), kp["k_rle_onepass"]["launches"], kp["k_rle_scatter"]["launches"])
    finally:
        eng.close()
    return out


def _child_run(env):
    """every case in a fresh process under `env`: {case: [sha256 of the stream, one-pass launches, scatter launches]}"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.json")
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path],
                           env=e, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(path) as f:
            return json.load(f), r.stderr


@pytest.fixture(scope="module")
def onepass():
    return _encode_all(list(CASES))


@pytest.fixture(scope="module")
def three_kernels():
    return _child_run({"BZ_RLE_ONEPASS": "0"})[0]


@pytest.mark.parametrize("name", list(CASES))
def test_onepass_case(oracle, onepass, three_kernels, name):
    data = CASES[name]()
    stream, ran, scattered = onepass[name]
    assert stream == oracle.encode(data, LEVEL)
    assert (ran, scattered) == (1, 0)  # the one-pass kernel wrote the image, k_rle_scatter did not run
    sha, ran0, scattered0 = three_kernels[name]
    assert sha == hashlib.sha256(stream).hexdigest()
    assert ran0 == 0 and scattered0 >= 1  # (the switch selects the three kernels from the start)


def test_cut_cases_cut_where_they_say(oracle):
    """the first block of the cut cases ends LIMIT image bytes in, which by construction is 3 * SPAN + delta input bytes"""
    for delta in (-4, 0, 3):
        data = cut_near_span_edge(delta)
        _, st = oracle.encode(data, LEVEL, with_stats=True)
        assert st[0]["nblock"] == LIMIT and len(st) == 2
        k = LIMIT - (3 * SPAN + delta)
        assert data.count(b"\xf0" * 4) + data.count(b"\xf1" * 4) == k


def test_failed_onepass_is_redone_with_the_three_kernels(onepass):
    """BZ_RLE_ONEPASS_FAILTEST=1: the host treats the engine's first one-pass split as failed, says so in one line,
    redoes it with the three kernels and stays on them -- the streams are the same"""
    res, err = _child_run({"BZ_RLE_ONEPASS_FAILTEST": "1"})
    assert err.count("one-pass RLE1 front end did not complete") == 1
    for i, name in enumerate(CASES):
        sha, ran, scattered = res[name]
        assert sha == hashlib.sha256(onepass[name][0]).hexdigest(), name
        assert scattered >= 1 and ran == (1 if i == 0 else 0), name


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    got = _encode_all(list(CASES))
    with open(sys.argv[1], "w") as f:
        json.dump({k: [hashlib.sha256(v[0]).hexdigest(), v[1], v[2]] for k, v in got.items()}, f)
