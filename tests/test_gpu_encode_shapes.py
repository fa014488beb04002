"""GPU tests of the level-1..9 encoder at the block shapes where its kernels branch (tests/encshapes.py): the table
count, the selector count and last group, the MTF kernel's alphabet and batch-size instances, zero runs against the
ZLE tiles, sort tiles and the block limit, and the table kernel's two forms.  Every case: the oracle's stream, which
decodes back to the input, and the oracle's per-block figures and section sizes.  Families A-D run again in child
processes under BZ_HUFF_SPLIT=0 (the Huffman stage in one workgroup per block) and BZ_FUSED_ZLE=0 (ZLE as three
kernels), switches that are read once per process."""
import bz2
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

import encshapes as S
from conftest import ROOT, product

pytestmark = pytest.mark.gpu

CASES = S.load()
STATS = ("nblock", "block_crc", "orig_ptr", "mtf_count", "in_use_count", "group_num", "n_selectors", "max_len")
SECTIONS = ("pass_size", "fave", "bits_mapping", "bits_selectors", "bits_lengths", "bits_codes")


def _engine_sizes(case):
    """batch sizes an input runs at: at most 16 blocks (SUB = 8 MTF lanes per chunk); the 17-block batch (SUB = 1);
    the 321-block input through 320 (six-wave pipelined tables, two batches) and 321 (a lane per table)"""
    if case["gen"] == "batch":
        return (17,) if len(case["args"][1]) == 17 else (320, 321)
    return (16,)


def _encode(eng, data, level):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = (product().encode_bound(len(data)) + 16 + 15) & ~15
    o = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = eng.encode_device(level, t.data_ptr(), len(data), o.data_ptr(), cap)
    return bytes(o[:n].cpu().numpy())


def _run(engines, case, sections=True):
    """{batch size: (sha256 of the stream, block_stats, block_sections or None)} of one case"""
    data = S.build(case)
    out = {}
    for nb in _engine_sizes(case):
        eng = engines(nb)
        stream = _encode(eng, data, case["level"])
        st = [{k: b[k] for k in STATS} for b in eng.block_stats()]
        sec = [{k: b[k] for k in SECTIONS} for b in eng.block_sections()] if sections else None
        out[nb] = (hashlib.sha256(stream).hexdigest(), st, sec, stream)
    return data, out


class _Engines:
    def __init__(self):
        self.e = {}

    def __call__(self, nb):
        if nb not in self.e:
            self.e[nb] = product().GpuEngine(0, nb)
            self.e[nb].profile(2)  # (bit 1: the per-pass figures of block_sections)
        return self.e[nb]

    def close(self):
        for e in self.e.values():
            e.close()
        self.e = {}


@pytest.fixture(scope="module")
def engines():
    e = _Engines()
    yield e
    e.close()


def _expected(oracle, data, level):
    stream, st = oracle.encode(data, level, with_stats=True)
    return stream, [{k: b[k] for k in STATS} for b in st], [{k: b[k] for k in SECTIONS} for b in st]


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_shape_case(engines, oracle, case):
    data, got = _run(engines, case)
    stream, st, sec = _expected(oracle, data, case["level"])
    assert hashlib.sha256(stream).hexdigest() == case["sha256"]  # (the bytes are the ones the CPU test pinned)
    for nb, (_, g_st, g_sec, g_stream) in got.items():
        assert g_stream == stream, nb
        assert g_st == st, nb
        assert g_sec == sec, nb
    assert bz2.decompress(next(iter(got.values()))[3]) == data


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 8191, 8192, 8193, 16383, 16384, 16385,
                               109 * 8192 - 1, 109 * 8192 + 1, S.limit(9)])
def test_bwt_at_sort_tile_edges(engines, oracle, n):
    """sort tiles of 8192 symbols, 110 of them for the largest level-9 block: random bytes, 4 symbols, a short period
    (above 20000 symbols one that does not divide n: the oracle's tie rule takes quadratic time on a whole-periodic block)"""
    p = next(p for p in (3, 4, 5, 7) if n % p or n < 20000)
    for data in (S.norun(n, n, 256), S.norun(n + 1, n, 4), (b"abcdefg"[:p] * (n // p + 1))[:n]):
        assert engines(16).debug_bwt(data) == oracle.bwt(data), n


def _child(path, env_name):
    """(run in a fresh process with one switch set) families A-D through the engines; results to `path`"""
    eng = _Engines()
    res = {}
    try:
        for c in CASES:
            if c["family"] in "ABCD":
                _, got = _run(eng, c, sections=env_name != "BZ_HUFF_SPLIT")
                res[S.case_id(c)] = {str(nb): [g[0], g[1], g[2]] for nb, g in got.items()}
    finally:
        eng.close()
    with open(path, "w") as f:
        json.dump(res, f)


@pytest.mark.parametrize("env_name", ["BZ_HUFF_SPLIT", "BZ_FUSED_ZLE"])
def test_shape_cases_other_forms(oracle, env_name):
    """the Huffman stage in one workgroup per block (the first copy of the table-count rule, k_huffman) and the ZLE
    stage as three kernels, at the shapes of families A-D: one child process, under its own time limit"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.json")
        env = dict(os.environ)
        env[env_name] = "0"
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path, env_name],
                           env=env, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(path) as f:
            res = json.load(f)
    sub = [c for c in CASES if c["family"] in "ABCD"]
    assert len(res) == len(sub)
    for c in sub:
        stream, st, sec = _expected(oracle, S.build(c), c["level"])
        for nb, (sha, g_st, g_sec) in res[S.case_id(c)].items():
            assert sha == hashlib.sha256(stream).hexdigest(), (env_name, S.case_id(c), nb)
            assert g_st == st, (env_name, S.case_id(c), nb)
            if env_name != "BZ_HUFF_SPLIT":  # (that form leaves the section figures zero)
                assert g_sec == sec, (env_name, S.case_id(c), nb)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1], sys.argv[2])
