"""GPU tests of k_block_symbols taking the bytes in use from the map of the byte pairs in use: position i sets the bit of
(T[i], T[(i + 1) mod n]), and byte b is in use iff row b of the map (words 8b .. 8b+7) is not empty.  The inputs: one and
two bytes; a byte that occurs only as the block's last, whose pair wraps to the block's first byte, alone and as the
middle block of three; first bytes at the word and row edges of the map; all 256 bytes.  Every case: the oracle's
stream and the oracle's in_use_count, by default and once more in a child process under BZ_PAIR_KEYS=0, where no map
is built and the kernel keeps its per-byte set."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import encshapes as S
from conftest import ROOT, product

pytestmark = pytest.mark.gpu

L1 = S.limit(1)
EDGES = (0, 31, 32, 63, 64, 255)


def _edges(seed, n):
    return np.asarray(EDGES, dtype=np.uint8)[np.frombuffer(S.norun(seed, n, len(EDGES)), dtype=np.uint8)].tobytes()


def _inputs():
    """name -> (bytes, level, in_use_count of every block).  norun pieces have no run of four equal bytes, so RLE1
    leaves them alone and a level-1 block is exactly the next L1 bytes."""
    last_only = S.norun(11, L1 - 1, 40, 10) + b"\xee"  # 0xee: only as the block's last byte
    assert last_only.count(b"\xee") == 1 and len(last_only) == L1
    first, third = S.norun(12, L1, 30, 100), S.norun(13, 5000, 30, 200)
    assert third[0] != last_only[0] and third[0] not in last_only  # (the next block's first byte is no byte of this one)
    return {
        "n=1": (b"\x07", 9, [1]),
        "n=2": (b"\x07\x09", 9, [2]),
        "n=2 equal": (b"\x07\x07", 9, [1]),
        "last only": (S.norun(10, 5000, 40, 10) + b"\xee", 9, [41]),
        "last only, middle block": (first + last_only + third, 1, [30, 41, 30]),
        "edges": (_edges(14, 3000), 9, [len(EDGES)]),
        "edges, two workgroups": (_edges(15, 70000), 9, [len(EDGES)]),
        "all 256": (S.norun(16, 3000, 256), 9, [256]),
    }


INPUTS = _inputs()


def _run(eng, data, level):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = (product().encode_bound(len(data)) + 16 + 15) & ~15
    o = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = eng.encode_device(level, t.data_ptr(), len(data), o.data_ptr(), cap)
    return bytes(o[:n].cpu().numpy()), [int(b["in_use_count"]) for b in eng.block_stats()]


@pytest.fixture(scope="module")
def engine():
    e = product().GpuEngine(0, 16)
    yield e
    e.close()


@pytest.fixture(scope="module")
def expected(oracle):
    """name -> (the oracle's stream, its in_use_count per block): computed once, shared with the child's check"""
    exp = {}
    for name, (data, level, use) in INPUTS.items():
        stream, st = oracle.encode(data, level, with_stats=True)
        assert [int(b["in_use_count"]) for b in st] == use, name  # (the input is what its name says)
        exp[name] = (stream, use)
    return exp


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_in_use_from_pair_map(engine, expected, name):
    data, level, _ = INPUTS[name]
    stream, use = _run(engine, data, level)
    assert use == expected[name][1]
    assert stream == expected[name][0]


def _child(path):
    """(run in a fresh process: BZ_PAIR_KEYS is read once per process) every input through one engine; results to `path`"""
    eng = product().GpuEngine(0, 16)
    res = {}
    try:
        for name, (data, level, _) in INPUTS.items():
            stream, use = _run(eng, data, level)
            res[name] = [stream.hex(), use]
    finally:
        eng.close()
    with open(path, "w") as f:
        json.dump(res, f)


def test_without_pair_map(expected):
    """BZ_PAIR_KEYS=0: pair_bits is null and the kernel's per-byte set is the only source of the bytes in use"""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.json")
        env = dict(os.environ)
        env["BZ_PAIR_KEYS"] = "0"
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path],
                           env=env, cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(path) as f:
            res = json.load(f)
    assert sorted(res) == sorted(INPUTS)
    for name, (stream, use) in expected.items():
        assert res[name][1] == use, name
        assert bytes.fromhex(res[name][0]) == stream, name


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
