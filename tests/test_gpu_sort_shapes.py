"""GPU tests of the rotation sort in every form its round driver can choose (tests/sortshapes.py, run_bwt_once in
rust-compression_amd/csrc/k_bwt.hip): the walk form carried and plain, the survivor form inside LDS, overflowing LDS
and without an attempt, the period round entered at once and later in its one-, two- and three-pass forms, link rounds
that pay and one that does not, the end by depth, and batches whose blocks disagree about all of that.

Every single-block case: the order of debug_bwt against the oracle's, in process with the default switches.  Every
batch case: the stream of encode_device at level 1 on an engine of 16 blocks against the oracle's, with nblock,
block_crc and orig_ptr per block.  Then one fresh child process with BZ_BWT_TRACE=1 runs every case again, compares
with the oracle itself and hands back the parsed rounds: the parent asserts per case the forms it was built for, that
the forms together are all there are, and -- single blocks -- that the unordered counts the driver printed are the
numpy profile's.  Two more children do the cases under BZ_ONESWEEP=0 and BZ_FUSED_REFINE=0 (read once per process).

The counts.  A round's line prints h = 2c << step and the counts m, mx the driver read before it: the rotations the
refinements so far left unordered, which compared 2c << step symbols.  So in every round before the first period or
link round m = mx = profile.m(h) at the printed h exactly; a period or link round orders groups without moving the
depth, and from then on m <= profile.m(h)."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import pytest

import sortshapes as S
from conftest import ROOT, product

pytestmark = pytest.mark.gpu

CASES = S.load()
SINGLE = [c for c in CASES if c["gen"] != "batch"]
BATCH = [c for c in CASES if c["gen"] == "batch"]
STATS = ("nblock", "block_crc", "orig_ptr")
MARK = "== sortshapes case %s"


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 16)
    yield e
    e.close()


_REF = {}


def _ref(oracle, case):
    """(computed once per case and left alone) the block and the oracle's order, or the input, the oracle's stream and
    its per-block figures"""
    k = S.case_id(case)
    if k not in _REF:
        data = S.build(case)
        assert hashlib.sha256(data).hexdigest() == case["sha256"]  # (the bytes are the ones the CPU test pinned)
        if case["gen"] == "batch":
            stream, st = oracle.encode(data, 1, with_stats=True)
            _REF[k] = (data, stream, [{s: b[s] for s in STATS} for b in st])
        else:
            _REF[k] = (data, oracle.bwt(data))
    return _REF[k]


def _encode(eng, data, level=1):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = (product().encode_bound(len(data)) + 16 + 15) & ~15
    o = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = eng.encode_device(level, t.data_ptr(), len(data), o.data_ptr(), cap)
    return bytes(o[:n].cpu().numpy()), [{s: b[s] for s in STATS} for b in eng.block_stats()]


@pytest.mark.parametrize("case", SINGLE, ids=S.case_id)
def test_order_of_single_block(eng, oracle, case):
    data, sa = _ref(oracle, case)
    assert eng.debug_bwt(data) == sa


@pytest.mark.parametrize("case", BATCH, ids=S.case_id)
def test_stream_of_batch(eng, oracle, case):
    data, stream, st = _ref(oracle, case)
    got, got_st = _encode(eng, data)
    assert got == stream
    assert got_st == st


# ------------------------------------------------------------------------------------------------- child processes
def _child(path):
    """(a fresh process, the switches of its environment) every case against the oracle; with BZ_BWT_TRACE also the
    parsed rounds: file descriptor 2 goes to a file, a marker line in front of every case"""
    from oracle import oracle
    traced = os.environ.get("BZ_BWT_TRACE") is not None
    with tempfile.TemporaryFile() as err:
        keep = os.dup(2)
        if traced:
            os.dup2(err.fileno(), 2)
        res = {}
        e = product().GpuEngine(0, 16)
        try:
            for c in CASES:
                k = S.case_id(c)
                os.write(2, (MARK % k + "\n").encode())
                data = S.build(c)
                if c["gen"] == "batch":
                    stream, st = oracle.encode(data, 1, with_stats=True)
                    got, got_st = _encode(e, data)
                    res[k] = {"ok": got == stream and got_st == [{s: b[s] for s in STATS} for b in st]}
                else:
                    res[k] = {"ok": e.debug_bwt(data) == oracle.bwt(data)}
                res[k]["fused_fallbacks"] = int(e.bwt_stats()["fused_fallbacks"])
        finally:
            e.close()
            os.dup2(keep, 2)
        if traced:
            err.seek(0)
            text = err.read().decode("utf-8", "replace")
            sys.stderr.write(text)  # (kept for whoever reads a failure)
            for part in text.split(MARK % "")[1:]:
                k, _, body = part.partition("\n")
                res[k]["sorts"] = S.parse_trace(body)
    with open(path, "w") as f:
        json.dump(res, f)


def _run_child(env_extra):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "out.json")
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path],
                           env=dict(os.environ, **env_extra), cwd=ROOT, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        with open(path) as f:
            res = json.load(f)
    assert sorted(res) == sorted(S.case_id(c) for c in CASES)
    return res


@pytest.fixture(scope="module")
def traced():
    return _run_child({"BZ_BWT_TRACE": "1"})


def _rounds(traced, case):
    """the rounds of a case's sorts.  A single block is one sort; a batch input of at most 16 blocks is one sort too
    (blocks of which the init leaves nothing unordered print no round)."""
    sorts = traced[S.case_id(case)]["sorts"]
    assert len(sorts) <= 1, sorts
    return sorts[0] if sorts else []


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_forms_of_case(traced, case):
    """the traced run gave the oracle's order or stream, took the forms the case was built for, in the order given
    where the case says so, and none of those it was built to stay clear of"""
    got = traced[S.case_id(case)]
    assert got["ok"]
    assert got["fused_fallbacks"] == 0  # (on the fused passes the walk form of round 1 is the carried one)
    rounds = _rounds(traced, case)
    seen = S.forms(rounds)
    assert set(case["forms"]) <= seen, (sorted(seen), rounds)
    assert not set(case["absent"]) & seen, (sorted(seen), rounds)
    S.check_sequence(case, rounds)


def test_every_form_seen(traced):
    """a form that became unreachable shows here: together the cases take every form the driver has"""
    seen = set()
    for c in CASES:
        seen |= S.forms(_rounds(traced, c))
    assert seen == S.FORMS, (sorted(S.FORMS - seen), sorted(seen - S.FORMS))
    # and no case is there for nothing: each one is the only one built for some form or target
    for c in CASES:
        others = set()
        for d in CASES:
            if d is not c:
                others |= set(d["targets"]) | set(d["forms"])
        assert (set(c["targets"]) | set(c["forms"])) - others, S.case_id(c)


@pytest.mark.parametrize("case", SINGLE, ids=S.case_id)
def test_unordered_counts_are_the_profile(traced, case):
    """m and mx of every round up to the first period or link round are profile.m at the printed depth; behind it they
    are no more than that (see the head of this file)"""
    rounds = _rounds(traced, case)
    p = S.Profile(S.build(case))
    exact = True
    for r in rounds:
        want = p.m(r["h"])
        print("round %d h=%d form=%s: m=%d mx=%d profile=%d" % (r["round"], r["h"], r["form"], r["m"], r["mx"], want))
        assert r["total"] == r["max_n"] == p.n
        assert r["m"] == r["mx"]
        if exact:
            assert r["m"] == want, r
        else:
            assert r["m"] <= want, r
        if r["form"] in ("period", "link"):
            exact = False


@pytest.mark.parametrize("env_name", ["BZ_ONESWEEP", "BZ_FUSED_REFINE"])
def test_cases_under_other_switches(env_name):
    """the three-kernel radix passes, and flags + apply as two kernels (the walk form of round 1 is then the plain one):
    every case in one child, orders and streams against the oracle"""
    res = _run_child({env_name: "0"})
    bad = [k for k, v in res.items() if not v["ok"]]
    assert not bad, (env_name, bad)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    _child(sys.argv[1])
