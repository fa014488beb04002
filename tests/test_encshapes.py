"""CPU tests of the encoder shape cases (tests/encshapes.py, tests/golden/enc_shapes.json): every committed case
still builds the bytes that give the oracle's recorded figures and stream, still hits the targets it claims, and the
cases together hit exactly the required set -- the fixture can neither drift nor lose a target unnoticed."""
import hashlib

import pytest

import encshapes as S

CASES = S.load()


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_hits_its_targets(oracle, case):
    got, stream, fig = S.hits(case, oracle)
    assert sorted(got) == case["targets"]
    assert hashlib.sha256(stream).hexdigest() == case["sha256"]
    if case["blocks"] is not None:
        assert fig == case["blocks"]


def test_required_targets_all_hit():
    hit = set().union(*(c["targets"] for c in CASES))
    assert hit == S.REQUIRED, (sorted(S.REQUIRED - hit), sorted(hit - S.REQUIRED))


def test_zero_runs_from_the_last_column(oracle):
    """the rank-0 shortcut of zero_runs against a full move-to-front over the oracle's last column"""
    import numpy as np
    for data in (S.zrun(3, 40, 9), S.norun(5, 3000, 3), b"abracadabra" * 7, S.mono(0, 1)):
        b = np.frombuffer(data, dtype=np.uint8)
        L = [int(b[(s - 1) % len(b)]) for s in oracle.bwt(data)]
        order = sorted(set(L))
        ranks = []
        for x in L:
            r = order.index(x)
            ranks.append(r)
            order.insert(0, order.pop(r))
        runs, i = [], 0
        while i < len(ranks):
            if ranks[i] == 0:
                j = i
                while j < len(ranks) and ranks[j] == 0:
                    j += 1
                runs.append((i, j))
                i = j
            else:
                i += 1
        assert S.zero_runs(oracle, data) == runs


def test_run_relations():
    T = S.TILE
    assert S.run_relations(T - 3, T) == {"ends"}
    assert S.run_relations(T, T + 3) == {"starts"}
    assert S.run_relations(T - 1, T + 1) == {"crosses"}
    assert S.run_relations(T - 1, T) == {"ends"}
    assert S.run_relations(T, T + 1) == {"starts"}
    assert S.run_relations(T, 3 * T) == {"starts", "ends", "crosses"}
    assert S.run_relations(5, 9) == set()
