"""CPU tests of the LZHUF encoder shape cases (tests/lzhshapes.py, tests/golden/lzh_enc_shapes.json): every committed case
still builds the bytes `--regen` made, still hits the targets it claims under every method it is meant for, decodes back
to its input with the model's decoder, and the cases together hit the required set; the restated parse is the oracle's;
and each named fault of the model's ENCODER changes the stream of some committed case."""
import hashlib

import pytest

import lzhref as R
import lzhshapes as S

FIX = S.load()
CASES = FIX["cases"]


@pytest.fixture(scope="module")
def analysed(oracle):
    """hits() of every case under every method it is meant for, once"""
    return {(S.case_id(c), m): S.hits(c, oracle, m) for c in CASES for m in c["methods"]}


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_is_what_regen_made(case):
    data = S.build(case)
    assert len(data) == case["len"] and hashlib.sha256(data).hexdigest() == case["sha256"]


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_hits_its_targets_and_decodes_back(analysed, case):
    for m in case["methods"]:
        got, a = analysed[(S.case_id(case), m)]
        assert sorted(t for t in got if t in S.REQUIRED) == case["targets"][str(m)]
        assert a["stream"] == R.encode(a["data"], m)
        assert R.decode(a["stream"], m)[:2] == (a["data"], R.OK)
        assert sum(b["bits"] for b in a["blocks"]) == sum(w for _, w in R.encode_fields(a["data"], m))


def test_the_widest_code_word_meets_several_phases(analysed):
    """47 bits: a 16-bit c-code, then the widest second piece (a 16-bit p-code and 15 more bits); the phases of the four
    cases differ, and one of them carries the code into a third 32-bit word of the stream"""
    phases = []
    for c in CASES:
        if c["name"].startswith("wide47"):
            got, a = analysed[(S.case_id(c), 7)]
            assert a["wide_phases"] == c["wide_phases"] and len(a["wide_phases"]) == 1
            assert max(max(b["stab"]) for b in a["blocks"]) == 16 == max(max(b["otab"]) for b in a["blocks"])
            phases += a["wide_phases"]
    assert len(set(phases)) == 4 and any(p + 47 > 64 for p in phases) and any(p + 47 <= 64 for p in phases)


def test_required_targets_all_hit():
    hit = set().union(*(set(t) for c in CASES for t in c["targets"].values()))
    assert hit >= S.REQUIRED, sorted(S.REQUIRED - hit)
    assert hit == S.REQUIRED
    assert FIX["total_bytes"] == sum(c["len"] for c in CASES) < 2 << 20


def test_the_restated_parse_is_the_oracles(oracle):
    for c in CASES:
        if c["len"] > 5000:
            continue
        data = S.build(c)
        for m in c["methods"]:
            toks = oracle.lzss_tokens(data, window=S.WIN[m], max_match=R.MAX_MATCH)
            assert S.steps_tokens(data, S.naive_steps(data, S.WIN[m])) == toks, S.case_id(c)


def test_unmutated_encoder_copy_is_the_model(oracle):
    for c in CASES:
        if c["len"] > 70000:
            continue
        data = S.build(c)
        m = c["methods"][-1]
        assert S.encode_mut(oracle, data, m) == R.encode(data, m), S.case_id(c)


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_named_fault_changes_some_case(oracle, mutation):
    slow = mutation in ("lazy_accepts_3", "no_pos_term")  # (they run the plain restatement of the parse)
    changed = []
    for c in CASES:
        if c["len"] > (5000 if slow else 140000):
            continue
        data = S.build(c)
        for m in c["methods"]:
            if S.encode_mut(oracle, data, m, (mutation,)) != R.encode(data, m):
                changed.append((S.case_id(c), m))
                break
        if changed:
            break
    assert changed, "no committed case tells the model from the fault %r" % mutation
