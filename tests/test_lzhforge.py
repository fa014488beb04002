"""The forged LZHUF corpus (tests/lzhforge.py, tests/golden/lzh_shapes.json) before any GPU sees it: every case is what
--regen made, hits the targets it claims, REQUIRED is hit in full, and the corpus tells each named fault of the model's
decoder (lzhref.MUTATIONS) from the model."""
import json

import pytest

import lzhforge as F
import lzhref as R


@pytest.fixture(scope="module")
def cases():
    return F.load()


def test_fixture_is_what_regen_makes(cases):
    plain = [{k: v for k, v in c.items() if k not in ("sha256", "hits")} for c in cases]
    assert plain == json.loads(json.dumps(F.base_cases()))
    for c in cases:
        assert F.digest(c) == c["sha256"], c["name"]


def test_cases_hit_what_they_claim_and_required_is_covered(cases):
    got = set()
    for c in cases:
        h = set().union(*[F.hits(dict(c, k=k)) for k in F.preambles(c)])
        assert sorted(h) == c["hits"], c["name"]
        got |= h
    assert got >= F.REQUIRED, sorted(F.REQUIRED - got)


def test_verdict_classes_and_the_large_cases(cases):
    small = [c for c in F.expand(cases) if c["shape"] not in F.BIG]
    verdicts = {F.expected(c)[1] for c in small if c["k"] in (0, 7)}
    assert verdicts == {F.OK, F.E_DATA, F.E_EOF}
    (big,) = [c for c in cases if c["name"] == "const_matches_max"]
    data, verdict, r = F.expected(dict(big, k=0))
    assert verdict == F.OK and data == b"\x42" * (1 + 65535 * 256) and (r.blocks, r.literals, r.matches) == (2, 1, 65535)
    (lit,) = [c for c in cases if c["name"] == "const_lits_max"]
    assert F.expected(dict(lit, k=0))[:2] == (b"\x41" * 65535, F.OK)


def test_truncations_come_in_both_classes():
    for m, s in F.truncations():
        data, verdict, _ = R.decode(s, m)
        assert verdict in (R.OK, R.E_EOF)           # a cut can never look like a data error


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_every_mutation_of_the_model_is_told_by_some_case(cases, mutation):
    assert len(R.MUTATIONS) >= 10
    for c in F.expand(cases):
        if c["k"] > 1 or c["shape"] in F.BIG:
            continue
        s = F.build(c)
        a = R.decode(s, c["method"], c.get("orig_len"), c.get("prefill", -1))
        b = R.decode(s, c["method"], c.get("orig_len"), c.get("prefill", -1), mutate=(mutation,))
        if a[:2] != b[:2]:
            return
    for m, s in F.truncations():
        if R.decode(s, m)[:2] != R.decode(s, m, mutate=(mutation,))[:2]:
            return
    pytest.fail("no committed case tells the mutation %r from the model" % mutation)
