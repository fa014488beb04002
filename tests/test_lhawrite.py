"""The LHA writer's restatement and corpus (tests/lhawrite.py) before any writer is held against them: the fixture is what
--regen made, every case meets the targets it claims, every expected archive reads back under the READER's restatement
(tests/lhaforge.py index()) with exactly the entries' fields, every stream decodes under the model, and named faults of the
restated writer each change a named case."""
import pytest

import lhaforge as F
import lhawrite as W
import lzhref as R

CASES = W.load()


def test_fixture_is_a_fresh_regen():
    text, missing, _ = W.regen()
    assert not missing
    with open(W.FIXTURE) as f:
        assert f.read() == text


def test_every_case_hits_what_it_claims_and_required_is_met():
    got = set()
    for c in CASES:
        h = W.hits(c)
        assert h == c["hits"], c["name"]
        assert set(h) & W.REQUIRED, "%s alone hits no required target" % c["name"]
        got |= set(h)
    assert W.REQUIRED <= got, sorted(W.REQUIRED - got)


def test_the_corpus_is_small():
    assert sum(len(W.build(c, m, lv)[0]) for c in CASES for m, lv in W.combos(c)) < 1_000_000


def test_the_model_meets_the_rule_where_the_corpus_says():
    """(b"ab" * 6)[:n] encodes to n + 1, n, n - 1 bytes at n = 10, 11, 12 and (b"abcdefg" * 3)[:n] at 13, 14, 15, under all four
    methods; a 1-byte input gives 7 bytes"""
    for m in (4, 5, 6, 7):
        assert [len(R.encode((b"ab" * 6)[:n], m)) - n for n in (10, 11, 12)] == [1, 0, -1]
        assert [len(R.encode((b"abcdefg" * 3)[:n], m)) - n for n in (13, 14, 15)] == [1, 0, -1]
        assert len(R.encode(b"x", m)) == 7


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_expected_archive_reads_back(case):
    ents = W.entries(case)
    for method, level in W.combos(case):
        arc, table, st = W.build(case, method, level)
        ms, fault, _ = F.index(arc)
        assert fault == F.OK and arc[-1] == 0, (method, level)
        assert [F.row(m) for m in ms] == [F.row(m) for m in table], (method, level)
        assert st[0] == len(ms) == len(ents) and st[1] + st[2] + st[3] + st[4] == st[0] and st[6] == len(arc)
        for m, (e, plain) in zip(ms, ents):
            assert arc[m["name_off"]:m["name_off"] + m["name_len"]] == e["name"]
            assert arc[m["dir_off"]:m["dir_off"] + m["dir_len"]] == e["dir"]
            assert (m["mtime"], m["attr"], m["orig_len"]) == (e["mtime"], e["attr"], len(plain))
            assert m["os_id"] == (e["os_id"] if level else 0)
            assert m["crc16"] == F.crc16(plain)
            data = arc[m["data_off"]:m["data_off"] + m["packed_len"]]
            if 4 <= m["method"] <= 7:
                assert m["method"] == method and len(data) < len(plain)
                assert R.decode(data, method, len(plain), -1)[:2] == (plain, F.OK)      # (nothing reaches in front of the output)
            else:
                assert m["id"] == (b"-lhd-" if e["is_dir"] else b"-lh0-") and data == plain
            assert arc[m["header_off"]] != 0


@pytest.mark.parametrize("fault", W.FAULTS)
def test_every_fault_of_the_writer_changes_its_case(fault):
    assert len(W.FAULTS) >= 7
    name, method, level = W.FAULT_CASE[fault]
    case = {c["name"]: c for c in CASES}[name]
    good = W.build(case, method, level)[0]
    bad = W.expected(W.entries(case), method, level, (fault,))[0]
    assert good != bad, "the case %s does not tell the fault %r from the rules" % (name, fault)
    if fault in ("skip_is_packed", "hcrc_with_field", "no_pad", "sum_from_p1"):
        ms, verdict, _ = F.index(bad)
        assert verdict != F.OK or len(ms) != len(case["members"]), fault
