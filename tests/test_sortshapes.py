"""CPU tests of the sort shape cases (tests/sortshapes.py, tests/golden/sort_shapes.json): every committed case still
builds the bytes and the profile figures that were recorded, still reaches the targets it claims, the cases together
reach exactly the required set, the numpy profile orders every block as the oracle does, and the trace parser reads
the committed sample of BZ_BWT_TRACE output and refuses a damaged line."""
import hashlib

import numpy as np
import pytest

import sortshapes as S

CASES = S.load()


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_is_current_and_ordered_like_the_oracle(oracle, case):
    data = S.build(case)
    assert hashlib.sha256(data).hexdigest() == case["sha256"] and len(data) == case["n"]
    got, fig = S.hits(case, data)
    assert sorted(got) == case["targets"]
    assert fig == case["figures"]
    for blk in S.blocks_of(case, data):
        assert S.order_matches(S._profile_of(blk), oracle.bwt(blk))


def test_generated_cases_are_the_committed_ones():
    """the fixture is what --regen would write, apart from the figures the test above recomputes"""
    keys = ("family", "gen", "args", "why", "forms", "absent", "sequence")
    assert [{k: c[k] for k in keys} for c in CASES] == [{k: c[k] for k in keys} for c in S.candidates()]


def test_required_targets_all_hit_and_no_case_idle():
    hit = set().union(*(c["targets"] for c in CASES))
    assert hit == S.REQUIRED, (sorted(S.REQUIRED - hit), sorted(hit - S.REQUIRED))
    for c in CASES:  # (take any one case away and a target is lost)
        others = set().union(*(d["targets"] for d in CASES if d is not c))
        assert set(c["targets"]) - others, S.case_id(c)
    named = set().union(*(set(c["forms"]) | set(c["absent"]) for c in CASES))
    assert named <= S.FORMS and set().union(*(c["forms"] for c in CASES)) == S.FORMS


def test_profile_on_small_blocks(oracle):
    """the profile against brute force: m, G and the group sizes from sorted Python slices, the order from the oracle"""
    rng = np.random.default_rng(5)
    blocks = [b"banana", b"abracadabra" * 3, b"aaaa", b"ab" * 6, bytes(rng.integers(0, 3, 200, dtype=np.uint8)), b"x",
              S.runs(1, 300, 0, 40, 20), S.pairs(2, 100, 50, 3, 30)]
    for blk in blocks:
        n = len(blk)
        p = S.Profile(blk)
        for h in (1, 2, 3, 5, 8, 12, 16, 24, 100):
            pre = sorted((blk * (h // n + 2))[i:i + h] for i in range(n))
            sizes = [pre.count(x) for x in sorted(set(pre))]
            assert p.sizes(h).tolist() == sizes, (blk, h)
            assert p.m(h) == sum(s for s in sizes if s > 1) and p.G(h) == max(sizes)
            assert p.groups(h).tolist() == [s for s in sizes if s > 1]
            assert S.profile(blk, [h])[h] == {"m": p.m(h), "G": p.G(h), "groups": p.groups(h).tolist()}
        assert S.order_matches(p, oracle.bwt(blk))
        if len(set(blk)) > 1 and p.m(2 * n) == 0:
            assert p.order().tolist() == list(oracle.bwt(blk))
            bad = list(oracle.bwt(blk))
            bad[0], bad[-1] = bad[-1], bad[0]
            assert not S.order_matches(p, bad)


def test_segments_model():
    """k_surv_local's segments of a list, from the sizes of its groups"""
    T, C = S.TILE, S.LOC_CAP
    assert S.segments([100, 50]) == [(0, 150, 2)]
    assert S.segments([10000]) == [(0, 10000, 1), None]  # (nothing starts in the second tile)
    assert S.segments([6000, 5000, 2]) == [(0, 11000, 2), (11000, 2, 1)]  # (the second group lies across the edge)
    assert S.segments([2] * 4096 + [2]) == [(0, T, 4096), (T, 2, 1)]
    assert S.segments([2000, 15000]) == [(0, 17000, 2), None, None] and not S.fits(S.segments([2000, 15000]))
    assert S.fits(S.segments([2, C - 2])) and not S.fits(S.segments([2, C - 1]))
    assert S.segments([50000, 50000])[0] == "lost"  # (no group start within reach of the second tile's first entry)
    assert S.segments([T + S.LOC_LOOK - 1, 5])[0] == (0, T + S.LOC_LOOK - 1, 1)
    assert S.segments([T + S.LOC_LOOK + 1, 5])[0] == "lost"


def test_key_chars():
    assert S.key_chars(bytes(range(256)) * 8) == 6  # eight bits a symbol: 4; but only 256 pairs, eight bits a pair: 2 * 3
    assert S.key_chars(S.filler(1, 50000)) == 4
    assert S.key_chars(b"ab" * 100) == 8
    assert S.key_chars(S.para(1, 5000)) == 8  # 9 letters: 4 bits, 7 symbols; 81 pairs: 7 bits, 8 symbols
    assert S.key_chars(S.golden("sample1.ref", 100000)) == 4


def test_trace_parser_on_the_committed_sample():
    with open(S.TRACE_SAMPLE) as f:
        text = f.read()
    sorts = S.parse_trace(text)
    assert [len(s) for s in sorts] == [12, 3]
    a, b = sorts
    assert [r["form"] for r in a] == ["walk", "period", "walk", "link", "walk", "link"] + ["walk"] * 5 + ["survivor"]
    assert a[1] == {"round": 2, "h": 16, "m": 47985, "total": 53000, "mx": 47985, "max_n": 53000, "form": "period",
                    "passes": 3}
    assert [r["h"] for r in a] == [8, 16, 16, 32, 32, 64, 64, 128, 256, 512, 1024, 2048]
    assert a[-1]["lds"] == "done" and a[-1]["m"] == 2944
    assert S.forms(a) == {"walk round 1", "walk later", "period later", "period 3 pass", "link paid", "link did not pay",
                          "survivor LDS done"}
    assert [r["lds"] for r in b] == ["did not fit", None, None]
    assert S.forms(b) == {"survivor LDS did not fit", "survivor global, sticky"}
    # other traces' lines between the rounds are passed over; a round line that lost a field is not
    assert S.parse_trace("bz_enc job 3\n" + text) == sorts
    lines = text.splitlines()
    first, passes, fit = lines[0], lines[2], lines[-3]
    assert "three passes" in passes and "did not fit" in fit
    for damaged in (text.replace(first, first.replace("rotations unordered", "rotations")),
                    text.replace(first, first.replace("walk form", "some form")),
                    text.replace(first, first.replace("(h = 8)", "(h = ?)")),
                    "\n".join(lines[1:]),  # (round 2 without round 1)
                    "\n".join(lines[:3] + lines[2:]),  # (the period round's line twice)
                    text.replace(passes, passes.replace("three passes", "nine passes")),
                    text.replace(fit, fit.replace("did not fit", "did fit")),
                    fit,  # (an LDS line without its round)
                    "\n".join(lines[:2] + [fit])):  # (and behind a round that is no survivor round)
        with pytest.raises(ValueError):
            S.parse_trace(damaged)
