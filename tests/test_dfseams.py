"""CPU tests of the Deflate part-seam cases (tests/dfseams.py, tests/golden/df_seams.json): every committed case still
builds the bytes it was made with, still hits the targets it claims, its seams are still the ones the model computes
from the oracle, the oracle's streams are the recorded ones and inflate; the cases together cover REQUIRED and every one
is needed; and the targets discriminate -- each named fault of the MODEL changes the seams of some case."""
import hashlib
import os
import zlib

import pytest

import dfseams as S

FIX = S.load()
CASES = FIX["cases"]


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_is_what_regen_made(case):
    assert S.digest(case) == case["sha256"]
    assert sum(len(d) for d, _ in S.build_pieces(case)) == case["bytes"]


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_hits_its_targets_and_its_seams_are_the_models(oracle, case):
    got, rows, f = S.hits(case, oracle)
    assert sorted(got) == case["targets"]
    assert rows == case["seams"]
    assert S.streams(case, oracle, f) == case["streams"]
    assert S.block_counts(f) == case["blocks"]
    # the raw stream (Finish behind every piece list; a Run piece is fed with Finish) inflates to the input
    d = zlib.decompressobj(-15, zdict=f.dict) if f.dict else zlib.decompressobj(-15)
    assert d.decompress(f.stream) + d.flush() == b"".join(s.data for s in f.segs) and d.eof
    # parts tile their segment; a part starts where its predecessor's kept bytes end
    for si, s in enumerate(f.segs):
        mine = [r for r in rows if r[0] == si]
        assert bool(mine) == (len(s.data) > S.PART + S.GUARD)
        pos = 0
        for r in mine:
            assert r[1] == pos and 0 <= r[3] <= 2 and 0 <= r[4] <= 7
            pos += r[2]
        assert not mine or pos == len(s.data)
        assert not mine or sum(r[7] for r in mine) == len(s.blocks)


def test_required_targets_all_hit_and_every_case_needed():
    hit = set().union(*(c["targets"] for c in CASES))
    assert hit >= S.REQUIRED, sorted(S.REQUIRED - hit)
    assert hit == S.REQUIRED
    for i, c in enumerate(CASES):
        others = set().union(*(x["targets"] for j, x in enumerate(CASES) if j != i))
        assert set(c["targets"]) - others, "%s hits nothing of its own" % S.case_id(c)


def test_cases_are_as_small_as_their_seams_allow():
    assert (FIX["part"], FIX["guard"]) == (S.PART, S.GUARD) == (1 << 20, 66560)
    for c in CASES:
        nseams = sum(1 for r in c["seams"] if r[5] >= 0)
        # (a last part of exactly PART + GUARD bytes makes a one-seam case as long as a two-seam one)
        full_last = any(r[5] < 0 and r[2] == S.PART + S.GUARD for r in c["seams"])
        assert c["bytes"] < (1_300_000 if nseams <= 1 and not full_last else 3_500_000), c["name"]
        # one seam needs PART + GUARD + 1 bytes of segment
        assert nseams == 0 or c["bytes"] >= S.PART + S.GUARD + 1


# fault of the model -> (the case that tells it, the first thing that changes: a field of part 0 / 1, or the count of parts)
TOLD_BY = {
    "lt_for_le": ("K-flush65519", (0, "kept")),
    "carry_not_subtracted": ("K-flush65519", (0, "kept")),
    "keep_by_block_end": ("K-flush65519", (0, "kept")),
    "bits_at_last_kept_block": ("K-flush65519", (0, "bits")),
    "guard_0x10000": ("E-guard", "parts"),
    "last_part_lt": ("E-guard", "parts"),
    "skip_ignored": ("B-stored-skip2-L8", (0, "kept")),
    "skip_added": ("B-stored-skip2-L8", (0, "kept")),
    "threshold_from_segment_start": ("M-two", (1, "kept")),
}
FIELDS = ("segment", "pos", "kept", "skip", "bits", "last", "first", "blocks")


@pytest.mark.parametrize("fault", S.FAULTS)
def test_each_fault_of_the_model_changes_some_case(oracle, fault):
    """the targets discriminate: a model with `<` for `<=`, a guard of 0x10000, `skip` ignored, the Flush carry left in
    the first block, ... computes OTHER seams, well formed, for the case named in TOLD_BY, and the named field is the
    first that differs.  A fault that merely makes the model raise does not count."""
    assert set(TOLD_BY) == set(S.FAULTS) and len(S.FAULTS) >= 8
    name, what = TOLD_BY[fault]
    case = next(c for c in CASES if c["name"] == name)
    f = S.facts(case, oracle)
    assert S.seams(case, oracle, f=f) == case["seams"]
    rows = S.seams(case, oracle, fault=fault, f=f)   # (an exception here fails the test)
    assert all(len(r) == 8 and 0 <= r[3] <= 2 and 0 <= r[4] <= 7 and r[2] > 0 for r in rows)
    if what == "parts":
        assert len(rows) != len(case["seams"])
    else:
        assert len(rows) == len(case["seams"])
        diff = [(i, FIELDS[k]) for i, (r, w) in enumerate(zip(rows, case["seams"])) for k in range(8) if r[k] != w[k]]
        assert diff and diff[0] == what, diff


def test_filler_makes_no_match_in_either_bank(oracle):
    d = S.filler(400000, S.BANK - 200000)
    assert 0 not in d and not oracle.lzss_tokens_raw(d)[:, 0].any()
    # a bank-1 trigram never shows the class pattern of a bank-0 trigram: nothing matches across the banks either
    d = S.filler(60000, 1000) + S.filler(60000, S.BANK + 1000)
    assert not oracle.lzss_tokens_raw(d)[:, 0].any()


def test_step_restatement_finds_the_planted_steps(oracle):
    """the lazy generator's block start lies `skip` bytes inside a step, and the restated step says so"""
    for skip in (1, 2):
        case = {"name": "t", "family": "Z", "kinds": [0],
                "pieces": [["script", [["lazy", S.B17, skip, 13, 1, 0], ["fill", S.B17 + 3000, 0]], S.FINISH]]}
        f = S.facts(case, oracle)
        got, steps = S.step_of(f.segs[0], S.B17)
        assert got == skip and steps[-1][1] == skip


def test_parse_trace_reads_the_sample():
    text = open(S.TRACE_SAMPLE).read()
    parts = S.parse_trace(text)
    assert parts and all(len(p) == 8 for p in parts)
    calls = S.trace_calls(parts)
    assert sum(len(c) for c in calls) == len(parts) and all(len(c) >= 2 for c in calls)
    for k, pos, ln, n, kept, sbytes, bits, nb in parts:
        assert pos + ln <= n and kept <= ln and bits <= 7 and nb >= 1
        assert ln == min(n - pos, S.PART + S.GUARD) and (kept == ln) == (pos + ln == n)
    # the sample is the trace of committed cases: its first call is the first multi-part case's
    first = next(c for c in CASES if c["seams"])
    assert calls[0] == S.model_calls(first)[0]
    # lines of other tools around it do not disturb it; a damaged part line is an error
    assert S.parse_trace("bz2_mi355x: something else\n" + text + "\nmore\n") == parts
    line = next(l for l in text.splitlines() if "deflate part" in l)
    with pytest.raises(ValueError):
        S.parse_trace(line.replace(" bits handed on", " bits"))


def test_no_case_bytes_in_the_fixture():
    assert os.path.getsize(S.FIXTURE) < 100_000
    assert all(set(c) <= {"name", "family", "kinds", "pieces", "dict", "targets", "sha256", "bytes", "seams", "streams", "blocks"}
               for c in CASES)
    assert all(len(hashlib.sha256(b"").hexdigest()) == len(c["sha256"]) for c in CASES)
