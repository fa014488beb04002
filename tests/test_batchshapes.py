"""CPU tests of the batch encoder's seam cases (tests/batchshapes.py, tests/golden/bz_batch_shapes.json): the committed
fixture is what `--regen` makes today, every case still builds the bytes it recorded and hits the targets it claims, the
cases together hit the required set, the restated front end gives the oracle's RLE1 image, length and CRC on every case,
and each named fault of the restated front end changes the image of some committed case."""
import hashlib
import os

import pytest

import batchshapes as S

FIX = S.load()
CASES = FIX["cases"]


@pytest.fixture(scope="module")
def analysed(oracle):
    """hits() of every case, once"""
    return {S.case_id(c): S.hits(c, oracle) for c in CASES}


def test_fixture_is_a_fresh_regen(oracle):
    fresh, missing = S.regen(oracle, log=lambda s: None)
    assert missing == []
    assert fresh == FIX


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_is_what_regen_made(case):
    data = S.build(case)
    assert len(data) == case["len"] and hashlib.sha256(data).hexdigest() == case["sha256"]
    assert set(case) <= {"family", "name", "gen", "args", "level", "sha256", "len", "targets", "trailer_bit"}  # no payload


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_hits_its_targets(analysed, case):
    got, a = analysed[S.case_id(case)]
    assert sorted(t for t in got if t in S.REQUIRED) == case["targets"]
    assert a.get("trailer_bit") == case.get("trailer_bit")


def test_required_targets_all_hit():
    hit = set().union(*(set(c["targets"]) for c in CASES))
    assert hit >= S.REQUIRED, sorted(S.REQUIRED - hit)
    assert hit == S.REQUIRED
    assert FIX["total_bytes"] == sum(c["len"] for c in CASES)
    assert len({S.case_id(c) for c in CASES}) == len(CASES)
    assert max(c["len"] for c in CASES) == 719986


def test_fixture_file_is_small():
    assert os.path.getsize(S.FIXTURE) < 256 << 10  # (the limit for a committed file is 1 MiB)


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_model_is_the_oracles_rle1(oracle, analysed, case):
    """image bytes, length and the CRC of every block; a piece's record adds up"""
    _, a = analysed[S.case_id(case)]
    data, image, pieces = a["data"], a["image"], a["pieces"]
    rle, block_ends, in_ends, crcs = oracle.rle1_blocks(data, case["level"])
    assert len(image) == (block_ends[-1] if block_ends else 0)
    assert image == rle
    if S.one_block(len(data), case["level"]):  # (the bound is sufficient, not necessary: a long run is one block too)
        assert len(block_ends) == (1 if data else 0)
    for k, crc in enumerate(crcs):
        assert crc == oracle.crc32_bzip2(data[in_ends[k - 1] if k else 0:in_ends[k]])
    assert (in_ends[-1] if in_ends else 0) == len(data)
    assert len(pieces) == (len(data) + S.PIECE - 1) // S.PIECE
    at = 0
    for q, r in enumerate(pieces):
        assert r["img"] == at
        at += r["emitted"]
        if q == 0:
            assert r["rs"] == -1 and r["phase"] is None
        else:
            assert 0 <= r["rs"] < q * S.PIECE
            cont = data[q * S.PIECE] == data[q * S.PIECE - 1]
            assert r["phase"] == ((q * S.PIECE - r["rs"]) % 255 if cont else None)
    assert at == len(image)


def test_the_bound_cases_sit_on_the_bound(oracle, analysed):
    for lv in S.LEVELS:
        fits = analysed["L-limit_level%d" % lv][1]
        over = analysed["L-limit+1_level%d" % lv][1]
        assert len(fits["image"]) == S.limit(lv) and len(over["image"]) == S.limit(lv) + 1
        assert over["data"][:-1] == fits["data"]
        assert S.one_block(len(fits["data"]), lv) and not S.one_block(len(over["data"]), lv)
        assert oracle.rle1_blocks(over["data"], lv)[1] == [S.limit(lv), S.limit(lv) + 1]
    assert S.limit(9) * 4 // 5 + 1 == 719985


def test_trailer_is_found_by_its_magic(oracle):
    for n in (0, 1, 7, 100):
        z, st = oracle.encode(S.text(n, n), 9, with_stats=True)
        tb = S.trailer_bit(z)
        assert 8 * len(z) - 7 <= tb + 80 <= 8 * len(z)
        assert tb >= 32 and (n > 0 or tb == 32)


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_named_fault_changes_some_case(analysed, mutation):
    changed = None
    for c in sorted(CASES, key=lambda c: c["len"]):
        _, a = analysed[S.case_id(c)]
        if S.front_end(a["data"], (mutation,))[0] != a["image"]:
            changed = S.case_id(c)
            break
    assert changed, "no committed case tells the front end from the fault %r" % mutation
