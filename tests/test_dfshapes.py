"""CPU tests of the Deflate encoder shape cases (tests/dfshapes.py, tests/golden/df_shapes.json): every committed case
still builds the bytes it was searched with, still hits the targets it claims, round-trips, and is chosen stored /
fixed / dynamic by the restated cost model exactly as the oracle chooses; the cases together hit the required set, and
every case is needed for it -- the fixture can neither drift nor lose a target unnoticed."""
import hashlib
import zlib

import pytest

import dfshapes as S

FIX = S.load()
CASES = FIX["cases"]
READ = [c for c in CASES if c["family"] in "THW"]


@pytest.fixture(scope="module")
def analysed(oracle):
    """hits() of every case that goes through the reader, once"""
    return {S.case_id(c): S.hits(c, oracle) for c in READ}


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_case_is_what_regen_made(case):
    assert hashlib.sha256(S.build(case)).hexdigest() == case["sha256"]


@pytest.mark.parametrize("case", [c for c in CASES if c["family"] in "CS"], ids=S.case_id)
def test_chain_and_checksum_cases_hit_their_targets(oracle, case):
    got, a = S.hits(case, oracle)
    assert sorted(got) == case["targets"]
    # the restated choice of block type is the oracle's here too (hits() asserts it block by block)
    assert [[m["original"], m["fixed"], m["custom"], m["btype"]] for m in a["model"]][:8] == case["blocks"]
    assert [m["btype"] for m in a["model"]] == [b[2] for b in a["blocks"]]


@pytest.mark.parametrize("case", READ, ids=S.case_id)
def test_case_hits_its_targets(oracle, analysed, case):
    got, a = analysed[S.case_id(case)]
    assert sorted(got) == case["targets"]
    assert S.widest(a) == case["widest"]
    # the restated choice of block type is the oracle's, block by block (hits() asserts it against the reader too)
    assert [m["btype"] for m in a["model"]] == [b[2] for b in a["blocks"]]
    assert [[m["original"], m["fixed"], m["custom"], m["btype"]] for m in a["model"]][:8] == case["blocks"]
    # round trip: by the reader (hits() checked it against the input), and by zlib wherever no block has the quirk
    if a["quirk"]:
        with pytest.raises(zlib.error):
            zlib.decompress(a["stream"], -15)
    else:
        assert zlib.decompress(a["stream"], -15) == a["data"]
    # the reader's start bits: block k + 1 starts where the oracle says block k ends
    pos = 0
    for rb, ob in zip(a["read"], a["blocks"]):
        assert rb.start == pos
        pos += ob[3]


def test_required_targets_all_hit_and_every_case_needed():
    hit = set().union(*(c["targets"] for c in CASES))
    assert hit >= S.REQUIRED, sorted(S.REQUIRED - hit)
    assert hit == S.REQUIRED
    for i, c in enumerate(CASES):
        others = set().union(*(x["targets"] for j, x in enumerate(CASES) if j != i))
        assert set(c["targets"]) - others, "%s hits nothing of its own" % S.case_id(c)


def test_strict_rule_falls_both_ways(oracle):
    """the match-free dynamic block becomes stored in one committed case and fixed in another under tests/bgzfref.py"""
    import bgzfref
    arms = {}
    for c in CASES:
        for arm in ("stored", "fixed"):
            if "T dcodes=0 bgzf %s" % arm in c["targets"]:
                arms[arm] = bgzfref.build(oracle, S.build(c))[2]
    assert arms == {"stored": [(0, True)], "fixed": [(1, True)]}


def test_fixture_records_the_widest_code_and_its_phases():
    assert FIX["widest_code_bits"] == max(c["widest"] for c in READ) == S.WIDEST >= S.WIDE_MIN
    assert FIX["three_word_phases"] == list(range(65 - S.WIDEST, 32))
    assert FIX["smallest_hclen"] <= 18


def test_flush_form_of_the_ties_is_chosen_alike(oracle):
    """family H as a non-final block (Action::Flush, then an empty Finish): same type, BFINAL clear, then the empty block"""
    for c in CASES:
        if c["family"] != "H":
            continue
        data = S.build(c)
        one, blocks = S.oracle_blocks(oracle, data)
        flushed, fblocks = S.oracle_blocks(oracle, data, flush=True)
        assert fblocks[0][:3] == blocks[0][:3] and len(blocks) == 1
        assert flushed[0] & 1 == 0 and one[0] & 1 == 1 and (flushed[0] >> 1) & 3 == blocks[0][2]


def test_reader_agrees_with_zlib_on_zlibs_own_streams():
    import random
    r = random.Random(5)
    text = b" ".join(bytes(r.choice(b"abcdefgh") for _ in range(r.randint(1, 7))) for _ in range(6000))
    noise = bytes(r.getrandbits(8) for _ in range(3000))
    for data in (b"", b"a", text, noise, text[:5000] + noise + text[:9000], bytes(70000)):
        for level in (0, 1, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY):
                co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
                z = co.compress(data) + co.flush()
                blocks, back = S.read_stream(z)
                assert back == data == zlib.decompress(z, -15)
                assert not any(b.quirk for b in blocks)


def test_reader_refuses_damage():
    z = zlib.compress(b"hello hello hello hello", 9)[2:-4]
    with pytest.raises(S.ReadError):
        S.read_stream(z[:-2])
    with pytest.raises(S.ReadError):
        S.read_stream(z, expect=b"hello hello hello hellp")


def test_run_coding_restated(oracle):
    """tab_runs on the forms the issue names: the automatic 16(3) and 18(127) reset the count, the symbol stays"""
    assert S.tab_runs([5] * 7) == [(5, 0), (16, 3)]
    assert S.tab_runs([5] * 8) == [(5, 0), (16, 3), (5, 0)]
    assert S.tab_runs([5] * 10) == [(5, 0), (16, 3), (16, 0)]
    assert S.tab_runs([5] * 13) == [(5, 0), (16, 3), (16, 3)]
    assert S.tab_runs([5] * 14) == [(5, 0), (16, 3), (16, 3), (5, 0)]
    assert S.tab_runs([0] * 2 + [1]) == [(0, 0), (0, 0), (1, 0)]
    assert S.tab_runs([0] * 10 + [1]) == [(17, 7), (1, 0)]
    assert S.tab_runs([0] * 11 + [1]) == [(18, 0), (1, 0)]
    assert S.tab_runs([0] * 138 + [1]) == [(18, 127), (1, 0)]
    assert S.tab_runs([0] * 140 + [1]) == [(18, 127), (0, 0), (0, 0), (1, 0)]
    assert S.tab_runs([0] * 141 + [1]) == [(18, 127), (17, 0), (1, 0)]
    assert S.tab_runs([0] * 149 + [1]) == [(18, 127), (18, 0), (1, 0)]


def test_builder_plants_what_it_is_told(oracle):
    """a designed match comes out of the oracle's parse as designed, and the filler around it makes none"""
    b = S.Builder(9)
    b.lits(S.uniform(0, 256, 3000))
    for L, D in ((3, 1), (3, 2), (4, 3), (258, 1), (5, 700), (258, 2999), (17, 20)):
        b.plant(L, D, list(range(256)))
        b.lits(S.uniform(0, 256, 5))
    toks = [(int(l), int(p) + 1) for l, p in oracle.lzss_tokens_raw(bytes(b.out)) if l]
    assert toks == [(3, 1), (3, 2), (4, 3), (258, 1), (5, 700), (258, 2999), (17, 20)]
    d = S.counter(200000)
    assert 0 not in d and not oracle.lzss_tokens_raw(d)[:, 0].any()
