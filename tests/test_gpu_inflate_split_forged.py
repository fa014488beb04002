"""GPU tests of the decode loop in the form that the pieces of a split entry run (inf_decode<kPiece, ..> in
csrc/k_inflate.hip: the one loop that the one-wave kernel and the BGZF reader instantiate too; DESIGN_deflate.md "One large
stream across many waves") on the whole forged corpus of tests/dfforge.py, and of what the piece form adds to the loop: a
start at any bit, the source map at a piece's start, `reach`, the jump rounds.

The threshold and the piece are 1 KiB here (BZ_DF_INF_SPLIT_KIB=1, BZ_DF_INF_PIECE_KIB=1), the smallest there are: the forged
streams are short, and a tail of 0xFF bytes (a.) or a preamble (b. to e.: dfforge.preamble, whose last block starts at the
first candidate of a later piece) brings each of them to split size.  Expected values: the forge's (data, verdict), pinned
by zlib in tests/test_dfforge.py -- where the preamble's candidates are pinned by csrc/inf_split.h itself -- and for every
entry the result of the one-wave path (split_run of tests/test_gpu_inflate_split.py).  Every test asserts through
deflate_decode_split_stats() that every entry was split: [0] == the number of entries.

The stats: [0] entries split, [1] candidates, [2] pieces confirmed (the first one included), [3] repair rounds, [4] bytes of
the serial tail, [5] bytes whose value the gather brought, [6] jump rounds, [7] launches."""
import math
import random

import pytest

import dfforge as F
from conftest import product
from test_gpu_inflate_split import split_run, window_chain_forged
from test_inf_split_host import HEADER_FAULTS

pytestmark = pytest.mark.gpu

KINDS = (0, 1, 2)
OK, E_DATA, E_EOF = 0, -1, -2
PREAMBLES = ((13, 0), (3, 1))
TABLE_SHAPES = ("lengths_up_to_15", "single_literal_plus_eob", "one_distance_code_of_length_1", "hlit286_hdist30_hclen5",
                "hlit286_hdist30_hclen19", "hclen4_all_zero", "run_across_hlit_16", "run_across_hlit_17", "run_across_hlit_18",
                "stored_65535", "stored_empty", "last_bit_at_7", "last_bit_at_0")       # those of test_gpu_inflate_batch.py
PHASE_CASES = ("lengths_up_to_15", "hlit286_hdist30_hclen19", "run_across_hlit_16", "stored_empty", "copy_chain_0", "copy_residue_5",
               "no_distance_codes", "no_end_of_block")


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def run_cases(eng, monkeypatch, kind, cases, **kw):
    assert cases and all(c.kind == kind and len(c.stream) >= 1024 for c in cases)
    got, st = split_run(eng, monkeypatch, kind, [c.stream for c in cases], [(c.data, c.verdict) for c in cases], 1, split=1, **kw)
    assert st[0] == len(cases), st
    return st


# ---- a. piece 0 runs the corpus: the container header, `head`, every table shape, copy and fault class
@pytest.fixture(scope="module")
def tailed():
    return F.tailed([c for c in F.clean_cases() + F.malformed_cases() if c.verdict != E_EOF])


@pytest.mark.parametrize("kind", KINDS)
def test_piece_0_runs_the_corpus(eng, monkeypatch, tailed, kind):
    cases = [c for c in tailed if c.kind == kind]
    assert len(cases) >= (150, 15, 20)[kind] and {len(c.stream) for c in cases} >= set(F.TAILS)
    assert any(c.verdict == E_DATA for c in cases)
    if kind == 2:
        assert {"gzip_all_tail", "gzip_hcrc_wrong_tail", "gzip_name_tail", "gzip_comment_tail"} <= {c.name for c in cases}
    # (a piece of 0xFF bytes has no candidate: most entries are their first piece alone, which is the point)
    run_cases(eng, monkeypatch, kind, cases, need_split=False)


# ---- b. a later piece runs the corpus
@pytest.fixture(scope="module")
def behind():
    return {pm: F.behind(*pm) for pm in PREAMBLES}


@pytest.mark.parametrize("preamble", PREAMBLES, ids=lambda pm: "p%dm%d" % pm)
@pytest.mark.parametrize("kind", KINDS)
def test_a_later_piece_runs_the_corpus(eng, monkeypatch, behind, kind, preamble):
    clean, bad = behind[preamble]
    # (the reference's match-free dynamic block has no verdict of the forge's own: tests/test_gpu_inflate_batch.py)
    cases = [c for c in clean + bad if c.kind == kind and c.base != "match_free_dynamic_block_of_the_reference"]
    names = {c.base for c in cases}
    if kind == 0:
        assert names >= set(TABLE_SHAPES) | set(HEADER_FAULTS) | {"distance_too_far", "distance_at_the_start"}
    assert sum(c.verdict == E_EOF for c in cases) == (6, 0, 0)[kind]
    st = run_cases(eng, monkeypatch, kind, cases)
    # the first piece ends at the preamble's mark and the piece from there is confirmed -- unless the container's header is
    # the fault, which ends the first piece; no candidate is false, so nothing is repaired
    header_faults = sum(c.kind != 0 and c.verdict == E_DATA and c.data == b"" for c in cases)
    assert header_faults == (0, 4, 8)[kind]
    assert st[2] >= 2 * (len(cases) - header_faults) + header_faults and st[3] == 0 and st[4] == 0, st


# ---- c. every start phase: 32 bit phases of a dynamic header, 4 byte phases of a stored block's LEN
@pytest.fixture(scope="module")
def phases():
    out = {}
    for mode, n in ((0, 32), (1, 4)):
        for phase in range(n):
            clean, bad = F.behind(phase, mode, names=PHASE_CASES)
            assert len(clean + bad) == len(PHASE_CASES)
            out[(phase, mode)] = {c.base: c for c in clean + bad}
    return out


@pytest.mark.parametrize("name", PHASE_CASES)
def test_every_start_phase(eng, monkeypatch, phases, name):
    cases = [by_name[name] for by_name in phases.values()]
    assert len(cases) == 36
    st = run_cases(eng, monkeypatch, 0, cases)
    assert st[2] >= 2 * len(cases) and st[3] == 0 and st[4] == 0, st


# ---- d. the source map at a piece's start
@pytest.fixture(scope="module")
def source_map():
    return F.source_map_cases()


@pytest.mark.parametrize("k", (0, 1, 2))
def test_source_map_at_a_piece_start(eng, monkeypatch, source_map, k):
    cases = [c for c in source_map if c.name.startswith("source_map_k%d_" % k)]
    assert len(cases) == 7 * sum(d > k for d in F.COPY_DIST)
    st = run_cases(eng, monkeypatch, 0, cases)
    # four pieces each (tests/test_dfforge.py: the search finds D, D2, D3 and nothing else), and in them exactly the bytes
    # whose first writer lies in front of their piece are left to the gather
    assert st[2] == 4 * len(cases) and st[3] == 0 and st[4] == 0, st
    assert all(c.unresolved > 0 for c in cases) and st[5] == sum(c.unresolved for c in cases), st


# ---- e. the bound on the jump rounds: every hop lands in an earlier piece, a round doubles what a pointer spans, and the
# round that changes nothing is counted
def jump_bound(st):
    return math.ceil(math.log2(st[2])) + 1


def test_jump_rounds_of_a_distance_1_run(eng, monkeypatch):
    z, data = window_chain_forged()
    got, st = split_run(eng, monkeypatch, 0, [z], [(data, OK)], 1)
    assert st[0] == 1 and st[5] > 0 and 1 <= st[6] <= jump_bound(st), st


def test_jump_rounds_of_a_pointer_to_a_pointer(eng, monkeypatch, source_map):
    c, = [c for c in source_map if c.name == "source_map_k1_d3_l65"]
    st = run_cases(eng, monkeypatch, 0, [c])
    assert st[2] == 4 and st[5] == c.unresolved and 2 <= st[6] <= jump_bound(st), st     # (two hops: at least two rounds)


# ---- f. garbage of split size
@pytest.mark.parametrize("kind", KINDS)
def test_garbage(eng, monkeypatch, kind):
    r = random.Random(31 + kind)
    head = (b"", b"\x78\x9c", F.gzip_wrap(b"", b"")[:10])[kind]          # (a container header that lets the bytes reach the loop)
    entries = [head + r.randbytes(n - len(head)) for n in (1024, 1025, 2049, 5000, 17000, 40000)]
    got, st = split_run(eng, monkeypatch, kind, entries, None, 1, need_split=False, split=1)
    assert st[0] == 6, st
