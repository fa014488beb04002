"""The rules of the split LZHUF decoder before any GPU sees them: csrc/lzh_split.h compiled by g++ (plain and under the
address and undefined-behaviour sanitizers) against their Python restatement (tests/lzhsplit.py), the restatement against
the model (tests/lzhref.py), the forged cases against what they were designed for, and named faults of the rules against
the cases."""
import os
import subprocess

import pytest

import lzhforge as F
import lzhref as R
import lzhsplit as S

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_stub")
SRC = os.path.join(STUB, "lzh_split_check.cpp")


@pytest.fixture(scope="module")
def cases():
    return S.cases()


@pytest.fixture(scope="module")
def sized(cases):
    """{name: (candidates behind bit 0, the sizes launch's pieces)} of every case, once"""
    return {c.name: S.sizes(c.stream, c.method, c.orig_len, c.prefill) for c in cases}


# ---- the restatement is the model
def test_one_piece_without_a_stop_is_the_model():
    """lzhsplit.piece from bit 0 with its place known and no stop, against lzhref.decode_full on the forged corpus"""
    n = 0
    for c in F.expand(F.load()):
        if c["shape"] in F.BIG or c["k"] not in (0, 5, 31):
            continue
        s, ol, pf = F.build(c), c.get("orig_len"), c.get("prefill", -1)
        want = R.decode_full(s, c["method"], ol, pf)
        got = S.piece(s, c["method"], 0, None, 0, ol, ol is not None, pf)
        assert (bytes(got.out), got.verdict, got.end, got.blocks, got.literals, got.matches) == \
               (bytes(want.out), want.verdict, want.bits, want.blocks, want.literals, want.matches), F.case_id(c)
        n += 1
    assert n > 200


def test_the_split_decode_of_every_case_is_the_models(cases, sized):
    for c in cases:
        got = S.decode(c.stream, c.method, c.orig_len, c.prefill, cands=sized[c.name][0])
        assert not got.broken and S.same(got, c.model()), c.name


def test_every_true_start_is_a_candidate(cases, sized):
    for c in cases:
        m = c.model()
        # (a block the stream never reaches whole -- behind a fault, or cut by the end -- need not be one)
        reached = [s for s in c.starts if S.header_end(c.stream, s, c.method) is not None]
        assert set(reached) - {0} <= set(sized[c.name][0]), c.name
        assert len(reached) >= min(len(c.starts), m.blocks), c.name


# ---- the cases are what they were designed to be: computed from the rules, never claimed
def test_cases_hit_their_targets(cases, sized):
    by = {c.name: c for c in cases}
    for m in (5, 7):
        c = by["phases_m%d" % m]
        assert {s % 32 for s in c.starts} == set(range(32)) and len(c.starts) > 64
    for name, at in (("d_eq_base", 80), ("d_base_plus_1_prefill", 80)):
        c = by[name]
        cands, prs = sized[name]
        k = 1 + cands.index(c.starts[2])
        assert prs[k].reach == (80 if name == "d_eq_base" else 81) and sum(len(prs[1 + cands.index(s)].out) for s in c.starts[1:2]) + len(prs[0].out) == at
    c = by["d_base_plus_1_strict"]
    r = S.decode(c.stream, c.method)
    assert (r.verdict, len(r.out), r.again) == (S.E_DATA, 80, 1)
    assert S.decode(by["run_ten_blocks"].stream, 5).depth == 9 and len(by["run_ten_blocks"].starts) == 10
    cands, prs = sized["straddle"]
    p = prs[1 + cands.index(by["straddle"].starts[1])]
    assert p.out[0] == -10 and p.out[10] == -10 and p.out[9] == -1          # the source starts in front of the piece and wraps
    cands, prs = sized["lh7_window_two_back"]
    c = by["lh7_window_two_back"]
    p = prs[1 + cands.index(c.starts[2])]
    assert p.out[0] == -65536 and len(prs[0].out) + p.out[0] + len(prs[1 + cands.index(c.starts[1])].out) < len(prs[0].out)
    cands, prs = sized["pending_at_end"]
    assert [len(prs[0].out) % 64, len(prs[1 + cands.index(by["pending_at_end"].starts[1])].out) % 64] == [6, 2]
    for m in (5, 7):
        c = by["false_candidates_m%d" % m]
        cands, prs = sized[c.name]
        first = S.header_end(c.stream, c.starts[1], m)                       # the flat block's first code
        ends = []
        for blk, off in c.expect["images"]:
            at = first + 8 * off
            assert at in cands and at not in c.starts, "the header image is a candidate and no true start"
            assert S.header_end(c.stream, at, m) == at + 16 + 10 + 18 + 2 * R.OFFSET_BITS[m]
            ends.append(prs[1 + cands.index(at)])
        assert ends[0].end < c.starts[2] < ends[1].end                       # the second one's piece runs past the next true start
        assert ends[1].matches == 100
        assert S.decode(c.stream, m, cands=cands).false >= 2
    for name, v in (("bad_header_in_block_k", S.E_DATA), ("distance_fault_in_block_k", S.E_DATA), ("header_cut_by_end", S.E_EOF)):
        m = by[name].model()
        assert m.verdict == v and m.blocks >= 2, name
    assert S.decode(by["distance_fault_in_block_k"].stream, 5).again == 1
    s = by["end_under_16_bits"].stream
    assert 0 < 8 * len(s) - by["end_under_16_bits"].model().bits < 16
    c = by["zero_count_then_junk"]
    m = c.model()
    assert m.verdict == S.OK and [x for x in sized[c.name][0] if x > m.bits], "candidates in the junk behind the zero count"
    want = {"ol_in_piece_0": (17, S.OK), "ol_at_seam": (40, S.OK), "ol_at_second_seam": (97, S.OK), "ol_mid_match": (76, S.OK),
            "ol_at_end": (142, S.OK), "ol_beyond": (142, S.E_EOF), "ol_zero": (0, S.OK), "ol_before_fault": (80, S.OK),
            "ol_behind_fault": (81, S.E_DATA)}
    for name, (n, v) in want.items():
        m = by[name].model()
        assert (len(m.out), m.verdict) == (n, v), name
    assert by["ol_at_seam"].model().bits == by["ol_at_seam"].starts[1] and by["ol_at_second_seam"].model().bits == by["ol_at_seam"].starts[2]
    for m in (4, 5, 6, 7):
        c = by["p_count_max_m%d" % m]
        assert S.header_end(c.stream, c.starts[2], m) is not None
        if m in (5, 7):  # (the same offset_bits, a smaller dictionary: the p-count is one too many there)
            assert S.header_end(c.stream, c.starts[2], m - 1) is None


def test_recorded_prefixes_are_the_models():
    s, rows = S.prefix_results()
    assert len(s) >= 3072
    full = R.decode_full(s, 5)
    assert full.verdict == S.OK and full.blocks >= 5
    _, starts = S.prefix_stream()
    near = {max(0, b // 8 + d) for b in starts for d in (-1, 0, 1, 2, 7)}
    for n in sorted(near | set(range(0, len(s) + 1, 101)) | {len(s), len(s) - 1}):
        assert S.prefix_row(s, n) == rows[n], n
        assert bytes(R.decode_full(s[:n], 5).out) == bytes(full.out[:rows[n][0]])
    assert {r[1] for r in rows} == {S.OK, S.E_EOF}


# ---- named faults of the rules
@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_every_fault_of_the_rules_changes_some_case(cases, sized, mutation):
    assert len(S.MUTATIONS) >= 5
    for c in cases:
        if len(c.stream) > 300:
            continue
        good = S.decode(c.stream, c.method, c.orig_len, c.prefill, cands=sized[c.name][0])
        bad = S.decode(c.stream, c.method, c.orig_len, c.prefill, mut=(mutation,))
        if (sized[c.name][0] != [x for x in S.candidates(c.stream, c.method, (mutation,)) if x > 0] or not S.same(good, bad)
                or (good.chain, good.false, good.broken) != (bad.chain, bad.false, bad.broken)):
            return
    pytest.fail("no case tells the fault %r from the rules" % mutation)


# ---- csrc/lzh_split.h, compiled as it is
@pytest.fixture(scope="module")
def streams_file(tmp_path_factory, cases, sized):
    path = tmp_path_factory.mktemp("lzhsplit") / "streams.txt"
    import random
    rng = random.Random(29)
    extra = [("noise_m5", 5, rng.randbytes(3000)), ("noise_m7", 7, rng.randbytes(3000)), ("empty", 5, b""), ("one_byte", 5, b"\x80")]
    s, _ = S.prefix_stream()
    extra += [("prefix_%d" % n, 5, s[:n]) for n in (len(s), len(s) - 1, 1500, 457, 456, 7)]
    with open(path, "w") as f:
        for c in cases:
            f.write("stream %s %d %s\n" % (c.name, c.method, c.stream.hex() or "-"))
            cands, prs = sized[c.name]
            f.write("ends %s %d %s\n" % (c.name, len(prs), " ".join("%d %d" % (p.end, p.ended) for p in prs)))
        for name, m, s in extra:
            f.write("stream %s %d %s\n" % (name, m, s.hex() or "-"))
    return str(path), extra


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _check(p, cases, sized, extra):
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]
    cand = {l.split()[1]: [int(x) for x in l.split()[2:]] for l in lines if l.startswith("cand ")}
    chain = {l.split()[1]: l.split()[2:] for l in lines if l.startswith("chain ")}
    for c in cases:
        assert [x for x in cand[c.name] if x > 0] == sized[c.name][0], c.name
        assert chain[c.name] == [str(x) for x in S.plain_walk(*sized[c.name])], c.name
    for name, m, s in extra:
        assert cand[name] == S.candidates(s, m), name
    print("candidates in 3 000 bytes of noise:", len(cand["noise_m5"]), "(lh5)", len(cand["noise_m7"]), "(lh7)")


def test_the_header_gives_the_restatements_candidates_and_chain(tmp_path, streams_file, cases, sized):
    exe = _build(tmp_path, "lzh_split_check", [])
    _check(subprocess.run([exe, streams_file[0]], capture_output=True, text=True, timeout=300), cases, sized, streams_file[1])


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_the_header_under_the_sanitizers(tmp_path, streams_file, cases, sized):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "lzh_split_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    _check(subprocess.run([exe, streams_file[0]], env=env, capture_output=True, text=True, timeout=600), cases, sized, streams_file[1])
