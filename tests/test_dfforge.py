"""The Deflate forge (tests/dfforge.py) pinned by an independent decoder, Python's zlib, before any GPU sees one of its
streams: every clean stream decodes to exactly the bytes the forge says, every malformed one makes zlib raise -- or, for
the truncations, leaves decompressobj().eof False -- and the bytes zlib hands out in front of the fault (fed byte by byte)
are the forge's prefix.  Where zlib cannot arbitrate the case says so in its note: FDICT set (zlib asks for a dictionary
instead of raising: pinned by the forge's own bookkeeping -- the FLG bit is set, FCHECK is right, no byte is yielded), a
stored block cut short (zlib yields the bytes that are there, the contract none of the block), and two faults that zlib
reports before it has handed out the literals in front of them.

The same holds for the whole corpus built BEHIND A PREAMBLE (dfforge.preamble: the case's blocks are then decoded, in a
split entry, by a wave that started in a later piece), and the preamble's promise -- its mark is the first candidate of
its piece under the rules of csrc/inf_split.h -- is pinned with those rules (tests/host_stub/inf_split_check.cpp --first)."""
import hashlib
import subprocess
import zlib

import pytest

import dfforge as F


def zlib_partial(case):
    """(bytes handed out, the zlib.error or None, eof) with the stream fed one byte at a time"""
    d = zlib.decompressobj(F.WBITS[case.kind])
    out = bytearray()
    try:
        for i in range(len(case.stream)):
            out += d.decompress(case.stream[i:i + 1])
    except zlib.error as e:
        return bytes(out), e, d.eof
    return bytes(out), None, d.eof


CLEAN = F.clean_cases()
MALFORMED = F.malformed_cases() + [F.quirk_like()]
PREAMBLES = ((13, 0), (3, 1))          # what tests/test_gpu_inflate_split_forged.py builds the corpus behind
BEHIND = [F.behind(phase, mode) for phase, mode in PREAMBLES]
CLEAN_BEHIND = [c for clean, _ in BEHIND for c in clean]
MALFORMED_BEHIND = [c for _, bad in BEHIND for c in bad]


def test_the_lists_are_what_the_gpu_tests_expect():
    names = [c.name for c in CLEAN + MALFORMED]
    assert len(set(names)) == len(names)
    assert len(F.copy_grid()) == len(F.COPY_DIST) * len(F.COPY_LEN) == 112
    assert all(c.verdict == F.OK for c in CLEAN) and all(c.verdict in (F.E_DATA, F.E_EOF) for c in MALFORMED)
    assert {c.kind for c in CLEAN} == {F.RAW, F.ZLIB, F.GZIP}
    assert sum(c.verdict == F.E_DATA for c in MALFORMED) >= 40 and sum(c.verdict == F.E_EOF for c in MALFORMED) >= 6


def digest(cases):
    h = hashlib.sha256()
    for c in cases:
        h.update(("%s|%d|%d|%d|%d|%s|" % (c.name, c.kind, len(c.stream), len(c.data), c.verdict, c.note)).encode())
        h.update(c.stream + b"|" + c.data)
    return len(cases), sum(len(c.stream) for c in cases), h.hexdigest()


def test_without_a_preamble_the_builders_give_the_streams_they_always_gave():
    """names, kinds, lengths, verdicts, notes and every byte of stream and data, as the builders gave them before they took
    a stream to begin from (recorded from a run at that commit)"""
    for builder, want in (
            (F.copy_grid, (112, 467205, "974f96d0eb6eff223a9549c9bd7ed39d838c5e47569d386dfb433dd736ce3f37")),
            (F.copy_chains, (4, 150, "3a8562e06bdc460d2877455ec9ea4840c93fff91a9744c7a793221078defe449")),
            (F.copy_residues, (32, 3136, "f4e998835caa9fddc41328c64eb92d3d413ebf55a8e869023b6a7143a7136720")),
            (F.table_shapes, (13, 66557, "8daaa25629ee5ac2d6c9c5c0555cbddeca3e99a9fb15a78d86473bfd3dec30be")),
            (F.containers, (44, 14033, "838577b760508868b87e952d02ca18ac22f6cd6a247137afba14138aa0851b0a")),
            (F.malformed, (28, 1347, "b99a572e9db97aa4e1f3e4a6c0ca2cae0d2d963b4802e7fce9a5cc80284944a3")),
            (F.clean_cases, (184, 544406, "c61265c204af2004010f0617968086e21f5a87ebe1136bba7bf1e41adcc5b7fa")),
            (F.malformed_cases, (49, 8022, "818deae79f78ce575c4f0a7bc62e4ae1d838d21e2ea83f0aa9c23432da56f30a"))):
        assert digest(builder()) == want, builder.__name__
        assert digest(builder(F.Stream)) == want, builder.__name__
    q = F.quirk_like()
    assert (q.name, q.data, q.verdict) == ("match_free_dynamic_block_of_the_reference", b"", F.E_DATA)
    assert hashlib.sha256(q.stream).hexdigest() == "293bb5d1a61dfe3993bc6dc0a1921a344b11d70b2acebab97ce0bef479e6db49"


def test_the_corpus_behind_a_preamble():
    for (phase, mode), (clean, bad) in zip(PREAMBLES, BEHIND):
        assert [c.base for c in clean] == [c.name for c in CLEAN] and [c.base for c in bad] == [c.name for c in MALFORMED]
        assert [(c.kind, c.verdict, c.note) for c in clean + bad] == [(c.kind, c.verdict, c.note) for c in CLEAN + MALFORMED]
        pre = F.preamble(phase, mode)
        assert 1024 <= len(pre.raw()) and len(pre.out) <= 4096
        for c, plain in zip(clean + bad, CLEAN + MALFORMED):
            assert len(c.stream) >= 1024                                      # at least one piece: the entry is split
            # the preamble's output comes first, then the case's own -- but for a fault in the container's header
            header_fault = c.kind != F.RAW and c.verdict == F.E_DATA and plain.data == b"" and not plain.name.endswith("_empty")
            if header_fault:
                assert c.data == b""
            elif plain.name in ("distance_too_far", "distance_at_the_start"):
                assert c.data.startswith(bytes(pre.out)) and c.data.endswith(plain.data)
            elif plain.name.startswith("last_bit_at_"):                       # (as many 9-bit literals as the alignment asks for)
                assert c.data.startswith(bytes(pre.out) + plain.data[:5])
            else:
                assert c.data[:len(pre.out)] == bytes(pre.out) and c.data[len(pre.out):] == plain.data, c.name


def test_a_tail_of_ff_changes_nothing():
    cases = F.tailed([c for c in CLEAN + F.malformed_cases() if c.verdict != F.E_EOF])
    assert len(cases) >= 184 + 40 and {len(c.stream) for c in cases} >= set(F.TAILS)
    for c in cases:
        out, err, eof = zlib_partial(c)
        if c.verdict == F.OK:
            assert err is None and eof and out == c.data, c.name
        else:
            assert err is not None and ("Error -3" in str(err) or c.name == "zlib_fdict_tail"), c.name
            assert (c.data.startswith(out) or out.startswith(c.data)) if c.note else out == c.data, c.name


@pytest.mark.parametrize("case", CLEAN + CLEAN_BEHIND, ids=lambda c: c.name)
def test_clean_streams_decode_to_the_forged_bytes(case):
    d = zlib.decompressobj(F.WBITS[case.kind])
    assert d.decompress(case.stream) == case.data
    assert d.eof
    out, err, eof = zlib_partial(case)
    assert err is None and eof and out == case.data


@pytest.mark.parametrize("case", MALFORMED + MALFORMED_BEHIND, ids=lambda c: c.name)
def test_malformed_streams_are_malformed_for_zlib(case):
    out, err, eof = zlib_partial(case)
    if case.verdict == F.E_EOF:
        assert err is None and not eof
    elif case.name.endswith("zlib_fdict"):
        # zlib's answer is Z_NEED_DICT (2), not a data error: the forge's own bookkeeping pins this one
        assert err is not None and "Error 2" in str(err)
        assert case.stream[1] & 0x20 and int.from_bytes(case.stream[:2], "big") % 31 == 0 and case.data == b""
    else:
        assert err is not None and "Error -3" in str(err)
    if case.note:
        assert case.data.startswith(out) or out.startswith(case.data)
    else:
        assert out == case.data


def test_last_bit_positions():
    """the two streams whose final bit is bit 7 / bit 0 of the last byte really end there: with the padding bits all
    ones, clearing the last code's final bit makes the stream end one code later or not at all"""
    for c in F.table_shapes():
        if c.name.startswith("last_bit_at_"):
            want = int(c.name[-1])
            broken = bytearray(c.stream)
            broken[-1] ^= 1 << want      # (end-of-block is 0000000: its last bit is 0; now it is a 1)
            d = zlib.decompressobj(-15)
            try:
                d.decompress(bytes(broken))
                assert not d.eof
            except zlib.error:
                pass
            if want < 7:
                assert c.stream[-1] >> (want + 1) == 0xFF >> (want + 1)   # only padding above it


def test_cut_points():
    pts = F.cut_points(1000)
    assert pts[:64] == list(range(64)) and pts[-64:] == list(range(936, 1000)) and len(pts) == 64 + 64 + 32
    assert F.cut_points(100) == list(range(100))


# ---- the preamble's promise, by the rules themselves
def first_candidates(tmp_path, items, piece):
    """{name: {piece: (bit, mode)}}: the first position of every piece but the first that csrc/inf_split.h accepts"""
    import test_inf_split_host as H
    exe = str(tmp_path / "inf_split_check")
    if not (tmp_path / "inf_split_check").exists():
        H._build(tmp_path, "inf_split_check", [])
    path = tmp_path / "streams.txt"
    with open(path, "w") as f:
        for name, z in items:
            f.write("stream %s %d 0\n%s\n" % (name, len(z), z.hex()))
    p = subprocess.run([exe, "--first", str(piece), str(path)], capture_output=True, text=True, timeout=600)
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]
    got = {name: {} for name, _ in items}
    for l in lines[:-1]:
        tag, name, k, bit, mode = l.split()
        assert tag == "first"
        got[name][int(k)] = (int(bit), int(mode))
    return got


def promised(s, piece):
    """the marks of a forged stream as {piece: (bit, mode)}"""
    want = {}
    for bit, mode, _ in s.marks:
        assert bit // (8 * piece) not in want and bit // (8 * piece) >= 1
        want[bit // (8 * piece)] = (bit, mode)
    return want


@pytest.mark.parametrize("piece", (1024, 4096))
def test_the_preamble_starts_a_piece_at_every_phase(tmp_path, piece):
    pres = {"p%dm%d" % (phase, mode): F.preamble(phase, mode, piece) for mode, n in ((0, 32), (1, 4)) for phase in range(n)}
    for name, s in pres.items():
        phase, mode = int(name[1:name.index("m")]), int(name[-1])
        (bit, m, at), = s.marks
        assert m == mode and (bit % 32 if mode == 0 else bit % 8 == 0 and bit // 8 % 4) == phase
        assert at < len(s.out) <= 4096 + piece and s.w.bit_length >= 8 * piece
    got = first_candidates(tmp_path, [(name, s.raw()) for name, s in pres.items()], piece)
    for name, s in pres.items():
        assert got[name] == promised(s, piece), name            # exactly the promised position, and no other candidate
    # ... and so it stays with any case behind it
    mark = {(phase, mode): promised(F.preamble(phase, mode), 1024) for phase, mode in PREAMBLES}
    if piece == 1024:
        raw = [c for c in CLEAN_BEHIND + MALFORMED_BEHIND if c.kind == F.RAW]
        got = first_candidates(tmp_path, [(c.name, c.stream) for c in raw], piece)
        for c in raw:
            (k, want), = mark[(int(c.name[1:c.name.index("m")]), int(c.name[c.name.index("m") + 1]))].items()
            assert got[c.name].get(k) == want, c.name


def test_the_cases_of_every_start_phase():
    """what tests/test_gpu_inflate_split_forged.py puts behind all 32 + 4 preambles: a case may depend on where its bits
    fall (no_end_of_block did: seven padding bits of zero are an end-of-block code)"""
    names = ("lengths_up_to_15", "hlit286_hdist30_hclen19", "run_across_hlit_16", "stored_empty", "copy_chain_0", "copy_residue_5",
             "no_distance_codes", "no_end_of_block")
    for mode, n in ((0, 32), (1, 4)):
        for phase in range(n):
            clean, bad = F.behind(phase, mode, names=names)
            assert sorted(c.base for c in clean + bad) == sorted(names)
            for c in clean:
                test_clean_streams_decode_to_the_forged_bytes(c)
            for c in bad:
                test_malformed_streams_are_malformed_for_zlib(c)


def test_source_map_cases(tmp_path):
    cases = F.source_map_cases()
    assert len(cases) == sum(d > k for k in (0, 1, 2) for d in F.COPY_DIST) * len(F.COPY_LEN) == 315
    for c in cases:
        assert zlib.decompress(c.stream, -15) == c.data, c.name
        assert c.pieces == 4 and c.unresolved >= 1 + 1 + 40     # of the match, of its copy, and all of D3's copy of that
    # D, D2 and D3 each start a piece, and the search finds nothing else
    got = first_candidates(tmp_path, [(c.name, c.stream) for c in cases], 1024)
    for c in cases:
        assert len(got[c.name]) == 3 and sorted(got[c.name].values()) == c.marks, c.name
