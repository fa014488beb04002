"""CPU tests of the stream forge (tests/bzforge.py): it parses and writes encoder streams byte for byte, its
forged valid streams decode to the intended bytes with libbzip2 and the oracle, and every case family of
tests/test_gpu_decode_forged.py gets the oracle verdict it is built for."""
import bz2
import os
import time

import numpy as np
import pytest

import bzforge as F
from conftest import GOLDEN, sample


def _seeded(seed, n, k):
    rng = np.random.default_rng(seed)
    return rng.integers(0, k, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("i", [1, 2, 3, 4])
@pytest.mark.parametrize("level", [1, 5, 9])
def test_round_trip_libbzip2(i, level):
    for d in (sample(i), _seeded(i * 10 + level, 150000, 4 + 60 * i), b"", b"a"):
        z = bz2.compress(d, level)
        assert F.write(F.parse(z)) == z


@pytest.mark.parametrize("level", [1, 9])
def test_round_trip_oracle_encoder(oracle, level):
    d = sample(2) + sample(1) + b"x" * 5000
    z = oracle.encode(d, level)
    streams = F.parse(z)
    assert F.write(streams) == z
    # CRCs recomputed from the oracle's decode of each block alone are the stored ones
    for st in streams:
        st.combined_crc = None
        for b in st.blocks:
            b.crc = None
    F.fill_crcs(streams, oracle)
    assert F.write(streams) == z


@pytest.mark.parametrize("i", [1, 2, 3, 4])
def test_round_trip_golden(i):
    with open(os.path.join(GOLDEN, "sample%d.bz2" % i), "rb") as f:
        z = f.read()
    streams = F.parse(z)
    assert len(streams) == (2 if i == 4 else 1)
    assert F.write(streams) == z


def test_canonical_codes_match_oracle(oracle):
    rng = np.random.default_rng(5)
    for _ in range(50):
        lens = [int(x) for x in rng.integers(0, 21, int(rng.integers(3, 259)))]
        if not any(lens):
            continue
        assert F.canonical_codes(lens) == [c[0] if c else None for c in oracle.canonical_codes(lens)]


def test_zle_digits():
    for run in range(1, 3000):
        v, w = 0, 1
        for dg in F.zle_digits(run):
            v += w if dg == F.RUNA else 2 * w
            w <<= 1
        assert v == run


def test_symbols_from_last_column_match_oracle(oracle):
    d = sample(1)[:40000]
    sa = oracle.bwt(d)
    L = bytes(d[(s - 1) % len(d)] for s in sa)
    sym, _, _, _ = oracle.mtf_zle(d, sa)
    assert F.symbols_from_last_column(L) == sym


def test_last_columns_with_cycles(oracle):
    for n, spec in ((1, [1]), (2, [2]), (50, [1, 2, 47]), (4000, [2000, 2000]), (9000, [3, 1, 8996])):
        L, orig = F.last_column_with_cycles(n, spec, 9)
        T = F.lf_map(L)
        assert len(F.cycle_of(T, orig)) == spec[0]
        lens = sorted(len(F.cycle_of(T, p)) for p in set(range(n)))
        assert sum(1 for x in lens if x == spec[0]) >= spec[0]
    L, orig = F.last_column_with_cycles(128 * 700, ("rows", 10), 3)
    cyc = F.cycle_of(F.lf_map(L), orig)
    samples = [i for i, p in enumerate(cyc) if p % 128 == 0]
    gaps = np.diff(samples)
    assert len(cyc) > 120 * 700 and len(samples) >= 10 and gaps.max() >= 10 * 700 - 1


def test_forged_valid_streams_decode_with_libbzip2(oracle):
    """the forged valid cases that keep to libbzip2's rules (a true BWT, lengths 1-20, no hole hit)"""
    seen = 0
    for c in F.all_cases(oracle, "acf"):
        if c.status != 0 or c.data is None or c.name.startswith(("A3", "A4")):
            continue
        assert bz2.decompress(c.z) == c.data, c.name
        assert oracle.decode(c.z) == (c.data, 0), c.name
        seen += 1
    assert seen >= 15


@pytest.mark.parametrize("fam", F.FAMILIES)
def test_family_oracle_verdicts(oracle, fam):
    """every case the GPU test runs gets the verdict it was built for (the over-subscribed tables and the hit hole
    are the oracle's documented deviation: DataError where the reference panics)"""
    cs = F.all_cases(oracle, fam)
    assert cs
    for c in cs:
        got, st = oracle.decode(c.z, c.cap) if c.cap else oracle.decode(c.z)
        if c.no_oracle:  # a block that ends behind four equal bytes: the oracle, like the reference, reads on around
            assert st == F.NO_COUNT, (c.name, st)  # the closed pointer chain until the capacity is used up
            continue
        assert st == c.status, (c.name, st)
        if c.data is not None:
            assert got == c.data, c.name
    names = " ".join(c.name for c in cs)
    for want in {"a": ["A1", "A2-max20", "A3-len21", "A4-incomplete-hole", "A5-oversubscribed-unpicked"],
                 "b": ["B-eob9", "B-eob13", "B-eob20", "al7", "B-tail"],
                 "c": ["C-tables6", "nsel32767", "nsel-1", "C-eob-at-49"],
                 "d": ["D-straddle", "D-run-to-nmax ", "D-lit-to-nmax", "D-digits21", "D-run-before-eob"],
                 "e": ["fixed", "2cycle", "half", "rows10", "mixed", "-rand"],
                 "f": ["orig0", "orig-10+900001", "alpha3", "alpha258", "empty-group16", "level1-100001"],
                 "g": ["G-300-blocks", "G-three-streams"],
                 "h": ["H-edges-sub-wave-group", "H-edges-share2", "H-edges-share14", "H-counts", "H-self-255", "H-period5",
                       "H-ends", "H-staging", "H-no-count-only", "H-no-count-middle", "H-no-count-last", "H-ff-899981"],
                 "i": ["I-grid", "I-pieces-a0", "I-pieces-a1", "I-pieces-a15", "I-wrong-crc-one-piece",
                       "I-wrong-crc-ragged-tile-seam", "I-wrong-crc-slice-seam"]}[fam]:
        assert want in names + " ", want


def test_eob_cuts_keep_bytes_only_up_to_12_bits(oracle):
    cs = F.family_b(oracle)
    kept = {int(c.name.split("-")[1][3:]) for c in cs if c.name.startswith("B-eob") and c.data}
    lost = {int(c.name.split("-")[1][3:]) for c in cs if c.name.startswith("B-eob") and c.data == b""}
    assert kept == {9, 10, 11, 12} and lost == {9, 10, 11, 12, 13, 20}


# ---- families h and i: the RLE1 undo and the block CRC at their tile seams (stage D4) ---------------------------------
def _plain_undo(img):
    """decoder.rs:555-577 byte by byte"""
    out, last, cnt = bytearray(), 0x100, 0
    for b in img:
        if cnt == 4:
            out += bytes([last]) * b
            cnt, last = 0, 0x100
        elif b == last:
            cnt += 1
            out.append(b)
        else:
            last, cnt = b, 1
            out.append(b)
    return bytes(out), cnt == 4


def test_rle1_undo_is_the_plain_state_machine():
    rng = np.random.default_rng(11)
    for _ in range(1500):
        img = rng.integers(0, int(rng.integers(1, 4)), int(rng.integers(1, 200)), dtype=np.uint8).tobytes()
        want = _plain_undo(img)
        assert F.rle1_undo(img) == want, img
        assert F.rle1_ends_in_count(np.frombuffer(img, np.uint8)) == want[1], img
    for img in (b"aaaa\x61", b"aaaa\x00aaaa\x02", b"\xff" * 70001, b"\x04" * 11, b"\x00" * 10, bytes([9, 9, 9, 9, 255]) * 7):
        assert F.rle1_undo(img) == _plain_undo(img)
    t0 = time.perf_counter()
    got = F.rle1_undo(b"\xff" * 899981)
    assert time.perf_counter() - t0 < 1.0
    assert len(got[0]) == 46618965 and got[1] is False and set(got[0]) == {255}


def test_h_i_decode_like_rle1_undo_with_oracle_and_libbzip2(oracle):
    """every status-0 case of the two families: the oracle and libbzip2 (which checks the CRCs with code of its own)
    give the bytes of rle1_undo.  A case libbzip2 cannot take would be listed here with its reason (at most 5)."""
    not_for_libbzip2 = {}
    assert len(not_for_libbzip2) <= 5
    seen = 0
    for c in F.all_cases(oracle, "hi"):
        if c.status != 0:
            continue
        assert c.data == b"".join(F.rle1_undo(im)[0] for im in c.images), c.name
        assert oracle.decode(c.z, c.cap or (8 << 20)) == (c.data, 0), c.name
        if c.name not in not_for_libbzip2:
            assert bz2.decompress(c.z) == c.data, c.name
        seen += 1
    assert seen >= 17


def test_h_no_count_cases_fail_in_libbzip2_behind_the_blocks_in_front(oracle):
    """four equal bytes and no count: libbzip2 rejects the stream (the oracle has no answer: status -100), and what
    it gave out before is the blocks in front, whole -- what the cases expect of the GPU (DESIGN_decode.md)"""
    cs = [c for c in F.family_h(oracle) if c.no_oracle]
    assert len(cs) == 3
    for c in cs:
        d = bz2.BZ2Decompressor()
        got = b""
        with pytest.raises(OSError):
            for i in range(0, len(c.z), 64):
                got += d.decompress(c.z[i:i + 64])
            raise AssertionError("libbzip2 took " + c.name)
        bad = 0 if len(c.images) == 1 else 1
        assert F.rle1_undo(c.images[bad])[1] and c.status == F.E_DATA
        assert c.data == b"".join(F.rle1_undo(im)[0] for im in c.images[:bad]) and got == c.data


def test_h_i_required_targets_and_sizes(oracle):
    for fam in "hi":
        cs = F.all_cases(oracle, fam)
        got = set()
        for c in cs:
            got |= F.hits(c)
        assert F.REQUIRED[fam] <= got, sorted(F.REQUIRED[fam] - got)
    sizes = sorted(sum(len(F.rle1_undo(im)[0]) for im in c.images) for c in F.all_cases(oracle, "hi"))
    assert sizes[-1] <= 64 << 20 and sum(sizes[:-1]) < 64 << 20
    assert len(F.REQUIRED["h"]) == 183 and len(F.REQUIRED["i"]) == 324


def _blocks_in_memory(c, k=0):
    """(memory image of the stream's output with 16 + k bytes in front and 16 behind, [(A, len)] per block)"""
    outs = [F.rle1_undo(im)[0] for im in c.images]
    rng = np.random.default_rng(len(c.z))
    mem = np.concatenate([rng.integers(1, 256, 16 + k, dtype=np.uint8), np.frombuffer(b"".join(outs), np.uint8),
                          rng.integers(1, 256, 32, dtype=np.uint8)])
    at, pos = [], 16 + k
    for o in outs:
        at.append((pos, len(o)))
        pos += len(o)
    return mem, at


def test_tiled_model_equals_rle1_undo_and_its_mutants_are_caught(oracle):
    """a model of the three-step undo (tabulate / compose / replay and flush, tests/bzforge.py tiled_undo) gives
    rle1_undo's bytes on every committed case, and each named mutation of it changes what it gives for at least one
    case: the corpus can tell these errors apart.  (Not a claim about the kernel.)  "staging test uses <" cannot
    change a byte -- a wave at total + shift == 8192 then writes the same bytes directly -- so for it the model's
    record of which waves were staged is what must change."""
    blocks = []
    for c in F.all_cases(oracle, "hi"):
        pos = 0
        for im in c.images:
            want, pending = F.rle1_undo(im)
            blocks.append((len(want), c.name, im, pos & 3, want, pending))
            pos += len(want)
    blocks.sort(key=lambda b: b[0])
    base = {}
    for i, (_, name, im, ph, want, pending) in enumerate(blocks):
        got = F.tiled_undo(im, ph)
        assert got[1] == (F.NO_COUNT if pending else None), name
        if not pending:
            assert got[0] == want, name
        base[i] = got
    for mut in F.RLE_MUTANTS:
        caught = None
        for i, (ln, name, im, ph, want, pending) in enumerate(blocks):
            if ln > 4 << 20:
                break
            if F.tiled_undo(im, ph, mut) != base[i]:
                caught = name
                break
        assert caught, mut


def test_crc_model_equals_crc32_and_its_mutants_are_caught(oracle):
    """the same for the CRC geometry (crc_model): aligned 16-byte pieces, 256-piece tiles, 4096-piece slices"""
    work = []
    for c in F.family_i(oracle):
        mem, at = _blocks_in_memory(c)
        for (A, ln), im in zip(at, c.images):
            work.append((ln, c.name, mem, A))
    work.sort(key=lambda w: w[0])
    for ln, name, mem, A in work:
        assert F.crc_model(mem, A, ln) == oracle.crc32_bzip2(mem[A:A + ln].tobytes()), (name, A, ln)
    for mut in F.CRC_MUTANTS:
        assert any(F.crc_model(mem, A, ln, mut) != F.crc_model(mem, A, ln) for ln, name, mem, A in work[:400]), mut
