"""CPU tests of the stream forge (tests/bzforge.py): it parses and writes encoder streams byte for byte, its
forged valid streams decode to the intended bytes with libbzip2 and the oracle, and every case family of
tests/test_gpu_decode_forged.py gets the oracle verdict it is built for."""
import bz2
import os

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
                 "g": ["G-300-blocks", "G-three-streams"]}[fam]:
        assert want in names + " ", want


def test_eob_cuts_keep_bytes_only_up_to_12_bits(oracle):
    cs = F.family_b(oracle)
    kept = {int(c.name.split("-")[1][3:]) for c in cs if c.name.startswith("B-eob") and c.data}
    lost = {int(c.name.split("-")[1][3:]) for c in cs if c.name.startswith("B-eob") and c.data == b""}
    assert kept == {9, 10, 11, 12} and lost == {9, 10, 11, 12, 13, 20}
