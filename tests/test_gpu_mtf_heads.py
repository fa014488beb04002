"""GPU tests of the MTF stage on the run heads of the last column (k_mtf_heads_mark / k_mtf_heads_pack, the MTF kernels
on (H, m) and the ZLE kernels' load through the head bitmap: csrc/k_mtf.hip).

Column cases go through bz_gpu_debug_mtf -- the stage alone on columns given by the host -- and are compared with the
oracle's MTF + ZLE of the same column (`oracle.mtf_zle(col, [(i + 1) % n ...])` reads `col[sa[i] - 1] = col[i]`): symbol
stream, count, bytes in use and symbol counts.  The shapes are those where the kernels branch: the 8192-position tile
of the head kernels and of ZLE, the 512-head chunk, the group of 32 chunks (16384 heads), the rank kernel's instances
(<= 96 symbols, more; batches of at most 16 blocks, more), and the head fraction of 3/4 above which a block stays in
the form with one rank per position.  Whole-encoder cases run in child processes, because
BZ_MTF_HEADS and BZ_FUSED_ZLE are read once per process."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, product

pytestmark = pytest.mark.gpu

TILE = 8192  # kSortTile: positions per tile of k_mtf_heads_* and the ZLE kernels
FORMS = (1, 0)  # heads: the collapsed form, and the form with one rank per position


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 24)
    yield e
    e.close()


def want(oracle, col):
    n = len(col)
    sym, freq, _, in_use = oracle.mtf_zle(col, [(i + 1) % n for i in range(n)])
    return sym, len(sym), in_use, list(freq)


def check(eng, oracle, cols, forms=FORMS):
    cols = [bytes(c) for c in cols]
    exp = [want(oracle, c) for c in cols]
    for heads in forms:
        got = eng.debug_mtf(cols, heads=heads)
        for i, (g, w) in enumerate(zip(got, exp)):
            assert g[1] == w[1], ("mtf_count", heads, i, len(cols[i]))
            assert g[2] == w[2], ("in_use_count", heads, i, len(cols[i]))
            assert g[3] == w[3], ("mtf_freq", heads, i, len(cols[i]))
            assert g[0] == w[0], ("symbols", heads, i, len(cols[i]))


def heads_of(col):
    a = np.frombuffer(bytes(col), dtype=np.uint8)
    return 1 + int(np.count_nonzero(a[1:] != a[:-1]))


def from_runs(syms, lens):
    return np.repeat(np.asarray(syms, dtype=np.uint8), np.asarray(lens)).tobytes()


def head_symbols(rng, m, alphabet):
    """m symbols of `alphabet` (sorted byte values), no two neighbours equal, every one of them used when m allows"""
    k = len(alphabet)
    if k == 1:
        assert m == 1
        return np.asarray(alphabet[:1], dtype=np.uint8)
    idx = np.empty(m, dtype=np.int64)
    idx[0] = rng.integers(k)
    idx[1:] = rng.integers(1, k, size=m - 1)  # a step of 1 .. k-1 around the ring: never the same symbol twice
    idx = np.cumsum(idx) % k
    if m >= k:  # every symbol in use: a stretch that walks the ring once (neighbours differ)
        at = int(rng.integers(0, m - k + 1))
        idx[at:at + k] = (idx[at] + np.arange(k)) % k
        if at + k < m and idx[at + k] == idx[at + k - 1]:
            idx[at + k:] = (idx[at + k:] + 1) % k
    out = np.asarray(alphabet, dtype=np.uint8)[idx]
    assert not np.any(out[1:] == out[:-1])
    return out


def column_with_heads(seed, m, k=40, maxrun=40):
    rng = np.random.default_rng(seed)
    col = from_runs(head_symbols(rng, m, list(range(60, 60 + k))), rng.integers(1, maxrun + 1, size=m))
    assert heads_of(col) == m
    return col


def geometric_column(seed, k, n=60000, p=0.3):
    rng = np.random.default_rng(seed)
    alphabet = sorted(rng.choice(256, size=k, replace=False).tolist())
    if k == 1:
        return bytes(alphabet) * n
    m = int(n * p)
    col = from_runs(head_symbols(rng, m, alphabet), rng.geometric(p, size=m))
    assert len(set(col)) == k
    return col


def fraction_column(seed, n, f, k=36):
    """n positions of which about f n are heads"""
    rng = np.random.default_rng(seed)
    if f >= 1.0:
        return head_symbols(rng, n, list(range(k))).tobytes()
    m = max(1, int(n * f))
    cuts = np.sort(rng.choice(np.arange(1, n), size=m - 1, replace=False))
    lens = np.diff(np.concatenate(([0], cuts, [n])))
    return from_runs(head_symbols(rng, m, list(range(k))), lens)


def test_lengths_one_and_two(eng, oracle):
    check(eng, oracle, [b"a"])
    check(eng, oracle, [b"aa"])
    check(eng, oracle, [b"ab"])
    check(eng, oracle, [b"ba"])


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE + 5])
def test_one_byte_value(eng, oracle, n):
    """m = 1: tiles without a head, one zero run to the end"""
    check(eng, oracle, [b"q" * n])


@pytest.mark.parametrize("n", [512, 513, 16384, 16385])
def test_every_position_a_head(eng, oracle, n):
    col = (b"xy" * (n // 2 + 1))[:n]
    assert heads_of(col) == n
    check(eng, oracle, [col])


@pytest.mark.parametrize("m", [511, 512, 513, 1024, 16383, 16384, 16385, 16896])
def test_exact_head_counts(eng, oracle, m):
    check(eng, oracle, [column_with_heads(m, m)])


@pytest.mark.parametrize("q", [128, 3000, 40000])
def test_dense_threshold(eng, oracle, q):
    """a block with more than 3/4 of its positions heads stays in the form with one rank per position (dense_permille = 750,
    k_mtf_heads_pack): n = 4 q positions with exactly 3 q heads (collapsed), with 3 q + 1 and with
    3 q - 1, alone and as neighbours in one batch"""
    cols = []
    for m in (3 * q, 3 * q + 1, 3 * q - 1):
        rng = np.random.default_rng(q + m)
        lens = np.ones(m, dtype=np.int64)
        lens[rng.choice(m, size=4 * q - m, replace=False)] = 2
        col = from_runs(head_symbols(rng, m, list(range(30, 70))), lens)
        assert len(col) == 4 * q and heads_of(col) == m
        cols.append(col)
        check(eng, oracle, [col], forms=(1,))
    check(eng, oracle, cols, forms=(1,))


def test_runs_at_tile_edges(eng, oracle):
    n = 4 * TILE + 77
    dense = bytearray((b"xy" * (n // 2 + 1))[:n])
    cols = []
    c = bytearray(dense)  # a run that begins on the last position of a tile
    c[TILE - 1:TILE + 30] = b"z" * 31
    cols.append(c)
    c = bytearray(dense)  # a run that ends on the first position of the next tile
    c[TILE - 30:TILE + 1] = b"z" * 31
    cols.append(c)
    c = bytearray(dense)  # a run over three tiles
    c[TILE - 100:2 * TILE + 100] = b"z" * (TILE + 200)
    cols.append(c)
    c = bytearray(dense)  # a run that is exactly one tile; one that ends on a tile's last position
    c[TILE:2 * TILE] = b"z" * TILE
    c[3 * TILE - 9:3 * TILE] = b"w" * 9
    cols.append(c)
    for c in cols:
        check(eng, oracle, [c])


@pytest.mark.parametrize("first", ["smallest", "largest"])
def test_first_symbol(eng, oracle, first):
    """head 0 has rank 0 when the column starts with the smallest byte in use"""
    col = bytearray(column_with_heads(7, 3000, k=50))
    col[0:3] = bytes([min(col) if first == "smallest" else max(col)]) * 3
    check(eng, oracle, [col])


@pytest.mark.parametrize("k", [1, 2, 3, 95, 96, 97, 128, 255, 256])
def test_symbols_in_use(eng, oracle, k):
    """both instances of the rank kernel, SUB = 8 (a batch of one block)"""
    check(eng, oracle, [geometric_column(1000 + k, k)])


@pytest.mark.parametrize("nb", [1, 16, 17])
def test_batch_sizes(eng, oracle, nb):
    """at most kMtfSubBlocks = 16 blocks: eight lanes per chunk; 17: one"""
    ks = (36, 97, 2, 256, 96, 13, 128, 60)
    cols = [geometric_column(2000 + i, ks[i % len(ks)], n=20000 + 997 * i, p=(0.1, 0.33, 0.7)[i % 3]) for i in range(nb)]
    check(eng, oracle, cols)


def test_batch_of_mixed_lengths(eng, oracle):
    cols = [b"k", fraction_column(31, 900000, 0.003), b"ab", fraction_column(32, 100001, 1.0), b"m" * (TILE + 1),
            geometric_column(33, 200, n=30000), fraction_column(34, 900000, 1.0, k=256), b"zz"]
    assert heads_of(cols[3]) == len(cols[3]) and heads_of(cols[6]) == len(cols[6])
    check(eng, oracle, cols, forms=(1,))


@pytest.mark.parametrize("f", [0.003, 0.15, 0.33, 0.68, 1.0])
def test_head_fractions(eng, oracle, f):
    check(eng, oracle, [fraction_column(int(f * 1000), 100003, f)])


# ---- the whole encoder under the default, BZ_MTF_HEADS=0 and BZ_FUSED_ZLE=0 -----------------------------------------
SHAPES = ("C batch17", "D run>2tiles", "C in_use=1", "C in_use=1 (zeros)", "C in_use=97", "C in_use=256", "D run=1 ends",
          "D run=1 starts", "E level=1 len=L+0")


def _shape_cases():
    import encshapes as S
    by_why = {}
    for c in S.load():
        by_why.setdefault(c["why"], c)
    missing = [w for w in SHAPES if w not in by_why]
    assert not missing, "shape cases gone from the fixture: %r" % missing
    return [by_why[w] for w in SHAPES]


def _child(path, text_path):
    import encshapes as S
    pkg = product()
    out = {}
    for c in _shape_cases():
        out[S.case_id(c)] = hashlib.sha256(pkg.compress(S.build(c), c["level"])).hexdigest()
    with open(text_path, "rb") as f:
        text = f.read()
    assert len(text) == 9_000_000
    out["bench text"] = hashlib.sha256(pkg.compress(text, 9)).hexdigest()
    with open(path, "w") as f:
        json.dump(out, f)


@pytest.fixture(scope="module")
def encoder_runs(tmp_path_factory):
    import corpus
    text_path = str(tmp_path_factory.mktemp("mtf_heads_text") / "text.bin")
    with open(text_path, "wb") as f:  # the first 9 000 000 bytes of the bench corpus, made once for the three children
        f.write(corpus.corpus_bytes(9_000_000))
    res = {}
    for name, env in (("default", {}), ("BZ_MTF_HEADS=0", {"BZ_MTF_HEADS": "0"}), ("BZ_FUSED_ZLE=0", {"BZ_FUSED_ZLE": "0"}),
                      # every block collapsed (also those of 256 symbols without runs), and none
                      ("BZ_MTF_DENSE_PERMILLE=1000", {"BZ_MTF_DENSE_PERMILLE": "1000"}),
                      ("BZ_MTF_DENSE_PERMILLE=0", {"BZ_MTF_DENSE_PERMILLE": "0"})):
        path = str(tmp_path_factory.mktemp("mtf_heads") / "out.json")
        e = dict(os.environ)
        e.pop("BZ_MTF_HEADS", None)
        e.pop("BZ_FUSED_ZLE", None)
        e.pop("BZ_MTF_DENSE_PERMILLE", None)
        e.update(env)
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path, text_path], env=e, cwd=ROOT,
                           capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr[-3000:])
        with open(path) as f:
            res[name] = json.load(f)
    return res


def test_encoder_same_bytes_under_all_three_settings(encoder_runs):
    base = encoder_runs["default"]
    assert "bench text" in base and len(base) == len(SHAPES) + 1
    for name, got in encoder_runs.items():
        assert got == base, name


def test_encoder_shapes_give_the_oracle_stream(encoder_runs):
    import encshapes as S
    for c in _shape_cases():
        for name, got in encoder_runs.items():
            assert got[S.case_id(c)] == c["sha256"], (name, S.case_id(c))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    _child(sys.argv[1], sys.argv[2])
