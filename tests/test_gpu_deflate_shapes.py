"""GPU tests of the Deflate encoder's block stage on the shape cases of tests/dfshapes.py (run with -m gpu on an MI355X):
k_df_cuts, k_df_block, k_df_offsets / k_df_batch_offsets, k_df_emit, k_df_sums / k_df_batch_wrap through the one-stream
path, the batch path, the BGZF writer and Inflater's Action::Flush.  Expected bytes are always the oracle's (for BGZF
those of tests/bgzfref.py), never the library's; the stats are checked against the forge's cost model."""
import zlib

import pytest

import dfshapes as S
import test_gpu_bgzf as tb
import test_gpu_deflate as td
import test_gpu_deflate_batch as tbatch
from conftest import product

pytestmark = pytest.mark.gpu

CASES = S.load()["cases"]


def fam(letters):
    return [c for c in CASES if c["family"] in letters]


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


_analysed = {}


def analysed(oracle, case):
    key = S.case_id(case)
    if key not in _analysed:
        _analysed[key] = S.analyse(case, oracle)
    return _analysed[key]


def check_stream(pkg, oracle, eng, data, want, blocks, quirk):
    """codes, blocks (bytes, btype, bits) and the stream against the oracle: check() of test_gpu_deflate.py, which
    inflates with zlib, or -- where the stream holds the reference's match-free dynamic block, which zlib refuses --
    the same comparisons and the forge's reader"""
    if not quirk:
        assert td.check(pkg, oracle, eng, data) == want
        return want
    got, tin = td.dev_encode(pkg, eng, data)
    assert (eng.deflate_debug_codes(tin.data_ptr(), len(data)) == oracle.lzss_tokens_raw(data)).all()
    assert [tuple(b[1:4]) for b in eng.deflate_debug_blocks()] == [tuple(b[1:4]) for b in blocks]
    assert got == want
    assert S.read_stream(got, data)[1] == data
    return got


def check_stats(eng, a):
    """deflate_stats() of the last call against the oracle's blocks and the forge's cost model"""
    st = eng.deflate_stats()
    bt = [b[2] for b in a["blocks"]]
    assert (st["blocks"], st["stored"], st["fixed"], st["dynamic"]) == (len(bt), bt.count(0), bt.count(1), bt.count(2))
    assert st["limited_tables"] == S.limited_tables(a)
    assert st["dynamic_without_distances"] == a["quirk"]
    assert st["stream_bytes"] == len(a["stream"])


def one_stream(pkg, oracle, eng, case):
    """codes, blocks and the stream, then the stats"""
    a = analysed(oracle, case)
    check_stream(pkg, oracle, eng, a["data"], a["stream"], a["blocks"], a["quirk"])
    check_stats(eng, a)


@pytest.mark.parametrize("case", fam("T"), ids=S.case_id)
def test_tables_and_header(pkg, oracle, eng, case):
    one_stream(pkg, oracle, eng, case)


@pytest.mark.parametrize("case", fam("H"), ids=S.case_id)
def test_choice_of_block_type(pkg, oracle, eng, case):
    one_stream(pkg, oracle, eng, case)


@pytest.mark.parametrize("case", fam("W"), ids=S.case_id)
def test_code_words_and_emission(pkg, oracle, eng, case):
    one_stream(pkg, oracle, eng, case)


@pytest.mark.parametrize("case", fam("C"), ids=S.case_id)
def test_chain_of_block_starts(pkg, oracle, eng, case, monkeypatch):
    """the chain beside the marking kernel (in pieces from 256 parse tiles on) and behind it"""
    a = analysed(oracle, case)
    loss = [S.BLOCK_MAX - b[1] for b in a["blocks"][:-1]]
    check_stream(pkg, oracle, eng, a["data"], a["stream"], a["blocks"], a["quirk"])
    assert [S.BLOCK_MAX - b[1] for b in eng.deflate_debug_blocks()][:-1] == loss
    check_stats(eng, a)
    monkeypatch.setenv("BZ_DF_CUTS", "after")
    check_stream(pkg, oracle, eng, a["data"], a["stream"], a["blocks"], a["quirk"])
    check_stats(eng, a)


@pytest.mark.parametrize("case", fam("S"), ids=S.case_id)
def test_checksums(pkg, oracle, eng, case):
    """codes, blocks, the raw stream and the stats as for every case; then the trailer against zlib's sums (an
    independent reference) and the containers against the oracle's"""
    one_stream(pkg, oracle, eng, case)
    data = S.build(case)
    z = pkg.deflate_compress(data, pkg.ZLIB)
    g = pkg.deflate_compress(data, pkg.GZIP)
    assert int.from_bytes(z[-4:], "big") == zlib.adler32(data)
    assert int.from_bytes(g[-8:-4], "little") == zlib.crc32(data) and int.from_bytes(g[-4:], "little") == len(data) & 0xFFFFFFFF
    assert z == oracle.deflate_encode(data, oracle.ZLIB)
    assert g == oracle.deflate_encode(data, oracle.GZIP)


@pytest.fixture(scope="module")
def batch_inputs(oracle):
    """-> (inputs, the cost model's one block of each)"""
    ins = [S.build(c) for c in CASES if len(S.build(c)) <= S.BLOCK_MAX]
    ins += [b"\xff" * n for n in (1, 5551, 5552, 5553, 65534)]  # (S on the batch path: k_df_batch_wrap's own sums)
    models = [S.model(oracle, x)[0] for x in ins]
    assert all(len(m) == 1 for m in models)
    return ins, [m[0] for m in models]


@pytest.mark.parametrize("kind", tbatch.KINDS)
def test_batch_path(oracle, eng, batch_inputs, kind):
    """every case of at most 65 535 bytes as an entry of one call: k_df_block<true, false>, k_df_batch_offsets,
    k_df_emit<true>, k_df_batch_wrap"""
    ins, models = batch_inputs
    want = [oracle.deflate_encode(x, kind) for x in ins]
    got = tbatch.check(eng, oracle, ins, kind, want=want)
    for x, g in zip(ins, got):
        if kind == 1:
            assert int.from_bytes(g[-4:], "big") == zlib.adler32(x)
        if kind == 2:
            assert int.from_bytes(g[-8:-4], "little") == zlib.crc32(x)
    st = dict(zip(eng.DEFLATE_BATCH_STATS, eng.deflate_batch_stats()))
    assert st["inputs_batched"] == len(ins) and st["inputs_one_by_one"] == 0
    first = [(w[0] >> 1) & 3 for w in [oracle.deflate_encode(x, 0) for x in ins]]
    assert first == [m["btype"] for m in models]
    assert (st["stored"], st["fixed"], st["dynamic"]) == (first.count(0), first.count(1), first.count(2))
    assert st["limited_tables"] == sum(sum(m["limited"]) for m in models)
    quirks = sum(1 for m in models if m["btype"] == 2 and m["dcodes"] == 0)
    assert st["dynamic_without_distances"] == quirks >= 2


@pytest.mark.parametrize("case", [c for c in fam("THW") if len(S.build(c)) <= S.BGZF_BLOCK], ids=S.case_id)
def test_bgzf_writer(oracle, eng, case):
    """each case alone as a BGZF file: k_df_block<true, true>, whose strict rule replaces the match-free dynamic block
    by a stored one (`T dcodes=0 bgzf stored`) or a fixed one (`T dcodes=0 bgzf fixed`); check() of test_gpu_bgzf.py
    compares the block types and the count of replaced blocks too"""
    data = S.build(case)
    r = tb.check(eng, oracle, data)
    a = analysed(oracle, case)
    assert r.stats[6] == a["quirk"]
    for arm, btype in (("stored", 0), ("fixed", 1)):
        if "T dcodes=0 bgzf %s" % arm in case["targets"]:
            assert r.stats[6] == 1 and r.stats[2:5] == [int(btype == 0), int(btype == 1), 0]
            assert (r.file[18] >> 1) & 3 == btype


@pytest.mark.parametrize("case", fam("H"), ids=S.case_id)
def test_ties_in_a_non_final_block(pkg, oracle, case):
    """Action::Flush closes the tie's block non-final; an empty Finish ends the stream"""
    A = pkg.Action
    data = S.build(case)
    got, want = td._flush_case(pkg, oracle, [(data, A.FLUSH), (b"", A.FINISH)])
    assert got == want
    assert got[0] & 1 == 0 and (got[0] >> 1) & 3 == analysed(oracle, case)["blocks"][0][2]
    got, want = td._flush_case(pkg, oracle, [(data, A.FLUSH), (data, A.FLUSH), (b"", A.FINISH)])
    assert got == want
