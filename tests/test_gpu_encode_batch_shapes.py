"""GPU tests of batched bzip2 encoding on the seam cases of tests/batchshapes.py (tests/golden/bz_batch_shapes.json):
k_rle_batch at its piece, wave and lane seams, its tails, its image offsets and the level bound; k_frame_batch at every
phase of the trailer; the sub-batches of the pipeline at ws - 1 .. 2 ws + 1 blocks with empty inputs in between; the
batches without a block and without a one-block input.  Every expected byte is oracle.encode(x, level) of that input
alone; every block's nblock, block_crc and orig_ptr are the oracle's."""
import pytest

import batchshapes as S
from conftest import product

pytestmark = pytest.mark.gpu

CASES = S.load()["cases"]
GUARD = 64
EMPTY9 = bytes.fromhex("425a683917724538509000000000")  # header and trailer, combined CRC 0


def touching_pairs():
    """A ends and B begins with the same run byte, and B begins where A ends (A's length is a multiple of 16)"""
    return [(S.text(901, S.PIECE - 6) + b"\xfa" * 6, b"\xfa" * 7 + S.text(902, 50)),
            (S.text(903, 13) + b"\xfb" * 3, b"\xfb" * 300)]


class Pack:
    """Inputs at 16-byte-aligned offsets behind a lead of 16 bytes.  Every other gap is as short as the alignment allows
    (none at all behind an input whose length is a multiple of 16), the others 16 bytes longer; `touch`: the inputs that
    the next one must touch.  The lead and the gaps hold the bytes that would continue the neighbours' edge runs: the
    first half of a gap the last byte of the input in front of it, the second half the first byte of the input behind it.
    The output lies between two guards of 64 bytes 0xEE."""

    def __init__(self, inputs, touch=()):
        import torch
        self.torch = torch
        self.inputs = inputs
        full = [x for x in inputs if x]
        buf = bytearray([full[0][0] if full else 0x61]) * 16
        self.off = []
        behind = 0x61
        for i, x in enumerate(inputs):
            assert len(buf) % 16 == 0
            self.off.append(len(buf))
            buf += x
            if x:
                behind = x[-1]
            ahead = next((y[0] for y in inputs[i + 1:] if y), 0x61)
            gap = -len(buf) % 16
            if i in touch:
                assert gap == 0 and x and inputs[i + 1] and x[-1] == inputs[i + 1][0]
            elif i % 2 == 0 or i + 1 == len(inputs):
                gap += 16
            buf += bytes([behind]) * ((gap + 1) // 2) + bytes([ahead]) * (gap // 2)
        self.len = [len(x) for x in inputs]
        self.t = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        self.cap = product().encode_batch_bound(self.len)
        self.o = torch.full((GUARD + self.cap + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")

    def encode(self, eng, level):
        o_off, o_len = eng.encode_batch_device(level, self.t.data_ptr(), self.off, self.len, self.o.data_ptr() + GUARD, self.cap)
        self.torch.cuda.synchronize()
        host = self.o.cpu().numpy().tobytes()
        assert host[:GUARD] == b"\xee" * GUARD, "bytes in front of the output"
        out = host[GUARD:]
        end = 0
        for a, n in zip(o_off, o_len):  # input order, multiples of 4 bytes, zeros in the slots' padding
            assert a % 4 == 0 and a == (end + 3) & ~3
            assert out[end:a] == bytes(a - end)
            end = a + n
        slot_end = (end + 3) & ~3
        assert out[end:slot_end] == bytes(slot_end - end)
        assert slot_end <= self.cap
        assert out[slot_end:] == b"\xee" * (self.cap - slot_end + GUARD), "bytes behind the last slot or behind cap"
        return [out[a:a + n] for a, n in zip(o_off, o_len)]


_WANT = {}


def want(oracle, x, level):
    """(stream, block statistics) of the oracle for this input alone, computed once"""
    if (x, level) not in _WANT:
        _WANT[(x, level)] = oracle.encode(x, level, with_stats=True)
    return _WANT[(x, level)]


def figures(st):
    return [(b["nblock"], b["block_crc"], b["orig_ptr"]) for b in st]


def check_streams(oracle, ins, got, level, names=None):
    assert len(got) == len(ins)
    for i, (x, g) in enumerate(zip(ins, got)):
        assert g == want(oracle, x, level)[0], "input %d (%s, %d bytes)" % (i, names[i] if names else "", len(x))


def check_blocks_of_small_batch(oracle, eng, ins, level):
    """after a batch of one-block inputs: all its blocks in input order (an empty input has none)"""
    expect = [f for x in ins for f in figures(want(oracle, x, level)[1])]
    assert figures(eng.block_stats()) == expect


@pytest.fixture(scope="module")
def eng8():
    e = product().GpuEngine(0, 8)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng4():
    e = product().GpuEngine(0, 4)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus():
    """per level: (names, inputs, indices that touch their successor) -- the touching pairs first, then the level's cases"""
    out = {}
    for level in S.LEVELS:
        names, ins, touch = [], [], []
        for a, b in touching_pairs():
            touch.append(len(ins))
            names += ["pair-a", "pair-b"]
            ins += [a, b]
        for c in CASES:
            if c["level"] == level:
                names.append(S.case_id(c))
                ins.append(S.build(c))
        out[level] = (names, ins, touch)
    return out


def reordered(names, ins, touch):
    """the pairs stay in front and in their order; the cases behind them are reversed"""
    k = 2 * len(touch)
    return names[:k] + names[k:][::-1], ins[:k] + ins[k:][::-1], touch


def test_corpus_has_every_case_once(corpus):
    assert sum(len(v[1]) for v in corpus.values()) == len(CASES) + 2 * len(touching_pairs()) * len(S.LEVELS)
    for level, (names, ins, touch) in corpus.items():
        assert len(ins) > 30
        assert any(not S.one_block(len(x), level) for x in ins) and any(len(x) == 0 for x in ins) == (level != 5)


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("level", S.LEVELS)
def test_corpus(eng8, oracle, corpus, level, order):
    """the whole corpus of a level as ONE device call: streams, placement, path counts, and the block figures the engine
    keeps -- those of the last input that took the one-input path"""
    names, ins, touch = corpus[level] if order == "forward" else reordered(*corpus[level])
    got = Pack(ins, touch).encode(eng8, level)
    check_streams(oracle, ins, got, level, names)
    small = [x for x in ins if S.one_block(len(x), level)]
    stats = eng8.batch_stats()
    assert stats[:2] == [len(small), len(ins) - len(small)]
    assert stats[2] == sum(1 for x in small if x) and stats[3] == (stats[2] + 7) // 8
    large = [x for x in ins if not S.one_block(len(x), level)]
    assert figures(eng8.block_stats()) == figures(want(oracle, large[-1], level)[1])


@pytest.mark.parametrize("level", S.LEVELS)
def test_front_end_blocks_are_the_oracles(eng8, oracle, corpus, level):
    """the one-block inputs of a level alone: EVERY block's nblock, block_crc and orig_ptr"""
    names, ins, touch = corpus[level]
    keep = [i for i, x in enumerate(ins) if S.one_block(len(x), level)]
    assert keep[:2 * len(touch)] == list(range(2 * len(touch)))
    ins = [ins[i] for i in keep]
    got = Pack(ins, touch).encode(eng8, level)
    check_streams(oracle, ins, got, level, [names[i] for i in keep])
    assert eng8.batch_stats()[:3] == [len(ins), 0, sum(1 for x in ins if x)]
    check_blocks_of_small_batch(oracle, eng8, ins, level)


def frame_inputs():
    return [S.build(c) for c in CASES if c["family"] == "F" and c["len"]]


@pytest.mark.parametrize("nb", [3, 4, 5, 8, 9])
def test_sub_batches(eng4, oracle, nb):
    """a workspace of 4 blocks: ws - 1, ws, ws + 1, 2 ws and 2 ws + 1 blocks, with empty inputs in front and in between, so
    that no input's number is its block's; then the same with the self-check on"""
    pool = frame_inputs()
    ins = [b""]
    for k in range(nb):
        ins.append(pool[(3 * nb + k) % len(pool)])
        if k % 2 == 1:
            ins.append(b"")
    blocks = [i for i, x in enumerate(ins) if x]
    assert len(blocks) == nb and all(i != k for k, i in enumerate(blocks)) and len(ins) > nb
    got = Pack(ins).encode(eng4, 9)
    check_streams(oracle, ins, got, 9)
    assert eng4.batch_stats() == [len(ins), 0, nb, (nb + 3) // 4]
    check_blocks_of_small_batch(oracle, eng4, ins, 9)
    before = list(eng4.verify_stats().values())
    eng4.set_verify(True)
    try:
        checked = Pack(ins).encode(eng4, 9)
        stats = eng4.batch_stats()
    finally:
        eng4.set_verify(False)
    after = list(eng4.verify_stats().values())
    assert checked == got
    assert stats == [len(ins), 0, nb, (nb + 3) // 4]
    assert after[0] - before[0] == nb and after[1] == before[1] and after[2] == before[2]  # every block checked, nothing redone


def test_all_empty(eng8, oracle):
    ins = [b""] * 5
    assert want(oracle, b"", 9) == (EMPTY9, [])
    assert Pack(ins).encode(eng8, 9) == [EMPTY9] * 5
    assert eng8.batch_stats() == [5, 0, 0, 0]
    assert eng8.block_stats() == []


def test_all_large(eng8, oracle):
    """two inputs of two blocks each at level 1: no one-block input, nothing for the front end"""
    ins = [S.build(next(c for c in CASES if c["name"] == "limit+1_level1")), S.fours(77, 30000, 3)]
    assert [len(want(oracle, x, 1)[1]) for x in ins] == [2, 2]
    got = Pack(ins).encode(eng8, 1)
    check_streams(oracle, ins, got, 1)
    assert eng8.batch_stats() == [0, 2, 0, 0]
    assert figures(eng8.block_stats()) == figures(want(oracle, ins[1], 1)[1])


@pytest.mark.parametrize("layout", ["ssLLss", "sLsLs", "LssL"])
def test_large_neighbours_between_small_inputs(eng8, oracle, layout):
    """the zeroed ranges of the small streams touch the large streams on both sides"""
    large = [S.build(next(c for c in CASES if c["name"] == "limit+1_level1")), S.fours(77, 30000, 3)]
    small = [S.text(31, 33), b"\xfa" * 255 + S.text(32, 4000), S.text(33, 1), S.fours(34, 9, 2), S.text(35, 150)]
    ins = [(large if ch == "L" else small).pop(0) for ch in layout]
    got = Pack(ins).encode(eng8, 1)
    check_streams(oracle, ins, got, 1)
    assert eng8.batch_stats()[:3] == [layout.count("s"), 2, layout.count("s")]


def test_host_interface(pkg, oracle):
    """compress_batch (bz_encode_batch) on the P and F families at level 9"""
    ins = [S.build(c) for c in CASES if c["family"] in "PF" and c["level"] == 9]
    assert len(ins) > 50 and b"" in ins
    streams = pkg.compress_batch(ins, level=9)
    check_streams(oracle, ins, streams, 9)
