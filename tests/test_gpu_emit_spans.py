"""GPU tests of k_emit_payload's bit spans: a workgroup of 256 lanes builds the bits of its 256 selector groups in LDS
and stores them as whole words; only a span's first and last word are shared, with the header or with the neighbouring
workgroup.  The inputs sit where a span ends against the 256-group seam, where a last group of one symbol shares its
word with two neighbours, where codes are one or two bits long, where they are 17 bits long, and where a block's first
payload word lies in the header's last word at many alignments.  Their parameters are those of tests/encshapes.py
(tests/golden/enc_shapes.json); what each case is for is asserted from the oracle's figures, and every stream is the
oracle's."""
import numpy as np
import pytest

import bzforge
import encshapes as S
from conftest import product

pytestmark = pytest.mark.gpu

G = S.G
WG = 256  # groups per workgroup of k_emit_payload
SPAN_BOUND = WG * G * 17  # bits: no table has a code above 17 bits (kLim), so no span is wider than the kernel's buffer
CASES = {S.case_id(c): c for c in S.load()}

# one block each; the figures beside them are asserted below
SEAM = ["B-norun(1,49,40)-l9", "B-norun(1,50,40)-l9", "B-norun(1,12749,256)-l9", "B-norun(1,12750,256)-l9",
        "B-norun(1,12799,256)-l9", "B-norun(1,12800,256)-l9", "B-norun(1,12848,256)-l9", "B-norun(1,25549,256)-l9",
        "B-norun(1,25550,256)-l9", "B-norun(1,25599,256)-l9", "B-norun(1,25600,256)-l9", "B-norun(1,25649,256)-l9"]
SEAM_SELECTORS = {1, 2, 255, 256, 257, 511, 512, 513}
SHORT = {"mono-fb": ("mono", (0xFB, 80)), "mono-zeros": ("mono", (0x00, 1)), "two-symbols": ("norun", (5, 70000, 2))}
LONG = "F-textmix(2,880000)-l9"
BATCH17 = "C-batch(300,x17)-l1"


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(nb):
        if nb not in made:
            made[nb] = product().GpuEngine(0, nb)
        return made[nb]
    yield get
    for e in made.values():
        e.close()


def _encode(eng, data, level):
    import torch
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cap = (product().encode_bound(len(data)) + 16 + 15) & ~15
    o = torch.empty(cap, dtype=torch.uint8, device="cuda")
    n = eng.encode_device(level, t.data_ptr(), len(data), o.data_ptr(), cap)
    return bytes(o[:n].cpu().numpy())


def _spans(stream):
    """per block of the stream: the bits of each workgroup's span (256 groups under the tables their selectors name)"""
    out = []
    for b in bzforge.parse(stream)[0].blocks:
        sym = np.asarray(b.symbols)
        nsel = (len(sym) + G - 1) // G
        lens = np.asarray(b.lengths)
        sel = np.asarray(b.selectors)[:nsel]
        pad = np.concatenate([sym, np.zeros(nsel * G - len(sym), dtype=sym.dtype)])
        per = lens[np.repeat(sel, G), pad]
        per[len(sym):] = 0
        cost = per.reshape(nsel, G).sum(axis=1)
        out.append([int(cost[i:i + WG].sum()) for i in range(0, nsel, WG)])
    return out


def _check(engines, oracle, data, level, nb=16):
    stream, st = oracle.encode(data, level, with_stats=True)
    assert _encode(engines(nb), data, level) == stream
    return stream, st


def test_seam_cases_cover_the_issue(oracle):
    """(the figures only; the streams are compared below) every selector count round the 256-group seam, and at the
    256/257 seam last groups of 50, 1 and 49 symbols"""
    fig = [CASES[i]["blocks"][0] for i in SEAM]
    assert {f["n_selectors"] for f in fig} == SEAM_SELECTORS
    assert {f["mtf_count"] % G for f in fig if f["n_selectors"] in (256, 257)} >= {0, 1, 49}
    assert {f["mtf_count"] for f in fig} >= {256 * G, 256 * G + 1, 256 * G + 49}


@pytest.mark.parametrize("cid", SEAM)
def test_span_ends_at_the_seam(engines, oracle, cid):
    c = CASES[cid]
    _, st = _check(engines, oracle, S.build(c), c["level"])
    assert len(st) == 1 and {k: int(st[0][k]) for k in ("mtf_count", "n_selectors")} == \
        {k: c["blocks"][0][k] for k in ("mtf_count", "n_selectors")}


@pytest.mark.parametrize("name", sorted(SHORT))
def test_short_codes(engines, oracle, name):
    """one symbol in use (codes of one and two bits, a single short group) and two symbols in use (codes of at most
    three bits: a group is 50 to 150 bits, so most of its words are shared with a neighbour)"""
    gen, args = SHORT[name]
    stream, st = _check(engines, oracle, S.GENS[gen](*args), 9)
    assert int(st[0]["in_use_count"]) == (2 if name == "two-symbols" else 1)
    assert int(st[0]["max_len"]) <= 3
    if name == "two-symbols":
        assert int(st[0]["n_selectors"]) > WG  # more than one workgroup


def test_long_codes(engines, oracle):
    """tables with 17-bit codes, and the block with the most selectors.  Every span stays inside the kernel's buffer,
    which is sized by 256 groups x 50 symbols x 17 bits: there is no second path to reach.  (Groups take the table
    that codes them in the fewest bits, so the spans of these blocks are about half that bound.)"""
    widest = 0
    for cid in (LONG, "B-norun(7,899981,256)-l9"):
        c = CASES[cid]
        stream, st = _check(engines, oracle, S.build(c), c["level"])
        if cid == LONG:
            assert int(st[0]["max_len"]) == 17
        spans = _spans(stream)[0]
        assert len(spans) == (int(st[0]["n_selectors"]) + WG - 1) // WG
        assert max(spans) <= SPAN_BOUND
        widest = max(widest, max(spans))
    assert widest > 100000  # more than 12 KB: a dozen words per lane in the copy, three 16-byte stores


def test_header_alignments(engines, oracle):
    """17 blocks at level 1 through a 17-block engine: the first payload word is the header's last, partial word, at
    many bit offsets"""
    c = CASES[BATCH17]
    stream, st = _check(engines, oracle, S.build(c), c["level"], nb=17)
    assert len(st) == 17
    hb = [int(s["bits"]) - int(s["bits_codes"]) for s in st]  # the bits in front of a block's first code
    assert len({h % 32 for h in hb}) >= 8
