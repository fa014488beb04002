"""The plain-Python LZHUF model (tests/lzhref.py) against the reference's own vectors (tests/golden/lzh_vectors.json, data
taken from src/lzhuf/encoder.rs and src/lzhuf/mod.rs): its encoder equals the expected streams bit for bit, the offset
conversions hold, and encode followed by decode gives the input back for all four methods."""
import json
import os
import random

import pytest

import lzhref as R
from conftest import GOLDEN, sample

with open(os.path.join(GOLDEN, "lzh_vectors.json")) as f:
    VEC = json.load(f)


def _text(d):
    return d["text"].encode() * d.get("repeat", 1)


@pytest.mark.parametrize("v", VEC["encoder_vectors"], ids=lambda v: v["name"])
def test_encoder_equals_the_reference_vectors(oracle, v):
    fields = [tuple(x) for x in v["fields"]]
    want = R.pack_bits(fields)
    assert want == (oracle.bitwriter_pack(fields) if fields else b"")    # BitWriter<Left> and the flush to a byte
    assert R.encode_fields(_text(v["input"]), v["method"]) == fields
    assert R.encode(_text(v["input"]), v["method"]) == want


def test_offset_conversions():
    cases = VEC["offset_conversions"]["cases"]
    assert len(cases) == 19
    for pos, po, sub in cases:
        assert R.convert_pos(pos) == (po, sub)
        if po > 1:                                   # what the decoder undoes: pos = 1 << (v - 1) | extra
            assert (1 << (po - 1)) | sub == pos
        else:
            assert po == pos and sub == 0


@pytest.fixture(scope="module")
def inputs():
    rng = random.Random(0x26)
    return ([_text(c) for c in VEC["round_trip_inputs"]["cases"]]
            + [sample(1), rng.randbytes(6), rng.randbytes(622), rng.randbytes(0x1_0000), rng.randbytes(0x1_0112),
               rng.randbytes(0x1_2000)])


@pytest.mark.parametrize("method", (R.LH4, R.LH5, R.LH6, R.LH7))
def test_round_trip(oracle, inputs, method):
    for x in inputs:
        z = R.encode(x, method)
        r = R.decode_full(z, method)
        assert (bytes(r.out), r.verdict) == (x, R.OK)
        assert (r.bits + 7) // 8 == len(z) and len(z) * 8 - r.bits < 8
        # a block holds 0xFFFF codes.  (Random bytes are not all literals: in 0x1_0000 of them chance matches of three
        # bytes bring the codes below 0xFFFF, so the reference's two lengths need not give two blocks; the last input does.)
        ncodes = len(oracle.lzss_tokens(x, window=1 << R.DICT_BITS[method], max_match=R.MAX_MATCH))
        assert r.blocks == -(-ncodes // R.BLOCK_CODES)
        if x is inputs[-1]:
            assert r.blocks == 2
        if len(x) > 1000:
            continue
        assert R.decode(z, method, orig_len=len(x))[:2] == (x, R.OK)
        if x:
            assert R.decode(z, method, orig_len=len(x) - 1)[:2] == (x[:-1], R.OK)
            assert R.decode(z, method, orig_len=len(x) + 1)[:2] == (x, R.E_EOF)
