"""GPU tests of the LHA archive writer (include/bz2_mi355x.h section 12, DESIGN_lzhuf.md section 13).  Every expected byte comes
from tests/lhawrite.py, which tests/test_lhawrite.py and tests/test_lha_write_host.py pin: member data is the model's stream
(tests/lzhref.py) or the plaintext, headers are the restated fixed shape -- nothing expected comes from the library."""
import contextlib
import ctypes as C
import os

import pytest

import lhaforge as F
import lhawrite as W
from conftest import product

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xEE, 64
SWITCHES = ("BZ_LHA_CRC_PART_KIB", "BZ_LZH_SPLIT_KIB", "BZ_LZH_SPLIT_CAND_BYTES")
CASES = W.load()
CORPUS = {c["name"]: c for c in CASES}


@contextlib.contextmanager
def env(values):
    """the switches are read per call"""
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in old:
        os.environ.pop(k, None)
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def eng():
    e = product().GpuEngine(0, 1)
    yield e
    e.close()


def lib_entries(ents):
    pkg = product()
    return [pkg.LhaEntry(e["name"], e["dir"], e["mtime"], e["attr"], e["os_id"], e["is_dir"]) for e, _ in ents]


def image(ents, gap=0):
    """the inputs at multiples of 16 behind a guard; gap: that many lines between neighbours, which CONTINUE the content in
    front of them (a read past an input's end would change its stream or its CRC) -> (bytes, offsets, lengths)"""
    buf, offs = bytearray([FILL]) * GUARD, []
    for _, plain in ents:
        offs.append(len(buf) - GUARD)
        buf += plain
        pad = -len(plain) % 16 + 16 * gap
        if gap and plain:   # the input goes on with its own smallest period: a match at its end could grow into the gap
            period = next(p for p in range(1, len(plain) + 1) if plain[p:] == plain[:-p])
            for _ in range(pad):
                buf.append(buf[-period])
        else:
            buf += bytes([FILL]) * pad
    return buf, offs, [len(p) for _, p in ents]


def rows(idx, arc_index):
    """an LhaIndex's records in the fields of lhaforge.FIELDS + id"""
    return [[getattr(r, f) for f in F.FIELDS] + [bytes(r.method_id).hex()] for r in idx._records[:len(idx)]]


def write_device(eng, ents, method, level, want, gap=0, short=True):
    """one device call between guards of 64 bytes of 0xEE with cap exactly the archive's length; capacity one byte short
    first; nothing written outside [0, out_len) -> (archive, LhaIndex)"""
    import torch
    pkg = product()
    buf, offs, lens = image(ents, gap)
    t = torch.frombuffer(buf + bytearray(16), dtype=torch.uint8).cuda()
    d_in = t.data_ptr() + GUARD
    assert d_in % 16 == 0
    cap = len(want)
    o = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    es = lib_entries(ents)
    if short:
        with pytest.raises(pkg.CompressionError) as ei:
            eng.lha_write_device(d_in, offs, lens, es, o.data_ptr() + GUARD, cap - 1, method, level)
        assert ei.value.code == pkg.BZ_E_CAPACITY
        torch.cuda.synchronize()
        assert bool((o == FILL).all())
    try:
        n, idx = eng.lha_write_device(d_in, offs, lens, es, o.data_ptr() + GUARD, cap, method, level)
    finally:
        torch.cuda.synchronize()
        host = o.cpu().numpy().tobytes()
    assert host[:GUARD] == bytes([FILL]) * GUARD and host[GUARD + n:] == bytes([FILL]) * (len(host) - GUARD - n)
    return host[GUARD:GUARD + n], idx


def check(eng, case, method, level, gap=0):
    pkg = product()
    ents = W.entries(case)
    want, table, st = W.build(case, method, level)
    got, idx = write_device(eng, ents, method, level, want, gap)
    stats = eng.lha_write_stats()
    where = (case["name"], method, level)
    assert len(got) == len(want), where
    assert got == want, where
    assert rows(idx, None) == [F.row(m) for m in table], where
    assert rows(idx, None) == rows(pkg.lha_index(got), None) and pkg.lha_index(got).fault == pkg.BZ_OK, where
    assert [(m.name, m.directory) for m in idx] == [(e["name"], e["dir"]) for e, _ in ents], where
    assert stats[:7] == st, where
    assert stats[7] >= 1
    return got


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_every_case_of_the_corpus(eng, name):
    case = CORPUS[name]
    with env(case.get("env", {})):
        for method, level in W.combos(case):
            check(eng, case, method, level)


def test_the_large_cases_at_the_default_part_size(eng):
    for name in ("L_text", "L_stored"):
        case = CORPUS[name]
        assert case["env"] == {"BZ_LHA_CRC_PART_KIB": "4"}
        for method, level in W.combos(case):
            with env({}):
                check(eng, case, method, level)


@pytest.mark.parametrize("name", ["P_lens", "R_tie", "M_mix"])
def test_inputs_with_gaps_between_them(eng, name):
    case = CORPUS[name]
    for method, level in W.combos(case):
        if level == 1:
            check(eng, case, method, level, gap=1 + method % 2)


def test_round_trip_on_the_device_without_the_host(eng):
    """the written archive goes into the reader as it lies in HBM"""
    import torch
    pkg = product()
    for name, method, level in (("M_mix", 5, 2), ("M_mix", 7, 1), ("R_kinds", 4, 0), ("L_text", 5, 2), ("L_stored", 0, 1), ("H_dir", 6, 2)):
        case = CORPUS[name]
        ents = W.entries(case)
        want, table, _ = W.build(case, method, level)
        buf, offs, lens = image(ents)
        t = torch.frombuffer(buf + bytearray(16), dtype=torch.uint8).cuda()
        arc = torch.full((len(want) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        n, idx = eng.lha_write_device(t.data_ptr() + GUARD, offs, lens, lib_entries(ents), arc.data_ptr(), len(want), method, level)
        assert n == len(want)
        need = sum((len(p) + 15) & ~15 for _, p in ents) + 16
        for prefill in (0x20, -1):
            o = torch.full((need,), FILL, dtype=torch.uint8, device="cuda")
            o_off, o_len, ver = eng.lha_read_device(arc.data_ptr(), n, idx, o.data_ptr(), need, None, prefill)
            torch.cuda.synchronize()
            host = o.cpu().numpy().tobytes()
            assert ver == [pkg.BZ_OK] * len(ents), (name, prefill)
            assert [host[a:a + k] for a, k in zip(o_off, o_len)] == [p for _, p in ents], (name, prefill)
            assert eng.lha_read_stats()[5] == 0


def test_the_host_forms(eng):
    pkg = product()
    for name, method, level in (("M_mix", 5, 2), ("M_mix", 0, 0), ("H_dir", 7, 1), ("R_tie", 4, 1), ("M_none", 5, 2), ("M_dirs", 5, 1),
                                ("M_dirs", 0, 0)):
        case = CORPUS[name]
        ents = W.entries(case)
        want = W.build(case, method, level)[0]
        assert pkg.lha_compress(list(zip(lib_entries(ents), [p for _, p in ents])), method, level) == want, (name, method, level)
        recs, keep = pkg._lha_entries(lib_entries(ents))
        k = len(ents)
        ins = (C.c_char_p * max(k, 1))(*[p for _, p in ents])
        lens = (C.c_size_t * max(k, 1))(*[len(p) for _, p in ents])
        out, n = C.POINTER(C.c_uint8)(), C.c_size_t(0)
        assert pkg.lib().bz_lha_write_buffer(method, level, 0, ins, lens, recs, k, C.byref(out), C.byref(n)) == pkg.BZ_OK
        try:
            assert C.string_at(out, n.value) == want, (name, method, level)
        finally:
            pkg.lib().bz_free(out)
    arc = pkg.lha_compress([("a.txt", b"hello " * 50), (pkg.LhaEntry("b", "docs\xff".encode("latin-1"), 7), b"x")])
    assert pkg.lha_extract(arc) == [(b"hello " * 50, pkg.BZ_OK), (b"x", pkg.BZ_OK)]
    idx = pkg.lha_index(arc)
    assert [m.method for m in idx] == [b"-lh5-", b"-lh0-"] and idx[1].directory == b"docs\xff" and idx[1].mtime == 7


def test_no_members_and_only_directories_on_the_device(eng):
    for name in ("M_none", "M_dirs"):
        case = CORPUS[name]
        for method, level in W.combos(case):
            got = check(eng, case, method, level)
            assert got[-1] == 0 and (name != "M_none" or got == b"\0")
