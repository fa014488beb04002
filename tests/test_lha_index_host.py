"""The LHA header rules before any GPU sees an archive: csrc/lha_archive.h compiled by g++ into a stand-alone program (plain
and under the address and undefined-behaviour sanitizers) against their Python restatement (tests/lhaforge.py index()) on the
whole forged corpus and on every prefix of one archive per level; named faults of the restatement against named cases; and
bz_lha_index_buffer (the library's export of the same header) against both."""
import ctypes as C
import os
import subprocess

import pytest

import lhaforge as F

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_stub")
SRC = os.path.join(STUB, "lha_archive_check.cpp")
PREFIXES = ("L_level0", "L_level1_ext", "L_level2")


@pytest.fixture(scope="module")
def corpus():
    return {a.name: a for a in F.archives()}


@pytest.fixture(scope="module")
def archive_file(tmp_path_factory, corpus):
    path = tmp_path_factory.mktemp("lha") / "archives.txt"
    extra = [("empty", b""), ("one_zero", b"\0"), ("one_byte", b"\x17"), ("noise", bytes((i * 37 + 11) & 255 for i in range(400)))]
    with open(path, "w") as f:
        for name, a in corpus.items():
            f.write("archive %s %s\n" % (name, a.data.hex() or "-"))
        for name, d in extra:
            f.write("archive %s %s\n" % (name, d.hex() or "-"))
        for name in PREFIXES:
            f.write("prefixes %s %s\n" % (name, corpus[name].data[:700].hex()))
    return str(path), extra


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _check(p, corpus, extra):
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]
    idx = {l.split()[1]: [int(x) for x in l.split()[2:]] for l in lines if l.startswith("index ")}
    rows = {}
    for l in lines:
        if l.startswith("m "):
            w = l.split()
            rows.setdefault(w[1], []).append([int(x) for x in w[3:-1]] + [w[-1]])

    def same(name, data):
        ms, fault, pos = F.index(data)
        assert idx[name] == [fault, pos, len(ms)], name
        assert rows.get(name, []) == [F.row(m) for m in ms], name

    for name, a in corpus.items():
        same(name, a.data)
    for name, d in extra:
        same(name, d)
    n = 0
    for name in PREFIXES:
        d = corpus[name].data[:700]
        verdicts = set()
        for k in range(len(d) + 1):
            same("%s@%d" % (name, k), d[:k])
            verdicts.add(F.index(d[:k])[1])
            n += 1
        assert verdicts == {F.OK, F.E_EOF}, name   # a header or a member's data cut at any byte is BZ_E_EOF, never BZ_E_DATA
    assert n > 1200


def test_the_header_gives_the_restatements_table(tmp_path, archive_file, corpus):
    exe = _build(tmp_path, "lha_archive_check", [])
    _check(subprocess.run([exe, archive_file[0]], capture_output=True, text=True, timeout=300), corpus, archive_file[1])


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_the_header_under_the_sanitizers(tmp_path, archive_file, corpus):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "lha_archive_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    _check(subprocess.run([exe, archive_file[0]], env=env, capture_output=True, text=True, timeout=600), corpus, archive_file[1])


# ---- the restatement is what the forge designed
def test_the_restatement_lists_what_the_forge_wrote(corpus):
    for name, a in corpus.items():
        ms, fault, pos = F.index(a.data)
        assert len(ms) == a.listed, name
        for m, spec, plain in zip(ms, a.specs, a.plains):
            assert m["id"] == spec["id"].encode() and m["level"] == spec["level"], name
            if spec.get("fault") != "stored_unequal":
                assert m["orig_len"] == len(plain), name
        stops = [q.get("fault") for q in a.case["members"] if q.get("fault") in F.STOPS]
        if stops:
            assert fault == F.E_DATA and pos == (ms[-1]["data_off"] + ms[-1]["packed_len"]), name
        elif a.case.get("cut"):
            assert (fault, pos) == (F.E_EOF, ms[-1]["header_off"]), name
        else:
            assert fault == F.OK, name
    ms = F.index(corpus["L_level1_ext"].data)[0]
    d = corpus["L_level1_ext"].data
    assert d[ms[1]["dir_off"]:ms[1]["dir_off"] + ms[1]["dir_len"]] == b"usr\xffshare\xff" and ms[1]["name_len"] == 255


# ---- named faults of the rules
@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_every_fault_of_the_rules_changes_its_case(corpus, mutation):
    assert len(F.MUTATIONS) >= 8
    a = corpus[F.MUTATION_CASE[mutation]]
    good, bad = F.index(a.data), F.index(a.data, (mutation,))
    assert good != bad, "the case %s does not tell the fault %r from the rules" % (a.name, mutation)


# ---- the library's export of the header
def _lib_index(pkg, data):
    idx = pkg.lha_index(data)
    fault = (0, 0) if idx.fault == pkg.BZ_OK else idx.fault
    return idx, fault


def test_bz_lha_index_buffer_is_the_restatement(pkg, corpus):
    for name, a in corpus.items():
        ms, fault, pos = F.index(a.data)
        idx, got = _lib_index(pkg, a.data)
        assert got == (fault, pos) and len(idx) == len(ms), name
        for q, m in zip(idx, ms):
            assert (q.method, q.level, q.packed_len, q.orig_len, q.crc16, q.mtime, q.os_id, q.data_off, q.header_off) == \
                   (m["id"], m["level"], m["packed_len"], m["orig_len"], m["crc16"], m["mtime"], m["os_id"], m["data_off"], m["header_off"]), name
            assert q.name == a.data[m["name_off"]:m["name_off"] + m["name_len"]], name
            assert q.directory == a.data[m["dir_off"]:m["dir_off"] + m["dir_len"]], name
    assert C.sizeof(pkg._LhaMemberRec) == 72


def test_counting_and_a_short_table(pkg, corpus):
    L = pkg.lib()
    d = corpus["M_methods"].data
    n, fault, pos = C.c_size_t(0), C.c_int32(9), C.c_uint64(9)
    assert L.bz_lha_index_buffer(d, len(d), None, 0, C.byref(n), C.byref(fault), C.byref(pos)) == pkg.BZ_OK
    assert (n.value, fault.value) == (16, 0)
    recs = (pkg._LhaMemberRec * 4)()
    assert L.bz_lha_index_buffer(d, len(d), recs, 3, C.byref(n), C.byref(fault), C.byref(pos)) == pkg.BZ_OK
    assert n.value == 16 and recs[2].header_off > 0 and recs[3].header_off == 0 and recs[3].data_off == 0
    assert L.bz_lha_index_buffer(d, len(d), None, 0, None, C.byref(fault), C.byref(pos)) == pkg.BZ_E_PARAM
    assert L.bz_lha_index_buffer(None, 5, None, 0, C.byref(n), C.byref(fault), C.byref(pos)) == pkg.BZ_E_PARAM
    assert L.bz_lha_index_buffer(None, 0, None, 0, C.byref(n), C.byref(fault), C.byref(pos)) == pkg.BZ_OK and n.value == 0
