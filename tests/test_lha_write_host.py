"""The LHA writer's header rules before any GPU lays an archive out: the writer half of csrc/lha_archive.h compiled by g++
into a stand-alone program (plain and under the address and undefined-behaviour sanitizers) against their Python restatement
(tests/lhawrite.py) on every member of the corpus -- header sizes, header bytes, and the assembled archive read back by
lha::index in the same program."""
import os
import subprocess

import pytest

import lhaforge as F
import lhawrite as W

STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_stub")
SRC = os.path.join(STUB, "lha_write_check.cpp")
# entries that have no header at some level: a directory name at level 0, H above 255, an extended header above 65 535
NO_HEADER = [(0, b"n", b"d\xff"), (0, b"x" * 234, b""), (1, b"x" * 65533, b""), (1, b"n", b"d" * 65533), (2, b"x" * 65533, b""),
             (2, b"x" * 40000, b"d" * 25499)]
HAS_HEADER = [(0, b"x" * 233, b""), (1, b"x" * 65532, b"d" * 65532), (2, b"x" * 40000, b"d" * 25498)]


def _hex(b):
    return bytes(b).hex() or "-"


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """the program's input, and what it must print"""
    path = tmp_path_factory.mktemp("lhaw") / "members.txt"
    want = {}
    with open(path, "w") as f:
        for c in W.load():
            ents = W.entries(c)
            for method, level in W.combos(c):
                arc, table, _ = W.build(c, method, level)
                name = "%s/lh%d/l%d" % (c["name"], method, level)
                f.write("archive %s\n" % name)
                for m, (e, _) in zip(table, ents):
                    f.write("member %d %s %s %d %d %d %d %d %d %d %s\n" % (
                        level, _hex(e["name"]), _hex(e["dir"]), e["mtime"], e["attr"], e["os_id"], m["method"], m["packed_len"], m["orig_len"],
                        m["crc16"], _hex(arc[m["data_off"]:m["data_off"] + m["packed_len"]])))
                f.write("end\n")
                want[name] = (arc, table)
        f.write("archive limits\n")
        for level, n, d in NO_HEADER + HAS_HEADER:
            f.write("member %d %s %s 1 2 3 0 0 0 0 -\n" % (level, _hex(n), _hex(d)))
    return str(path), want


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _check(p, want):
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]
    heads, rows, idx = {}, {}, {}
    for l in lines:
        w = l.split()
        if w[0] == "h":
            heads.setdefault(w[1], []).append((int(w[3]), w[4]))
        elif w[0] == "m":
            rows.setdefault(w[1], []).append([int(x) for x in w[3:-1]] + [w[-1]])
        elif w[0] == "index":
            idx[w[1]] = [int(x) for x in w[2:]]
    n = 0
    for name, (arc, table) in want.items():
        got = heads.get(name, [])
        assert len(got) == len(table), name
        for (size, hx), m in zip(got, table):
            h = arc[m["header_off"]:m["data_off"]]
            assert size == len(h) and hx == h.hex(), (name, m["header_off"])
            n += 1
        assert idx[name] == [F.OK, 0, len(table)], name
        assert rows.get(name, []) == [F.row(m) for m in table], name
    assert n > 1000
    lim = heads["limits"]
    assert [s for s, _ in lim[:len(NO_HEADER)]] == [0] * len(NO_HEADER)
    for (size, hx), (level, name, d) in zip(lim[len(NO_HEADER):], HAS_HEADER):
        e = dict(name=name, dir=d, mtime=1, attr=2, os_id=3)
        assert size == W.header_size(level, e) and hx == W.header(level, e, b"-lh0-", 0, 0, 0)[0].hex(), (level, len(name))
    for level, name, d in NO_HEADER:
        assert W.header_size(level, dict(name=name, dir=d)) is None


def test_the_header_writes_the_restatements_bytes(tmp_path, job):
    exe = _build(tmp_path, "lha_write_check", [])
    _check(subprocess.run([exe, job[0]], capture_output=True, text=True, timeout=300), job[1])


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_the_header_under_the_sanitizers(tmp_path, job):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "lha_write_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    _check(subprocess.run([exe, job[0]], env=env, capture_output=True, text=True, timeout=600), job[1])
