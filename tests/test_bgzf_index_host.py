"""CPU-side checks of the BGZF block index (include/bz2_mi355x.h section 8): the rules of csrc/bgzf_index.h, compiled AS THEY
ARE by g++ (tests/host_stub/bgzf_index_check.cpp) plain and under AddressSanitizer + UBSan on buffers of exactly their
length, and df_bgzf_index_buffer / bgzf_index, which parse on the host and need no GPU.

The expected index never comes from the library: it is the forge's own offsets (tests/bgzfforge.py) and the chain written
there from the contract's words."""
import os
import subprocess

import pytest

import bgzfforge as F
import bgzfref
from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "bgzf_index_check.cpp")


def scan(buf):
    return [p for p in range(len(buf) - 17) if buf[p:p + 4] == b"\x1f\x8b\x08\x04" and buf[p + 10:p + 16] == b"\x06\x00BC\x02\x00"]


def buffers():
    out = [(name, f.file) for name, f in sorted(F.clean_files().items())]
    out.append(("phases", F.phase_file().file))
    out.append(("nested", F.nested()[0].file))
    out += [(name, data) for name, data, _, _, _ in F.chain_faults()]
    out += F.bsize_spoilt()
    head = F.HEAD + b"\x1b\x00"
    for off in range(8):                                        # a header at every offset 0..7, exactly 18 bytes behind it
        out.append(("offset_%d" % off, b"\xAA" * off + head))
    for k in range(1, 18):                                      # the buffer ends inside a header
        out.append(("prefix_%d" % k, b"\x01\x02\x03" + head[:k]))
    out.append(("repeated", head * 20))
    out.append(("zeros", bytes(40)))
    return out


@pytest.fixture(scope="module")
def buffers_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("bgzf_index") / "buffers.txt"
    with open(path, "w") as f:
        for name, buf in buffers():
            f.write("%s %s\n" % (name, buf.hex()))
    return str(path)


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _run(exe, args, env):
    p = subprocess.run([exe] + args, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


def _check(exe, buffers_file, env=None):
    got = {}
    for line in _run(exe, ["scan", buffers_file], env).splitlines():
        name, _, rest = line.partition(":")
        got[name] = [int(x) for x in rest.split()]
    want = {name: scan(buf) for name, buf in buffers()}
    assert got == want
    for off in range(8):
        assert want["offset_%d" % off] == [off]
    for k in range(1, 18):
        assert want["prefix_%d" % k] == []
    assert want["repeated"] == list(range(0, 360, 18))
    assert len(want["nested"]) == 66
    got = {}
    for line in _run(exe, ["chain", buffers_file], env).splitlines():
        name, _, rest = line.partition(":")
        v, c, u = rest.split("|")
        got[name] = ([int(x) for x in c.split()], [int(x) for x in u.split()], int(v))
    assert got == {name: F.chain(buf) for name, buf in buffers()}
    assert _run(exe, ["rules"], env).strip().splitlines()[-1] == "ok"


def test_rules_as_compiled(tmp_path, buffers_file):
    _check(_build(tmp_path, "bgzf_index_check", []), buffers_file)


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_rules_under_address_sanitizer(tmp_path, buffers_file):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "bgzf_index_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check(exe, buffers_file, dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))


# ---- df_bgzf_index_buffer / bgzf_index: on the host, no GPU
@pytest.mark.parametrize("name", sorted(F.clean_files()) + ["phases", "nested"])
def test_index_of_clean_files(pkg, name):
    f = F.phase_file() if name == "phases" else F.nested()[0] if name == "nested" else F.clean_files()[name]
    ix = pkg.bgzf_index(f.file)
    assert (ix.coff, ix.uoff, ix.verdict) == (f.coff, f.uoff, pkg.BZ_OK)
    assert ix.blocks == f.count and ix.total == len(f.data)
    if name == "nested":
        assert ix.blocks == 2         # the 64 headers inside the stored block are never landed on


def test_index_of_the_writers_own_output(pkg, oracle):
    data = F.text(3 * 4093 + 17, 4)
    file, offs, _ = bgzfref.build(oracle, data, 4093, eof=True)
    ix = pkg.bgzf_index(file)
    assert ix.verdict == pkg.BZ_OK and ix.blocks == 5                       # four blocks and the marker
    assert ix.coff == offs + [len(file)]
    assert ix.uoff == [0, 4093, 8186, 12279, len(data), len(data)]


@pytest.mark.parametrize("case", F.chain_faults(), ids=lambda c: c[0])
def test_every_verdict_of_the_chain(pkg, case):
    name, data, v, n, base = case
    ix = pkg.bgzf_index(data)
    assert ix.verdict == v
    assert ix.coff == base.coff[:n + 1] and ix.uoff == base.uoff[:n + 1]     # the clean prefix is still indexed
    assert (ix.coff, ix.uoff, ix.verdict) == F.chain(data)


@pytest.mark.parametrize("case", F.bsize_spoilt(), ids=lambda c: c[0])
def test_a_spoilt_bsize_ends_the_chain(pkg, case):
    name, data = case
    ix = pkg.bgzf_index(data)
    assert ix.verdict != pkg.BZ_OK and ix.blocks in (2, 3)
    assert (ix.coff, ix.uoff, ix.verdict) == F.chain(data)


def test_virtual_offsets_are_inverse(pkg):
    f = F.clean_files()["empty_in_the_middle"]
    ix = pkg.bgzf_index(f.file)
    for k in range(f.count):
        size = f.uoff[k + 1] - f.uoff[k]
        for o in sorted({0, 1, size // 2, size - 1}) if size else ():        # block edges and inside
            u = f.uoff[k] + o
            v = ix.voffset(u)
            assert v == (f.coff[k] << 16 | o)
            assert ix.upos(v) == u
    for u in range(ix.total):                                              # every position of every non-empty block
        assert ix.upos(ix.voffset(u)) == u
    assert ix.voffset(ix.total) == f.coff[-1] << 16 and ix.upos(f.coff[-1] << 16) == ix.total
    assert ix.voffset(300) == f.coff[2] << 16                               # the edge belongs to the block that starts there,
    with pytest.raises(ValueError):                                         # not to the empty block in front of it
        ix.upos(f.coff[1] << 16 | 0 + 1)
    with pytest.raises(ValueError):
        ix.upos((f.coff[0] + 1) << 16)
    with pytest.raises(ValueError):
        ix.voffset(ix.total + 1)
