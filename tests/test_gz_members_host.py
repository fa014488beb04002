"""CPU-side checks of "every member of a gzip file" (include/bz2_mi355x.h section 6): the candidate rule and the walk's rules
of csrc/gz_members.h, compiled AS THEY ARE by g++ (tests/host_stub/gz_members_check.cpp), and the parameter errors of the new
entry points that never reach a device (those of the device call that need an engine: tests/test_gpu_gz_members.py).

The candidate rule is checked against a scan written here from the issue's words: position p is a candidate iff the four
bytes at p are 1f 8b 08 and a byte without any of the bits 0xE0, all four inside the buffer.  The program runs plain, and
again under AddressSanitizer + UBSan on buffers of exactly their length (nothing at or behind the end is read)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "gz_members_check.cpp")
HEAD = bytes([0x1F, 0x8B, 8])


def scan(buf):
    return [p for p in range(len(buf) - 3) if buf[p:p + 3] == HEAD and not buf[p + 3] & 0xE0]


def buffers():
    out = []
    for off in range(8):                                       # a header at every offset 0..7
        out.append(("offset_%d" % off, b"\xAA" * off + HEAD + b"\x00" + b"\x55" * 9))
    full = HEAD + b"\x08"
    for k in range(1, 5):                                      # the buffer's last 1..4 bytes are a prefix of a header
        out.append(("prefix_%d" % k, b"\x01\x02\x03\x04\x05" + full[:k]))
        out.append(("only_prefix_%d" % k, full[:k]))
    out.append(("flg_all", b"".join(HEAD + bytes([flg]) for flg in range(256))))     # FLG 0x00..0xFF
    out.append(("repeated", (HEAD + b"\x00") * 300))
    out.append(("overlapping", HEAD + HEAD + HEAD + b"\x1F"))   # 1f is a FLG byte without reserved bits
    out.append(("empty", b""))
    out.append(("zeros", bytes(40)))
    return out


@pytest.fixture(scope="module")
def buffers_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("gz_members") / "buffers.txt"
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


def _check(exe, buffers_file, env=None):
    p = subprocess.run([exe, "scan", buffers_file], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    got = {}
    for line in p.stdout.splitlines():
        name, _, rest = line.partition(":")
        got[name] = [int(x) for x in rest.split()]
    want = {name: scan(buf) for name, buf in buffers()}
    assert got == want
    # the scan itself, on the shapes whose answer is known without it
    for off in range(8):
        assert want["offset_%d" % off] == [off]
    for k in range(1, 5):
        assert want["prefix_%d" % k] == ([5] if k == 4 else []) and want["only_prefix_%d" % k] == ([0] if k == 4 else [])
    assert want["flg_all"] == [4 * flg for flg in range(32)]
    assert want["repeated"] == list(range(0, 1200, 4))
    assert want["overlapping"] == [0, 3, 6]
    p = subprocess.run([exe, "walk"], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]


def test_candidate_rule_and_walk(tmp_path, buffers_file):
    _check(_build(tmp_path, "gz_members_check", []), buffers_file)


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_candidate_rule_and_walk_under_address_sanitizer(tmp_path, buffers_file):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "gz_members_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check(exe, buffers_file, dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))


# ---- the ABI without a device
def test_device_entry_point_without_an_engine(pkg):
    """(no engine can be made without a device: the other parameter errors of the device call are asserted with a real one,
    tests/test_gpu_gz_members.py::test_parameter_errors_with_an_engine)"""
    L = pkg.lib()
    n, v = C.c_uint64(7), C.c_int32(7)
    s8 = (C.c_uint64 * 8)()
    t4 = (C.c_double * 4)()
    assert L.df_gpu_decode_members_device(None, None, 0, None, 0, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_gpu_decode_members_device(None, 16, 16, None, 0, C.byref(n), C.byref(v)) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_decode_members_stats(None, s8) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_decode_members_stats(None, None) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_decode_members_timings(None, t4) == pkg.BZ_E_PARAM
    assert L.df_gpu_last_decode_members_timings(None, None) == pkg.BZ_E_PARAM


def test_host_form_parameter_errors_before_the_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    assert L.df_decode_members_buffer(0, b"x", 1, None, C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_members_buffer(0, b"x", 1, C.byref(out), None) == pkg.BZ_E_PARAM
    assert L.df_decode_members_buffer(0, None, 1, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert L.df_decode_members_buffer(0, b"x", 1 << 32, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM               # 4 GiB: before any byte is read
    assert L.df_decode_members_buffer(0, b"x", (1 << 32) + 5, C.byref(out), C.byref(n)) == pkg.BZ_E_PARAM
    assert not out


def test_a_file_of_no_bytes_touches_no_device(pkg):
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(5)
    assert L.df_decode_members_buffer(0, None, 0, C.byref(out), C.byref(n)) == pkg.BZ_OK
    assert bool(out) and n.value == 0        # an empty buffer that bz_free takes
    L.bz_free(out)
    assert pkg.gzip_decompress_members(b"") == (b"", pkg.BZ_OK)
    assert pkg.MultiGZipDecoder().decode_all(b"") == b""


def test_fails_loudly_without_gpu(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is present")
    L = pkg.lib()
    out = C.POINTER(C.c_uint8)()
    n = C.c_size_t(0)
    assert L.df_decode_members_buffer(0, b"\x1f\x8b", 2, C.byref(out), C.byref(n)) == pkg.BZ_E_NOGPU
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.gzip_decompress_members(b"\x1f\x8b")
    assert ei.value.kind == "NoGpu"
    with pytest.raises(pkg.CompressionError) as ei:
        pkg.MultiGZipDecoder().decode_all(b"\x1f\x8b")         # there is no CPU path behind the class either
    assert ei.value.kind == "NoGpu"


def test_names_are_exported(pkg):
    d = pkg.MultiGZipDecoder()
    assert d.KIND == pkg.GZIP and callable(d.next) and callable(d.decode_all)
    assert issubclass(pkg.MultiGZipDecoder, pkg.Deflater) and not issubclass(pkg.MultiGZipDecoder, pkg.GZipDecoder)
    for name in ("MultiGZipDecoder", "gzip_decompress_members"):
        assert name in pkg.__all__
    for name in ("df_gpu_decode_members_device", "df_gpu_last_decode_members_stats", "df_gpu_last_decode_members_timings",
                 "df_decode_members_buffer"):
        assert name in pkg.EXPORTS
    assert len(pkg.GpuEngine.GZIP_MEMBERS_STATS) == 8 and len(pkg.GpuEngine.GZIP_MEMBERS_STAGES) == 4
    with pytest.raises(ValueError):
        pkg.deflate_decompress(b"x", kind=3)                   # every member is an entry point of its own, not a fourth kind
