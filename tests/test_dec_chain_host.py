"""csrc/dec_chain.h on the CPU: the record chain of a .bz2 file (stream header, block, end-of-stream record, next
stream) -- the rules that decide every decoder verdict, shared by the host loop of decode_core and k_dec_chain_batch.

The header is compiled AS IT IS by g++ (plain C++17, no HIP headers).  tests/host_stub/dec_chain_check.cpp drives
chain_open_record / chain_take_block with an in-memory reader over forged byte strings -- trailers at all eight bit
phases, several streams, level digits, the combined CRC with a rotation that wraps, unknown head bytes, inputs cut at
every byte and bit of their end, the clean end, both head-byte paths -- and compares every verdict with a transcription
of the host loop as it stood before the header existed.  It runs plain, and again under AddressSanitizer + UBSan (the
short-read contract: no read behind the input)."""
import os
import subprocess

import pytest

from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "dec_chain_check.cpp")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_chain_rules(tmp_path):
    exe = _build(tmp_path, "dec_chain_check", [])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-500:] + p.stderr[-2000:]


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_chain_rules_under_address_sanitizer(tmp_path):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "dec_chain_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-500:] + p.stderr[-4000:]
