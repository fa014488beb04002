"""csrc/dev_buf.h on the CPU: DevBuf owns its device memory (destructor, move only) and ensure() keeps its allocation
policy (one eighth + 256 bytes of slack, the exact size when that is refused, free before grow).

The header is compiled AS IT IS by g++ with -DBZ_HOST_PIPELINE_TEST, which takes the HIP calls from
tests/host_stub/hip_shim.h: "device memory" is malloc, the shim counts the blocks that are live and can refuse the
next N hipMalloc calls.  tests/host_stub/devbuf_check.cpp checks every rule and exits non-zero at the first one that
fails; it runs plain, and again under AddressSanitizer + UBSan with leak detection (a block the destructor forgets, or
frees twice, is then the sanitizer's finding as well)."""
import os
import subprocess

import pytest

from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "devbuf_check.cpp")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-DBZ_HOST_PIPELINE_TEST", "-I", STUB] + flags + \
          [SRC, "-o", exe, "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_devbuf_rules(tmp_path):
    exe = _build(tmp_path, "devbuf_check", [])
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


def test_devbuf_rules_under_address_sanitizer(tmp_path):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "devbuf_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-500:] + p.stderr[-4000:]
