"""csrc/host_call.h on the CPU: the engine lease of the host-to-host calls (one take or create, then exactly one put
or destroy, decided by the call's infrastructure status; the caller's HIP device put back on every path, the failed
creation included) and the batch layout (offsets, total and packing equal to the loops it replaced).  With it
csrc/one_shot.h, the round trip of the calls that make one device call (the bytes a stand-in device call wrote come back,
a failed dec_in / oneshot_out allocation or a failed download leaves *out null and destroys the engine, BZ_E_PARAM parks it
under the LZHUF/LHA settle rule only), and csrc/batch_decode.h, the frame of the batch decoders (the range check as a
table, the outputs' places and `need`, the split entries' reservation, the jump rounds against scripted launchers).

The headers are compiled AS THEY ARE by g++ with -DBZ_HOST_PIPELINE_TEST, which takes the HIP calls from
tests/host_stub/hip_shim.h (four devices).  tests/host_stub/host_call_check.cpp supplies counting stand-ins for the
engine cache and the engine, checks every rule and exits non-zero at the first one that fails; it runs plain, and again as
a stand-alone program under AddressSanitizer + UBSan with leak detection (an engine the lease forgets or ends twice, a
byte packed behind the image, is then the sanitizer's finding as well).  Nothing is loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "host_call_check.cpp")


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-DBZ_HOST_PIPELINE_TEST", "-I", STUB] + flags + \
          [SRC, "-o", exe, "-lpthread"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_host_call_rules(tmp_path):
    exe = _build(tmp_path, "host_call_check", [])
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


def test_host_call_rules_under_address_sanitizer(tmp_path):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "host_call_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-500:] + p.stderr[-4000:]
