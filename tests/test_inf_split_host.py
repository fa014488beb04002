"""csrc/inf_split.h on the CPU: where a piece of one large Deflate stream may start (the candidate rules the search kernel
runs with one bit offset per lane) and whether it does (the chain the host loop of df_split_sizes runs).

The header is compiled AS IT IS by g++ (plain C++17, no HIP headers).  This file writes streams and the bit positions it
knows about to a file; tests/host_stub/inf_split_check.cpp reads them, checks every listed position, runs EVERY bit
position of every stream through the rules (printing the accepted positions that are not listed: the false candidates the
chain has to survive) and then drives infsplit::chain_next over synthetic streams -- false candidates in first, middle,
last and consecutive positions, empty pieces, a final block in a middle piece, an error in a confirmed piece, more than
four repairs -- against a straightforward serial walk.  It runs plain, and again under AddressSanitizer + UBSan (no read
behind the entry)."""
import os
import random
import subprocess
import zlib

import pytest

import dfforge as F
from conftest import ROOT

STUB = os.path.join(ROOT, "tests", "host_stub")
SRC = os.path.join(STUB, "inf_split_check.cpp")
# malformed() cases whose fault is the block HEADER at the position behind their good first block
HEADER_FAULTS = ("btype3", "stored_len_nlen", "hlit_287", "hdist_31", "repeat_16_first", "run_overshoots", "lit_oversubscribed",
                 "dist_oversubscribed", "lit_incomplete", "dist_incomplete", "dist_single_code_of_length_2", "cl_incomplete",
                 "cl_oversubscribed", "no_end_of_block_code", "cut_in_dynamic_header")
# ... and those whose header is fine (the fault is a code of the block)
HEADER_FINE = ("unused_distance_code", "no_distance_codes")


def words(seed, n):
    r = random.Random(seed)
    w = [bytes(r.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(r.randint(1, 9))) for _ in range(300)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(w) + b" "
    return bytes(out[:n])


def flushed(level, text, step):
    """a raw stream flushed every `step` input bytes, sync and full flushes alternating, and what is known about it: the
    empty stored block of every flush (its LEN field: the four bytes 00 00 FF FF) and the header of the block behind it"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    z, marks = b"", []
    for k, at in enumerate(range(0, len(text), step)):
        z += c.compress(text[at:at + step])
        if at + step < len(text):
            z += c.flush(zlib.Z_SYNC_FLUSH if k % 2 else zlib.Z_FULL_FLUSH)
            assert z[-4:] == b"\x00\x00\xff\xff"
            marks.append(len(z))
    z += c.flush()
    pos = []
    for m in marks:
        head = z[m] & 7                                       # BFINAL, BTYPE of the block behind the flush
        final, btype = head & 1, head >> 1
        assert btype != 3
        # a true non-final stored start: accepted when the header behind its payload can be checked (stored or dynamic;
        # a fixed block has nothing to check, and a stored block in front of one is no candidate)
        pos.append((8 * (m - 4), 1, 0 if btype == 1 else 1))
        if btype == 2:
            pos.append((8 * m, 0, 0 if final else 1))         # dynamic: accepted unless final
        else:
            pos.append((8 * m, 0, 0))                         # a fixed (or stored) header is no dynamic candidate
    return z, pos


def clear_final(stream, bit):
    s = bytearray(stream)
    s[bit >> 3] &= ~(1 << (bit & 7)) & 0xFF
    return bytes(s)


def forged():
    """dfforge layouts whose block positions the forge knows"""
    out = []
    ll = F.balanced([ord(c) for c in "abcdefgh"] + [256, 257, 258], 259)
    dl = F.balanced(list(range(8)), 8)
    s, pos = F.Stream(), []
    for k in range(12):
        at = s.w.bit_length
        kind = k % 4
        if kind == 0:
            s.dynamic(ll, dl).lit(b"abcdefgh" * 5).match(4, 8).eob()
            pos.append((at, 0, 1))
        elif kind == 1:
            s.fixed().lit(F.text(30, k)).eob()
            pos.append((at, 0, 0))
        elif kind == 2:
            s.stored(F.text(100 + k, k))                         # (the empty stored block follows)
            pos.append(((at + 3 + 7) // 8 * 8, 1, 1))
        else:
            s.stored(b"")                                         # an empty stored block
            pos.append(((at + 3 + 7) // 8 * 8, 1, 1))
    at = s.w.bit_length
    s.dynamic(ll, dl, final=True).lit(b"hgfedcba").eob()          # the final block: no candidate
    pos.append((at, 0, 0))
    out.append(("forged_layout", s.raw(), pos))
    at = s.w.bit_length
    # a stored block in front of a fixed one, and a final stored block at the end: their LEN fields are no candidates
    s3 = F.Stream().fixed().lit(b"xyz").eob()
    at = s3.w.bit_length
    s3.stored(b"in front of a fixed block").fixed(final=True).lit(b"abc").eob()
    out.append(("stored_then_fixed", s3.raw(), [((at + 3 + 7) // 8 * 8, 1, 0)]))
    s2 = F.Stream().fixed().lit(b"xyz").eob()
    at = s2.w.bit_length
    s2.stored(b"the end", final=True)
    out.append(("final_stored", s2.raw(), [((at + 3 + 7) // 8 * 8, 1, 0)]))
    # every table shape the decoder accepts, as a non-final block in front of a final one
    first = F.Stream().fixed().lit(F.text(40, 6)).eob().w.bit_length
    for c in F.table_shapes():
        if c.verdict == F.OK and c.stream and (c.stream[0] >> 1) & 3 == 2:
            out.append(("shape_" + c.name, clear_final(c.stream, 0), [(0, 0, 1)]))
            out.append(("shape_final_" + c.name, c.stream, [(0, 0, 0)]))
    for c in F.malformed():
        if c.kind != F.RAW or not c.stream:
            continue
        stored = c.name == "stored_len_nlen"
        at = (first + 3 + 7) // 8 * 8 if stored else first
        if 8 * len(c.stream) <= at:
            continue
        out.append(("bad_" + c.name, c.stream, [(at, 1 if stored else 0, 0)]))                      # as it is: final, rejected
        if c.name in HEADER_FAULTS:
            out.append(("bad_nonfinal_" + c.name, clear_final(c.stream, first), [(at, 1 if stored else 0, 0)]))
        elif c.name in HEADER_FINE:
            out.append(("fine_nonfinal_" + c.name, clear_final(c.stream, first), [(at, 0, 1)]))
    names = {n for n, _, _ in out}
    assert all("bad_nonfinal_" + n in names for n in HEADER_FAULTS) and all("fine_nonfinal_" + n in names for n in HEADER_FINE)
    return out


@pytest.fixture(scope="module")
def streams_file(tmp_path_factory):
    text = words(7, 60000)
    items = []
    for level in (1, 6, 9):
        z, pos = flushed(level, text, 3000)
        assert sum(e for _, m, e in pos if m == 0) >= 5 and sum(e for _, m, e in pos if m == 1) >= 15
        items.append(("zlib_level_%d" % level, z, pos))
    items += forged()
    items.append(("random_bytes", random.Random(5).randbytes(20000), []))
    path = tmp_path_factory.mktemp("inf_split") / "streams.txt"
    with open(path, "w") as f:
        for name, z, pos in items:
            f.write("stream %s %d %d\n%s\n" % (name, len(z), len(pos), z.hex()))
            for p in pos:
                f.write("%d %d %d\n" % p)
    return str(path)


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror"] + flags + [SRC, "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def _check(p):
    lines = p.stdout.strip().splitlines()
    assert p.returncode == 0 and lines and lines[-1] == "ok", p.stdout[-3000:] + p.stderr[-3000:]
    false_hits = {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith("false ")}
    assert "random_bytes" in false_hits
    print("false candidates per stream (the chain survives any number of them):", false_hits)


def test_candidate_rules_and_chain(tmp_path, streams_file):
    exe = _build(tmp_path, "inf_split_check", [])
    _check(subprocess.run([exe, streams_file], capture_output=True, text=True, timeout=300))


def _sanitizer_starts(tmp_path):
    """(a sandbox may forbid the address-space tricks a sanitizer runtime needs: an empty program tells)"""
    src = tmp_path / "empty.cpp"
    src.write_text("#include <cstdio>\nint main() { printf(\"ok\\n\"); return 0; }\n")
    exe = str(tmp_path / "empty_asan")
    p = subprocess.run(["g++", "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return "ok" in p.stdout, p.stderr[-500:]


def test_candidate_rules_and_chain_under_address_sanitizer(tmp_path, streams_file):
    ok, why = _sanitizer_starts(tmp_path)
    if not ok:
        pytest.skip("AddressSanitizer cannot run here: " + why)
    exe = _build(tmp_path, "inf_split_check_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    _check(subprocess.run([exe, streams_file], env=env, capture_output=True, text=True, timeout=600))
