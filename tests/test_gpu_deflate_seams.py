"""GPU tests of the one-stream Deflate encoder at its PART SEAMS (run with -m gpu on an MI355X): every case of
tests/golden/df_seams.json (tests/dfseams.py made them: inputs placed at each branch of the hand-over between two parts)
through df_gpu_encode_device for kinds 0, 1 and 2, through the host call, through the Inflater / ZlibEncoder / GZipEncoder
classes for the Flush, Run and dictionary cases, and two of them inside one batch call.

BZ_DF_PART_MIB is read once per process, so ONE child process (BZ_DF_PART_MIB=1 BZ_DF_TRACE=1) runs everything and the
tests only read its records:
  1. the bytes of each path are the oracle's (recorded length and SHA-256; the streaming class piece by piece);
  2. the trace's (pos, kept bytes, bits handed on, blocks) of every part are the seam model's -- without this the forge's
     targets could drift off the library's seams unseen;
  3. after a multi-part call deflate_debug_blocks() describes the last part (its bytes sum to n - pos_last less the
     `skip` literals that went out with the part before, and its first block starts behind them), and deflate_stats()
     counts the oracle's blocks and types over all parts.
Every case that hits a target of family K, Z or B -- every case with a seam -- runs a second time with BZ_DF_CUTS=after
(the block chain behind the marking kernel); tests/dfseams_child.py is the child.

Out of scope: the host-buffer pipeline that overlaps copies with parts; it starts at inputs of 64 MiB."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import dfseams as S
import dfseams_child

pytestmark = pytest.mark.gpu

CASES = S.load()["cases"]
BY_NAME = {c["name"]: c for c in CASES}
FATAL = (124, 134, 137, 139, -6, -9, -11)


class Child:
    def __init__(self, rc, out, err, dump, seconds):
        self.rc, self.out, self.err, self.dump, self.seconds = rc, out, err, dump, seconds
        self.records, self.traces = {}, {}
        for line in out.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                self.records[(r["case"], r["path"])] = r
        key, chunk = None, []
        for line in err.splitlines() + ["dfseams case - path -"]:
            if line.startswith("dfseams case "):
                if key:
                    self.traces[key] = "\n".join(chunk)
                w = line.split()
                key, chunk = (w[2], w[4]), []
            else:
                chunk.append(line)

    def require(self):
        """a child that did not come to its end fails every test of the module"""
        bad = self.rc != 0 or "illegal memory access" in self.err or ("done", "done") not in self.records
        if bad:
            pytest.fail("the child ended with status %s%s\n%s" % (self.rc, " (fatal)" if self.rc in FATAL else "", self.err[-3000:]),
                        pytrace=False)


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    import time
    dump = str(tmp_path_factory.mktemp("dfseams"))
    env = dict(os.environ, BZ_DF_PART_MIB="1", BZ_DF_TRACE="1", DFSEAMS_DUMP=dump)
    env.pop("BZ_DF_CUTS", None)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, os.path.join(S.HERE, "dfseams_child.py")], env=env, capture_output=True,
                           text=True, timeout=420)
        rc, out, err = p.returncode, p.stdout, p.stderr
    except subprocess.TimeoutExpired as e:
        rc, out, err = 124, (e.stdout or b"").decode(errors="replace"), (e.stderr or b"").decode(errors="replace")
    c = Child(rc, out, err, dump, time.time() - t0)
    print("dfseams child: %.1f s, %d records" % (c.seconds, len(c.records)))
    return c


def paths_of(case):
    pieces = case["pieces"]
    after = S.runs_after(case)
    if len(pieces) == 1 and pieces[0][2] == S.FINISH:
        p = [("dev%d" % k, "kind%d" % k) for k in case["kinds"]] + [("host0", "kind%d" % case["kinds"][0])]
        if after:
            p.append(("dev%d-after" % case["kinds"][0], "kind%d" % case["kinds"][0]))
        return p
    if pieces[0][2] == S.RUN:
        return [("run%d" % k, "run%d" % k) for k in case["kinds"]] + (
            [("run%d-after" % case["kinds"][0], "run%d" % case["kinds"][0])] if after else [])
    return [("inflater", "pieces")] + ([("inflater-after", "pieces")] if after else [])


def explain(child, case, path, want_key, oracle):
    """the first byte that differs from the oracle's stream, and the block that holds it"""
    f = S.facts(case, oracle)
    if want_key.startswith("kind"):
        want = oracle.deflate_encode(f.segs[0].data, int(want_key[4:]), f.dict)
        head = {0: 0, 1: 6 if f.dict else 2, 2: 10}[int(want_key[4:])]
    elif want_key == "pieces":
        want, head = f.stream, 0
    else:
        want = oracle.WrapperEncoder(int(want_key[3:]), f.dict).encode_iter(f.segs[0].data, S.RUN)
        head = {1: 6 if f.dict else 2, 2: 10}[int(want_key[3:])]
    got = b""
    i = 0
    while os.path.exists(os.path.join(child.dump, "%s.%s.%d.bin" % (case["name"], path, i))):
        got += open(os.path.join(child.dump, "%s.%s.%d.bin" % (case["name"], path, i)), "rb").read()
        i += 1
    k = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
    bit, where = 8 * head, "behind the last block"
    for si, s in enumerate(f.segs):
        bit = 8 * (head + s.out0)
        for bi, b in enumerate(s.blocks):
            if bit <= 8 * k < bit + b[3]:
                where = "segment %d block %d (type %d, %d bytes, stream bits [%d, %d))" % (si, bi, b[2], b[1], bit, bit + b[3])
            bit += b[3]
    return "%s %s: %d bytes for %d; first difference at byte %d, in %s" % (case["name"], path, len(got), len(want), k, where)


def test_child_ran_every_case_and_path(child):
    child.require()
    for case in CASES:
        for path, _ in paths_of(case):
            assert (case["name"], path) in child.records, (case["name"], path)
    assert ("batch", "batch") in child.records
    assert child.seconds < 300


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_bytes_are_the_oracles(child, oracle, case):
    child.require()
    for path, key in paths_of(case):
        got = child.records[(case["name"], path)]["streams"]
        want = case["streams"][key]
        want = want if key == "pieces" else [want]
        assert got == want, explain(child, case, path, key, oracle)


@pytest.mark.parametrize("case", [c for c in CASES if c["seams"]], ids=S.case_id)
def test_trace_shows_the_models_seams(child, case):
    child.require()
    want = S.model_calls(case)
    for path, _ in paths_of(case):
        got = S.trace_calls(S.parse_trace(child.traces[(case["name"], path)]))
        if path.startswith("run"):
            # (the last part of a wrapper under Action::Run drops the blocks not yet closed)
            assert got[0][-1][3] <= want[0][-1][3]
            got = [got[0][:-1] + [want[0][-1]]]
        # (pos, kept bytes, bits handed on) part by part -- and the blocks each part wrote: beside the marking kernel or
        # behind it (BZ_DF_CUTS=after), a part that is not the last keeps exactly the model's blocks
        assert got == want, (path, got, want)


def test_a_segment_of_exactly_part_and_guard_is_one_call(child):
    child.require()
    case = next(c for c in CASES if "E n=PART+GUARD no seam" in c["targets"])
    for path, _ in paths_of(case):
        assert S.parse_trace(child.traces[(case["name"], path)]) == []


@pytest.mark.parametrize("case", [c for c in CASES if len(c["pieces"]) == 1 and c["pieces"][0][2] == S.FINISH], ids=S.case_id)
def test_last_parts_blocks_and_the_stats_over_all_parts(child, case):
    child.require()
    n = case["bytes"]
    parts = [r for r in case["seams"]]
    skip_in = parts[-2][3] if parts else 0
    last_bytes = (parts[-1][2] - skip_in) if parts else n
    last_blocks = parts[-1][7] if parts else case["blocks"][0]
    for path, _ in paths_of(case):
        if not path.startswith("dev"):
            continue
        r = child.records[(case["name"], path)]
        assert r["debug_blocks"] == [last_blocks, last_bytes, skip_in], path
        assert [r["stats"][k] for k in ("blocks", "stored", "fixed", "dynamic")] == case["blocks"], path


def test_large_inputs_inside_a_batch_call(child, oracle):
    """two seam cases among small inputs: every stream is the one-shot stream"""
    child.require()
    got = child.records[("batch", "batch")]["streams"]
    small = [[len(z), hashlib.sha256(z).hexdigest()] for z in (oracle.deflate_encode(d, 0) for d in dfseams_child.SMALL)]
    big = [BY_NAME[name]["streams"]["kind0"] for name in dfseams_child.BATCH]
    assert got == [small[0], big[0], small[1], small[2], big[1], small[3]]
    assert len(S.parse_trace(child.traces[("batch", "batch")])) == sum(len(BY_NAME[name]["seams"]) for name in dfseams_child.BATCH)
