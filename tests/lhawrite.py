"""Test helper (not collected by pytest): a Python RESTATEMENT of the LHA writer's fixed header shape and stored rule
(include/bz2_mi355x.h section 12, DESIGN_lzhuf.md section 13) with named faults, and the corpus the writer is tested on -- in the
conventions of tests/lhaforge.py.

A case is PARAMETERS: {name, family, members: [...], methods, levels, env}.  A member is {name | name_len, dir, src, is_dir,
mtime, attr, os_id}: `src` names its plaintext.  `expected(entries, method, level)` makes the archive and its member table from
(entry, plaintext) pairs: member data is lzhref.encode's stream (the model) or the plaintext, never the library's.  `hits(case)`
lists, from the built bytes, which named targets the case really meets; REQUIRED is the set the committed cases must cover.
The cases live in tests/golden/lha_write_shapes.json with the SHA-256 of every archive they stand for (parameters only);
`python tests/lhawrite.py --regen` rewrites it.  Pure Python."""
import functools
import hashlib
import json
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lhaforge as F  # noqa: E402
import lzhref as R  # noqa: E402
import lzhsplit as S  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lha_write_shapes.json")
STORED, DIR = 0, 1
METHODS = (STORED, 4, 5, 6, 7)
LEVELS = (0, 1, 2)
CHUNK = 16384                    # bytes of a span per k_lha_pack workgroup and step
DATA_LENS = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 33)
FAULTS = ("tie_compressed", "skip_is_packed", "hcrc_with_field", "no_pad", "sum_from_p1", "crc_of_stream", "no_end_byte")
# the case and (method, level) each fault is known to change (tests/test_lhawrite.py asserts it)
FAULT_CASE = {"tie_compressed": ("R_tie", 5, 1), "skip_is_packed": ("H_l1_both_ext", 5, 1), "hcrc_with_field": ("H_fields", 5, 2),
              "no_pad": ("H_l2_pad", 5, 2), "sum_from_p1": ("H_fields", 5, 0), "crc_of_stream": ("H_fields", 5, 1),
              "no_end_byte": ("H_fields", 5, 2)}


def method_id(code):
    return b"-lhd-" if code == DIR else b"-lh%d-" % code


# ------------------------------------------------------------------------------------------------------ the restated writer
def header_size(level, e):
    """the bytes of a member's header, or None where there is none (BZ_E_PARAM)"""
    N, D = len(e["name"]), len(e["dir"])
    if level == 0:
        return 24 + N if D == 0 and 22 + N <= 255 else None
    if N + 3 > 65535 or D + 3 > 65535:
        return None
    if level == 1:
        return 27 + (N if 25 + N <= 255 else N + 3) + (D + 3 if D else 0)
    T = 26 + 5 + (N + 3) + (D + 3 if D else 0)
    T += 1 if T & 255 == 0 else 0
    return T if T <= 65535 else None


def _chain(exts):
    """[(type, data)] -> (the size of the first one, the bytes, {type: offset of its data in them})"""
    out, at = b"", {}
    for i, (t, dat) in enumerate(exts):
        at[t] = len(out) + 1
        nxt = len(exts[i + 1][1]) + 3 if i + 1 < len(exts) else 0
        out += bytes([t]) + dat + struct.pack("<H", nxt)
    return (len(exts[0][1]) + 3 if exts else 0), out, at


def header(level, e, mid, packed, orig, crc, mut=()):
    """-> (bytes, name offset, dir offset or None): the fixed shape of DESIGN_lzhuf.md section 13"""
    name, d = e["name"], e["dir"]
    fixed = struct.pack("<II", orig, e["mtime"]) + bytes([e["attr"], level])
    if level < 2:
        base_name = name if level == 0 or 25 + len(name) <= 255 else b""
        exts = ([] if base_name == name else [(1, name)]) + ([(2, d)] if d else [])
        assert level == 1 or not exts
        first, chain, at = _chain(exts)
        skip = packed + (0 if "skip_is_packed" in mut else len(chain))
        body = mid + struct.pack("<I", skip) + fixed + bytes([len(base_name)]) + base_name + struct.pack("<H", crc)
        if level:
            body += bytes([e["os_id"]]) + struct.pack("<H", first)
        assert len(body) <= 255
        s = sum(body[:-1] if "sum_from_p1" in mut else body)    # (from p + 1: H bytes, one place early)
        h = bytes([len(body), s & 255]) + body
        return h + chain, (22 if base_name == name else len(h) + at[1]), (len(h) + at[2] if d else None)
    exts = [(0, b"\0\0"), (1, name)] + ([(2, d)] if d else [])
    first, chain, at = _chain(exts)
    T = 26 + len(chain)
    pad = T & 255 == 0 and "no_pad" not in mut
    T += pad
    h = bytearray(struct.pack("<H", T) + mid + struct.pack("<I", packed) + fixed + struct.pack("<H", crc) + bytes([e["os_id"]]) +
                  struct.pack("<H", first) + chain + (b"\0" if pad else b""))
    c = F.crc16(h)
    if "hcrc_with_field" in mut:          # (a second pass over the header with the first value in place)
        h[27:29] = struct.pack("<H", c)
        c = F.crc16(h)
    h[27:29] = struct.pack("<H", c)
    return bytes(h), 26 + at[1], (26 + at[2] if d else None)


@functools.lru_cache(maxsize=None)
def stream(plain, method):
    """the model's stream"""
    return R.encode(plain, method)


def expected(entries, method, level, mut=()):
    """[(entry, plaintext)] -> (archive, member table in lhaforge.FIELDS + id, stats [0..6] of the write call)"""
    out, table = b"", []
    st = [len(entries), 0, 0, 0, 0, 0, 0]
    for e, plain in entries:
        data, code = plain, STORED
        if e["is_dir"]:
            assert not plain
            code = DIR
            st[4] += 1
        elif method == STORED:
            st[3] += 1
        else:
            s = stream(plain, method) if plain else b""
            if len(s) < len(plain) or ("tie_compressed" in mut and len(s) == len(plain) and plain):
                data, code = s, method
                st[1] += 1
            else:
                st[2] += 1
        crc = F.crc16(data if "crc_of_stream" in mut else plain)
        h, name_at, dir_at = header(level, e, method_id(code), len(data), len(plain), crc, mut)
        p = len(out)
        table.append(dict(header_off=p, data_off=p + len(h), packed_len=len(data), orig_len=len(plain), name_off=p + name_at,
                          name_len=len(e["name"]), dir_off=p + dir_at if dir_at else 0, dir_len=len(e["dir"]), mtime=e["mtime"], crc16=crc,
                          method=code, level=level, os_id=e["os_id"] if level else 0, attr=e["attr"], id=method_id(code)))
        out += h + data
        st[5] += len(plain)
    out += b"" if "no_end_byte" in mut else b"\0"
    st[6] = len(out)
    return out, table, st


def spans(table, total):
    """the byte ranges the layout kernel copies: every header, every non-empty data, the end byte"""
    sp = []
    for m in table:
        sp.append((m["header_off"], m["data_off"]))
        if m["packed_len"]:
            sp.append((m["data_off"], m["data_off"] + m["packed_len"]))
    return sp + [(total - 1, total)]


# ------------------------------------------------------------------------------------------------------ the cases
def _name(spec, k):
    if "name" in spec:
        return spec["name"].encode("latin-1")
    return (b"%02d" % k + b"abcdefghijklmnopqrstuvwxyz" * 12)[:spec.get("name_len", 5)]


@functools.lru_cache(maxsize=None)
def source(src):
    kind = src[0]
    if kind == "text":
        return S.text(random.Random(src[1]), src[2])
    if kind == "rand":
        return random.Random(src[1]).randbytes(src[2])
    if kind == "nibbles":      # sixteen letters at random: short matches, more than 65 535 codes in 200 KB, and it still compresses
        rng = random.Random(src[1])
        return bytes(0x41 + rng.randrange(16) for _ in range(src[2]))
    if kind == "ab":
        return (b"ab" * 6)[:src[1]]
    if kind == "abc":
        return (b"abcdefg" * 3)[:src[1]]
    if kind == "none":
        return b""
    raise ValueError(kind)


def entries(case):
    out = []
    for k, spec in enumerate(case["members"]):
        e = dict(name=_name(spec, k), dir=spec.get("dir", "").encode("latin-1"), mtime=spec.get("mtime", 0x5A216000 + k),
                 attr=spec.get("attr", 0x20), os_id=spec.get("os_id", 0x55), is_dir=bool(spec.get("is_dir")))
        out.append((e, source(tuple(spec.get("src", ["none"])))))
    return out


def combos(case):
    return [(m, lv) for m in case.get("methods", METHODS) for lv in case.get("levels", LEVELS)]


@functools.lru_cache(maxsize=None)
def _built(params, method, level):
    return expected(entries(json.loads(params)), method, level)


def build(case, method, level):
    """(archive, table, stats) of a case under one method and level (built once)"""
    return _built(json.dumps({f: v for f, v in case.items() if f not in ("sha256", "hits")}, sort_keys=True), method, level)


# ------------------------------------------------------------------------------------------------------ the targets
def _required():
    r = {"level_0", "level_1", "level_2", "dir_l1", "dir_l2", "l2_pad", "l2_T_ff", "l2_T_01", "l1_name_230", "l1_name_231", "l1_both_ext",
         "fields_distinct", "short_span", "empty_input", "one_byte_stored", "random_stored", "stored_by_request", "directory",
         "multi_block", "stored_rows", "crc_parts", "no_members", "all_directories"}
    r |= {"name_len_%d" % n for n in tuple(range(17)) + (230, 231)}
    r |= {"header_phase_%d" % k for k in range(16)} | {"data_phase_%d" % k for k in range(16)}
    r |= {"data_len_%d" % n for n in DATA_LENS}
    r |= {"meet_%d" % k for k in range(1, 16)}
    r |= {"%s_lh%d" % (t, m) for t in ("rule_tie", "rule_shorter_by_1", "rule_longer_by_1", "mix") for m in (4, 5, 6, 7)}
    r |= {"mix_level_%d" % lv for lv in LEVELS}
    return frozenset(r)


REQUIRED = _required()


def hits(case):
    """the targets a case meets, computed from the built bytes and tables"""
    t = set()
    part4 = case.get("env", {}).get("BZ_LHA_CRC_PART_KIB") == "4"
    for method, level in combos(case):
        arc, table, st = build(case, method, level)
        ents = entries(case)
        t.add("level_%d" % level)
        if not table:
            t.add("no_members")
        elif st[4] == len(table):
            t.add("all_directories")
        kinds = set()
        for m, (e, plain) in zip(table, ents):
            N = m["name_len"]
            t.add("name_len_%d" % N)
            t.add("header_phase_%d" % (m["header_off"] % 16))
            if m["packed_len"]:
                t.add("data_phase_%d" % (m["data_off"] % 16))
            t.add("data_len_%d" % m["packed_len"])
            if m["dir_len"]:
                t.add("dir_l%d" % level)
            if level == 1 and N in (230, 231):
                assert (m["name_off"] == m["header_off"] + 22) == (N == 230)
                t.add("l1_name_%d" % N)
            if level == 1 and N > 230 and m["dir_len"]:
                t.add("l1_both_ext")
            if level == 2:
                T = m["data_off"] - m["header_off"]
                raw = 26 + 5 + N + 3 + (m["dir_len"] + 3 if m["dir_len"] else 0)
                if T == raw + 1:
                    assert raw & 255 == 0
                    t.add("l2_pad")
                t |= {"l2_T_ff"} if T & 255 == 255 else {"l2_T_01"} if raw & 255 == 1 else set()
            fields = struct.pack("<I", m["mtime"]) + bytes([m["attr"], m["os_id"]])
            if level and len(set(fields)) == 6 and 0 not in fields:
                t.add("fields_distinct")
            if m["method"] == DIR:
                t.add("directory")
                kinds.add("dir")
            elif method == STORED:
                t.add("stored_by_request")
            elif m["method"] == STORED:
                n, s = len(plain), len(stream(plain, method)) if plain else 0
                assert s >= n
                kinds.add("empty" if n == 0 else "rule")
                t |= {"empty_input"} if n == 0 else {"one_byte_stored"} if n == 1 else set()
                t |= {"rule_tie_lh%d" % method} if s == n and n else {"rule_longer_by_1_lh%d" % method} if s == n + 1 else set()
                if len(set(plain)) > 200:
                    t.add("random_stored")
            else:
                kinds.add("comp")
                if m["packed_len"] == m["orig_len"] - 1:
                    t.add("rule_shorter_by_1_lh%d" % method)
                if m["orig_len"] > 65535 and R.decode_full(arc[m["data_off"]:m["data_off"] + m["packed_len"]], method, m["orig_len"], -1).blocks >= 2:
                    t.add("multi_block")
            if m["method"] == STORED and m["packed_len"] > 2 * CHUNK:
                t.add("stored_rows")
            if part4 and m["orig_len"] > 2 * 4096:
                t.add("crc_parts")
        if kinds == {"dir", "empty", "rule", "comp"}:
            t |= {"mix_lh%d" % method, "mix_level_%d" % level}
        sp = spans(table, len(arc))
        for (a, b), (c, _) in zip(sp, sp[1:]):
            assert b == c
            if b % 16:
                t.add("meet_%d" % (b % 16))
        if any(a % 16 and b % 16 and a // 16 == b // 16 for a, b in sp):
            t.add("short_span")
    return sorted(x for x in t if x in REQUIRED)


def _m(src=None, **kw):
    d = dict(kw)
    if src is not None:
        d["src"] = list(src)
    return d


def base_cases():
    cs = []

    def add(name, members, **kw):
        cs.append(dict(name=name, family=name[0], members=members, **kw))

    # ---- P: headers and data at every byte phase, spans that meet inside a line, spans inside one line
    add("P_names", [_m(("text", 10 + n, DATA_LENS[n % len(DATA_LENS)]), name_len=n) for n in range(17)])
    add("P_lens", [_m(("text", 40 + k, n), name_len=3 + (5 * k) % 7) for k, n in enumerate(DATA_LENS * 2)])
    add("P_meet", [_m(("text", 70 + k, 1 + (k * 3) % 14), name_len=(k * 7) % 16) for k in range(40)])
    add("P_l1_name", [_m(("text", 120, 33), name_len=230), _m(("text", 121, 17), name_len=231), _m(("text", 122, 400), name_len=229),
                      _m(("text", 123, 5), name_len=233)], levels=[1, 2])
    # ---- R: the stored rule
    add("R_tie", [_m((kind, n), name_len=4 + k) for k, (kind, n) in enumerate((k, n) for k in ("ab",) for n in (10, 11, 12))] +
        [_m(("abc", n), name_len=7 + k) for k, n in enumerate((13, 14, 15))], methods=[4, 5, 6, 7])
    add("R_kinds", [_m(("none",), name_len=3), _m(("text", 130, 1), name_len=4), _m(("rand", 131, 700), name_len=5),
                    _m(("text", 132, 900), name_len=6)])
    # ---- H: the header shapes
    add("H_fields", [_m(("text", 140, 300), name_len=9, mtime=0x12345678, attr=0x9A, os_id=0xBC),
                     _m(("text", 141, 40), name_len=2, mtime=0x0A0B0C0D, attr=0x0E, os_id=0x4D)])
    add("H_dir", [_m(("text", 150, 250), name_len=6, dir="usr\xffshare\xff"), _m(("text", 151, 20), name_len=7),
                  _m(None, name_len=0, dir="sub\xff", is_dir=True), _m(None, name_len=4, is_dir=True)], levels=[1, 2])
    # level 2: T = 34 + N (+ D + 3); N = 222 gives 256 (padded to 257), 221 gives 255, 223 gives 257
    add("H_l2_pad", [_m(("text", 160, 100), name_len=222), _m(("text", 161, 100), name_len=221), _m(("text", 162, 100), name_len=223),
                     _m(("text", 163, 50), name_len=212, dir="abcde\xff")], levels=[2])
    add("H_l1_both_ext", [_m(("text", 170, 500), name_len=240, dir="a\xffbc\xff"), _m(("text", 171, 9), name_len=8)], levels=[1])
    # ---- M: compressed, stored by the rule, directory and empty members interleaved
    add("M_mix", [_m(("text", 180, 800), name_len=5), _m(("ab", 11), name_len=6), _m(None, name_len=7, is_dir=True), _m(("none",), name_len=8),
                  _m(("text", 181, 1500), name_len=9), _m(("rand", 182, 64), name_len=10), _m(None, name_len=3, is_dir=True),
                  _m(("text", 183, 77), name_len=11), _m(("none",), name_len=1)])
    add("M_none", [])
    add("M_dirs", [_m(None, name_len=3 + k, is_dir=True) for k in range(3)], methods=[STORED, 5])
    # ---- L: a member of several LZHUF blocks, a stored member over several chunk rows, the CRC in parts
    add("L_text", [_m(("nibbles", 190, 200000), name_len=5), _m(("text", 191, 100), name_len=6)], methods=[5], levels=[2],
        env={"BZ_LHA_CRC_PART_KIB": "4"})
    add("L_stored", [_m(("text", 192, 50), name_len=4), _m(("rand", 193, 5 * CHUNK + 1234), name_len=7)], methods=[STORED, 5], levels=[0, 1],
        env={"BZ_LHA_CRC_PART_KIB": "4"})
    return cs


def digests(case):
    return {"lh%d_l%d" % (m, lv): hashlib.sha256(build(case, m, lv)[0]).hexdigest() for m, lv in combos(case)}


def load():
    """the committed cases"""
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def regen():
    """the fixture's text from base_cases(), or the targets no case hits"""
    cases, got = [], set()
    for c in base_cases():
        c = dict(c)
        c["sha256"] = digests(c)
        c["hits"] = hits(c)
        got |= set(c["hits"])
        cases.append(c)
    missing = sorted(REQUIRED - got)
    text = json.dumps({"about": "tests/lhawrite.py --regen: the LHA writer's corpus as parameters (members, methods, levels, env), the SHA-256 "
                                "of each archive (method, level) and the targets the case hits", "cases": cases}, indent=0) + "\n"
    return text, missing, cases


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/lhawrite.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    text, missing, cases = regen()
    if missing:
        print("targets no case hits:", missing)
        return 1
    with open(FIXTURE, "w") as f:
        f.write(text)
    print("%d cases, %d archives, %d bytes built" % (len(cases), sum(len(combos(c)) for c in cases),
                                                     sum(len(build(c, m, lv)[0]) for c in cases for m, lv in combos(c))))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
