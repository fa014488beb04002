"""Test helper (not collected by pytest): a WRITER of LHA archives (.lzh) from the header table of DESIGN_lzhuf.md section 12,
a Python RESTATEMENT of that table (index()) with named faults, and the corpus of archives the reader is tested on -- in the
conventions of tests/bgzfforge.py and tests/lzhsplit.py.

An archive is PARAMETERS: {name, family, members: [...], end, cut, env, prefills}.  A member is {level, id, name | name_len,
src, ext, pad, hcrc, fault}: `src` names its plaintext and how its stream is made, `fault` what is wrong with it.
`build(case)` makes the bytes and what a reader must give for them -- expected bytes are the forge's own plaintexts, compressed
members are lzhref.encode's streams (or hand-made token lists through lzhsplit.build).  `hits(case)` lists, from the forged
bytes, which named targets the archive really meets; REQUIRED is the set the committed cases must cover.  The cases live in
tests/golden/lha_shapes.json with the SHA-256 of their bytes (parameters only); `python tests/lhaforge.py --regen` rewrites it.
Pure Python."""
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
import lzhref as R  # noqa: E402
import lzhsplit as S  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "lha_shapes.json")
OK, E_DATA, E_EOF, E_UNEXPECTED = 0, -1, -2, -3
STORED, DIR, OTHER = 0, 1, 255
PART = 4096                      # BZ_LHA_CRC_PART_KIB=4 of family C
CRC_SIZES = (0, 1, 15, 16, 17, 255 * 16, 256 * 16, 256 * 16 + 1, PART - 1, PART, PART + 1, 3 * PART + 5)


# ------------------------------------------------------------------------------------------------------ CRC-16/ARC
def crc16(data, crc=0):
    """bit by bit: reflected polynomial 0xA001, initial value 0, no final XOR"""
    for b in bytes(data):
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


assert crc16(b"123456789") == 0xBB3D

CRC_TABLE = [crc16(bytes([i])) for i in range(256)]


def crc16_table(data, crc=0):
    """the table-driven form a host loop would use"""
    t = CRC_TABLE
    for b in data:
        crc = t[(crc ^ b) & 255] ^ (crc >> 8)
    return crc


# ------------------------------------------------------------------------------------------------------ the restatement
MUTATIONS = ("h_plus_1", "sum_from_p1", "skip_is_packed", "pad_required", "hcrc_as_stored", "ext_size_2_ok", "dir_is_name",
             "level_3_as_0", "zero_is_no_end", "l1_min_22")
# the case each fault is known to change (tests/test_lha_index_host.py asserts it)
MUTATION_CASE = {"h_plus_1": "L_level0", "sum_from_p1": "L_level0", "skip_is_packed": "L_level1_ext", "pad_required": "L_level2",
                 "hcrc_as_stored": "L_level2", "ext_size_2_ok": "F_ext_size_2", "dir_is_name": "L_level1_ext", "level_3_as_0": "F_level_3",
                 "zero_is_no_end": "L_end_junk", "l1_min_22": "F_l1_header_short"}


def method_code(mid):
    if mid[1:3] == b"lh" and mid[3:4] in (b"4", b"5", b"6", b"7"):
        return mid[3] - 48
    if mid in (b"-lh0-", b"-lz4-"):
        return STORED
    return DIR if mid == b"-lhd-" else OTHER


class _Fault(Exception):
    def __init__(self, verdict, why):
        self.verdict, self.why = verdict, why


def _u16(d, p):
    return d[p] | d[p + 1] << 8


def _u32(d, p):
    return _u16(d, p) | _u16(d, p + 2) << 16


def _walk_ext(d, q, s, bound, over, m, mut, trace):
    total, hcrc, n = 0, None, 0
    while s != 0:
        if s < 3:
            if "ext_size_2_ok" in mut:
                break
            raise _Fault(E_DATA, "ext_size")
        if q + s > bound:
            raise _Fault(over, "ext_past")
        t, d0, dn = d[q], q + 1, s - 3
        if t == 0:
            if dn < 2:
                raise _Fault(E_DATA, "hcrc_short")
            hcrc = d0
        elif t == 1 or (t == 2 and "dir_is_name" in mut):
            m["name_off"], m["name_len"] = d0, dn
            trace.add("ext_name")
        elif t == 2:
            m["dir_off"], m["dir_len"] = d0, dn
            trace.add("ext_dir")
        else:
            trace.add("ext_unknown")
        total += s
        q += s
        n += 1
        s = _u16(d, q - 2)
    return q, total, hcrc, n


def _header(d, p, mut, trace):
    ln = len(d)
    if p + 21 > ln:
        raise _Fault(E_EOF, "eof_header")
    level = d[p + 20]
    if level == 3 and "level_3_as_0" in mut:
        level = 0
    if level > 2:
        raise _Fault(E_DATA, "level")
    m = dict(header_off=p, level=level, name_off=0, name_len=0, dir_off=0, dir_len=0, os_id=0)
    if level < 2:
        H = d[p]
        end = p + (1 if "h_plus_1" in mut else 2) + H
        if end > ln:
            raise _Fault(E_EOF, "eof_header")
        if H < 20:
            raise _Fault(E_DATA, "h_small")
        N = d[p + 21]
        if H < (25 if level and "l1_min_22" not in mut else 22) + N:
            raise _Fault(E_DATA, "h_small")
        if sum(d[p + (1 if "sum_from_p1" in mut else 2):end]) & 255 != d[p + 1]:
            raise _Fault(E_DATA, "sum")
        if d[p + 2] != 0x2D or d[p + 6] != 0x2D:
            raise _Fault(E_DATA, "method_form")
        size = _u32(d, p + 7)
        m.update(id=bytes(d[p + 2:p + 7]), orig_len=_u32(d, p + 11), mtime=_u32(d, p + 15), attr=d[p + 19], name_off=p + 22, name_len=N,
                 crc16=_u16(d, p + 22 + N))
        if level == 0:
            m.update(data_off=end, packed_len=size)
        else:
            m["os_id"] = d[p + 24 + N]
            q, total, _, n = _walk_ext(d, end, _u16(d, end - 2), ln, E_EOF, m, mut, trace)
            trace.add("l1_ext_%d" % n)
            if "skip_is_packed" in mut:
                total = 0
            if size < total:
                raise _Fault(E_DATA, "skip")
            m.update(data_off=q, packed_len=size - total)
    else:
        if p + 26 > ln:
            raise _Fault(E_EOF, "eof_header")
        T = _u16(d, p)
        if T < 26:
            raise _Fault(E_DATA, "h_small")
        if p + T > ln:
            raise _Fault(E_EOF, "eof_header")
        if d[p + 2] != 0x2D or d[p + 6] != 0x2D:
            raise _Fault(E_DATA, "method_form")
        m.update(id=bytes(d[p + 2:p + 7]), packed_len=_u32(d, p + 7), orig_len=_u32(d, p + 11), mtime=_u32(d, p + 15), attr=d[p + 19],
                 crc16=_u16(d, p + 21), os_id=d[p + 23])
        q, _, hcrc, _ = _walk_ext(d, p + 26, _u16(d, p + 24), p + T, E_DATA, m, mut, trace)
        slack = p + T - q
        if slack > 1 or ("pad_required" in mut and slack != 1):
            raise _Fault(E_DATA, "pad")
        trace.add("l2_pad" if slack else "l2_nopad")
        trace.add("l2_hcrc" if hcrc is not None else "l2_nohcrc")
        if hcrc is not None:
            h = bytearray(d[p:p + T])
            if "hcrc_as_stored" not in mut:
                h[hcrc - p:hcrc - p + 2] = b"\0\0"
            if crc16(h) != _u16(d, hcrc):
                raise _Fault(E_DATA, "hcrc")
        m["data_off"] = p + T
    m["method"] = method_code(m["id"])
    return m, m["data_off"] + m["packed_len"]


def index(data, mut=(), trace=None):
    """-> (members, fault verdict, fault position): the table of DESIGN_lzhuf.md section 12, restated"""
    d, p, out = bytes(data), 0, []
    trace = set() if trace is None else trace
    while p < len(d) and (d[p] != 0 or "zero_is_no_end" in mut):
        try:
            m, nxt = _header(d, p, mut, trace)
        except _Fault as f:
            trace.add("fault_" + f.why)
            return out, f.verdict, p
        out.append(m)
        if nxt > len(d):
            trace.add("fault_data_cut")
            return out, E_EOF, p
        p = nxt
    trace.add("end_eof" if p == len(d) else "end_junk" if p + 1 < len(d) else "end_zero")
    return out, OK, 0


FIELDS = ("header_off", "data_off", "packed_len", "orig_len", "name_off", "name_len", "dir_off", "dir_len", "mtime", "crc16", "method", "level",
          "os_id", "attr")


def row(m):
    """a member of index() as the host test program prints it"""
    return [m[f] for f in FIELDS] + [m["id"].hex()]


# ------------------------------------------------------------------------------------------------------ the writer
def _name(spec, k):
    if "name" in spec:
        return spec["name"].encode("latin-1")
    n = spec.get("name_len", 5)
    return (b"m%02d_" % k + b"abcdefghijklmnopqrstuvwxyz" * 10)[:n]


@functools.lru_cache(maxsize=None)
def _source(src, method):
    """-> (the bytes a reader must give, the member's data) for a `src` tuple under the method code"""
    kind = src[0]
    if kind == "text":
        plain = S.text(random.Random(src[1]), src[2])
    elif kind == "rand":
        plain = random.Random(src[1]).randbytes(src[2])
    elif kind == "blocks":      # (seed, n, codes per block, blocks dropped at the end): a hand-cut multi-block stream
        plain = S.text(random.Random(src[1]), src[2])
        blocks = S.cut(S.parse(plain, method), [src[3]])
        stream = S.build(blocks[:len(blocks) - src[4]], method)[0]
        return plain, stream
    elif kind == "first_match":  # the first code reaches ten bytes in front of the output; the CRC is that of window value src[1]
        return bytes([src[1]]) * 10 + b"xyz", S.build([[S.ref(10, 5)] + S.lits(b"xyz")], method)[0]
    else:
        raise ValueError(kind)
    return plain, (R.encode(plain, method) if 4 <= method <= 7 else plain)


def _ext(kind, arg, k):
    if kind == "name":
        return 1, (b"x%02d_" % k + b"0123456789" * 26)[:arg]
    if kind == "dir":
        return 2, arg.encode("latin-1")
    return arg, b"\xAA" * 4  # an unknown type


def wrap(entries, mid="-lh5-", level=2):
    """(plain, stream[, CRC-16 of plain]) tuples from any encoder as one archive of that method and level"""
    out = []
    for k, e in enumerate(entries):
        spec = dict(level=level, id=mid, name_len=8, ext=[["name", 8]] if level == 2 else [])
        h, data, _, _ = member_bytes(spec, k, (bytes(e[0]), bytes(e[1])) + tuple(e[2:]))
        out += [h, data]
    return b"".join(out) + b"\0"


def member_bytes(spec, k, raw=None):
    """-> (header, data, plain, member CRC in the header); raw: (plain, data[, CRC-16 of plain]) from elsewhere"""
    mid = spec["id"].encode()
    method = method_code(mid)
    fault = spec.get("fault", "")
    if raw is not None:
        plain, data = raw[:2]
    elif method == DIR:
        plain, data = b"", b""
    else:
        plain, data = _source(tuple(spec["src"]), method)
    orig = len(plain) + (1 if fault == "stored_unequal" else 0)
    crc = (raw[2] if raw is not None and len(raw) > 2 else crc16(plain)) ^ (0x0100 if fault == "crc" else 0)
    level = spec["level"]
    name = _name(spec, k)
    exts = [_ext(e[0], e[1], k) for e in spec.get("ext", [])]
    if spec.get("hcrc"):
        exts.insert(0, (0, b"\0\0"))
    sizes = [len(dat) + 3 for _, dat in exts]
    if fault == "ext_size_2":
        sizes[-1] = 2
    chain = b"".join(bytes([t]) + dat + struct.pack("<H", sizes[i + 1] if i + 1 < len(exts) else 0) for i, (t, dat) in enumerate(exts))
    first = struct.pack("<H", sizes[0] if exts else 0)
    tm = 0x5A21_6000 + k
    if level < 2:
        skip = len(data) + (sum(sizes) if level else 0) - (4 if fault == "skip_small" else 0)
        body = mid + struct.pack("<III", skip if level else len(data), orig, tm) + bytes([0x20, 3 if fault == "level_3" else level, len(name)]) + \
            name + struct.pack("<H", crc)
        if level:
            body += b"U" + (first if fault != "l1_header_short" else b"")
        assert len(body) <= 255, "a base header of levels 0 and 1 has at most 257 bytes"
        s = (sum(body) + (1 if fault == "sum" else 0)) & 255
        return bytes([len(body), s]) + body + (chain if level else b""), data, plain, crc
    T = 26 + len(chain) + (1 if spec.get("pad") else 0)
    assert T & 255, "a level-2 header whose size ends in a 0 byte looks like the end of the archive: pad it"
    h = bytearray(struct.pack("<H", T) + mid + struct.pack("<III", len(data), orig, tm) + bytes([0x20, 2]) + struct.pack("<H", crc) + b"U" + first +
                  chain + (b"\0" if spec.get("pad") else b""))
    if spec.get("hcrc"):
        h[27:29] = struct.pack("<H", crc16(h) ^ (1 if fault == "hcrc" else 0))
    return bytes(h), data, plain, crc


STOPS = ("sum", "hcrc", "ext_size_2", "skip_small", "level_3", "l1_header_short")  # faults at which the index stops


class Archive:
    """the bytes of a case and what a reader must make of them"""

    def __init__(self, case):
        self.case, self.name = case, case["name"]
        out, self.specs, self.plains, self.listed = b"", [], [], 0
        stopped = False
        for k, spec in enumerate(case["members"]):
            h, data, plain, _ = member_bytes(spec, k)
            out += h + data
            stopped = stopped or spec.get("fault") in STOPS
            if not stopped:
                self.listed += 1
                self.specs.append(spec)
                self.plains.append(plain)
        end = case.get("end", "zero")
        out += b"" if end == "eof" else b"\0" if end == "zero" else b"\0" + b"junk\x05-lh5-" * 3
        self.data = out[:len(out) - case.get("cut", 0)]
        self.env = case.get("env", {})
        self.prefills = case.get("prefills", [0x20])

    def expect(self, prefill=0x20):
        """[(bytes, verdict)] of the listed members, from the forge's own plaintexts"""
        res = []
        for k, (spec, plain) in enumerate(zip(self.specs, self.plains)):
            method = method_code(spec["id"].encode())
            fault = spec.get("fault", "")
            last_cut = self.case.get("cut") and k == self.listed - 1
            if method == OTHER:
                res.append((b"", E_UNEXPECTED))
            elif method == DIR:
                res.append((b"", OK))
            elif last_cut:
                res.append((b"", E_EOF))
            elif fault == "stored_unequal":
                res.append((b"", E_DATA))
            elif spec["src"][0] == "first_match":
                got = bytes([prefill & 255]) * 10 + b"xyz"
                res.append((b"", E_DATA) if prefill < 0 else (got, OK if got == plain else E_DATA))
            elif spec["src"][0] == "blocks" and spec["src"][4]:
                stream = _source(tuple(spec["src"]), method)[1]
                n = len(R.decode_full(stream, method, len(plain), prefill).out)   # (how far the shortened stream goes: the model's)
                assert 0 < n < len(plain)
                res.append((plain[:n], E_EOF))
            else:
                res.append((plain, E_DATA if fault == "crc" else OK))
        return res

    def stats(self, prefill=0x20):
        """bz_gpu_last_lha_read_stats [0..6] of a read of all listed members"""
        e = self.expect(prefill)
        codes = [method_code(q["id"].encode()) for q in self.specs]
        # a verdict that is the CRC's: the member's bytes are whole and the header's CRC-16 is not theirs
        crc_bad = sum(1 for q, (b, v) in zip(self.specs, e) if v == E_DATA and b)
        return [sum(v == OK for _, v in e), sum(v != OK for _, v in e), codes.count(STORED), codes.count(DIR), codes.count(OTHER), crc_bad,
                sum(len(b) for b, _ in e)]


@functools.lru_cache(maxsize=None)
def _built(params):
    return Archive(json.loads(params))


def build(case):
    """the archive of a case (built once per set of parameters)"""
    return _built(json.dumps({f: v for f, v in case.items() if f not in ("sha256", "hits")}, sort_keys=True))


# ------------------------------------------------------------------------------------------------------ the targets
def _required():
    r = {"level_0", "level_1", "level_2", "levels_mixed", "l1_ext_0", "l1_ext_1", "l1_ext_3", "ext_name", "ext_dir", "ext_unknown", "l2_pad",
         "l2_nopad", "l2_hcrc", "l2_nohcrc", "end_zero", "end_eof", "end_junk", "same_name", "crc_default_part", "p_first_code_match",
         "s_many_blocks", "f_member_crc", "f_stored_unequal", "f_stream_short", "fault_sum", "fault_hcrc", "fault_ext_size", "fault_skip",
         "fault_level", "fault_data_cut", "fault_h_small"}
    r |= {"name_len_%d" % n for n in (0, 1, 2, 3, 4, 255)}
    r |= {"data_phase4_%d" % k for k in range(4)} | {"data_phase16_%d" % k for k in range(16)}
    r |= {"method_" + m for m in ("lh0", "lh4", "lh5", "lh6", "lh7", "lhd", "lh1")} | {"empty_" + m for m in ("lh0", "lh4", "lh5", "lh6", "lh7")}
    r |= {"crc_%s_%d" % (m, n) for m in ("lh0", "lh5") for n in CRC_SIZES}
    return frozenset(r)


REQUIRED = _required()


def hits(case):
    """the targets an archive meets, computed from its bytes by the restatement (and the model decoder for the streams)"""
    a = build(case)
    t = set()
    ms, fault, _ = index(a.data, (), t)
    assert len(ms) == a.listed, case["name"]
    t |= {"level_%d" % m["level"] for m in ms}
    if {m["level"] for m in ms} == {0, 1, 2}:
        t.add("levels_mixed")
    names = [a.data[m["name_off"]:m["name_off"] + m["name_len"]] for m in ms]
    if len(set(names)) < len(names):
        t.add("same_name")
    part4 = a.env.get("BZ_LHA_CRC_PART_KIB") == "4"
    for m, plain in zip(ms, a.plains):
        tag = m["id"][1:4].decode()
        t.add("name_len_%d" % m["name_len"])
        t.add("method_" + tag)
        if m["packed_len"]:
            t |= {"data_phase4_%d" % (m["data_off"] % 4), "data_phase16_%d" % (m["data_off"] % 16)}
        if m["orig_len"] == 0 and m["method"] != DIR:
            t.add("empty_" + tag)
        end = m["data_off"] + m["packed_len"]
        if end > len(a.data):
            continue
        data = a.data[m["data_off"]:end]
        if m["method"] == STORED:
            if m["packed_len"] != m["orig_len"]:
                t.add("f_stored_unequal")
            elif crc16(data) != m["crc16"]:
                t.add("f_member_crc")
        if m["method"] in (STORED, 5) and crc16(plain) == m["crc16"] and m["orig_len"] == len(plain):
            if part4:
                t.add("crc_%s_%d" % (tag, m["orig_len"]))
            elif m["orig_len"] >= 2 * PART:
                t.add("crc_default_part")
        if 4 <= m["method"] <= 7 and len(data) < 6000:
            strict = R.decode_full(data, m["method"], m["orig_len"], -1)
            loose = R.decode_full(data, m["method"], m["orig_len"], 0x20)
            if strict.verdict == E_DATA and not strict.out and loose.verdict == OK:
                t.add("p_first_code_match")
            if loose.verdict == E_EOF and loose.blocks >= 1:
                t.add("f_stream_short")
            if loose.verdict == OK and loose.blocks >= 20 and a.env.get("BZ_LZH_SPLIT_KIB"):
                t.add("s_many_blocks")
    return sorted(x for x in t if x in REQUIRED)


# ------------------------------------------------------------------------------------------------------ the cases
def _m(level, mid, src=None, **kw):
    d = dict(level=level, id=mid, **kw)
    if src is not None:
        d["src"] = list(src)
    return d


def base_cases():
    cs = []

    def add(name, members, **kw):
        cs.append(dict(name=name, family=name[0], members=members, **kw))

    # ---- L: the levels, names, extended headers and ends
    lens = (0, 1, 2, 3, 4)
    add("L_level0", [_m(0, "-lh5-", ("text", 10 + n, 300 + 7 * n), name_len=n) for n in lens] +
        [_m(0, "-lh0-", ("text", 20 + n, 11 + n), name_len=n) for n in lens] + [_m(0, "-lh0-", ("text", 19, 33), name_len=233)], end="zero")
    add("L_level1", [_m(1, "-lh5-", ("text", 30 + n, 200 + 3 * n), name_len=n) for n in lens] +
        [_m(1, "-lh0-", ("text", 40 + n, 5 + n), name_len=n) for n in lens], end="eof")
    add("L_level1_ext", [_m(1, "-lh5-", ("text", 50, 400), name_len=0, ext=[["name", 9]]),
                         _m(1, "-lh0-", ("text", 51, 40), name_len=3, ext=[["name", 255], ["dir", "usr\xffshare\xff"], ["unk", 0x40]]),
                         _m(1, "-lh6-", ("text", 52, 500), name_len=2, ext=[["dir", "a\xff"], ["unk", 0x54], ["unk", 0x7F]]),
                         _m(1, "-lh0-", ("text", 53, 17), name_len=4)], end="junk")
    add("L_level2", [_m(2, "-lh5-", ("text", 60, 350), ext=[["name", 1]]),
                     _m(2, "-lh0-", ("text", 61, 21), ext=[["name", 2]], pad=True),
                     _m(2, "-lh7-", ("text", 62, 600), ext=[["name", 3], ["dir", "d\xff"]], hcrc=True),
                     _m(2, "-lh0-", ("text", 63, 30), ext=[["name", 4], ["unk", 0x41]], hcrc=True, pad=True),
                     _m(2, "-lh4-", ("text", 64, 222), ext=[["name", 255]], hcrc=True),
                     _m(2, "-lh0-", ("text", 65, 9))], end="zero")
    add("L_mixed", [_m(0, "-lh5-", ("text", 70, 500), name_len=6), _m(1, "-lh0-", ("text", 71, 64), name_len=7, ext=[["dir", "x\xff"]]),
                    _m(2, "-lh6-", ("text", 72, 777), ext=[["name", 8]], hcrc=True), _m(0, "-lh0-", ("text", 73, 13), name_len=1)], end="eof")
    add("L_phases", [_m(0, "-lh0-", ("text", 80 + n, 1 + n), name_len=5 + (n * 7) % 11) for n in range(24)], end="zero")
    add("L_end_junk", [_m(0, "-lh5-", ("text", 90, 120), name_len=4), _m(2, "-lh0-", ("text", 91, 12), ext=[["name", 5]])], end="junk")
    # ---- M: every method interleaved, empty members, a name twice
    mm = []
    for k, (mid, n) in enumerate((("-lh0-", 100), ("-lh4-", 900), ("-lhd-", 0), ("-lh5-", 1500), ("-lh1-", 77), ("-lh6-", 2000), ("-lh0-", 0),
                                  ("-lh7-", 2500), ("-lh4-", 0), ("-lh5-", 0), ("-lh1-", 5), ("-lh6-", 0), ("-lh7-", 0), ("-lh0-", 1000),
                                  ("-lh5-", 3000), ("-lz4-", 50))):
        if mid == "-lhd-":
            mm.append(_m(1, mid, None, name_len=0, ext=[["dir", "sub\xff"]]))
        elif k in (3, 13):   # (levels 0 and 1)
            mm.append(_m(k % 3, mid, ("text", 100 + k, n), name="same.txt"))
        elif k % 3 == 2:
            mm.append(_m(2, mid, ("text", 100 + k, n), ext=[["name", 6 + k % 4]], hcrc=bool(k & 1)))
        else:
            mm.append(_m(k % 3, mid, ("text", 100 + k, n), name_len=6 + k % 4))
    add("M_methods", mm, end="zero")
    # ---- C: the CRC's slices and parts
    add("C_parts", [_m(k % 3, mid, ("text", 200 + k, n), **(dict(name_len=k % 5) if k % 3 < 2 else dict(ext=[["name", 1 + k % 5]])))
                    for k, (n, mid) in enumerate((n, mid) for n in CRC_SIZES for mid in ("-lh0-", "-lh5-"))],
        end="zero", env={"BZ_LHA_CRC_PART_KIB": "4"})
    add("C_default", [_m(0, "-lh0-", ("text", 250, 3 * PART + 5), name_len=3), _m(2, "-lh5-", ("text", 251, 9000), ext=[["name", 3]])], end="eof")
    # ---- F: faults; the neighbours stay clean
    good = [_m(0, "-lh5-", ("text", 300, 310), name_len=5), _m(1, "-lh0-", ("text", 301, 45), name_len=6)]
    tail = [_m(2, "-lh5-", ("text", 302, 280), ext=[["name", 4]], hcrc=True), _m(0, "-lh0-", ("text", 303, 19), name_len=2)]
    add("F_member_crc", good + [_m(0, "-lh0-", ("text", 304, 100), name_len=3, fault="crc"), _m(2, "-lh5-", ("text", 305, 400), ext=[["name", 2]],
                                                                                                  fault="crc")] + tail)
    add("F_header_sum", good + [_m(0, "-lh0-", ("text", 306, 20), name_len=3, fault="sum")] + tail)
    add("F_header_crc", good + [_m(2, "-lh0-", ("text", 307, 20), ext=[["name", 3]], hcrc=True, fault="hcrc")] + tail)
    add("F_ext_size_2", good + [_m(1, "-lh0-", ("text", 308, 20), name_len=3, ext=[["name", 4], ["unk", 0x42]], fault="ext_size_2")] + tail)
    add("F_skip_small", good + [_m(1, "-lh0-", ("text", 309, 2), name_len=3, ext=[["name", 4]], fault="skip_small")] + tail)
    add("F_level_3", good + [_m(0, "-lh0-", ("text", 310, 20), name_len=3, fault="level_3")] + tail)
    add("F_l1_header_short", good + [_m(1, "-lh0-", ("text", 311, 20), name_len=3, fault="l1_header_short")] + tail)
    add("F_stored_unequal", good + [_m(1, "-lh0-", ("text", 312, 50), name_len=3, fault="stored_unequal")] + tail)
    add("F_data_cut", good + tail + [_m(0, "-lh5-", ("text", 313, 700), name_len=3)], end="eof", cut=9)
    add("F_stream_short", good + [_m(2, "-lh5-", ("blocks", 314, 1200, 60, 1), ext=[["name", 5]])] + tail)
    # ---- P: a stream whose first code reaches in front of the output (the CRC of one member fits spaces, the other's zeros)
    add("P_prefill", [good[0], _m(0, "-lh5-", ("first_match", 0x20), name_len=4), _m(1, "-lh5-", ("first_match", 0), name_len=5), tail[1]],
        prefills=[0x20, 0, -1])
    # ---- S: one member in many small blocks beside one-wave members of its method
    add("S_split", [_m(0, "-lh5-", ("text", 400, 200), name_len=4), _m(2, "-lh5-", ("blocks", 401, 6000, 16, 0), ext=[["name", 9]]),
                    _m(1, "-lh5-", ("text", 402, 150), name_len=6), _m(0, "-lh0-", ("text", 403, 300), name_len=2)],
        env={"BZ_LZH_SPLIT_KIB": "0.25", "BZ_LZH_SPLIT_CAND_BYTES": "1"})
    return cs


def digest(case):
    return hashlib.sha256(Archive(case).data).hexdigest()


def load():
    """the committed cases"""
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def archives():
    """every committed case, built"""
    return [build(c) for c in load()]


def main(argv):
    if "--regen" not in argv:
        print("usage: python tests/lhaforge.py --regen   (rewrites %s)" % os.path.relpath(FIXTURE, ROOT))
        return 2
    cases, got = [], set()
    for c in base_cases():
        c = dict(c)
        c["sha256"] = digest(c)
        c["hits"] = hits(c)
        got |= set(c["hits"])
        cases.append(c)
    missing = sorted(REQUIRED - got)
    if missing:
        print("targets no case hits:", missing)
        return 1
    with open(FIXTURE, "w") as f:
        json.dump({"about": "tests/lhaforge.py --regen: forged LHA archives as parameters (members, end, cut, env, prefills), the SHA-256 "
                            "of each archive's bytes and the targets it hits", "cases": cases}, f, indent=0)
        f.write("\n")
    print("%d cases, %d targets" % (len(cases), len(got & REQUIRED)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
