"""TEST INFRASTRUCTURE -- a plain-Python model of LZHUF (-lh4- .. -lh7-).

encode(data, method) restates the reference's `LzhufEncoder` (src/lzhuf/encoder.rs) bit for bit on top of the oracle's
restatements of its parts: `LzssEncoder` (oracle.lzss_tokens), `make_table` (oracle.make_tab_with_fn) and
`BitWriter<Left>` (pack_bits here, held against oracle.bitwriter_pack).  decode(stream, method, orig_len, prefill) is the decoder under the contract
of section 9 of include/bz2_mi355x.h (DESIGN_lzhuf.md), written for reading, not speed.  Expected values of the LZHUF
tests come from here or from a forge's own plaintext, never from the library.

`mutate` (decode only) names deliberate faults of the model; tests/test_lzhforge.py shows that the forged corpus tells
each of them from the model.
"""
from oracle import oracle

OK, E_DATA, E_EOF = 0, -1, -2
LH4, LH5, LH6, LH7 = 4, 5, 6, 7
DICT_BITS = {4: 12, 5: 13, 6: 15, 7: 16}
OFFSET_BITS = {4: 4, 5: 4, 6: 5, 7: 5}
BLOCK_CODES = 0xFFFF
MAX_MATCH, MIN_MATCH = 256, 3
NC, NT = 510, 19

MUTATIONS = ("run1_base", "run2_base", "skip_at_2", "skip_at_4", "extra_lsb_first", "distance_is_pos", "kraft_le",
             "length_base", "unary_from_6", "data_before_eof", "end_needs_17_bits", "no_cut_at_orig_len",
             "ccount_511_ok", "tcount_20_ok", "run_may_overshoot", "len17_ok")


# ---------------------------------------------------------------------------------------------- shared pieces
def canonical(lengths):
    """{symbol: (code, length)}: shorter lengths first, equal lengths by ascending symbol; a code's bits MSB first."""
    out, code, prev = {}, 0, 0
    for ln, s in sorted((ln, s) for s, ln in enumerate(lengths) if ln):
        code <<= ln - prev
        out[s] = (code, ln)
        code += 1
        prev = ln
    return out


def convert_pos(pos):
    """`LzhufLzssCode::from` (encoder.rs:94-108): pos -> (pos_offset, pos_sublen)."""
    po = 1 << pos.bit_length()  # (pos + 1).next_power_of_two()
    return po.bit_length() - 1, pos - (po >> 1)


def len_fields(ln):
    """`enc_len` (encoder.rs:285-296)."""
    if ln >= 7:
        return [(7, 3)] + [(1, 1)] * (ln - 7) + [(0, 1)]
    return [(ln, 3)]


def pack_bits(fields):
    """(value, width) fields MSB first, padded with zeros to a byte: what `BitWriter<Left>` and the encoder's flush leave
    (tests/test_lzhref.py holds it against oracle.bitwriter_pack)."""
    acc = n = 0
    for v, w in fields:
        acc = (acc << w) | (v & ((1 << w) - 1))
        n += w
    pad = -n % 8
    return ((acc << pad).to_bytes((n + pad) // 8, "big")) if n else b""


# ---------------------------------------------------------------------------------------------- the encoder
def _symb_tab_fields(tab):
    """`write_symb_tab` (encoder.rs:298-433): the t-table and the c-table of one block."""
    used = [(i, l) for i, l in enumerate(tab) if l]
    if not tab:
        return [(0, 5), (0, 5), (0, 9), (0, 9)], None
    if len(used) == 1:
        return [(0, 5), (0, 5), (0, 9), (used[0][0], 9)], None
    sym_list, freq, i = [], [0] * NT, 0
    for ind, ln in used:
        gap = ind - i
        i = ind + 1
        if gap > 19:
            sym_list.append((2, gap - 20))
            freq[2] += 1
        elif gap == 19:
            sym_list += [(1, 15), (0, 0)]
            freq[1] += 1
            freq[0] += 1
        elif gap > 2:
            sym_list.append((1, gap - 3))
            freq[1] += 1
        elif gap > 0:
            sym_list += [(0, 0)] * gap
            freq[0] += gap
        sym_list.append((3, ln + 2))
        freq[ln + 2] += 1
    ttab, _ = oracle.make_tab_with_fn(freq, 16, 0)
    tused = [(i, l) for i, l in enumerate(ttab) if l]
    ret = []
    if len(tused) == 1:
        ret += [(0, 5), (tused[0][0], 5)]
        tcode = None
    else:
        ret.append((tused[-1][0] + 1, 5))
        i = 0
        for ind, ln in tused:
            while ind >= i:
                if i == 3:
                    skip = 3 if ind > 6 else ind - 3
                    ret.append((skip, 2))
                    i += skip
                ret += [(0, 3)] if ind != i else len_fields(ln)
                i += 1
        tcode = canonical(ttab)
    ret.append((used[-1][0] + 1, 9))
    for s, l in sym_list:
        k = l if s == 3 else s
        if tcode is not None:
            ret.append(tcode[k])
        if s == 1:
            ret.append((l, 4))
        elif s == 2:
            ret.append((l, 9))
    return ret, canonical(tab)


def _offset_tab_fields(tab, pbits):
    """`write_offset_tab` (encoder.rs:435-472)."""
    used = [(i, l) for i, l in enumerate(tab) if l]
    if not used:
        return [(0, pbits), (0, pbits)], None
    if len(used) == 1:
        return [(0, pbits), (used[0][0], pbits)], None
    ret, i = [(used[-1][0] + 1, pbits)], 0
    for ind, ln in used:
        while ind >= i:
            ret += [(0, 3)] if ind != i else len_fields(ln)
            i += 1
    return ret, canonical(tab)


def block_fields(codes, pbits):
    """`write_block` (encoder.rs:474-520) for codes = [("sym", b) | ("ref", len, pos)]."""
    sfreq, ofreq, conv = [0] * NC, [0] * 32, []
    for c in codes:
        if c[0] == "sym":
            sfreq[c[1]] += 1
            conv.append((c[1],))
        else:
            po, sub = convert_pos(c[2])
            sfreq[c[1] + 256 - MIN_MATCH] += 1
            ofreq[po] += 1
            conv.append((c[1] + 256 - MIN_MATCH, po, sub))
    stab, _ = oracle.make_tab_with_fn(sfreq, 16, 0)
    otab, _ = oracle.make_tab_with_fn(ofreq, 16, 0)
    f = [(len(codes), 16)]
    sf, scode = _symb_tab_fields(stab)
    of, ocode = _offset_tab_fields(otab, pbits)
    f += sf + of
    for c in conv:
        if scode is not None:
            f.append(scode[c[0]])
        if len(c) == 3:
            if ocode is not None:
                f.append(ocode[c[1]])
            if c[1] > 1:
                f.append((c[2], c[1] - 1))
    return f


def encode_fields(data, method):
    toks = oracle.lzss_tokens(bytes(data), window=1 << DICT_BITS[method], max_match=MAX_MATCH)
    f = []
    for i in range(0, len(toks), BLOCK_CODES):
        f += block_fields(toks[i:i + BLOCK_CODES], OFFSET_BITS[method])
    return f


def encode(data, method=LH7):
    """`data.encode(&mut LzhufEncoder::new(&method), Action::Finish).collect()`"""
    return pack_bits(encode_fields(data, method))


# ---------------------------------------------------------------------------------------------- the decoder
class _Eof(Exception):
    pass


class _Data(Exception):
    pass


class _Bits:
    def __init__(self, data, late=False):
        self.d = bytes(data)
        self.total = 8 * len(self.d)
        self.pos = 0
        self.late = late  # (a mutation: the end is looked at behind a whole table or code only)

    def peek(self, n):  # n <= 32; zeros behind the end
        bi = self.pos >> 3
        chunk = int.from_bytes(self.d[bi:bi + 5].ljust(5, b"\0"), "big")
        return (chunk >> (40 - (self.pos & 7) - n)) & ((1 << n) - 1)

    def take(self, n):
        """n bits; _Eof when one of them lies behind the entry's end (looked at before the value is judged)."""
        v = self.peek(n) if n else 0
        self.pos += n
        if self.pos > self.total and not self.late:
            raise _Eof()
        return v

    def check(self):
        if self.pos > self.total:
            raise _Eof()


class Result:
    def __init__(self):
        self.out = bytearray()
        self.verdict = OK
        self.bits = 0
        self.blocks = self.literals = self.matches = 0


def _read_len(b, mut, T, tag):
    c = b.take(3)
    if c == (6 if "unary_from_6" in mut else 7):
        while b.take(1):
            c += 1
            if c > (17 if "len17_ok" in mut else 16):
                T("%s_len_17" % tag)
                raise _Data()
    T("%s_len_%d" % (tag, c))
    return c


def _table(lengths, mut, T, tag):
    """{(length, code): symbol} of an explicit length set; the Kraft sum must be exactly 1."""
    one = 1 << 32
    kraft = sum(one >> l for l in lengths if l)
    if kraft != one:
        T("%s_kraft_%s" % (tag, "over" if kraft > one else "zero" if kraft == 0 else "under"))
    if kraft > one or (kraft < one and "kraft_le" not in mut) or kraft == 0:
        raise _Data()
    return {(l, c): s for s, (c, l) in canonical(lengths).items()}


def _sym(b, tab, T=None, tag=""):
    if isinstance(tab, int):
        return tab
    for l in range(1, 17):
        s = tab.get((l, b.peek(l)))
        if s is not None:
            if T and b.pos // 2048 != (b.pos + l - 1) // 2048:
                T("stage_cross")  # the code lies across the edge of a 64-word stage
            b.take(l)
            if T:
                T("%s_code_%d" % (tag, l))
            return s
    b.take(16)  # (an incomplete set under a mutation: no code)
    raise _Data()


def decode_full(stream, method=LH7, orig_len=None, prefill=-1, mutate=(), trace=None):
    """trace: a set that receives the names of what the decode met (tests/lzhforge.py: the targets a case hits)."""
    mut = set(mutate)

    def T(name):
        if trace is not None:
            trace.add(name)

    assert mut <= set(MUTATIONS)
    dbits, pbits = DICT_BITS[method], OFFSET_BITS[method]
    b, r = _Bits(stream, "data_before_eof" in mut), Result()
    out = r.out
    L = orig_len
    try:
        while True:
            if L is not None and len(out) >= L:
                T("ol_0" if L == 0 else "ol_at_block_end")
                break
            if b.total - b.pos < (17 if "end_needs_17_bits" in mut else 16):
                T("end_rem_%d" % (b.total - b.pos))
                if L is not None and len(out) < L:
                    T("ol_beyond")
                    r.verdict = E_EOF
                break
            T("hdr_phase_%d" % (b.pos % 32))
            ncodes = b.take(16)
            if ncodes == 0:
                T("end_zero_len_junk" if b.total - b.pos >= 16 else "end_zero_len")
                if L is not None and len(out) < L:
                    r.verdict = E_EOF
                break
            T("block_%d" % min(r.blocks + 1, 3))
            # t-table
            n = b.take(5)
            if n == 0:
                ttab = b.take(5)
                T("t_const")
                if ttab > 18:
                    T("t_const_19")
                    raise _Data()
            else:
                T("t_count_%d" % n)
                if n > (20 if "tcount_20_ok" in mut else NT):
                    raise _Data()
                ll = []
                skip_at = 2 if "skip_at_2" in mut else 4 if "skip_at_4" in mut else 3
                while len(ll) < n:
                    if len(ll) == skip_at:
                        sk = b.take(2)
                        T("t_skip_%d" % sk)
                        ll += [0] * sk
                        if len(ll) > n:
                            T("t_skip_past")
                            raise _Data()
                        if len(ll) == n:
                            break
                    ll.append(_read_len(b, mut, T, "t"))
                ttab = _table(ll, mut, T, "t")
            # c-table
            n = b.take(9)
            if n == 0:
                ctab = b.take(9)
                T("c_const")
                if ctab > NC - 1:
                    T("c_const_510")
                    raise _Data()
            else:
                T("c_count_%d" % n)
                if n > (511 if "ccount_511_ok" in mut else NC):
                    raise _Data()
                ll, last = [], (0, 0)
                while len(ll) < n:
                    k = _sym(b, ttab, T, "t")
                    if k == 0:
                        run = 1
                    elif k == 1:
                        run = (4 if "run1_base" in mut else 3) + b.take(4)
                    elif k == 2:
                        run = (21 if "run2_base" in mut else 20) + b.take(9)
                    else:
                        run = 0
                    if k <= 2:
                        T("run_%d" % run)
                        if last == (0, 1) and k == 0:
                            T("run_2")
                        if last[1] and last[1] + run == 19:
                            T("run_19_as_%d_%d" % (last[1], run))
                    last = (k, run if k <= 2 else 0)
                    if len(ll) + max(run, 1) > n:
                        T("run_past")
                        if "run_may_overshoot" in mut:
                            run = n - len(ll)
                        else:
                            raise _Data()
                    ll += [0] * run if run else [k - 2]
                ctab = _table(ll, mut, T, "c")
            # p-table
            n = b.take(pbits)
            if n == 0:
                ptab = b.take(pbits)
                T("p_const")
                if ptab > dbits:
                    T("p_const_over")
                    raise _Data()
            else:
                if n > dbits + 1:
                    T("p_count_over_m%d" % method)
                    raise _Data()
                ptab = _table([_read_len(b, mut, T, "p") for _ in range(n)], mut, T, "p")
            if isinstance(ttab, int) and isinstance(ctab, int) and isinstance(ptab, int):
                T("all_const")
            b.check()
            # the codes (pend: literals since the last match, as the kernel holds them back: 1 .. 64)
            pend = 0
            for _ in range(ncodes):
                b.check()
                if L is not None and len(out) >= L:
                    T("ol_mid_literals" if pend else "ol_inside_block")
                    break
                s = _sym(b, ctab, T, "c")
                if s < 256:
                    out.append(s)
                    r.literals += 1
                    pend = pend % 64 + 1
                    continue
                ln = s - (254 if "length_base" in mut else 253)
                v = _sym(b, ptab, T, "p")
                T("p_sym_%d" % v)
                if v == dbits:
                    T("p_sym_max_m%d" % method)
                pos = v
                if v > 1:
                    x = b.take(v - 1)
                    if "extra_lsb_first" in mut:
                        x = int(format(x, "0%db" % (v - 1))[::-1], 2)
                    pos = (1 << (v - 1)) | x
                d = pos if "distance_is_pos" in mut else pos + 1
                T("len_%d" % ln)
                T("dist_%d" % d)
                if d == len(out):
                    T("dist_eq_p")
                if d == len(out) + 1:
                    T("dist_p_plus_1_%s" % ("strict" if prefill < 0 else "prefill"))
                if d == 1 << dbits and len(out) > d:
                    T("dist_window_m%d" % method)
                if 0 < pend < 64 and d <= pend:
                    T("match_reads_pending")
                pend = 0
                if d > (1 << dbits) or d < 1 or (prefill < 0 and d > len(out)):
                    raise _Data()  # (with the bytes in front of the failing code)
                if L is not None and ln > L - len(out):
                    T("ol_mid_match")
                    if "no_cut_at_orig_len" not in mut:
                        ln = L - len(out)
                p = len(out)
                for i in range(ln):
                    q = p - d + i % d
                    out.append(prefill if q < 0 else out[q])
                r.matches += 1
            else:
                b.check()
                r.blocks += 1
                continue
            break  # the known length was reached inside the block
    except _Eof:
        r.verdict = E_EOF
    except _Data:
        r.verdict = E_DATA  # (every bit looked at lay inside the entry: take() raises first otherwise)
    r.bits = min(b.pos, b.total)
    return r


def decode(stream, method=LH7, orig_len=None, prefill=-1, mutate=()):
    """-> (bytes, verdict, bits consumed) under the contract of section 9."""
    r = decode_full(stream, method, orig_len, prefill, mutate)
    return bytes(r.out), r.verdict, r.bits
