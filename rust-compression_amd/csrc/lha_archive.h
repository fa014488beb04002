// lha_archive.h -- the member headers of an LHA archive (.lzh / .lha; include/bz2_mi355x.h section 11, DESIGN_lzhuf.md
// section 12): the ONE place where the header rules stand.  bz_lha_index_buffer (lha_engine.hip) and the host test program
// (tests/host_stub/lha_archive_check.cpp) share it; tests/lhaforge.py restates it in Python.  The writer of section 12 of the
// header (header_size, write_header; DESIGN_lzhuf.md section 13) stands behind the parser: bz_gpu_lha_write_device and
// tests/host_stub/lha_write_check.cpp share it, tests/lhawrite.py restates it.
//
// All integers are little-endian.  A header starts at p; the archive ends cleanly where p == len or in[p] == 0.
//   levels 0 and 1: in[p] = H, the base header is [p, p + 2 + H); in[p + 1] = the sum of [p + 2, p + 2 + H) mod 256;
//     method id at p + 2 (five bytes, -xxx-), packed (level 1: skip) size at p + 7, original size at p + 11, time at p + 15,
//     attribute at p + 19, level at p + 20, name length N at p + 21, the name, CRC-16 at p + 22 + N, level 1: OS id at
//     p + 24 + N and the size of the first extended header in the last two bytes of the base header.
//     H >= 22 + N (level 0), 25 + N (level 1).
//   level 2: u16 at p = T, the whole header with its extended headers and padding; CRC-16 at p + 21, OS id at p + 23, the
//     size of the first extended header at p + 24; T >= 26; the extended headers end at p + T or one byte in front of it.
//   an extended header of size S: a type byte, S - 3 data bytes, the u16 size of the next one; 0 ends the list, 1 and 2 are
//     BZ_E_DATA.  Type 0: header CRC (checked in level 2, with the field read as zero), 1: file name, 2: directory.
// Plain C++17 without HIP headers.
#pragma once
#include "../../include/bz2_mi355x.h"

#include <cstddef>
#include <cstdint>
#include <cstring>

namespace lha {

inline uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }

// CRC-16/ARC (reflected 0xA001, initial value 0, no final XOR) of in[0, n) with the bytes [z, z + 2) read as zero
inline uint16_t crc16(const uint8_t *in, uint64_t n, uint64_t z = ~0ull)
{
    uint32_t c = 0;
    for (uint64_t i = 0; i < n; ++i) {
        c ^= (i >= z && i - z < 2u) ? 0u : in[i];
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xA001u : c >> 1;
    }
    return (uint16_t)c;
}

// the method code of a well-formed id (-xxx-)
inline uint8_t method_of(const uint8_t *id)
{
    if (id[1] == 'l' && id[2] == 'h') {
        if (id[3] >= '4' && id[3] <= '7') return (uint8_t)(id[3] - '0'); // BZ_LHA_LH4 .. 7 == BZ_LZH_LH4 .. 7
        if (id[3] == '0') return BZ_LHA_STORED;
        if (id[3] == 'd') return BZ_LHA_DIR;
    }
    if (id[1] == 'l' && id[2] == 'z' && id[3] == '4') return BZ_LHA_STORED;
    return BZ_LHA_OTHER;
}

struct ExtWalk {
    uint64_t end = 0;   // behind the last extended header
    uint64_t total = 0; // their sizes
    uint64_t hcrc = ~0ull; // where a type-0 header's two bytes lie
};

// The extended headers from q on, the first of size s, none reaching past `bound`; `over`: the verdict of one that does.
inline int walk_ext(const uint8_t *in, uint64_t q, uint32_t s, uint64_t bound, int over, bz_lha_member &m, ExtWalk &w)
{
    while (s != 0) {
        if (s < 3) return BZ_E_DATA;
        if (q + s > bound) return over;
        const uint8_t type = in[q];
        const uint64_t d0 = q + 1;
        const uint32_t dn = s - 3;
        if (type == 0x00) {
            if (dn < 2) return BZ_E_DATA;
            w.hcrc = d0;
        } else if (type == 0x01) {
            m.name_off = d0;
            m.name_len = dn;
        } else if (type == 0x02) {
            m.dir_off = d0;
            m.dir_len = dn;
        }
        w.total += s;
        q += s;
        s = rd16(in + q - 2);
    }
    w.end = q;
    return BZ_OK;
}

// One header at p (p < len, in[p] != 0).  BZ_OK: m is filled and *next is the position behind the member's data (which may
// lie behind len: the member's data is cut).  Else the fault's verdict.
inline int parse_header(const uint8_t *in, uint64_t len, uint64_t p, bz_lha_member &m, uint64_t *next)
{
    memset(&m, 0, sizeof m);
    if (p + 21 > len) return BZ_E_EOF;
    const uint32_t level = in[p + 20];
    if (level > 2) return BZ_E_DATA;
    m.header_off = p;
    m.level = (uint8_t)level;
    if (level < 2) {
        const uint32_t H = in[p];
        const uint64_t end = p + 2 + H;
        if (end > len) return BZ_E_EOF;
        if (H < 20) return BZ_E_DATA;
        const uint32_t N = in[p + 21];
        if (H < (level ? 25u : 22u) + N) return BZ_E_DATA;
        uint32_t sum = 0;
        for (uint64_t i = p + 2; i < end; ++i) sum += in[i];
        if ((sum & 255u) != in[p + 1]) return BZ_E_DATA;
        if (in[p + 2] != '-' || in[p + 6] != '-') return BZ_E_DATA;
        memcpy(m.method_id, in + p + 2, 5);
        m.orig_len = rd32(in + p + 11);
        m.mtime = rd32(in + p + 15);
        m.attr = in[p + 19];
        m.name_off = p + 22;
        m.name_len = N;
        m.crc16 = (uint16_t)rd16(in + p + 22 + N);
        const uint64_t size = rd32(in + p + 7);
        if (level == 0) {
            m.data_off = end;
            m.packed_len = size;
        } else {
            m.os_id = in[p + 24 + N];
            ExtWalk w;
            const int rc = walk_ext(in, end, rd16(in + p + H), len, BZ_E_EOF, m, w);
            if (rc != BZ_OK) return rc;
            if (size < w.total) return BZ_E_DATA;
            m.data_off = w.end;
            m.packed_len = size - w.total;
        }
    } else {
        if (p + 26 > len) return BZ_E_EOF;
        const uint32_t T = rd16(in + p);
        if (T < 26) return BZ_E_DATA;
        if (p + T > len) return BZ_E_EOF;
        if (in[p + 2] != '-' || in[p + 6] != '-') return BZ_E_DATA;
        memcpy(m.method_id, in + p + 2, 5);
        m.packed_len = rd32(in + p + 7);
        m.orig_len = rd32(in + p + 11);
        m.mtime = rd32(in + p + 15);
        m.attr = in[p + 19];
        m.crc16 = (uint16_t)rd16(in + p + 21);
        m.os_id = in[p + 23];
        ExtWalk w;
        const int rc = walk_ext(in, p + 26, rd16(in + p + 24), p + T, BZ_E_DATA, m, w);
        if (rc != BZ_OK) return rc;
        if (p + T - w.end > 1) return BZ_E_DATA; // (one padding byte may follow them)
        if (w.hcrc != ~0ull && crc16(in + p, T, w.hcrc - p) != rd16(in + w.hcrc)) return BZ_E_DATA;
        m.data_off = p + T;
    }
    m.method = method_of(m.method_id);
    *next = m.data_off + m.packed_len;
    return BZ_OK;
}

// The member table.  At most cap records are written (out may be NULL: counting); *count = the members found.  Returns the
// verdict of the fault that ended the walk (*fault_pos: the header it lies in), BZ_OK at a clean end.  A member whose data
// is cut by the end of the archive is listed, and the verdict is BZ_E_EOF at its header.
inline int index(const uint8_t *in, uint64_t len, bz_lha_member *out, size_t cap, size_t *count, uint64_t *fault_pos)
{
    uint64_t p = 0;
    size_t n = 0;
    int verdict = BZ_OK;
    while (p < len && in[p] != 0) {
        bz_lha_member m;
        uint64_t next = 0;
        verdict = parse_header(in, len, p, m, &next);
        if (verdict != BZ_OK) break;
        if (out && n < cap) out[n] = m;
        ++n;
        if (next > len) {
            verdict = BZ_E_EOF;
            break;
        }
        p = next;
    }
    *count = n;
    *fault_pos = verdict == BZ_OK ? 0 : p;
    return verdict;
}

// ---- the writer (include/bz2_mi355x.h section 12, DESIGN_lzhuf.md section 13): ONE header shape per level ----------------
//   level 0: H = 22 + N, the name in the base header; no directory.
//   level 1: H = 25 + Nb; Nb = N while 25 + N <= 255, else Nb = 0 and the name is a type-0x01 extended header; a non-empty
//     directory is a type-0x02 extended header behind it; skip size = packed size + the sizes of the extended headers.
//   level 2: type 0x00 (header CRC, size 5), type 0x01 (the name, always), type 0x02 (a non-empty directory), and ONE 0 byte
//     of padding when the low byte of T would be 0.
// crc16() through a byte table: a level-2 header's CRC is on the write call's host step once per member
inline uint16_t crc16_table(const uint8_t *in, uint64_t n)
{
    static const struct Tab {
        uint16_t t[256];
        Tab()
        {
            for (uint32_t i = 0; i < 256; ++i) {
                uint32_t c = i;
                for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xA001u : c >> 1;
                t[i] = (uint16_t)c;
            }
        }
    } tab;
    uint32_t c = 0;
    for (uint64_t i = 0; i < n; ++i) c = tab.t[(c ^ in[i]) & 0xFFu] ^ (c >> 8);
    return (uint16_t)c;
}

inline void wr16(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v, p[1] = (uint8_t)(v >> 8); }
inline void wr32(uint8_t *p, uint32_t v) { wr16(p, v), wr16(p + 2, v >> 16); }

// the five bytes of a BZ_LHA_* method the writer emits (STORED, DIR, LH4 .. LH7)
inline void method_id_of(uint8_t method, uint8_t id[5])
{
    memcpy(id, "-lh0-", 5);
    id[3] = method == BZ_LHA_DIR ? 'd' : (uint8_t)('0' + method);
}

inline bool name_in_base(int level, const bz_lha_entry &e) { return level == 0 || (level == 1 && 25u + e.name_len <= 255u); }

// The bytes of a member's header with its extended headers and padding; 0: there is no such header (a level outside 0 .. 2,
// a directory at level 0, H above 255, an extended header or T above 65 535).
inline uint64_t header_size(int level, const bz_lha_entry &e)
{
    const uint64_t N = e.name_len, D = e.dir_len;
    if (level == 0) return D == 0 && 22 + N <= 255 ? 2 + 22 + N : 0;
    if (N + 3 > 65535 || D + 3 > 65535) return 0;
    if (level == 1) return 2 + 25 + (name_in_base(1, e) ? N : N + 3) + (D ? D + 3 : 0);
    if (level != 2) return 0;
    uint64_t T = 26 + 5 + (N + 3) + (D ? D + 3 : 0);
    if ((T & 255u) == 0) ++T;
    return T <= 65535 ? T : 0;
}

// The header at out[0, header_size(level, e)): `packed` bytes of data follow it, they stand for `orig` bytes with CRC-16 `crc`.
inline void write_header(int level, const bz_lha_entry &e, const uint8_t id[5], uint64_t packed, uint64_t orig, uint16_t crc, uint8_t *out)
{
    const uint32_t N = e.name_len, D = e.dir_len;
    const uint64_t size = header_size(level, e);
    uint8_t *q; // where the extended headers go; `first` holds the size of the first one
    uint8_t *first;
    memcpy(out + 2, id, 5);
    wr32(out + 11, (uint32_t)orig);
    wr32(out + 15, e.mtime);
    out[19] = e.attr;
    out[20] = (uint8_t)level;
    if (level < 2) {
        const uint32_t Nb = name_in_base(level, e) ? N : 0u, H = (level ? 25u : 22u) + Nb;
        out[0] = (uint8_t)H;
        wr32(out + 7, (uint32_t)(packed + (size - 2 - H))); // (level 0: no extended headers)
        out[21] = (uint8_t)Nb;
        if (Nb) memcpy(out + 22, e.name, Nb);
        wr16(out + 22 + Nb, crc);
        if (level == 0) {
            uint32_t sum = 0;
            for (uint32_t i = 2; i < 2 + H; ++i) sum += out[i];
            out[1] = (uint8_t)sum;
            return;
        }
        out[24 + Nb] = e.os_id;
        first = out + H;
        q = out + 2 + H;
    } else {
        wr16(out, (uint32_t)size);
        wr32(out + 7, (uint32_t)packed);
        wr16(out + 21, crc);
        out[23] = e.os_id;
        first = out + 24;
        q = out + 26;
    }
    wr16(first, 0);
    const auto ext = [&](uint8_t type, const uint8_t *data, uint32_t n) {
        wr16(first, n + 3);
        q[0] = type;
        if (n) memcpy(q + 1, data, n);
        first = q + 1 + n;
        wr16(first, 0);
        q += n + 3;
    };
    static const uint8_t zero2[2] = {0, 0};
    if (level == 2) ext(0x00, zero2, 2);
    if (level == 2 || !name_in_base(level, e)) ext(0x01, e.name, N);
    if (D) ext(0x02, e.dir, D);
    if (level == 1) {
        const uint32_t H = out[0];
        uint32_t sum = 0;
        for (uint32_t i = 2; i < 2 + H; ++i) sum += out[i];
        out[1] = (uint8_t)sum;
    } else {
        if (q < out + size) *q = 0;                      // (the padding byte)
        wr16(out + 27, crc16_table(out, size));          // (its field still reads as zero)
    }
}

} // namespace lha
