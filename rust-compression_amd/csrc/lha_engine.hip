// lha_engine.hip -- the drivers of the LHA archive reader and writer (include/bz2_mi355x.h sections 11, 12; header rules: lha_archive.h;
// kernels: k_lha.hip, k_gz_member_gather of k_gz_members.hip and, through lzh_decode_batch_placed, k_lzhuf.hip): the member
// table on the host, the device call, its figures, and the host-to-host form on an engine of the per-process cache.
#include "engine_state.h"
#include "k_lha.h"
#include "lha_archive.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

using namespace lhagpu;
using dfgpu::GzSpan;

struct LhaWorkspace {
    DevBuf image, spans, jobs, parts, res; // a method's packed spans, span records, CRC jobs, their partials, their results
    u64 stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    DevBuf w_streams, w_blob; // the writer: the encode call's streams, the headers
    u64 w_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

void lha_workspace_free(LhaWorkspace *w) { delete w; }

extern "C" int bz_lha_index_buffer(const uint8_t *in, size_t in_len, bz_lha_member *members, size_t cap, size_t *count, int32_t *fault,
                                   uint64_t *fault_pos)
{
    if (!count || !fault || !fault_pos || (in_len && !in)) return BZ_E_PARAM;
    *fault = lha::index(in, in_len, members, members ? cap : 0, count, fault_pos);
    return BZ_OK;
}

extern "C" int bz_gpu_last_lha_read_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->lha ? g->lha->stats[i] : 0;
    return BZ_OK;
}

// bytes of a CRC part: BZ_LHA_CRC_PART_KIB KiB (default 1024, read per call), a multiple of kCrcPartMin, at most 1 GiB
static u32 lha_crc_part_bytes()
{
    const char *s = getenv("BZ_LHA_CRC_PART_KIB");
    double kib = s && *s ? atof(s) : 1024.0;
    if (!(kib >= kCrcPartMin / 1024.0)) kib = kCrcPartMin / 1024.0;
    if (kib > 1048576.0) kib = 1048576.0;
    return (u32)((u64)(kib * 1024.0) / kCrcPartMin * kCrcPartMin);
}

// What is known of a selection before any launch: each member's place, the bytes its slot holds and its verdict so far.
struct LhaPlan {
    std::vector<const bz_lha_member *> m;
    std::vector<u64> place, slot;
    std::vector<int32_t> verdict;
    u64 need = 0; // the end of the last slot's bytes
    int status = BZ_OK;

    LhaPlan(size_t in_len, const bz_lha_member *members, size_t nmembers, const size_t *sel, size_t nsel) : m(nsel), place(nsel), slot(nsel), verdict(nsel)
    {
        if (!members || (!sel && nsel != nmembers)) {
            status = BZ_E_PARAM;
            return;
        }
        u64 cursor = 0;
        for (size_t k = 0; k < nsel; ++k) {
            const size_t i = sel ? sel[k] : k;
            if (i >= nmembers || (sel && k && sel[k - 1] >= i)) {
                status = BZ_E_PARAM;
                return;
            }
            const bz_lha_member &q = members[i];
            if (q.header_off >= in_len || q.data_off > in_len || q.data_off < q.header_off || q.orig_len > 0xFFFFFFFFull ||
                q.packed_len > 0xFFFFFFFFull) {
                status = BZ_E_PARAM;
                return;
            }
            m[k] = &q;
            const bool lzh = q.method >= BZ_LHA_LH4 && q.method <= BZ_LHA_LH7;
            if (q.method == BZ_LHA_DIR) verdict[k] = BZ_OK;
            else if (q.method != BZ_LHA_STORED && !lzh) verdict[k] = BZ_E_UNEXPECTED;
            else if (q.packed_len > in_len - q.data_off) verdict[k] = BZ_E_EOF;
            else if (q.method == BZ_LHA_STORED && q.packed_len != q.orig_len) verdict[k] = BZ_E_DATA;
            else {
                verdict[k] = BZ_OK;
                slot[k] = q.orig_len;
            }
            place[k] = cursor;
            if (slot[k]) need = cursor + slot[k];
            cursor += (slot[k] + 15u) & ~(u64)15;
        }
    }
    bool has_bytes(size_t k) const { return verdict[k] == BZ_OK && m[k]->method != BZ_LHA_DIR; } // (before the launches)
};

static int lha_read_core(bz_gpu_engine *g, const void *d_in, size_t in_len, const LhaPlan &plan, int prefill, void *d_out, size_t cap,
                         uint64_t *h_out_off, uint64_t *h_out_len, int32_t *h_verdict)
{
    const size_t nsel = plan.m.size();
    if (d_out && plan.need > cap) return BZ_E_CAPACITY;
    HIPCHK(hipSetDevice(g->device));
    if (!g->lha) g->lha = new LhaWorkspace();
    LhaWorkspace *w = g->lha;
    for (u64 &s : w->stats) s = 0;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    u8 *out8 = static_cast<u8 *>(d_out);
    for (size_t k = 0; k < nsel; ++k) {
        h_out_off[k] = plan.place[k];
        h_out_len[k] = 0;
        h_verdict[k] = plan.verdict[k];
    }
    int rc;
    // ---- the compressed members, method by method: their spans side by side at multiples of 16, one decode call
    for (int method = BZ_LHA_LH4; method <= BZ_LHA_LH7; ++method) {
        std::vector<size_t> who;
        for (size_t k = 0; k < nsel; ++k)
            if (plan.m[k]->method == method && plan.has_bytes(k)) who.push_back(k);
        if (who.empty()) continue;
        const size_t n = who.size();
        std::vector<GzSpan> spans(n);
        std::vector<u64> off(n), len(n), orig(n), place(n), got(n);
        std::vector<int32_t> verdict(n);
        u64 total = 0;
        u32 max_len = 0;
        for (size_t j = 0; j < n; ++j) {
            const bz_lha_member &q = *plan.m[who[j]];
            spans[j].src = q.data_off;
            spans[j].dst = off[j] = total;
            spans[j].len = (u32)q.packed_len;
            spans[j].pad = 0;
            len[j] = q.packed_len;
            orig[j] = q.orig_len;
            place[j] = plan.place[who[j]];
            max_len = std::max(max_len, spans[j].len);
            total += (q.packed_len + 15u) & ~(u64)15;
        }
        if ((rc = w->image.ensure((size_t)total + 64)) != BZ_OK) return rc;
        if ((rc = w->spans.ensure(n * sizeof(GzSpan))) != BZ_OK) return rc;
        HIPCHK(hipMemcpyAsync(w->spans.p, spans.data(), n * sizeof(GzSpan), hipMemcpyHostToDevice, g->st));
        if (dfgpu::df_launch_gz_gather(g->st, in8, w->spans.as<GzSpan>(), (u32)n, max_len, w->image.as<u8>()) != 0) return BZ_E_UNEXPECTED;
        w->stats[7] += 1;
        rc = lzh_decode_batch_placed(g, method, prefill, w->image.p, off.data(), len.data(), orig.data(), n, d_out, cap, place.data(), got.data(),
                                     verdict.data());
        if (rc != BZ_OK) return rc;
        u64 ls[8];
        bz_gpu_last_lzh_decode_stats(g, ls);
        w->stats[7] += ls[7];
        for (size_t j = 0; j < n; ++j) {
            h_out_len[who[j]] = got[j];
            h_verdict[who[j]] = verdict[j];
        }
    }
    // ---- the stored members
    std::vector<GzSpan> stored;
    u32 stored_max = 0;
    for (size_t k = 0; k < nsel; ++k) {
        if (plan.m[k]->method != BZ_LHA_STORED || !plan.has_bytes(k)) continue;
        h_out_len[k] = plan.slot[k];
        if (plan.slot[k]) stored.push_back(GzSpan{plan.m[k]->data_off, plan.place[k], (u32)plan.slot[k], 0u});
        stored_max = std::max(stored_max, (u32)plan.slot[k]);
    }
    if (out8 && !stored.empty()) {
        if (stored.size() > 0x7FFFFFFFu) return BZ_E_PARAM;
        if ((rc = w->spans.ensure(stored.size() * sizeof(GzSpan))) != BZ_OK) return rc;
        HIPCHK(hipMemcpyAsync(w->spans.p, stored.data(), stored.size() * sizeof(GzSpan), hipMemcpyHostToDevice, g->st));
        if (lha_launch_store(g->st, in8, in_len, w->spans.as<GzSpan>(), (u32)stored.size(), stored_max, out8) != 0) return BZ_E_UNEXPECTED;
        HIPCHK(hipStreamSynchronize(g->st));
        w->stats[7] += 1;
    }
    // ---- the CRC-16 of every member that is clean so far
    if (out8) {
        const u32 part_bytes = lha_crc_part_bytes();
        std::vector<LhaCrcJob> jobs;
        std::vector<size_t> who;
        u64 nparts = 0, max_parts = 0;
        for (size_t k = 0; k < nsel; ++k) {
            if (h_verdict[k] != BZ_OK || plan.m[k]->method == BZ_LHA_DIR) continue;
            const u64 parts = lha_crc_parts(h_out_len[k], part_bytes);
            jobs.push_back(LhaCrcJob{h_out_off[k], h_out_len[k], (u32)nparts, plan.m[k]->crc16});
            who.push_back(k);
            nparts += parts;
            max_parts = std::max(max_parts, parts);
        }
        if (nparts > 0xFFFFFFFFull || jobs.size() > 0x7FFFFFFFu) return BZ_E_PARAM;
        if (!jobs.empty()) {
            const u32 nj = (u32)jobs.size();
            std::vector<LhaCrcRes> res(nj);
            if ((rc = w->jobs.ensure(nj * sizeof(LhaCrcJob))) != BZ_OK) return rc;
            if ((rc = w->parts.ensure(((size_t)nparts + 1) * 4)) != BZ_OK) return rc;
            if ((rc = w->res.ensure(nj * sizeof(LhaCrcRes))) != BZ_OK) return rc;
            HIPCHK(hipMemcpyAsync(w->jobs.p, jobs.data(), nj * sizeof(LhaCrcJob), hipMemcpyHostToDevice, g->st));
            if (lha_launch_crc16(g->st, out8, w->jobs.as<LhaCrcJob>(), nj, max_parts, part_bytes, w->parts.as<u32>()) != 0) return BZ_E_UNEXPECTED;
            if (lha_launch_crc16_join(g->st, w->jobs.as<LhaCrcJob>(), nj, part_bytes, w->parts.as<u32>(), w->res.as<LhaCrcRes>()) != 0)
                return BZ_E_UNEXPECTED;
            HIPCHK(hipMemcpyAsync(res.data(), w->res.p, nj * sizeof(LhaCrcRes), hipMemcpyDeviceToHost, g->st));
            HIPCHK(hipStreamSynchronize(g->st));
            w->stats[7] += max_parts ? 2 : 1;
            for (u32 j = 0; j < nj; ++j)
                if (res[j].verdict != BZ_OK) {
                    h_verdict[who[j]] = res[j].verdict;
                    w->stats[5] += 1;
                }
        }
    }
    for (size_t k = 0; k < nsel; ++k) {
        const uint8_t method = plan.m[k]->method;
        w->stats[h_verdict[k] == BZ_OK ? 0 : 1] += 1;
        if (method == BZ_LHA_STORED) w->stats[2] += 1;
        else if (method == BZ_LHA_DIR) w->stats[3] += 1;
        else if (method == BZ_LHA_OTHER) w->stats[4] += 1;
        w->stats[6] += h_out_len[k];
    }
    return BZ_OK;
}

extern "C" int bz_gpu_lha_read_device(bz_gpu_engine *g, const void *d_in, size_t in_len, const bz_lha_member *h_members, size_t nmembers,
                                      const size_t *h_sel, size_t nsel, int prefill, void *d_out, size_t cap, uint64_t *h_out_off,
                                      uint64_t *h_out_len, int32_t *h_verdict)
{
    if (!g || prefill < -1 || prefill > 255) return BZ_E_PARAM;
    if (((uintptr_t)d_in & 15u) || ((uintptr_t)d_out & 15u)) return BZ_E_PARAM;
    if (nsel == 0) return BZ_OK;
    if (!h_out_off || !h_out_len || !h_verdict || !d_in) return BZ_E_PARAM;
    const LhaPlan plan(in_len, h_members, nmembers, h_sel, nsel);
    if (plan.status != BZ_OK) return plan.status;
    return lha_read_core(g, d_in, in_len, plan, prefill, d_out, cap, h_out_off, h_out_len, h_verdict);
}

extern "C" int bz_lha_read_buffer(int device, const uint8_t *in, size_t in_len, const size_t *sel, size_t nsel, int prefill, uint8_t **out,
                                  uint64_t *out_off, uint64_t *out_len, int32_t *verdict, int32_t *fault)
{
    if (!out) return BZ_E_PARAM;
    *out = nullptr;
    if (!fault || prefill < -1 || prefill > 255 || (in_len && !in)) return BZ_E_PARAM;
    if (nsel && (!out_off || !out_len || !verdict)) return BZ_E_PARAM;
    size_t count = 0;
    uint64_t fault_pos = 0;
    *fault = lha::index(in, in_len, nullptr, 0, &count, &fault_pos);
    std::vector<bz_lha_member> members(count ? count : 1);
    *fault = lha::index(in, in_len, members.data(), count, &count, &fault_pos);
    const LhaPlan plan(in_len, members.data(), count, sel, nsel);
    if (plan.status != BZ_OK) return plan.status;
    if (nsel == 0) return one_shot_empty(out);
    // (a call the decode path refused leaves a sound engine; so do the members' verdicts)
    return one_shot(device, 0, OneShotIn(in, in_len), (size_t)plan.need, kSettleParamSound, out, [&](bz_gpu_engine *g, size_t *total) {
        *total = (size_t)plan.need;
        return lha_read_core(g, g->dec_in.p, in_len, plan, prefill, g->oneshot_out.p, (size_t)plan.need, out_off, out_len, verdict);
    });
}

// ---- the writer (section 12 of the header; DESIGN_lzhuf.md section 13) ------------------------------------------------
constexpr u64 kLhaMaxCompressed = 1ull << 30; // the encoder's limit

// What of (method, level, entries, lengths) is checked before any device is touched.  hsize: every member's header size.
static int lha_write_check(int method, int level, const bz_lha_entry *e, const uint64_t *len, size_t count, std::vector<u64> *hsize)
{
    const bool stored = method == BZ_LHA_STORED;
    if (!stored && (method < BZ_LHA_LH4 || method > BZ_LHA_LH7)) return BZ_E_PARAM;
    if (level < 0 || level > 2) return BZ_E_PARAM;
    if (count > 0x3FFFFFFFu || (count && (!e || !len))) return BZ_E_PARAM; // (two spans a member and the end byte: one launch)
    if (hsize) hsize->resize(count);
    for (size_t i = 0; i < count; ++i) {
        const bz_lha_entry &q = e[i];
        if ((q.name_len && !q.name) || (q.dir_len && !q.dir)) return BZ_E_PARAM;
        const u64 hs = lha::header_size(level, q);
        if (!hs || (q.is_dir && len[i]) || (!stored && len[i] > kLhaMaxCompressed)) return BZ_E_PARAM;
        const u64 ext = level == 1 ? hs - 27 - (lha::name_in_base(1, q) ? q.name_len : 0u) : 0; // (in the level-1 skip size)
        if (len[i] + ext >= 0xFFFFFFFFull) return BZ_E_PARAM;
        if (hsize) (*hsize)[i] = hs;
    }
    return BZ_OK;
}

extern "C" size_t bz_lha_write_bound(int level, const bz_lha_entry *e, const uint64_t *in_len, size_t count)
{
    if (level < 0 || level > 2 || (count && (!e || !in_len))) return 0;
    size_t s = 1;
    for (size_t i = 0; i < count; ++i) {
        const u64 hs = lha::header_size(level, e[i]);
        if (!hs) return 0;
        s += (size_t)(hs + in_len[i]);
    }
    return s;
}

extern "C" int bz_gpu_last_lha_write_stats(bz_gpu_engine *g, uint64_t out[8])
{
    if (!g || !out) return BZ_E_PARAM;
    for (int i = 0; i < 8; ++i) out[i] = g->lha ? g->lha->w_stats[i] : 0;
    return BZ_OK;
}

// One call, its parameters checked: CRC launches, the encode call, the host step, the layout launch.
static int lha_write_core(bz_gpu_engine *g, int method, int level, const void *d_in, const uint64_t *h_in_off, const uint64_t *h_in_len,
                          const bz_lha_entry *h_entries, const std::vector<u64> &hsize, size_t count, void *d_out, size_t cap, size_t *out_len,
                          bz_lha_member *h_members)
{
    const bool stored = method == BZ_LHA_STORED;
    const u32 part_bytes = lha_crc_part_bytes();
    std::vector<LhaCrcJob> jobs(count);
    std::vector<LhaCrcRes> res(count);
    u64 nparts = 0, max_parts = 0;
    for (size_t i = 0; i < count; ++i) {
        const u64 parts = lha_crc_parts(h_in_len[i], part_bytes);
        jobs[i] = LhaCrcJob{h_in_off[i], h_in_len[i], (u32)nparts, 0u};
        nparts += parts;
        max_parts = std::max(max_parts, parts);
    }
    if (nparts > 0xFFFFFFFFull) return BZ_E_PARAM;
    HIPCHK(hipSetDevice(g->device));
    if (!g->lha) g->lha = new LhaWorkspace();
    LhaWorkspace *w = g->lha;
    for (u64 &s : w->w_stats) s = 0;
    const u8 *in8 = static_cast<const u8 *>(d_in);
    int rc;
    // ---- the CRC-16 of every input: launched here, downloaded behind the encode call
    if (count) {
        const u32 nj = (u32)count;
        if ((rc = w->jobs.ensure(nj * sizeof(LhaCrcJob))) != BZ_OK) return rc;
        if ((rc = w->parts.ensure(((size_t)nparts + 1) * 4)) != BZ_OK) return rc;
        if ((rc = w->res.ensure(nj * sizeof(LhaCrcRes))) != BZ_OK) return rc;
        HIPCHK(hipMemcpyAsync(w->jobs.p, jobs.data(), nj * sizeof(LhaCrcJob), hipMemcpyHostToDevice, g->st));
        if (lha_launch_crc16(g->st, in8, w->jobs.as<LhaCrcJob>(), nj, max_parts, part_bytes, w->parts.as<u32>()) != 0) return BZ_E_UNEXPECTED;
        if (lha_launch_crc16_join(g->st, w->jobs.as<LhaCrcJob>(), nj, part_bytes, w->parts.as<u32>(), w->res.as<LhaCrcRes>()) != 0)
            return BZ_E_UNEXPECTED;
        w->w_stats[7] += max_parts ? 2 : 1;
    }
    // ---- the streams of every input that has bytes, in the engine's buffer
    std::vector<u64> e_off, e_len, s_off, s_len;
    for (size_t i = 0; !stored && i < count; ++i)
        if (h_in_len[i]) {
            e_off.push_back(h_in_off[i]);
            e_len.push_back(h_in_len[i]);
        }
    if (!e_len.empty()) {
        const size_t bound = bz_lzh_encode_batch_bound(e_len.data(), e_len.size());
        s_off.resize(e_len.size());
        s_len.resize(e_len.size());
        if ((rc = w->w_streams.ensure(bound + 64)) != BZ_OK) return rc;
        rc = bz_gpu_lzh_encode_batch_device(g, method, d_in, e_off.data(), e_len.data(), e_len.size(), w->w_streams.p, bound, s_off.data(),
                                            s_len.data());
        if (rc != BZ_OK) return rc;
    }
    // the one look at the device that is the writer's own: the CRCs (the encode call has waited for its work, and for theirs)
    if (count) HIPCHK(hipMemcpyAsync(res.data(), w->res.p, count * sizeof(LhaCrcRes), hipMemcpyDeviceToHost, g->st));
    HIPCHK(hipStreamSynchronize(g->st));
    // ---- the host step: the stored rule, the headers (each at a blob offset congruent mod 16 to its place), the places
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_out);
    std::vector<u8> blob;
    std::vector<LhaPackSpan> spans;
    std::vector<u64> h_at(count), place(count);
    spans.reserve(2 * count + 1);
    u64 cursor = 0, max_len = 1;
    const auto blob_room = [&](u64 n) {
        const size_t at = blob.size() + (size_t)((base + cursor - blob.size()) & 15u);
        blob.resize(at + (size_t)n);
        spans.push_back(LhaPackSpan{at, cursor, n, kPackBlob, 0u});
        max_len = std::max(max_len, n);
        cursor += n;
        return at;
    };
    for (size_t i = 0, k = 0; i < count; ++i) {
        const bz_lha_entry &q = h_entries[i];
        u64 packed = h_in_len[i], src = h_in_off[i];
        bool compressed = false;
        if (!stored && h_in_len[i]) {
            if (s_len[k] < h_in_len[i]) { // (the tie goes to stored)
                compressed = true;
                packed = s_len[k];
                src = s_off[k];
            }
            ++k;
        }
        uint8_t id[5];
        lha::method_id_of(q.is_dir ? BZ_LHA_DIR : compressed ? (uint8_t)method : BZ_LHA_STORED, id);
        place[i] = cursor;
        h_at[i] = blob_room(hsize[i]);
        lha::write_header(level, q, id, packed, h_in_len[i], (uint16_t)res[i].crc, blob.data() + h_at[i]);
        if (packed) {
            spans.push_back(LhaPackSpan{src, cursor, packed, compressed ? kPackStream : kPackInput, 0u});
            max_len = std::max(max_len, packed);
            cursor += packed;
        }
        w->w_stats[q.is_dir ? 4 : compressed ? 1 : stored ? 3 : 2] += 1;
        w->w_stats[5] += h_in_len[i];
    }
    blob_room(1); // (the end byte: blob.resize wrote the 0)
    w->w_stats[0] = count;
    w->w_stats[6] = cursor;
    if (cursor > cap) return BZ_E_CAPACITY;
    // ---- the archive, in one launch
    if ((rc = w->w_blob.ensure(blob.size() + 64)) != BZ_OK) return rc;
    if ((rc = w->spans.ensure(spans.size() * sizeof(LhaPackSpan))) != BZ_OK) return rc;
    HIPCHK(hipMemcpyAsync(w->w_blob.p, blob.data(), blob.size(), hipMemcpyHostToDevice, g->st));
    HIPCHK(hipMemcpyAsync(w->spans.p, spans.data(), spans.size() * sizeof(LhaPackSpan), hipMemcpyHostToDevice, g->st));
    if (lha_launch_pack(g->st, w->w_blob.as<u8>(), w->w_streams.as<u8>(), in8, w->spans.as<LhaPackSpan>(), (u32)spans.size(), max_len,
                        static_cast<u8 *>(d_out)) != 0)
        return BZ_E_UNEXPECTED;
    HIPCHK(hipStreamSynchronize(g->st));
    HIPCHK(hipGetLastError());
    w->w_stats[7] += 1;
    for (size_t i = 0; h_members && i < count; ++i) { // the parser's own reading of each header, moved to its place
        bz_lha_member &m = h_members[i];
        uint64_t next = 0;
        if (lha::parse_header(blob.data() + h_at[i], hsize[i], 0, m, &next) != BZ_OK) return BZ_E_UNEXPECTED;
        m.header_off += place[i];
        m.data_off += place[i];
        m.name_off += place[i];
        if (m.dir_len) m.dir_off += place[i];
    }
    *out_len = (size_t)cursor;
    return BZ_OK;
}

extern "C" int bz_gpu_lha_write_device(bz_gpu_engine *g, int method, int level, const void *d_in, const uint64_t *h_in_off,
                                       const uint64_t *h_in_len, const bz_lha_entry *h_entries, size_t count, void *d_out, size_t cap,
                                       size_t *out_len, bz_lha_member *h_members)
{
    if (!g || !out_len || !d_out || (count && !h_in_off)) return BZ_E_PARAM;
    std::vector<u64> hsize;
    const int rc = lha_write_check(method, level, h_entries, h_in_len, count, &hsize);
    if (rc != BZ_OK) return rc;
    if ((uintptr_t)d_in & 15u) return BZ_E_PARAM;
    u64 in_end = 0;
    for (size_t i = 0; i < count; ++i) {
        if ((h_in_off[i] & 15u) || h_in_off[i] < in_end || h_in_off[i] + h_in_len[i] < h_in_off[i]) return BZ_E_PARAM;
        in_end = h_in_off[i] + h_in_len[i];
    }
    if (in_end && !d_in) return BZ_E_PARAM;
    return lha_write_core(g, method, level, d_in, h_in_off, h_in_len, h_entries, hsize, count, d_out, cap, out_len, h_members);
}

extern "C" int bz_lha_write_buffer(int method, int level, int device, const uint8_t *const *ins, const size_t *lens, const bz_lha_entry *entries,
                                   size_t count, uint8_t **out, size_t *out_len)
{
    if (!out || !out_len) return BZ_E_PARAM;
    *out = nullptr;
    *out_len = 0;
    if (count && (!ins || !lens)) return BZ_E_PARAM;
    const std::vector<u64> len64(lens, lens + count);
    std::vector<u64> hsize;
    int rc = lha_write_check(method, level, entries, len64.data(), count, &hsize);
    if (rc != BZ_OK) return rc;
    const BatchLayout lay(ins, lens, count, 16);
    if (lay.status != BZ_OK) return lay.status;
    if (count == 0) { // the end byte alone
        if ((rc = one_shot_empty(out)) != BZ_OK) return rc;
        (*out)[0] = 0;
        *out_len = 1;
        return BZ_OK;
    }
    const size_t bound = bz_lha_write_bound(level, entries, len64.data(), count);
    size_t n = 0;
    rc = one_shot(device, 0, lay, bound, kSettleStatus, out, [&](bz_gpu_engine *g, size_t *total) {
        const int wrc = lha_write_core(g, method, level, g->dec_in.p, lay.in_off.data(), lay.in_len.data(), entries, hsize, count,
                                       g->oneshot_out.p, bound, &n, nullptr);
        *total = n;
        return wrc;
    });
    if (rc == BZ_OK) *out_len = n;
    return rc;
}
