// inf_split_check.cpp -- csrc/inf_split.h on the CPU (tests/test_inf_split_host.py).
//
//   inf_split_check FILE
//   inf_split_check --first PIECE_BYTES FILE
//
// 1. The candidate rules.  FILE holds streams, each with the bit positions the test knows about:
//        stream NAME NBYTES NPOS
//        HEX
//        POS MODE EXPECT        (NPOS lines; MODE 0: a dynamic header at that bit, 1: the LEN field of a stored block;
//                                EXPECT 1: must be accepted, 0: must be rejected)
//    Every listed position is checked; then EVERY bit position of the stream is run through the rules as the search kernel
//    runs them (prefilter, then the whole header), and the accepted positions that are not listed are counted and printed
//    ("false NAME COUNT").  The prefilter may never reject what the whole check accepts.
// 2. The chain.  Synthetic streams -- true block boundaries, true and false candidates, an end -- driven through
//    infsplit::chain_next as the host loop of df_split_sizes drives it, against a straightforward serial walk.
// --first: the search alone.  For every stream of FILE (the listed positions are read and ignored) and every piece of
//    PIECE_BYTES but the first, the first position of the piece's own span that the rules accept, as k_df_split_search
//    finds it (a dynamic header goes before a LEN field at the same bit): "first NAME PIECE POS MODE"; nothing for a piece
//    without a candidate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../rust-compression_amd/csrc/inf_split.h"

using namespace infsplit;

static int fails = 0;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            ++fails;                  \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");             \
        }                             \
    } while (0)

// bits [bit, bit + 128) as the kernel's lanes put them together
static void bits128(const BitSrc &s, uint64_t bit, uint64_t &lo, uint64_t &hi)
{
    lo = hi = 0;
    for (uint32_t k = 0; k < 128; ++k) {
        const uint64_t b = bit + k;
        const uint64_t v = (b >> 3) < s.len ? (s.base[b >> 3] >> (b & 7u)) & 1u : 0u;
        (k < 64 ? lo : hi) |= v << (k & 63u);
    }
}
static bool dyn_at(const BitSrc &s, uint64_t bit, bool &pre)
{
    uint64_t lo, hi;
    bits128(s, bit, lo, hi);
    pre = dyn_prefilter(lo, hi);
    return dyn_header_ok(s, bit, false);
}

static void candidate_rules(const char *path)
{
    FILE *f = fopen(path, "r");
    if (!f) {
        printf("FAIL: cannot open %s\n", path);
        ++fails;
        return;
    }
    char name[256];
    unsigned long long nbytes, npos;
    int streams = 0;
    while (fscanf(f, " stream %255s %llu %llu", name, &nbytes, &npos) == 3) {
        ++streams;
        // (an exact-size heap block: a read behind the entry is AddressSanitizer's to find)
        uint8_t *buf = (uint8_t *)malloc(nbytes ? nbytes : 1);
        for (unsigned long long i = 0; i < nbytes; ++i) {
            unsigned v = 0;
            if (fscanf(f, "%2x", &v) != 1) CHECK(false, "%s: short hex", name);
            buf[i] = (uint8_t)v;
        }
        const BitSrc s{buf, nbytes};
        std::set<std::pair<uint64_t, uint32_t>> listed;
        for (unsigned long long k = 0; k < npos; ++k) {
            unsigned long long pos;
            unsigned mode, expect;
            if (fscanf(f, "%llu %u %u", &pos, &mode, &expect) != 3) {
                CHECK(false, "%s: short position list", name);
                break;
            }
            listed.insert({pos, mode});
            bool pre = false;
            const bool got = mode == 0 ? dyn_at(s, pos, pre) && pre : stored_ok(s, pos);
            CHECK(got == (expect != 0), "%s: position %llu mode %u: %s, expected %s", name, pos, mode, got ? "accepted" : "rejected",
                  expect ? "accepted" : "rejected");
        }
        unsigned long long extra = 0;
        for (uint64_t bit = 0; bit < 8 * nbytes; ++bit) {
            bool pre = false;
            const bool ok = dyn_at(s, bit, pre);
            CHECK(pre || !ok, "%s: bit %llu: the prefilter rejects a header the whole check accepts", name, (unsigned long long)bit);
            if (ok && pre && !listed.count({bit, 0u})) ++extra;
            if ((bit & 7u) == 0 && stored_ok(s, bit) && !listed.count({bit, 1u})) ++extra;
        }
        printf("false %s %llu\n", name, extra);
        free(buf);
    }
    fclose(f);
    CHECK(streams > 0, "no stream in %s", path);
}

static void first_candidates(const char *path, unsigned long long piece_bytes)
{
    FILE *f = fopen(path, "r");
    if (!f || piece_bytes == 0) {
        printf("FAIL: cannot open %s, or a piece of no bytes\n", path);
        ++fails;
        return;
    }
    char name[256];
    unsigned long long nbytes, npos;
    int streams = 0;
    while (fscanf(f, " stream %255s %llu %llu", name, &nbytes, &npos) == 3) {
        ++streams;
        uint8_t *buf = (uint8_t *)malloc(nbytes ? nbytes : 1);
        for (unsigned long long i = 0; i < nbytes; ++i) {
            unsigned v = 0;
            if (fscanf(f, "%2x", &v) != 1) CHECK(false, "%s: short hex", name);
            buf[i] = (uint8_t)v;
        }
        for (unsigned long long k = 0; k < npos; ++k) {
            unsigned long long pos;
            unsigned mode, expect;
            if (fscanf(f, "%llu %u %u", &pos, &mode, &expect) != 3) {
                CHECK(false, "%s: short position list", name);
                break;
            }
        }
        const BitSrc s{buf, nbytes};
        const uint64_t total = 8 * nbytes;
        for (uint64_t k = 1; 8 * k * piece_bytes < total; ++k) {
            const uint64_t lo = 8 * k * piece_bytes, hi = lo + 8 * piece_bytes < total ? lo + 8 * piece_bytes : total;
            for (uint64_t bit = lo; bit < hi; ++bit) {
                bool pre = false;
                const bool dyn = dyn_at(s, bit, pre) && pre;
                if (dyn || ((bit & 7u) == 0 && stored_ok(s, bit))) {
                    printf("first %s %llu %llu %u\n", name, (unsigned long long)k, (unsigned long long)bit, dyn ? 0u : 1u);
                    break;
                }
            }
        }
        free(buf);
    }
    fclose(f);
    CHECK(streams > 0, "no stream in %s", path);
}

// ---- the chain
struct Model {
    std::vector<Cand> bounds;    // the true block boundaries from the stream's first bit on, ascending
    size_t last;                 // the stream ends inside the block that starts at bounds[last] (its final block, or an error) ...
    uint64_t end_pos;            // ... at this bit
    std::vector<Cand> cands;     // what the search found, ascending: some of bounds[1 ..], and some that are no boundary
};
struct Step {
    uint64_t start, stop;
    uint32_t mode, how; // 0 first, 1 confirmed, 2 repair, 3 tail
    bool operator==(const Step &o) const { return start == o.start && stop == o.stop && mode == o.mode && how == o.how; }
};
static bool is_bound(const Model &m, uint64_t pos, uint32_t mode, size_t *at)
{
    for (size_t i = 0; i < m.bounds.size(); ++i)
        if (m.bounds[i].pos == pos && m.bounds[i].mode == mode) {
            *at = i;
            return true;
        }
    return false;
}
// what a wave that starts at (pos, mode) reports: from a true boundary the truth, from anywhere else something plausible
static PieceEnd decode(const Model &m, uint64_t pos, uint32_t mode, uint64_t stop, uint32_t &rng)
{
    size_t i;
    if (!is_bound(m, pos, mode, &i) || i > m.last) { // (a boundary behind the stream's end is junk like any other)
        rng = rng * 1664525u + 1013904223u;
        if (rng & 0x10000u) return PieceEnd{pos + 1 + (rng >> 20) % 97u, 0, true}; // an error soon
        return PieceEnd{(stop == kNoStop ? pos : stop) + (rng >> 20) % 5u, (rng >> 8) & 1u, stop == kNoStop}; // or a "boundary"
    }
    for (size_t k = i;; ++k) { // block k, then the boundary behind it
        if (k > i && m.bounds[k].pos >= stop) return PieceEnd{m.bounds[k].pos, m.bounds[k].mode, false};
        if (k == m.last) return PieceEnd{m.end_pos, 0, true};
    }
}
// the host loop of df_split_sizes
static std::vector<Step> drive(const Model &m, uint32_t seed)
{
    std::vector<Step> out;
    uint32_t rng = seed;
    const size_t n = m.cands.size();
    std::vector<PieceEnd> ends(n + 1);
    ends[0] = decode(m, 0, 0, n ? m.cands[0].pos : kNoStop, rng);
    for (size_t k = 0; k < n; ++k) ends[k + 1] = decode(m, m.cands[k].pos, m.cands[k].mode, k + 1 < n ? m.cands[k + 1].pos : kNoStop, rng);
    Step cur{0, n ? m.cands[0].pos : kNoStop, 0, 0};
    PieceEnd e = ends[0];
    uint64_t j = 0;
    uint32_t repairs = 0;
    for (int guard = 0; guard < 100000; ++guard) {
        out.push_back(cur);
        uint64_t stop = kNoStop;
        const Next nx = chain_next(m.cands.data(), n, e, repairs, j, stop);
        if (nx == Next::Done) return out;
        if (nx == Next::Confirmed) {
            cur = Step{m.cands[j].pos, j + 1 < n ? m.cands[j + 1].pos : kNoStop, m.cands[j].mode, 1};
            e = ends[j + 1];
            ++j;
            continue;
        }
        cur = Step{e.pos, stop, e.mode, nx == Next::Repair ? 2u : 3u};
        e = decode(m, e.pos, e.mode, stop, rng);
        if (nx == Next::Repair) ++repairs;
    }
    CHECK(false, "the chain does not end");
    return out;
}
// the same stream walked block by block
static std::vector<Step> serial(const Model &m)
{
    std::vector<Step> out;
    size_t i = 0;
    uint32_t how = 0, repairs = 0;
    for (;;) {
        const uint64_t pos = m.bounds[i].pos;
        uint64_t stop = kNoStop;
        if (how != 3)
            for (const Cand &c : m.cands)
                if (c.pos > pos) {
                    stop = c.pos;
                    break;
                }
        out.push_back(Step{pos, stop, m.bounds[i].mode, how});
        size_t k = i + 1;
        while (k <= m.last && m.bounds[k].pos < stop) ++k;
        if (k > m.last) return out; // the stream ended in this piece
        bool cand = false;
        for (const Cand &c : m.cands) cand = cand || (c.pos == m.bounds[k].pos && c.mode == m.bounds[k].mode);
        if (cand) how = 1;
        else if (repairs < kRepairRounds) {
            how = 2;
            ++repairs;
        } else how = 3;
        i = k;
    }
}
static void chain_case(const char *what, const Model &m, uint32_t seed)
{
    const std::vector<Step> a = drive(m, seed), b = serial(m);
    bool same = a.size() == b.size();
    for (size_t i = 0; same && i < a.size(); ++i) same = a[i] == b[i];
    CHECK(same, "chain %s (seed %u): %zu pieces against %zu of the serial walk", what, seed, a.size(), b.size());
    if (!same)
        for (size_t i = 0; i < a.size() || i < b.size(); ++i) {
            if (i < a.size()) printf("   chain  %llu..%llu mode %u how %u\n", (unsigned long long)a[i].start, (unsigned long long)a[i].stop, a[i].mode, a[i].how);
            if (i < b.size()) printf("   serial %llu..%llu mode %u how %u\n", (unsigned long long)b[i].start, (unsigned long long)b[i].stop, b[i].mode, b[i].how);
        }
}
// nb blocks 1000 bits apart (every third boundary a stored block's LEN); a candidate at the true boundaries in `truth`, false
// ones at the (boundary, offset) pairs in `falses`; the stream ends in block `last`
static Model model(size_t nb, size_t last, const std::vector<size_t> &truth, const std::vector<std::pair<size_t, uint32_t>> &falses)
{
    Model m;
    for (size_t i = 0; i < nb; ++i) m.bounds.push_back(Cand{i ? 1000ull * i + (i % 3 == 0 ? 0 : i % 7) : 0, i && i % 3 == 0 ? 1u : 0u, 0});
    m.last = last;
    m.end_pos = m.bounds[last].pos + 500;
    std::set<std::pair<uint64_t, uint32_t>> c;
    for (size_t t : truth) c.insert({m.bounds[t].pos, m.bounds[t].mode});
    for (auto &f : falses) c.insert({m.bounds[f.first].pos + f.second, f.second == 0 ? 1u - m.bounds[f.first].mode : (uint32_t)(f.second & 1u)});
    std::set<uint64_t> seen; // (the search finds at most one candidate per piece: one per position here)
    for (auto &x : c)
        if (seen.insert(x.first).second) m.cands.push_back(Cand{x.first, x.second, 0});
    return m;
}
static void chain_rules()
{
    const std::vector<size_t> all = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    for (uint32_t seed = 1; seed <= 8; ++seed) {
        chain_case("no candidate at all", model(12, 11, {}, {}), seed);
        chain_case("every boundary", model(12, 11, all, {}), seed);
        chain_case("false first", model(12, 11, all, {{0, 400}}), seed);
        chain_case("false in the middle", model(12, 11, all, {{5, 300}}), seed);
        chain_case("false last", model(12, 11, all, {{11, 200}}), seed);
        chain_case("two false in a row", model(12, 11, all, {{4, 100}, {4, 301}}), seed);
        chain_case("four false in a row", model(12, 11, all, {{4, 100}, {4, 301}, {4, 502}, {4, 703}}), seed);
        chain_case("empty pieces", model(12, 11, {2, 9}, {}), seed);
        chain_case("empty pieces and a false one", model(12, 11, {2, 9}, {{5, 11}}), seed);
        chain_case("the final block in a middle piece", model(12, 5, all, {}), seed);
        chain_case("the final block in the first piece", model(12, 0, all, {{0, 77}}), seed);
        chain_case("an error in a confirmed piece behind a false one", model(12, 7, all, {{3, 123}}), seed);
        chain_case("five repairs: the tail", model(12, 11, all, {{1, 100}, {3, 301}, {5, 502}, {7, 703}, {9, 104}}), seed);
        chain_case("seven false in a row: the tail", model(12, 11, {1, 10, 11}, {{2, 1}, {3, 2}, {4, 3}, {5, 4}, {6, 5}, {7, 6}, {8, 9}}), seed);
        chain_case("the tail ends in the middle", model(12, 9, {1}, {{2, 1}, {3, 2}, {4, 3}, {5, 4}, {6, 5}, {7, 6}}), seed);
        chain_case("a LEN field and a header bit at one position", model(12, 11, {1, 2, 4, 5}, {{3, 0}, {6, 0}}), seed);
        chain_case("only false ones", model(12, 11, {}, {{1, 50}, {2, 51}, {6, 52}}), seed);
    }
    // ... and at random
    uint32_t r = 12345;
    auto next = [&r](uint32_t n) {
        r = r * 1664525u + 1013904223u;
        return (r >> 8) % n;
    };
    for (int t = 0; t < 4000; ++t) {
        const size_t nb = 2 + next(30), last = next((uint32_t)nb);
        std::vector<size_t> truth;
        std::vector<std::pair<size_t, uint32_t>> falses;
        const uint32_t pt = next(101), pf = next(60);
        for (size_t i = 1; i < nb; ++i)
            if (next(100) < pt) truth.push_back(i);
        for (size_t i = 0; i < nb; ++i)
            for (uint32_t k = 0; k < 3; ++k)
                if (next(100) < pf) falses.push_back({i, k == 0 && i ? 0u : 8u + next(900)});
        chain_case("random", model(nb, last, truth, falses), (uint32_t)t);
    }
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "--first") == 0) {
        first_candidates(argv[3], strtoull(argv[2], nullptr, 10));
        if (fails == 0) printf("ok\n");
        return fails ? 1 : 0;
    }
    if (argc != 2) {
        printf("usage: inf_split_check FILE | inf_split_check --first PIECE_BYTES FILE\n");
        return 2;
    }
    candidate_rules(argv[1]);
    chain_rules();
    if (fails == 0) printf("ok\n");
    return fails ? 1 : 0;
}
