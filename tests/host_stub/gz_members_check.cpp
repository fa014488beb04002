// gz_members_check.cpp -- csrc/gz_members.h on the CPU (tests/test_gz_members_host.py), compiled by g++ as it is.
//
//   gz_members_check scan FILE    FILE holds lines "name hex-bytes"; prints "name: p p p ..." -- every position of the buffer
//                                 that gzmem::candidate_at accepts.  Each buffer is copied into a block of exactly its length
//                                 first, so that a read at or behind its end is an error under AddressSanitizer.
//   gz_members_check walk         drives gzmem::walk_step / extend_to, as the driver's loop does, over synthetic files whose
//                                 members, zeros, junk and false candidates are known, against the serial loop of the
//                                 contract; prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rust-compression_amd/csrc/gz_members.h"

using u64 = uint64_t;

static int scan(const char *path)
{
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string name, hex;
        ss >> name >> hex; // (an empty buffer has no second word)
        const size_t n = hex.size() / 2;
        uint8_t *buf = static_cast<uint8_t *>(malloc(n ? n : 1));
        for (size_t i = 0; i < n; ++i) buf[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        printf("%s:", name.c_str());
        for (u64 p = 0; p < n + 2; ++p) // (positions at and behind the end are asked about too: never a candidate)
            if (gzmem::candidate_at(buf, n, p)) printf(" %llu", (unsigned long long)p);
        printf("\n");
        free(buf);
    }
    return 0;
}

// ---- a synthetic file: what lies where is known, no byte is needed
struct Member {
    u64 start, end;  // [start, end): header to trailer
    int verdict;     // of the member decoded from all the bytes behind its start
};
struct File {
    u64 len = 0;
    std::vector<Member> members;  // in file order; zeros lie between them unless `junk` says otherwise
    std::vector<u64> falses;      // false candidates (inside members)
    u64 junk = ~0ull;             // a byte that is neither zero nor a candidate
};

struct Result {
    int verdict = 0;
    u64 members = 0, redecodes = 0, zeros = 0, unconfirmed = 0;
};

static const Member *member_at(const File &f, u64 p)
{
    for (const Member &m : f.members)
        if (m.start == p) return &m;
    return nullptr;
}
// the first byte at or behind p that is not zero: a member's start, the junk byte, or the file's end
static u64 nonzero_from(const File &f, u64 p)
{
    u64 best = f.len;
    for (const Member &m : f.members)
        if (m.start >= p && m.start < best) best = m.start;
    if (f.junk >= p && f.junk < best) best = f.junk;
    return best;
}

// the contract's loop
static Result serial(const File &f)
{
    Result r;
    u64 pos = 0;
    for (;;) {
        const u64 nz = nonzero_from(f, pos);
        r.zeros += nz - pos;
        pos = nz;
        if (pos == f.len) return r;
        const Member *m = member_at(f, pos);
        if (!m) {
            r.verdict = -1;
            return r;
        }
        r.members += 1;
        if (m->verdict != 0) {
            r.verdict = m->verdict;
            return r;
        }
        pos = m->end;
    }
}

// the driver's loop over the candidate list, with a decoder that sees only [start, span_end)
static Result walked(const File &f)
{
    std::vector<u64> cand;
    for (const Member &m : f.members) cand.push_back(m.start);
    for (u64 p : f.falses) cand.push_back(p);
    std::sort(cand.begin(), cand.end());
    Result r;
    const u64 total = cand.size();
    u64 p = nonzero_from(f, 0), i = 0;
    r.zeros += p;
    u64 confirmed = 0;
    while (p != f.len) {
        if (i >= total || cand[i] != p) { // no candidate: junk
            r.verdict = -1;
            break;
        }
        const Member *m = member_at(f, p);
        if (!m) { // the walk confirmed a false candidate: the rules are broken
            fprintf(stderr, "a false candidate at %llu was confirmed\n", (unsigned long long)p);
            exit(1);
        }
        u64 span_end = i + 1 < total ? cand[i + 1] : f.len;
        auto decode = [&](u64 end_of_span, u64 *end) { // section 5 on [p, end_of_span)
            if (m->verdict == 0 && m->end <= end_of_span) {
                *end = m->end;
                return 0;
            }
            if (m->verdict != 0 && m->verdict != gzmem::kEof && m->end <= end_of_span) {
                *end = m->end;
                return m->verdict; // (a data error at m->end)
            }
            *end = end_of_span;
            return gzmem::kEof;
        };
        u64 e = 0;
        int v = decode(span_end, &e);
        u64 next = i + 1;
        auto bound_of = [&]() { return next < total ? cand[next] : f.len; };
        u64 bound = bound_of(), nz = v == 0 ? std::min(nonzero_from(f, e), bound) : bound;
        gzmem::Step st = gzmem::walk_step(v, span_end, nz, bound, f.len);
        for (uint32_t round = 1; st == gzmem::Step::Extend; ++round) {
            r.redecodes += 1;
            const u64 ei = gzmem::extend_to(i, round);
            span_end = ei < total ? cand[ei] : f.len;
            v = decode(span_end, &e);
            if (v == gzmem::kEof && span_end < f.len) continue;
            while (next < total && cand[next] < e) ++next;
            bound = bound_of();
            nz = v == 0 ? std::min(nonzero_from(f, e), bound) : bound;
            st = gzmem::walk_step(v, span_end, nz, bound, f.len);
        }
        r.members += 1;
        confirmed += 1;
        if (st == gzmem::Step::Fault) {
            r.verdict = v;
            break;
        }
        r.zeros += nz - e;
        p = st == gzmem::Step::End ? f.len : nz;
        i = next;
    }
    r.unconfirmed = total - confirmed;
    return r;
}

static int fails = 0;
static void expect(const char *name, const File &f, u64 redecodes)
{
    const Result a = serial(f), b = walked(f);
    const bool same = a.verdict == b.verdict && a.members == b.members && a.zeros == b.zeros;
    if (!same || b.redecodes != redecodes) {
        printf("FAIL %s: serial verdict %d members %llu zeros %llu; walk verdict %d members %llu zeros %llu redecodes %llu (want %llu)\n", name, a.verdict,
               (unsigned long long)a.members, (unsigned long long)a.zeros, b.verdict, (unsigned long long)b.members, (unsigned long long)b.zeros,
               (unsigned long long)b.redecodes, (unsigned long long)redecodes);
        ++fails;
    }
}

static u64 ceil_log2(u64 x)
{
    u64 r = 0;
    while ((1ull << r) < x) ++r;
    return r;
}

static int walk()
{
    { // members back to back
        File f;
        f.len = 300;
        f.members = {{0, 100, 0}, {100, 200, 0}, {200, 300, 0}};
        expect("confirmed", f, 0);
    }
    { // zeros in front, between and behind
        File f;
        f.len = 400;
        f.members = {{7, 100, 0}, {105, 200, 0}, {200, 300, 0}};
        expect("zeros", f, 0);
        if (walked(f).zeros != 7 + 5 + 100) ++fails, printf("FAIL zeros counted\n");
    }
    { // nothing but zeros, and nothing at all
        File f;
        f.len = 64;
        expect("zeros_only", f, 0);
        f.len = 0;
        expect("empty", f, 0);
    }
    for (u64 k : {1, 2, 3, 5, 8, 9, 100}) { // k false candidates inside the middle member, then inside the last one
        File f;
        f.len = 10000;
        f.members = {{0, 100, 0}, {100, 5000, 0}, {5000, 10000, 0}};
        for (u64 q = 0; q < k; ++q) f.falses.push_back(200 + 20 * q);
        expect("false_middle", f, ceil_log2(k + 1));
        if (walked(f).unconfirmed != k) ++fails, printf("FAIL unconfirmed %llu\n", (unsigned long long)k);
        File g;
        g.len = 10000;
        g.members = {{0, 100, 0}, {100, 10000, 0}};
        for (u64 q = 0; q < k; ++q) g.falses.push_back(200 + 20 * q);
        expect("false_last", g, ceil_log2(k + 1));
    }
    { // an extension that runs over the members behind: they are still found
        File f;
        f.len = 1000;
        f.members = {{0, 500, 0}, {500, 600, 0}, {600, 700, 0}, {700, 800, 0}, {800, 1000, 0}};
        f.falses = {100, 200, 300};
        expect("overshoot", f, 2);
    }
    { // junk behind a member, with and without zeros in front of it
        File f;
        f.len = 300;
        f.members = {{0, 100, 0}, {100, 200, 0}};
        f.junk = 200;
        expect("junk", f, 0);
        f.junk = 250;
        expect("zeros_then_junk", f, 0);
        File g;
        g.len = 10;
        g.junk = 0;
        expect("junk_only", g, 0);
    }
    { // faults: a data error in the middle member, a file cut inside the last member, a cut member in front of an intact one
        File f;
        f.len = 300;
        f.members = {{0, 100, 0}, {100, 150, -1}, {200, 300, 0}};
        expect("data_error", f, 0);
        File g;
        g.len = 300;
        g.members = {{0, 100, 0}, {100, 300, gzmem::kEof}};
        expect("cut_last", g, 0);
        File h; // the second member never ends: the walk extends it over the third to the input's end
        h.len = 300;
        h.members = {{0, 100, 0}, {100, 300, gzmem::kEof}};
        h.falses = {200};
        expect("cut_then_candidate", h, 1);
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "scan")) return scan(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "walk")) return walk();
    fprintf(stderr, "usage: gz_members_check scan FILE | walk\n");
    return 2;
}
