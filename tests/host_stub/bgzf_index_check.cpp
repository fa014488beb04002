// bgzf_index_check.cpp -- csrc/bgzf_index.h on the CPU (tests/test_bgzf_index_host.py), compiled by g++ as it is.
//
//   bgzf_index_check scan FILE    FILE holds lines "name hex-bytes"; prints "name: p p p ..." -- every position of the buffer
//                                 that bgzf::candidate_at accepts.  Each buffer is copied into a block of exactly its length
//                                 first, so that a read at or behind its end is an error under AddressSanitizer.
//   bgzf_index_check chain FILE   the same buffers through bgzf::chain_host; prints "name: verdict | coff ... | uoff ...".
//   bgzf_index_check rules        head_verdict / isize_verdict at their edges and bgzf::touched against a search by hand
//                                 over synthetic indexes (empty blocks at every place); prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../rust-compression_amd/csrc/bgzf_index.h"

using u64 = uint64_t;

template <class F> static int each_buffer(const char *path, F &&f)
{
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string name, hex;
        ss >> name >> hex; // (an empty buffer has no second word)
        const size_t n = hex.size() / 2;
        uint8_t *buf = static_cast<uint8_t *>(malloc(n ? n : 1));
        for (size_t i = 0; i < n; ++i) buf[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        printf("%s:", name.c_str());
        f(buf, n);
        printf("\n");
        free(buf);
    }
    return 0;
}

static int scan(const char *path)
{
    return each_buffer(path, [](const uint8_t *buf, size_t n) {
        for (u64 p = 0; p < n + 2; ++p) // (positions at and behind the end are asked about too: never a candidate)
            if (bgzf::candidate_at(buf, n, p)) printf(" %llu", (unsigned long long)p);
    });
}

static int chain(const char *path)
{
    return each_buffer(path, [](const uint8_t *buf, size_t n) {
        std::vector<u64> c, u;
        u64 ec = 0, eu = 0;
        int v = 0;
        const int rc = bgzf::chain_host(buf, n, [&](u64 a, u64 b) { c.push_back(a); u.push_back(b); }, &ec, &eu, &v);
        if (rc != 0) exit(3);
        c.push_back(ec);
        u.push_back(eu);
        printf(" %d |", v);
        for (u64 x : c) printf(" %llu", (unsigned long long)x);
        printf(" |");
        for (u64 x : u) printf(" %llu", (unsigned long long)x);
    });
}

static int fails = 0;
#define EXPECT(c)                                      \
    do {                                               \
        if (!(c)) {                                    \
            printf("FAIL line %d: %s\n", __LINE__, #c); \
            ++fails;                                   \
        }                                              \
    } while (0)

static int rules()
{
    using namespace bgzf;
    EXPECT(head_verdict(17, true, 28) == kEof);      // a cut header, whatever its bytes are
    EXPECT(head_verdict(1, false, 0) == kEof);
    EXPECT(head_verdict(18, false, 28) == kData);
    EXPECT(head_verdict(18, true, 27) == kData);     // BSIZE + 1 < 28 comes before "does not fit"
    EXPECT(head_verdict(18, true, 28) == kEof);
    EXPECT(head_verdict(27, true, 28) == kEof);
    EXPECT(head_verdict(28, true, 28) == kOk);
    EXPECT(head_verdict(65536, true, 65536) == kOk);
    EXPECT(head_verdict(65535, true, 65536) == kEof);
    EXPECT(isize_verdict(0) == kOk && isize_verdict(65536) == kOk && isize_verdict(65537) == kData && isize_verdict(0xFFFFFFFFu) == kData);
    EXPECT(header_words(0x04088B1Fu, 0x0006FF00u, 0x00024342u));
    EXPECT(header_words(0x04088B1Fu, 0x00061234u, 0x00024342u));
    EXPECT(!header_words(0x0C088B1Fu, 0x0006FF00u, 0x00024342u));
    EXPECT(!header_words(0x04088B1Fu, 0x000AFF00u, 0x00024342u));
    EXPECT(!header_words(0x04088B1Fu, 0x0006FF00u, 0x01024342u));
    // touched(): block sizes drawn from {0, 1, 5}, every range of every index of up to six blocks
    for (u64 code = 0; code < 729; ++code) {
        for (u64 count = 1; count <= 6; ++count) {
            static const u64 sizes[3] = {0, 1, 5};
            std::vector<u64> uoff(1, 7); // (uoff[0] need not be 0)
            u64 c = code;
            for (u64 k = 0; k < count; ++k, c /= 3) uoff.push_back(uoff.back() + sizes[c % 3]);
            for (u64 s = uoff[0]; s < uoff[count]; ++s)
                for (u64 e = s + 1; e <= uoff[count]; ++e) {
                    u64 first = ~0ull, last = ~0ull, wf = ~0ull, wl = ~0ull;
                    touched(uoff.data(), count, s, e, &first, &last);
                    for (u64 k = 0; k < count; ++k) {
                        if (uoff[k] <= s && s < uoff[k + 1]) wf = k;         // the block that holds byte s
                        if (uoff[k] <= e - 1 && e - 1 < uoff[k + 1]) wl = k; // the block that holds byte e - 1
                    }
                    if (first != wf || last != wl) {
                        printf("FAIL touched: code %llu count %llu range %llu %llu: %llu %llu, want %llu %llu\n", (unsigned long long)code,
                               (unsigned long long)count, (unsigned long long)s, (unsigned long long)e, (unsigned long long)first,
                               (unsigned long long)last, (unsigned long long)wf, (unsigned long long)wl);
                        ++fails;
                    }
                }
        }
    }
    if (!fails) printf("ok\n");
    return fails ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "scan")) return scan(argv[2]);
    if (argc == 3 && !strcmp(argv[1], "chain")) return chain(argv[2]);
    if (argc == 2 && !strcmp(argv[1], "rules")) return rules();
    fprintf(stderr, "usage: bgzf_index_check scan FILE | chain FILE | rules\n");
    return 2;
}
