// lzh_split_check.cpp -- csrc/lzh_split.h compiled AS IT IS by g++ (plain C++17, no HIP headers), plain and under
// -fsanitize=address,undefined (tests/test_lzhsplit.py).
//
//   lzh_split_check FILE
//
// FILE holds lines
//   stream NAME METHOD HEX          the entry's bytes
//   ends NAME K (END ENDED){K}      where piece k ended (piece 0 starts at bit 0, piece k >= 1 at the k-th candidate behind
//                                   bit 0) and whether the stream ended in it: what the sizes launch would leave
// For every stream the program prints "cand NAME POS ..." -- every bit offset of the entry run through prefilter() and
// header_ok(), as k_lzh_split_search runs them -- and for every ends line "chain NAME PIECE ... done|broken": the walk of
// lzhsplit::chain_next from piece 0.  The bytes of an entry live in a heap block of exactly their size, so a read behind the
// entry's end is the sanitizer's to find.  A position that header_ok() accepts and prefilter() refuses is an error: the
// prefilter may only refuse what the whole check refuses.
#include "../../rust-compression_amd/csrc/lzh_split.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

namespace {
struct Entry {
    std::unique_ptr<uint8_t[]> bytes;
    uint64_t len = 0;
    int method = 0;
    std::vector<uint64_t> cands; // ascending, bit 0 included when it is one
};

// bits [bit, bit + 64) of the entry, MSB first, zeros behind its end: what the search kernel puts together from five words
uint64_t window(const Entry &e, uint64_t bit)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < 64; ++k) {
        const uint64_t b = bit + k;
        const uint32_t x = (b >> 3) < e.len ? (e.bytes[b >> 3] >> (7u - (b & 7u))) & 1u : 0u;
        v = v << 1 | x;
    }
    return v;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: lzh_split_check FILE\n");
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::map<std::string, Entry> entries;
    std::string line;
    int bad = 0;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        std::string kind, name;
        ls >> kind >> name;
        if (kind == "stream") {
            std::string hex;
            Entry e;
            ls >> e.method >> hex;
            if (hex == "-") hex.clear();
            e.len = hex.size() / 2;
            e.bytes.reset(new uint8_t[e.len ? e.len : 1]);
            for (uint64_t i = 0; i < e.len; ++i) e.bytes[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
            const uint32_t dbits = e.method == 4 ? 12 : e.method == 5 ? 13 : e.method == 6 ? 15 : 16, pbits = e.method < 6 ? 4 : 5;
            printf("cand %s", name.c_str());
            for (uint64_t bit = 0; bit < 8 * e.len; ++bit) {
                const bool pre = lzhsplit::prefilter(window(e, bit), window(e, bit + 64));
                const bool whole = lzhsplit::header_ok(e.bytes.get(), e.len, bit, dbits, pbits);
                if (whole && !pre) {
                    fprintf(stderr, "%s: the prefilter refuses bit %llu, the whole check accepts it\n", name.c_str(), (unsigned long long)bit);
                    ++bad;
                }
                if (pre && whole) {
                    e.cands.push_back(bit);
                    printf(" %llu", (unsigned long long)bit);
                }
            }
            printf("\n");
            entries[name] = std::move(e);
        } else if (kind == "ends") {
            const Entry &e = entries.at(name);
            std::vector<uint64_t> c;
            for (uint64_t p : e.cands)
                if (p != 0) c.push_back(p);
            size_t k = 0;
            ls >> k;
            std::vector<lzhsplit::PieceEnd> ends(k);
            for (auto &x : ends) {
                int ended = 0;
                ls >> x.pos >> ended;
                x.ended = ended != 0;
            }
            printf("chain %s", name.c_str());
            uint64_t j = 0;
            size_t cur = 0;
            for (;;) {
                if (cur >= ends.size()) {
                    fprintf(stderr, "%s: piece %zu has no end\n", name.c_str(), cur);
                    return 1;
                }
                printf(" %zu", cur);
                const lzhsplit::Next nx = lzhsplit::chain_next(c.data(), c.size(), ends[cur], j);
                if (nx == lzhsplit::Next::Done) {
                    printf(" done\n");
                    break;
                }
                if (nx == lzhsplit::Next::Broken) {
                    printf(" broken\n");
                    break;
                }
                cur = 1 + (size_t)j++;
            }
        }
    }
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
