// host_call_check.cpp -- csrc/host_call.h, csrc/one_shot.h and csrc/batch_decode.h on the host
// (tests/test_host_call_host.py): the keep-or-destroy rule of EngineLease against stand-ins for the engine cache and the
// engine that count their calls, the caller's device on every path, BatchLayout against a transcription of the four
// packing loops it replaced, the round trip of the one-shot calls around a stand-in device call (its bytes, its failed
// allocations, its two settle rules), and the frame of the batch decoders (ranges, places, the split entries' reservation,
// the jump rounds) against stand-ins for the two launchers.  Exits non-zero at the first failure.
#include "../../rust-compression_amd/csrc/host_call.h"
#include "../../rust-compression_amd/csrc/dev_buf.h"

#include <algorithm>
#include <cstdio>
#include <type_traits>

static_assert(!std::is_copy_constructible<EngineLease>::value && !std::is_copy_assignable<EngineLease>::value,
              "a lease is not copied: one engine, one end");

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "host_call_check: line %d: %s\n", __LINE__, #cond);    \
            return 1;                                                              \
        }                                                                          \
    } while (0)

// ---- stand-ins: an engine is a heap block, so that one the lease forgets or ends twice is the sanitizer's finding too
struct bz_gpu_engine {
    int device;
    DevBuf dec_in, oneshot_out;
};
#include "../../rust-compression_amd/csrc/batch_decode.h"
#include "../../rust-compression_amd/csrc/one_shot.h" // (behind the engine, as in engine_state.h)

// the download's block of an absurd size is refused, not fatal, under the sanitizer too
extern "C" const char *__asan_default_options() { return "allocator_may_return_null=1"; }
static int n_take, n_put, n_create, n_destroy, last_prefer, put_device, create_fails_with;
static size_t last_max_blocks;
static bz_gpu_engine *parked; // what the cache holds (one engine is enough here)

bz_gpu_engine *dec_cache_take(int device, int prefer)
{
    ++n_take;
    last_prefer = prefer;
    bz_gpu_engine *g = parked && parked->device == device ? parked : nullptr;
    if (g) parked = nullptr;
    return g;
}
void dec_cache_put(int device, bz_gpu_engine *g)
{
    ++n_put;
    put_device = device;
    delete parked;
    parked = g;
}
void dec_release_cached()
{
    delete parked;
    parked = nullptr;
}
extern "C" int bz_gpu_engine_create(bz_gpu_engine **out, int device, size_t max_blocks)
{
    ++n_create;
    last_max_blocks = max_blocks;
    *out = nullptr;
    if (create_fails_with) return create_fails_with;
    (void)hipSetDevice(device); // (as the engine does: in front of the steps that can fail)
    *out = new bz_gpu_engine{device};
    return BZ_OK;
}
extern "C" void bz_gpu_engine_destroy(bz_gpu_engine *g)
{
    ++n_destroy;
    delete g;
}
static void reset_counts() { n_take = n_put = n_create = n_destroy = 0; }
static int device_now()
{
    int d = -1;
    (void)hipGetDevice(&d);
    return d;
}

static int check_lease()
{
    const int mine = 1, theirs = 3; // the caller's device and the lease's (the shim reports four)
    CHECK(hipSetDevice(mine) == hipSuccess);

    reset_counts(); // settled OK: parked
    {
        EngineLease lease(theirs, 2, 1);
        CHECK(lease.status() == BZ_OK && lease.engine() && lease.engine()->device == theirs && device_now() == theirs);
        CHECK(n_take == 1 && last_prefer == 2 && n_create == 1 && last_max_blocks == 1);
        lease.settle(BZ_OK);
    }
    CHECK(n_put == 1 && put_device == theirs && n_destroy == 0 && device_now() == mine);

    reset_counts(); // the next call finds it; settled with an error: destroyed
    {
        EngineLease lease(theirs, 1, 0);
        CHECK(lease.status() == BZ_OK && lease.engine() && n_take == 1 && last_prefer == 1 && n_create == 0 && device_now() == theirs);
        lease.settle(BZ_E_NOMEM);
    }
    CHECK(n_put == 0 && n_destroy == 1 && parked == nullptr && device_now() == mine);

    reset_counts(); // never settled: destroyed
    {
        EngineLease lease(theirs, 1, 0);
        CHECK(lease.status() == BZ_OK && n_create == 1 && last_max_blocks == 0);
    }
    CHECK(n_put == 0 && n_destroy == 1 && device_now() == mine);

    reset_counts(); // an OK that a later error replaces: the last word counts
    {
        EngineLease lease(theirs, 1, 0);
        lease.settle(BZ_OK);
        lease.settle(BZ_E_UNEXPECTED);
    }
    CHECK(n_put == 0 && n_destroy == 1 && device_now() == mine);

    for (int code : {BZ_E_PARAM, BZ_E_NOGPU, BZ_E_UNEXPECTED}) { // create fails: nothing to end, the status passed on
        reset_counts();
        create_fails_with = code;
        {
            EngineLease lease(theirs, 2, 1);
            CHECK(lease.status() == code && lease.engine() == nullptr);
            CHECK(hipSetDevice(2) == hipSuccess); // (whatever the failed creation left selected)
            lease.settle(BZ_OK);                  // (even so: there is no engine to park)
        }
        create_fails_with = 0;
        CHECK(n_create == 1 && n_put == 0 && n_destroy == 0 && device_now() == mine);
    }

    reset_counts(); // a device the runtime refuses: the status says so, the new engine is not kept
    {
        EngineLease lease(hipshim::kDevices, 2, 1);
        CHECK(lease.status() == BZ_E_UNEXPECTED);
    }
    CHECK(n_put == 0 && n_destroy == 1 && device_now() == mine);

    for (int end : {BZ_OK, BZ_E_UNEXPECTED}) { // release / adopt: a context holds the engine across calls
        reset_counts();
        bz_gpu_engine *held = nullptr;
        {
            EngineLease lease(theirs, 2, 0);
            CHECK(lease.status() == BZ_OK);
            held = lease.release();
            CHECK(held && lease.engine() == nullptr && lease.status() == BZ_OK);
            lease.settle(BZ_OK); // (nothing left to settle)
        }
        CHECK(n_put == 0 && n_destroy == 0 && device_now() == mine);
        { // a later call of the context
            EngineLease lease(theirs, held);
            CHECK(lease.status() == BZ_OK && lease.engine() == held && device_now() == theirs && n_take == 1 && n_create == 1);
            CHECK(lease.release() == held);
        }
        CHECK(n_put == 0 && n_destroy == 0 && device_now() == mine);
        EngineLease(theirs, held).settle(end); // the context's end
        CHECK(n_put == (end == BZ_OK ? 1 : 0) && n_destroy == (end == BZ_OK ? 0 : 1) && device_now() == mine);
        dec_release_cached();
    }
    return 0;
}

// ---- BatchLayout against the loops as they stood in bz_encode_batch / df_encode_batch (16), df_decode_batch and
// bz_decode_batch (4)
static void old_offsets(int form, const size_t *lens, size_t count, std::vector<uint64_t> &off, uint64_t &total)
{
    off.assign(count, 0);
    total = 0;
    for (size_t i = 0; i < count; ++i) {
        off[i] = total;
        if (form == 0) total += ((uint64_t)lens[i] + 15u) & ~(uint64_t)15;     // bz_encode_batch, df_encode_batch
        else if (form == 1) total += ((uint64_t)lens[i] + 3u) & ~(uint64_t)3; // df_decode_batch
        else total = (total + lens[i] + 3ull) & ~3ull;                        // bz_decode_batch
    }
}

static int check_layout()
{
    static const size_t kLens[10] = {0, 1, 3, 4, 5, 15, 16, 17, 65535, 65536};
    std::vector<uint8_t> src(65536);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(1 + i % 255); // (no zero byte: padding shows)
    uint32_t rnd = 12345;
    for (uint64_t align : {(uint64_t)4, (uint64_t)16})
        for (size_t count : {(size_t)0, (size_t)1, (size_t)7})
            for (int round = 0; round < 40; ++round) {
                std::vector<size_t> lens(count);
                std::vector<const uint8_t *> ins(count);
                for (size_t i = 0; i < count; ++i) {
                    rnd = rnd * 1664525u + 1013904223u;
                    lens[i] = round < 10 && count == 1 ? kLens[round] : kLens[(rnd >> 16) % 10];
                    ins[i] = lens[i] || (rnd & 1u) ? src.data() + (rnd >> 8) % (src.size() - lens[i] + 1) : nullptr; // (null with length 0 is fine)
                }
                const BatchLayout lay(ins.data(), lens.data(), count, align);
                std::vector<uint64_t> off;
                uint64_t total = 0;
                old_offsets(align == 16 ? 0 : 1, lens.data(), count, off, total);
                if (align == 4) {
                    std::vector<uint64_t> off2;
                    uint64_t total2 = 0;
                    old_offsets(2, lens.data(), count, off2, total2);
                    CHECK(off2 == off && total2 == total);
                }
                CHECK(lay.status == BZ_OK && lay.total == total && lay.in_off == off && lay.in_len.size() == count);
                for (size_t i = 0; i < count; ++i) CHECK(lay.in_len[i] == lens[i] && lay.in_off[i] % align == 0);
                // packed into a zeroed image that ends at `total`, with guard bytes behind it (and the sanitizer's red zone)
                std::vector<uint8_t> img((size_t)total + 64, 0);
                std::fill(img.begin() + (ptrdiff_t)total, img.end(), (uint8_t)0xEE);
                lay.pack_into(img.data());
                uint64_t at = 0;
                for (size_t i = 0; i < count; ++i) {
                    for (; at < off[i]; ++at) CHECK(img[(size_t)at] == 0);
                    CHECK(lens[i] == 0 || memcmp(img.data() + at, ins[i], lens[i]) == 0);
                    at += lens[i];
                }
                for (; at < total; ++at) CHECK(img[(size_t)at] == 0);
                for (size_t k = (size_t)total; k < img.size(); ++k) CHECK(img[k] == 0xEE);
                std::vector<uint8_t> exact((size_t)total); // (no slack at all: a byte behind `total` is out of bounds)
                size_t copies = 0;
                lay.pack_into(exact.data(), [&](uint8_t *d, const uint8_t *s, size_t n) { memcpy(d, s, n); ++copies; });
                CHECK(total == 0 || memcmp(exact.data(), img.data(), (size_t)total) == 0);
                size_t nonempty = 0;
                for (size_t n : lens) nonempty += n ? 1 : 0;
                CHECK(copies == nonempty);
            }
    { // bytes announced without a pointer
        const uint8_t *ins[3] = {src.data(), nullptr, src.data()};
        const size_t lens[3] = {4, 1, 4};
        CHECK(BatchLayout(ins, lens, 3, 4).status == BZ_E_PARAM && BatchLayout(ins, lens, 3, 16).status == BZ_E_PARAM);
        const size_t fine[3] = {4, 0, 4};
        CHECK(BatchLayout(ins, fine, 3, 4).status == BZ_OK);
    }
    CHECK(BatchLayout(nullptr, nullptr, 0, 16).status == BZ_OK && BatchLayout(nullptr, nullptr, 0, 16).total == 0);
    return 0;
}

// ---- the round trip: the stand-in device call writes the uploaded bytes, each + 1, `shift` bytes into oneshot_out
static int check_one_shot()
{
    const int mine = 1, theirs = 2;
    CHECK(hipSetDevice(mine) == hipSuccess);
    dec_release_cached();
    std::vector<uint8_t> a(5000), b(300);
    for (size_t i = 0; i < a.size(); ++i) a[i] = (uint8_t)(i * 7 + 1);
    for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i * 13 + 5);
    const uint8_t *ins[3] = {a.data(), nullptr, b.data()};
    const size_t lens[3] = {a.size(), 0, b.size()};
    const BatchLayout lay(ins, lens, 3, 16);
    size_t seen_in_cap = 0, seen_out_cap = 0;
    int calls = 0;
    const auto plus_one = [&](size_t n, size_t result, int status) {
        return [&, n, result, status](bz_gpu_engine *g, size_t *total) {
            ++calls;
            seen_in_cap = g->dec_in.cap;
            seen_out_cap = g->oneshot_out.cap;
            if (status != BZ_OK) return status;
            if (g->oneshot_out.ensure(n + 64) != BZ_OK) return (int)BZ_E_NOMEM; // (a core grows it between its launches)
            for (size_t i = 0; i < n; ++i) g->oneshot_out.as<uint8_t>()[i] = (uint8_t)(g->dec_in.as<uint8_t>()[i] + 1);
            *total = result;
            return (int)BZ_OK;
        };
    };
    uint8_t *out = nullptr;

    reset_counts(); // a batch image up, its bytes + 1 down; the large result first
    CHECK(one_shot(theirs, 2, lay, kOutGrown, kSettleStatus, &out, plus_one((size_t)lay.total, (size_t)lay.total, BZ_OK)) == BZ_OK);
    CHECK(out && calls == 1 && last_prefer == 2 && last_max_blocks == 1 && seen_in_cap >= lay.total + 64);
    for (size_t i = 0; i < a.size(); ++i) CHECK(out[lay.in_off[0] + i] == (uint8_t)(a[i] + 1));
    for (size_t i = 0; i < b.size(); ++i) CHECK(out[lay.in_off[2] + i] == (uint8_t)(b[i] + 1));
    free(out);
    CHECK(n_create == 1 && n_put == 1 && n_destroy == 0 && device_now() == mine);

    reset_counts(); // one span on the parked engine, the output bounded in advance; a small result behind the large one
    out = nullptr;
    CHECK(one_shot(theirs, 0, OneShotIn(b.data(), b.size()), 100000, kSettleStatus, &out, plus_one(b.size(), b.size(), BZ_OK)) == BZ_OK);
    CHECK(out && calls == 2 && last_prefer == 0 && n_create == 0 && seen_out_cap >= 100000 + 64);
    for (size_t i = 0; i < b.size(); ++i) CHECK(out[i] == (uint8_t)(b[i] + 1));
    free(out);
    CHECK(n_put == 1 && n_destroy == 0 && device_now() == mine);

    reset_counts(); // no bytes: a block all the same (nothing is read from the device)
    out = nullptr;
    CHECK(one_shot(theirs, 0, OneShotIn(nullptr, 0), kOutGrown, kSettleStatus, &out, plus_one(0, 0, BZ_OK)) == BZ_OK && out);
    free(out);
    out = nullptr;
    CHECK(one_shot_empty(&out) == BZ_OK && out);
    free(out);
    CHECK(n_put == 1 && n_destroy == 0);

    // the two settle rules: a device call that answers BZ_E_PARAM
    reset_counts();
    out = nullptr;
    CHECK(one_shot(theirs, 0, lay, kOutGrown, kSettleParamSound, &out, plus_one(0, 0, BZ_E_PARAM)) == BZ_E_PARAM && !out);
    CHECK(n_put == 1 && n_destroy == 0 && parked && device_now() == mine);
    CHECK(one_shot(theirs, 2, lay, kOutGrown, kSettleStatus, &out, plus_one(0, 0, BZ_E_PARAM)) == BZ_E_PARAM && !out);
    CHECK(n_put == 1 && n_destroy == 1 && !parked && device_now() == mine);
    CHECK(one_shot(theirs, 0, lay, kOutGrown, kSettleParamSound, &out, plus_one(0, 0, BZ_E_UNEXPECTED)) == BZ_E_UNEXPECTED && !out);
    CHECK(n_put == 1 && n_destroy == 2 && !parked); // (only BZ_E_PARAM is forgiven)

    // a failed allocation: its status, nothing in *out, no device call, the engine destroyed, the caller's device back
    reset_counts();
    calls = 0;
    hipshim::fail_next_mallocs() = 2; // (DevBuf::ensure asks twice) dec_in of a new engine
    CHECK(one_shot(theirs, 2, lay, 1000, kSettleStatus, &out, plus_one(0, 0, BZ_OK)) == BZ_E_NOMEM && !out && calls == 0);
    CHECK(n_create == 1 && n_put == 0 && n_destroy == 1 && device_now() == mine && hipshim::fail_next_mallocs() == 0);
    CHECK(one_shot(theirs, 2, lay, 1000, kSettleStatus, &out, plus_one((size_t)lay.total, 4, BZ_OK)) == BZ_OK && out); // parks an engine whose dec_in suffices
    free(out);
    out = nullptr;
    reset_counts();
    calls = 0;
    hipshim::fail_next_mallocs() = 2; // oneshot_out, which has to grow
    CHECK(one_shot(theirs, 2, lay, 1 << 20, kSettleStatus, &out, plus_one(0, 0, BZ_OK)) == BZ_E_NOMEM && !out && calls == 0);
    CHECK(n_create == 0 && n_put == 0 && n_destroy == 1 && !parked && device_now() == mine && hipshim::fail_next_mallocs() == 0);

    // the download's malloc fails: BZ_E_NOMEM, nothing in *out, the engine ended once
    reset_counts();
    volatile size_t absurd = ~(size_t)0 / 2;
    CHECK(one_shot(theirs, 2, lay, kOutGrown, kSettleStatus, &out, plus_one(16, absurd, BZ_OK)) == BZ_E_NOMEM && !out);
    CHECK(n_put == 0 && n_destroy == 1 && device_now() == mine);
    uint8_t word[4] = {1, 2, 3, 4};
    CHECK(one_shot_download(&out, word, absurd) == BZ_E_NOMEM && !out);
    CHECK(one_shot_download(&out, word, 4) == BZ_OK && out && memcmp(out, word, 4) == 0);
    free(out);
    out = nullptr;

    // the order of the answers: BZ_E_NOGPU in front of the lease, then the lease's status
    reset_counts();
    CHECK(device_in_range(0) == BZ_OK && device_in_range(hipshim::kDevices - 1) == BZ_OK);
    CHECK(device_in_range(-1) == BZ_E_NOGPU && device_in_range(hipshim::kDevices) == BZ_E_NOGPU);
    create_fails_with = BZ_E_PARAM;
    CHECK(one_shot(hipshim::kDevices, 2, lay, kOutGrown, kSettleStatus, &out, plus_one(0, 0, BZ_OK)) == BZ_E_NOGPU && n_take == 0 && n_create == 0);
    CHECK(one_shot(theirs, 2, lay, kOutGrown, kSettleStatus, &out, plus_one(0, 0, BZ_OK)) == BZ_E_PARAM && n_take == 1 && n_create == 1 && !out);
    create_fails_with = 0;
    CHECK(device_now() == mine);
    dec_release_cached();
    CHECK(hipshim::live_allocs() == 0);
    return 0;
}

// ---- the frame of the batch decoders
struct Rec { // what batch_place reads of DfInfRec and LzhRec
    uint32_t len;
    int32_t verdict;
    uint32_t flags;
};
struct SplitEntry { // ... and split_reserve of DfSplitEntry and LzhSplitEntry
    size_t index;
    Rec rec;
};

static int check_ranges()
{
    alignas(16) static uint8_t mem[64];
    const uint64_t big = 1ull << 32;
    struct Row {
        const void *d_in, *d_out;
        uint64_t off[2], len[2];
        size_t count;
        bool ok;
    };
    const Row rows[] = {
        {mem, mem, {0, 8}, {5, 3}, 2, true},
        {mem, mem, {0, 4}, {4, 0}, 2, true},                     // (touching is not overlapping)
        {nullptr, nullptr, {0, 0}, {0, 0}, 2, true},             // the all-empty batch: no pointer needed
        {nullptr, nullptr, {0, 0}, {0, 0}, 0, true},
        {mem, mem, {2, 8}, {1, 1}, 2, false},                    // an offset that is no multiple of 4
        {mem, mem, {0, 4}, {5, 1}, 2, false},                    // two entries that overlap
        {mem, mem, {8, 0}, {1, 1}, 2, false},                    // descending
        {mem, mem, {0, ~0ull - 3}, {1, 8}, 2, false},            // off + len wraps
        {mem, mem, {0, 8}, {big, 0}, 1, false},                  // an entry of 4 GiB
        {mem, mem, {0, 8}, {big - 1, 0}, 1, true},
        {nullptr, mem, {0, 8}, {0, 1}, 2, false},                // bytes announced without d_in
        {mem + 8, mem, {0, 8}, {1, 1}, 2, false},                // d_in at 16k + 8
        {mem, mem + 8, {0, 8}, {1, 1}, 2, false},                // d_out at 16k + 8
        {mem, nullptr, {0, 8}, {1, 1}, 2, true},                 // (the sizes alone)
    };
    for (const Row &r : rows) CHECK(batch_ranges_ok(r.d_in, r.d_out, r.off, r.len, r.count) == r.ok);
    CHECK(!batch_ranges_ok(nullptr, nullptr, nullptr, nullptr, (size_t)0x80000000u)); // (refused before any entry is read)
    return 0;
}

static int check_places()
{
    { // no places given: input order, multiples of 16
        Rec rec[5] = {{0, 0, 0}, {1, BZ_E_EOF, 0}, {15, 0, 0}, {16, BZ_E_DATA, 0}, {17, 0, 0}};
        uint64_t off[5], len[5], need = 0;
        int32_t verdict[5];
        CHECK(batch_place(rec, 5, nullptr, off, len, verdict, &need) == BZ_OK && need == 65);
        const uint64_t want[5] = {0, 0, 16, 32, 48};
        for (int i = 0; i < 5; ++i) CHECK(off[i] == want[i] && len[i] == rec[i].len && verdict[i] == rec[i].verdict);
        alignas(16) uint8_t mem[16];
        uint8_t *out8 = nullptr;
        CHECK(batch_output(need, mem, 65, nullptr, &out8) == BZ_OK && out8 == mem);
        CHECK(batch_output(need, mem, 64, nullptr, &out8) == BZ_E_CAPACITY);
        CHECK(batch_output(need, nullptr, 0, nullptr, &out8) == BZ_OK && out8 == nullptr); // the sizes alone
        DevBuf grow;
        CHECK(batch_output(need, nullptr, 0, &grow, &out8) == BZ_OK && out8 == grow.p && grow.cap >= 65 + 64);
        hipshim::fail_next_mallocs() = 2;
        CHECK(batch_output(1 << 20, nullptr, 0, &grow, &out8) == BZ_E_NOMEM && hipshim::fail_next_mallocs() == 0);
        rec[4].len = 0; // an empty last entry: its offset still counts
        CHECK(batch_place(rec, 5, nullptr, off, len, verdict, &need) == BZ_OK && need == 48 && off[4] == 48);
        rec[2].flags = 1; // 4 GiB or more of output
        CHECK(batch_place(rec, 5, nullptr, off, len, verdict, &need) == BZ_E_PARAM);
    }
    { // places given, out of order: the largest end, not the last entry's
        const Rec rec[3] = {{5, 0, 0}, {40, 0, 0}, {7, 0, 0}};
        const uint64_t place[3] = {64, 0, 32};
        uint64_t off[3], len[3], need = 0;
        int32_t verdict[3];
        CHECK(batch_place(rec, 3, place, off, len, verdict, &need) == BZ_OK && need == 69);
        for (int i = 0; i < 3; ++i) CHECK(off[i] == place[i] && len[i] == rec[i].len);
    }
    return 0;
}

static int check_split_reserve()
{
    const uint64_t in_len[4] = {10, 2000, 30, 4000};
    std::vector<uint64_t> small(3, 7);
    DevBuf map, counter;
    std::vector<SplitEntry> splits; // none is split: nothing reserved
    CHECK(split_reserve(splits, true, map, counter, in_len, 4, small) == 0 && small.empty() && !map.p && !counter.p);
    splits = {{1, {100, 0, 0}}, {3, {1000, 0, 0}}};
    CHECK(split_reserve(splits, false, map, counter, in_len, 4, small) == 0 && splits.size() == 2 && !map.p); // the sizes alone
    CHECK((small == std::vector<uint64_t>{10, 0, 30, 0}));
    CHECK(split_reserve(splits, true, map, counter, in_len, 4, small) == 0 && splits.size() == 2);
    CHECK(map.cap >= 1000 * 4 + 64 && counter.cap >= 64 && (small == std::vector<uint64_t>{10, 0, 30, 0}));
    splits[1].rec.len = 1 << 20; // the map cannot be had: every entry goes back
    hipshim::fail_next_mallocs() = 2;
    CHECK(split_reserve(splits, true, map, counter, in_len, 4, small) == 2 && splits.empty() && small.empty());
    return 0;
}

// stand-ins for the two launchers: a script of (left, moved) per jump round
static std::vector<std::pair<uint32_t, uint32_t>> jump_script;
static size_t n_jump, n_gather;
namespace dfgpu {
int df_launch_split_jump(hipStream_t, uint32_t *, uint32_t, uint32_t *cnt)
{
    if (cnt[0] || cnt[1] || n_jump >= jump_script.size()) return -1; // (the counter is cleared in front of every round)
    cnt[0] = jump_script[n_jump].first;
    cnt[1] = jump_script[n_jump].second;
    ++n_jump;
    return 0;
}
int df_launch_split_gather(hipStream_t, uint8_t *, const uint32_t *, uint32_t)
{
    ++n_gather;
    return 0;
}
} // namespace dfgpu

static int check_split_tail()
{
    uint32_t map[4] = {0, 0, 0, 0}, cnt[2] = {9, 9};
    uint8_t out[4];
    const auto run = [&](bool jump, std::vector<std::pair<uint32_t, uint32_t>> script, SplitTail &t) {
        jump_script = std::move(script);
        n_jump = n_gather = 0;
        t = SplitTail();
        return split_jump_gather(nullptr, jump, map, 4, cnt, out, t);
    };
    SplitTail t;
    CHECK(run(true, {{12, 5}, {8, 2}, {3, 0}}, t) == BZ_OK); // rounds until one moves nothing; `left` is round 0's
    CHECK(t.rounds == 3 && t.left == 12 && t.launches == 4 && n_jump == 3 && n_gather == 1 && t.jump_ms >= 0 && t.gather_ms >= 0);
    CHECK(run(true, {{0, 0}}, t) == BZ_OK); // every byte in its place: one round, no gather
    CHECK(t.rounds == 1 && t.left == 0 && t.launches == 1 && n_gather == 0);
    CHECK(run(true, {{6, 0}}, t) == BZ_OK); // bytes to fetch, all of them one hop away
    CHECK(t.rounds == 1 && t.left == 6 && t.launches == 2 && n_gather == 1);
    CHECK(run(false, {}, t) == BZ_OK); // one piece: no round, no gather
    CHECK(t.rounds == 0 && t.left == 0 && t.launches == 0 && n_jump == 0 && n_gather == 0);
    CHECK(run(true, {{4, 1}}, t) == BZ_E_UNEXPECTED); // a launch that fails (here: the script ran out)
    return 0;
}

int main()
{
    const int rc = check_lease() || check_layout() || check_one_shot() || check_ranges() || check_places() || check_split_reserve() || check_split_tail();
    if (rc == 0) printf("ok\n");
    return rc;
}
