// host_call_check.cpp -- csrc/host_call.h on the host (tests/test_host_call_host.py): the keep-or-destroy rule of
// EngineLease against stand-ins for the engine cache and the engine that count their calls, the caller's device on every
// path, and BatchLayout against a transcription of the four packing loops it replaced.  Exits non-zero at the first
// failure.
#include "../../rust-compression_amd/csrc/host_call.h"

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
};
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

int main()
{
    const int rc = check_lease() || check_layout();
    if (rc == 0) printf("ok\n");
    return rc;
}
