// engine_cache.hip -- the engines that the host-to-host calls and the streaming contexts of both codecs (bzip2 decode,
// Deflate encode and decode) park between uses.  Taken and put back through EngineLease (host_call.h), nowhere else.
#include "engine_state.h"

#include <mutex>
#include <utility>
#include <vector>

// Two engines per device are kept between one-shot calls and contexts (its decode workspace -- 13 MB per block in flight -- and the
// buffer for the compressed bytes cost more to make than a GiB costs to decode); bz_release_cached_resources frees them.
namespace {
std::mutex g_dec_cache_mu;
std::vector<std::pair<int, bz_gpu_engine *>> g_dec_cache;
} // namespace
// prefer: 1 = an engine that has decoded before (it holds the decode workspace), 2 = one that has a Deflate workspace;
// otherwise the engine that was put back last (two engines are kept since the streaming decoder has two lanes: taking the
// OLDEST one made consecutive one-shot calls alternate between them, each paying for a workspace of its own)
bz_gpu_engine *dec_cache_take(int device, int prefer)
{
    std::lock_guard<std::mutex> lk(g_dec_cache_mu);
    size_t pick = ~(size_t)0;
    for (size_t i = g_dec_cache.size(); i-- > 0;) {
        if (g_dec_cache[i].first != device) continue;
        const bz_gpu_engine *c = g_dec_cache[i].second;
        const bool match = prefer == 1 ? c->dec != nullptr : (prefer == 2 ? c->df != nullptr : true);
        if (pick == ~(size_t)0) pick = i; // (the newest one of the device)
        if (match) {
            pick = i;
            break;
        }
    }
    if (pick == ~(size_t)0) return nullptr;
    bz_gpu_engine *g = g_dec_cache[pick].second;
    g_dec_cache.erase(g_dec_cache.begin() + (ptrdiff_t)pick);
    return g;
}
void dec_cache_put(int device, bz_gpu_engine *g)
{
    {
        std::lock_guard<std::mutex> lk(g_dec_cache_mu);
        size_t have = 0;
        for (const auto &e : g_dec_cache) have += e.first == device ? 1 : 0;
        if (have < 2) { // (two: the lanes of a streaming context)
            g_dec_cache.emplace_back(device, g);
            return;
        }
    }
    bz_gpu_engine_destroy(g); // (more calls side by side on one device: their engines are not kept)
}
void dec_release_cached()
{
    std::vector<std::pair<int, bz_gpu_engine *>> all;
    {
        std::lock_guard<std::mutex> lk(g_dec_cache_mu);
        all.swap(g_dec_cache);
    }
    for (auto &e : all) {
        (void)hipSetDevice(e.first);
        bz_gpu_engine_destroy(e.second);
    }
    dec_spare_bufs_clear();
}
