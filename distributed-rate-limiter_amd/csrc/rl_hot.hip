// rl_hot.hip -- the top keys (rl_hot.h): its kernels as a translation unit of
// their own, and the rl_hot_* entry points.
#define RL_HOT_DEVICE
#include "rl_hot.h"

#include <algorithm>

#include "rl_engine_impl.h"

using namespace rl;

static int hot_grid(uint64_t m) { return std::max(1, grid_for(m, HOT_BLOCK, HOT_GRID)); }

// k_hot_add over m requests on stream s
static hipError_t hot_add_launch(rl_engine* e, uint64_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n,
                                 const uint8_t* dec, hipStream_t s) {
    k_hot_add<<<hot_grid(m), HOT_BLOCK, 0, s>>>(m, key, cfg, n, dec, (uint32_t)e->h_cfg.size(), e->hot_weight,
                                                e->d_hot_sketch, e->hot_width, e->d_hot_glob);
    return hipGetLastError();
}

// k_hot_pick over the same requests (probe bound min(slots, HOT_PROBES))
static hipError_t hot_pick_launch(rl_engine* e, uint64_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n,
                                  const uint8_t* dec, hipStream_t s) {
    k_hot_pick<<<hot_grid(m), HOT_BLOCK, 0, s>>>(m, key, cfg, n, dec, (uint32_t)e->h_cfg.size(), e->hot_weight,
                                                 e->d_hot_sketch, e->hot_width, e->hot_min, e->d_hot_glob,
                                                 e->d_hot_keys, e->hot_slots - 1,
                                                 std::min<uint64_t>(e->hot_slots, HOT_PROBES));
    return hipGetLastError();
}

// k_hot_add_routed, then k_hot_pick_routed, over the merged routed step `io` of bound m_max
static hipError_t hot_routed_launch(rl_engine* e, uint64_t m_max, const RoutedIo& io, hipStream_t s) {
    const uint32_t ncfg = (uint32_t)e->h_cfg.size();
    k_hot_add_routed<<<hot_grid(m_max), HOT_BLOCK, 0, s>>>(m_max, io, ncfg, e->hot_weight, e->d_hot_sketch,
                                                           e->hot_width, e->d_hot_glob);
    hipError_t st = hipGetLastError();
    if (st != hipSuccess) return st;
    k_hot_pick_routed<<<hot_grid(m_max), HOT_BLOCK, 0, s>>>(m_max, io, ncfg, e->hot_weight, e->d_hot_sketch,
                                                            e->hot_width, e->hot_min, e->d_hot_glob, e->d_hot_keys,
                                                            e->hot_slots - 1,
                                                            std::min<uint64_t>(e->hot_slots, HOT_PROBES));
    return hipGetLastError();
}

static hipError_t hot_clear_launch(rl_engine* e, hipStream_t s) {
    k_hot_clear<<<256, 256, 0, s>>>(e->d_hot_sketch, (uint64_t)HOT_DEPTH * e->hot_width, e->d_hot_keys, e->hot_slots,
                                    e->d_hot_glob);
    return hipGetLastError();
}

// Both kernels run on the caller's stream, behind the finish of the batch they
// count; they touch the feature's own memory only, so they need no order
// against the engine's streams.  What must wait for them -- a read, a clear,
// destroy -- waits through side_record's events (drain(), rl_hot_read).
static int run_hot(rl_engine* e, size_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n,
                   const uint8_t* dec, hipStream_t s) {
    HIPCHK(e, hot_add_launch(e, m, key, cfg, n, dec, s));
    HIPCHK(e, hot_pick_launch(e, m, key, cfg, n, dec, s));
    const int r = side_record(e, s);
    if (r != RL_OK) return r;
    e->hot_batches++;
    e->hot_requests += m;
    return RL_OK;
}

static void hot_free(rl_engine* e) {
    (void)hipFree(e->d_hot_sketch); (void)hipFree(e->d_hot_keys); (void)hipFree(e->d_hot_glob);
    e->d_hot_sketch = nullptr; e->d_hot_keys = nullptr; e->d_hot_glob = nullptr;
}

extern "C" int rl_hot_enable(rl_engine* e, const rl_hot_opts* o) {
    if (!e || !o || o->struct_size != sizeof(rl_hot_opts) || e->hot_on) return RL_EINVAL;
    if (o->width > (1u << 24)) return fail(e, RL_EINVAL, "hot width above 1 << 24");
    if (o->key_slots > (1u << 24)) return fail(e, RL_EINVAL, "hot key_slots above 1 << 24");
    if (o->weight > RL_HOT_UNITS) return fail(e, RL_EINVAL, "hot weight: RL_HOT_REQUESTS or RL_HOT_UNITS");
    if (o->hot_min < 1) return fail(e, RL_EINVAL, "hot_min must be at least 1");
    (void)hipSetDevice(e->device);
    e->hot_width = pow2_at_least(std::max<uint64_t>(o->width ? o->width : 1u << 18, 16));
    e->hot_slots = pow2_at_least(std::max<uint64_t>(o->key_slots ? o->key_slots : 65536, 16));
    e->hot_weight = o->weight;
    e->hot_min = o->hot_min;
    bool ok = hipMalloc(&e->d_hot_sketch, sizeof(hot_u64) * HOT_DEPTH * e->hot_width) == hipSuccess;
    ok = ok && hipMalloc(&e->d_hot_keys, sizeof(HotKey) * e->hot_slots) == hipSuccess;
    ok = ok && hipMalloc(&e->d_hot_glob, sizeof(hot_u64) * HG_WORDS) == hipSuccess;
    if (ok) {
        ok = hot_clear_launch(e, e->stream) == hipSuccess;
        // empty launches load the kernels now, not in front of the first batch
        ok = ok && hot_add_launch(e, 0, nullptr, nullptr, nullptr, nullptr, e->stream) == hipSuccess;
        ok = ok && hot_pick_launch(e, 0, nullptr, nullptr, nullptr, nullptr, e->stream) == hipSuccess;
        // the routed forms on a zero count
        ok = ok && hot_routed_launch(e, 0, RoutedIo{nullptr, nullptr, e->d_zero, nullptr, nullptr, e->d_eflags},
                                     e->stream) == hipSuccess;
        k_hot_read<<<1, 256, 0, e->stream>>>(e->d_hot_keys, 0, e->d_hot_sketch, e->hot_width);
        ok = ok && hipGetLastError() == hipSuccess;
        ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;
    }
    if (!ok) {
        hot_free(e);
        return fail(e, RL_ENOMEM, "hot allocation failed");
    }
    e->hot_batches = e->hot_requests = 0;
    e->hot_on = true;
    return RL_OK;
}

extern "C" int rl_hot_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                                   const int64_t* n, const uint8_t* decision, void* stream) {
    if (!e || !e->hot_on || (m && (!key_id || !cfg_id || !n || !decision))) return RL_EINVAL;
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    return run_hot(e, m, key_id, cfg_id, n, decision, stream ? (hipStream_t)stream : e->stream);
}

extern "C" int rl_hot_batch(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id, const int64_t* n,
                            const uint8_t* decision) {
    if (!e || !e->hot_on || (m && (!key_id || !cfg_id || !n || !decision))) return RL_EINVAL;
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    // Chunks of max_batch, the size of the host API's staging arrays.  The
    // call's keys are looked at once all of its adds are in: a call of more
    // than one chunk stages every chunk twice, all adds first.
    const bool one = m <= e->max_batch;
    for (int pass = 0; pass < (one ? 1 : 2); pass++) {
        for (size_t off = 0; off < m; off += e->max_batch) {
            const uint32_t c = (uint32_t)std::min<size_t>(e->max_batch, m - off);
            const int r = stage_in(e, off, c, key_id, nullptr, n, cfg_id, nullptr, s);
            if (r != RL_OK) return r;
            // the one input that arrives through a result array
            HIPCHK(e, hipMemcpyAsync(e->d_dec, decision + off, c, hipMemcpyHostToDevice, s));
            if (one || pass == 0) HIPCHK(e, hot_add_launch(e, c, e->d_key, e->d_cfgid, e->d_n, e->d_dec, s));
            if (one || pass == 1) HIPCHK(e, hot_pick_launch(e, c, e->d_key, e->d_cfgid, e->d_n, e->d_dec, s));
            HIPCHK(e, hipStreamSynchronize(s));
        }
    }
    e->hot_batches++;   // one call, one batch, however many chunks
    e->hot_requests += m;
    return RL_OK;
}

extern "C" int rl_hot_read(rl_engine* e, rl_hot_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                           rl_hot_info* info, int clear) {
    if (!e || !e->hot_on) return RL_EINVAL;
    if (info && info->struct_size < 8) return RL_EINVAL;
    static_assert(sizeof(rl_hot_key) == sizeof(HotKey), "rl_hot_key is a table record");
    (void)hipSetDevice(e->device);
    {
        const int r = side_wait(e);
        if (r != RL_OK) return r;
    }
    hipStream_t s = e->stream;
    hot_u64 glob[HG_WORDS];
    HIPCHK(e, hipMemcpyAsync(glob, e->d_hot_glob, sizeof(glob), hipMemcpyDeviceToHost, s));
    std::vector<rl_hot_key> tab;
    if (key_out && key_cap) {
        // the estimates as the sketch is now, then the records to the host
        k_hot_read<<<std::max(1, grid_for(e->hot_slots, 256, 256)), 256, 0, s>>>(e->d_hot_keys, e->hot_slots,
                                                                                e->d_hot_sketch, e->hot_width);
        HIPCHK(e, hipGetLastError());
        tab.resize(e->hot_slots);
        HIPCHK(e, hipMemcpyAsync(tab.data(), e->d_hot_keys, sizeof(rl_hot_key) * e->hot_slots, hipMemcpyDeviceToHost,
                                 s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    if (!tab.empty()) {
        // the top keys, selected on the host from the copy
        auto end = std::remove_if(tab.begin(), tab.end(), [](const rl_hot_key& r) { return r.key_id == EMPTY_KEY; });
        const size_t want = std::min<size_t>(key_cap, (size_t)(end - tab.begin()));
        std::partial_sort(tab.begin(), tab.begin() + want, end, [](const rl_hot_key& a, const rl_hot_key& b) {
            return a.estimate != b.estimate ? a.estimate > b.estimate : a.key_id < b.key_id;
        });
        memcpy(key_out, tab.data(), sizeof(rl_hot_key) * want);
    }
    if (keys_tracked) *keys_tracked = glob[HG_KEYS];
    if (info) {
        rl_hot_info I{};
        I.width = e->hot_width;
        I.depth = HOT_DEPTH;
        I.key_slots = e->hot_slots;
        I.hot_min = e->hot_min;
        I.weight = e->hot_weight;
        I.keys_tracked = glob[HG_KEYS];
        I.dropped = glob[HG_DROPPED];
        I.total = glob[HG_TOTAL];
        I.skipped = glob[HG_SKIPPED];
        I.batches = e->hot_batches;
        I.requests = e->hot_requests;
        const int r = copy_out(info, I);
        if (r != RL_OK) return r;
    }
    if (clear) {
        HIPCHK(e, hot_clear_launch(e, s));
        HIPCHK(e, hipStreamSynchronize(s));
        e->hot_batches = e->hot_requests = 0;
    }
    return RL_OK;
}

// The routed form (include/rl_route.h): the adds, then the pick, on the
// caller's stream behind the step's results; like the array form they touch
// the feature's own memory only (and re-raise EF_ROUTED_OVER on a count above
// m_max), so they use none of the engine's streams and are waited for through
// side_record's events.  hot_batches / hot_requests count array calls only.
extern "C" int rl_hot_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                    const uint32_t* order, const int64_t* server_ms, const rl_route_res* res,
                                    void* stream) {
    if (!e || !e->hot_on || m_max > 0xffffffffull) return RL_EINVAL;
    if (m_max == 0) return RL_OK;
    if (!count || !recv || !order || !server_ms || !res) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const RoutedIo io{recv, order, count, server_ms, const_cast<rl_route_res*>(res), e->d_eflags};   // res is only read
    HIPCHK(e, hot_routed_launch(e, (uint64_t)m_max, io, s));
    return side_record(e, s);
}

extern "C" int rl_hot_grid_cap(void) { return HOT_GRID * HOT_BLOCK; }
