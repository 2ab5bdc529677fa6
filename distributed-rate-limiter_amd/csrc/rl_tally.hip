// rl_tally.hip -- the usage tally (rl_tally.h): its kernels as a translation
// unit of their own, and the rl_tally_* entry points.
#define RL_TALLY_DEVICE
#include "rl_tally.h"

#include <algorithm>

#include "rl_engine_impl.h"

using namespace rl;

// k_tally over m requests on stream s (probe bound min(slots, TALLY_PROBES))
static hipError_t tally_launch(uint64_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n,
                               const uint8_t* dec, uint32_t ncfg, tally_u64* cfgc, tally_u64* glob, TallyKey* keys,
                               uint64_t slots, hipStream_t s) {
    // m == 0 (rl_tally_enable's warm-up): one block that finds nothing to do
    const int grid = std::max(1, grid_for(m, TALLY_BLOCK, TALLY_GRID));
    k_tally<<<grid, TALLY_BLOCK, 0, s>>>(m, key, cfg, n, dec, ncfg, cfgc, glob, keys, slots - 1,
                                         std::min<uint64_t>(slots, TALLY_PROBES));
    return hipGetLastError();
}

// k_tally_routed over the merged routed step `io` of bound m_max on stream s
static hipError_t tally_routed_launch(rl_engine* e, uint64_t m_max, const RoutedIo& io, const int64_t* recv_info,
                                      uint32_t world, hipStream_t s) {
    // m_max == 0 (the warm-up): one block that finds nothing to do
    const int grid = std::max(1, grid_for(m_max, TALLY_BLOCK, TALLY_GRID));
    k_tally_routed<<<grid, TALLY_BLOCK, 0, s>>>(m_max, io, recv_info, world, (uint32_t)e->h_cfg.size(), e->d_tally_cfg,
                                                e->d_tally_glob, e->d_tally_keys, e->tally_slots - 1,
                                                std::min<uint64_t>(e->tally_slots, TALLY_PROBES));
    return hipGetLastError();
}

// k_tally_clear: every record free, every counter 0
static hipError_t tally_clear_launch(TallyKey* keys, uint64_t slots, tally_u64* cfgc, uint64_t cfg_words,
                                     tally_u64* glob, hipStream_t s) {
    k_tally_clear<<<256, 256, 0, s>>>(keys, slots, cfgc, cfg_words, glob);
    return hipGetLastError();
}

// k_tally runs on the caller's stream, behind the finish of the batch it
// counts; it touches the tally's own memory only, so it needs no order against
// the engine's streams.  What must wait for it -- a read, a clear, a new
// config's row, destroy -- waits for the event recorded behind the last call
// of every stream one was enqueued on (side_record; drain()).
static int run_tally(rl_engine* e, size_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n,
                     const uint8_t* dec, hipStream_t s) {
    HIPCHK(e, tally_launch((uint64_t)m, key, cfg, n, dec, (uint32_t)e->h_cfg.size(), e->d_tally_cfg, e->d_tally_glob,
                           e->d_tally_keys, e->tally_slots, s));
    const int r = side_record(e, s);
    if (r != RL_OK) return r;
    e->tally_batches++;
    e->tally_requests += m;
    return RL_OK;
}

extern "C" int rl_tally_enable(rl_engine* e, const rl_tally_opts* o) {
    if (!e || !o || o->struct_size != sizeof(rl_tally_opts) || e->tally_on) return RL_EINVAL;
    if (o->key_slots > (1u << 24)) return fail(e, RL_EINVAL, "tally key_slots above 1 << 24");
    (void)hipSetDevice(e->device);
    const uint64_t slots = pow2_at_least(std::max<uint64_t>(o->key_slots ? o->key_slots : 65536, 16));
    const uint32_t cap = std::max<uint32_t>(64, (uint32_t)pow2_at_least(e->h_cfg.size() + 1));
    bool ok = hipMalloc(&e->d_tally_keys, sizeof(TallyKey) * slots) == hipSuccess;
    ok = ok && hipMalloc(&e->d_tally_cfg, sizeof(tally_u64) * TALLY_CFG_WORDS * cap) == hipSuccess;
    ok = ok && hipMalloc(&e->d_tally_glob, sizeof(tally_u64) * TG_WORDS) == hipSuccess;
    if (ok) {
        ok = tally_clear_launch(e->d_tally_keys, slots, e->d_tally_cfg, (uint64_t)TALLY_CFG_WORDS * cap,
                                e->d_tally_glob, e->stream) == hipSuccess;
        // an empty launch loads the kernel now, not in front of the first batch
        ok = ok && tally_launch(0, nullptr, nullptr, nullptr, nullptr, 0, e->d_tally_cfg, e->d_tally_glob,
                                e->d_tally_keys, slots, e->stream) == hipSuccess;
        // the routed form on a zero count
        e->tally_slots = slots;
        const RoutedIo io{nullptr, nullptr, e->d_zero, nullptr, nullptr, e->d_eflags};
        ok = ok && tally_routed_launch(e, 0, io, nullptr, 0, e->stream) == hipSuccess;
        ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;
    }
    if (!ok) {
        e->tally_slots = 0;
        (void)hipFree(e->d_tally_keys); (void)hipFree(e->d_tally_cfg); (void)hipFree(e->d_tally_glob);
        e->d_tally_keys = nullptr; e->d_tally_cfg = nullptr; e->d_tally_glob = nullptr;
        return fail(e, RL_ENOMEM, "tally allocation failed");
    }
    e->tally_slots = slots;
    e->tally_cfg_cap = cap;
    e->tally_batches = e->tally_requests = e->tally_routed_steps = 0;
    e->tally_on = true;
    return RL_OK;
}

extern "C" int rl_tally_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                                     const int64_t* n, const uint8_t* decision, void* stream) {
    if (!e || !e->tally_on || (m && (!key_id || !cfg_id || !n || !decision))) return RL_EINVAL;
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    return run_tally(e, m, key_id, cfg_id, n, decision, stream ? (hipStream_t)stream : e->stream);
}

extern "C" int rl_tally_batch(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                              const int64_t* n, const uint8_t* decision) {
    if (!e || !e->tally_on || (m && (!key_id || !cfg_id || !n || !decision))) return RL_EINVAL;
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    const uint64_t b0 = e->tally_batches;
    // chunks of max_batch: the size of the host API's staging arrays
    for (size_t off = 0; off < m; off += e->max_batch) {
        const uint32_t c = (uint32_t)std::min<size_t>(e->max_batch, m - off);
        int r = stage_in(e, off, c, key_id, nullptr, n, cfg_id, nullptr, s);
        if (r != RL_OK) return r;
        // the one input that arrives through a result array
        HIPCHK(e, hipMemcpyAsync(e->d_dec, decision + off, c, hipMemcpyHostToDevice, s));
        r = run_tally(e, c, e->d_key, e->d_cfgid, e->d_n, e->d_dec, s);
        if (r != RL_OK) return r;
        HIPCHK(e, hipStreamSynchronize(s));
    }
    e->tally_batches = b0 + 1;   // one call, one batch, however many chunks
    return RL_OK;
}

extern "C" int rl_tally_read(rl_engine* e, rl_tally_cfg* cfg_out, size_t cfg_cap, uint32_t* ncfg,
                             rl_tally_key* key_out, size_t key_cap, uint64_t* keys_tracked, rl_tally_info* info,
                             int clear) {
    if (!e || !e->tally_on) return RL_EINVAL;
    if (info && info->struct_size < 8) return RL_EINVAL;
    static_assert(sizeof(rl_tally_cfg) == sizeof(tally_u64) * TALLY_CFG_WORDS, "rl_tally_cfg is a counter row");
    static_assert(sizeof(rl_tally_key) == sizeof(TallyKey), "rl_tally_key is a table record");
    (void)hipSetDevice(e->device);
    {
        const int r = side_wait(e);
        if (r != RL_OK) return r;
    }
    hipStream_t s = e->stream;
    const uint32_t nc = (uint32_t)e->h_cfg.size();
    tally_u64 glob[TG_WORDS];
    HIPCHK(e, hipMemcpyAsync(glob, e->d_tally_glob, sizeof(glob), hipMemcpyDeviceToHost, s));
    const size_t rows = cfg_out ? std::min<size_t>(cfg_cap, nc) : 0;
    if (rows) HIPCHK(e, hipMemcpyAsync(cfg_out, e->d_tally_cfg, sizeof(rl_tally_cfg) * rows, hipMemcpyDeviceToHost, s));
    std::vector<rl_tally_key> tab;
    if (key_out && key_cap) {
        tab.resize(e->tally_slots);
        HIPCHK(e, hipMemcpyAsync(tab.data(), e->d_tally_keys, sizeof(rl_tally_key) * e->tally_slots,
                                 hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    if (!tab.empty()) {
        // the top keys, selected on the host from the copy
        auto end = std::remove_if(tab.begin(), tab.end(), [](const rl_tally_key& r) { return r.key_id == EMPTY_KEY; });
        const size_t want = std::min<size_t>(key_cap, (size_t)(end - tab.begin()));
        std::partial_sort(tab.begin(), tab.begin() + want, end, [](const rl_tally_key& a, const rl_tally_key& b) {
            return a.denied != b.denied ? a.denied > b.denied : a.key_id < b.key_id;
        });
        memcpy(key_out, tab.data(), sizeof(rl_tally_key) * want);
    }
    if (ncfg) *ncfg = nc;
    if (keys_tracked) *keys_tracked = glob[TG_KEYS];
    if (info) {
        rl_tally_info I{};
        I.key_slots = e->tally_slots;
        I.keys_tracked = glob[TG_KEYS];
        I.untracked_requests = glob[TG_UNTRACKED_REQ];
        I.untracked_units = glob[TG_UNTRACKED_UNITS];
        I.unknown_cfg = glob[TG_UNKNOWN];
        I.bad_codes = glob[TG_BAD];
        I.batches = e->tally_batches;
        I.requests = e->tally_requests;
        const int r = copy_out(info, I);
        if (r != RL_OK) return r;
    }
    if (clear) {
        HIPCHK(e, tally_clear_launch(e->d_tally_keys, e->tally_slots, e->d_tally_cfg,
                                     (uint64_t)TALLY_CFG_WORDS * e->tally_cfg_cap, e->d_tally_glob, s));
        HIPCHK(e, hipStreamSynchronize(s));
        e->tally_batches = e->tally_requests = e->tally_routed_steps = 0;
    }
    return RL_OK;
}

// The routed form (include/rl_route.h): one launch on the caller's stream,
// behind the step's results; like k_tally it touches the tally's own memory
// only (and re-raises EF_ROUTED_OVER on a count above m_max), so it uses none
// of the engine's streams and is waited for through side_record's events.
extern "C" int rl_tally_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                      const uint32_t* order, const int64_t* server_ms, const rl_route_res* res,
                                      const int64_t* recv_info, uint32_t world, void* stream) {
    if (!e || !e->tally_on || m_max > 0xffffffffull) return RL_EINVAL;
    if (m_max == 0) return RL_OK;
    if (!count || !recv || !order || !server_ms || !res) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    const RoutedIo io{recv, order, count, server_ms, const_cast<rl_route_res*>(res), e->d_eflags};   // res is only read
    HIPCHK(e, tally_routed_launch(e, (uint64_t)m_max, io, recv_info, recv_info ? world : 0, s));
    const int r = side_record(e, s);
    if (r != RL_OK) return r;
    e->tally_routed_steps++;
    return RL_OK;
}

extern "C" int rl_tally_routed_read(rl_engine* e, rl_tally_routed_info* out) {
    if (!e || !e->tally_on || !out || out->struct_size < 8) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    {
        const int r = side_wait(e);
        if (r != RL_OK) return r;
    }
    tally_u64 glob[TG_WORDS];
    HIPCHK(e, hipMemcpyAsync(glob, e->d_tally_glob, sizeof(glob), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    rl_tally_routed_info I{};
    I.steps = e->tally_routed_steps;
    I.requests = glob[TG_ROUTED_REQ];
    I.dropped_requests = glob[TG_ROUTED_DROPPED];
    return copy_out(out, I);
}

extern "C" int rl_tally_grid_cap(void) { return TALLY_GRID * TALLY_BLOCK; }
