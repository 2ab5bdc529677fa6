// rl_hot.h -- top keys (rl_hot_*, include/rl_engine.h): which keys carry the
// traffic, over all decisions, counted on the device.
//
// A count-min sketch of HOT_DEPTH rows by `width` 64-bit counters (row r at
// sketch + r * width; the column of key k in row r is
// mix64(k ^ mix64(r + 1)) & (width - 1)), plus a fixed-capacity table of
// candidate keys that follows the tally's rule (rl_tally.h): home slot
// mix64(key) & mask, linear probing over at most min(slots, HOT_PROBES) slots,
// an empty slot claimed with one CAS, never released before a clear.
//
// One rl_hot_batch* call is two launches on the caller's stream over the same
// finished batch in the decide layout (key id, config id, n, decision byte; one
// request per thread):
//   k_hot_add   every counted request adds its weight to its four counters;
//   k_hot_pick  every key with a counted request in the batch: estimate = the
//               minimum of its four counters; at or above hot_min the key is
//               looked up in the candidate table and inserted when absent.
// Stream order between the two is the grid-wide "all adds are in".
//
// Contention.  One key can be a whole batch, and a word sustains far fewer
// atomics than the batch has requests, so no per-request global atomic may
// land on a hot key's counters.  k_hot_add merges as k_tally does:
//   1. in the wave: the first pending lane's key is broadcast (readlane of a
//      ballot's first bit), the lanes that hold it drop out, their weight is
//      the ballot's popcount (requests) or a wave sum (units); at most 64 rounds;
//   2. in the block: the group's leader adds to an LDS table of HOT_LDS_KEYS
//      keys (linear probing over HOT_LDS_PROBES slots, an LDS CAS on an empty
//      one), flushed once when the block ends -- four global adds per key and
//      block, 4096 at most per counter and launch; a group whose LDS run is
//      taken by other keys makes its four global adds at once.
// k_hot_pick merges per wave the same way; only a group's leader loads the four
// counters and probes the table, and a key already present costs no atomic.
// Every global add is a no-return atomic; the only returning atomic is the CAS
// that claims a candidate record.  `dropped` is set with a store, not counted:
// a hot key without a slot would otherwise add to one word from every wave.
// Nothing waits on another thread; every loop is bounded by 64, a probe bound
// or m.  The kernels hold pointers to the four input arrays and the feature's
// own three allocations only.
//
// k_hot_add_routed / k_hot_pick_routed count a finished routed step on the
// key's owner GPU (include/rl_route.h rl_hot_routed_device):
// the same texts, hot_add_requests<Read> / hot_pick_requests<Read>, with
// hot_request reading request p from its 32-byte record and the decision from
// the 32-byte result record at the same receive index.
//
// The kernels are compiled in a translation unit of their own (rl_hot.hip,
// which defines RL_HOT_DEVICE, with the rl_hot_* entry points): the other units
// include this header through rl_engine_impl.h for the types only and gain no
// device code.
#pragma once

#include <hip/hip_runtime.h>

#include "rl_table.h"
#ifdef RL_HOT_DEVICE
#include "rl_routed.h"
#endif

namespace rl {

constexpr int HOT_BLOCK = 256;
// the grid of k_hot_add / k_hot_pick is min(ceil(m / HOT_BLOCK), HOT_GRID) blocks; a larger batch strides
constexpr int HOT_GRID = 1024;
constexpr int HOT_DEPTH = 4;              // RL_HOT_DEPTH
constexpr uint32_t HOT_LDS_KEYS = 256;    // keys merged per block in LDS ...
constexpr uint32_t HOT_LDS_PROBES = 8;    // ... linear probing over this many slots
constexpr uint64_t HOT_PROBES = 64;       // probe bound of the candidate table (min with its slots)

// global words
constexpr int HG_TOTAL = 0, HG_SKIPPED = 1, HG_KEYS = 2, HG_DROPPED = 3, HG_WORDS = 4;

struct HotKey {        // rl_hot_key
    uint64_t key;      // EMPTY_KEY: free
    uint64_t est;      // written by k_hot_read
    uint32_t cfg;      // the config of the request that claimed the slot
    uint32_t pad;
};
static_assert(sizeof(HotKey) == 24, "HotKey must be 24 bytes");

typedef unsigned long long hot_u64;

// the column of key k in row r
RL_HD inline uint64_t hot_col(uint64_t k, int r, uint64_t wmask) { return mix64(k ^ mix64((uint64_t)r + 1)) & wmask; }

#ifdef RL_HOT_DEVICE

__device__ __forceinline__ void hot_add(hot_u64* p, hot_u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void hot_add_lds(hot_u64* p, hot_u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ hot_u64 hot_wave_sum(hot_u64 v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// weight w of key k into its four counters
__device__ __forceinline__ void hot_sketch_add(hot_u64* sketch, uint64_t width, uint64_t k, hot_u64 w) {
#pragma unroll
    for (int r = 0; r < HOT_DEPTH; r++) hot_add(&sketch[(uint64_t)r * width + hot_col(k, r, width - 1)], w);
}

// the minimum of key k's four counters
__device__ __forceinline__ hot_u64 hot_estimate(const hot_u64* sketch, uint64_t width, uint64_t k) {
    hot_u64 est = ~0ull;
#pragma unroll
    for (int r = 0; r < HOT_DEPTH; r++) {
        const hot_u64 v = __hip_atomic_load(&sketch[(uint64_t)r * width + hot_col(k, r, width - 1)], __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
        est = v < est ? v : est;
    }
    return est;
}

// request i of a finished batch in the decide layout: the array form's reader
// (n is read in units mode only)
struct HotArrays {
    const uint64_t* __restrict__ key;
    const uint32_t* __restrict__ cfg;
    const int64_t* __restrict__ n;
    const uint8_t* __restrict__ dec;
    __device__ __forceinline__ void operator()(uint64_t i, bool want_n, uint64_t& k, uint32_t& c, int64_t& nn,
                                               uint32_t& d) const {
        k = key[i];
        c = cfg[i];
        d = dec[i];
        nn = want_n ? n[i] : 0;
    }
};

// request i of the batch as `rd` reads it (HotArrays, or RoutedCount of
// rl_routed.h for a routed step): key, config and weight; whether it counts.
// i >= m is neither counted nor skipped (*valid false).
template <class Read>
__device__ __forceinline__ bool hot_request(uint64_t i, uint64_t m, const Read& rd, uint32_t ncfg, uint32_t units,
                                            uint64_t* k, uint32_t* c, hot_u64* w, bool* valid) {
    *valid = i < m;
    *k = EMPTY_KEY;
    *c = 0xffffffffu;
    *w = 0;
    if (!*valid) return false;
    int64_t nn;
    uint32_t d;
    rd(i, units != 0, *k, *c, nn, d);
    bool counted = *c < ncfg && d <= 2u && *k != EMPTY_KEY;
    if (units) {
        counted = counted && nn > 0;
        *w = counted ? (hot_u64)nn : 0;
    } else {
        *w = counted ? 1 : 0;
    }
    return counted;
}

// The adds of requests 0 .. m - 1 as `rd` reads them: the text of k_hot_add and
// k_hot_add_routed.  m must be uniform over the block.
template <class Read>
__device__ __forceinline__ void hot_add_requests(uint64_t m, const Read& rd, uint32_t ncfg, uint32_t units,
                                                 hot_u64* __restrict__ sketch, uint64_t width,
                                                 hot_u64* __restrict__ glob) {
    __shared__ hot_u64 s_key[HOT_LDS_KEYS], s_w[HOT_LDS_KEYS];
    __shared__ hot_u64 s_glob[2];                        // HG_TOTAL, HG_SKIPPED
    const uint32_t tid = threadIdx.x;
    if (tid < HOT_LDS_KEYS) { s_key[tid] = EMPTY_KEY; s_w[tid] = 0; }
    if (tid < 2) s_glob[tid] = 0;
    __syncthreads();
    const uint32_t lane = tid & 63u;
    // block-uniform trip count: every lane of a wave stays in the loop, so the
    // ballots and shuffles below see all 64 lanes
    for (uint64_t base = blockIdx.x * (uint64_t)HOT_BLOCK; base < m; base += (uint64_t)gridDim.x * HOT_BLOCK) {
        uint64_t k;
        uint32_t c;
        hot_u64 w;
        bool valid;
        const bool counted = hot_request(base + tid, m, rd, ncfg, units, &k, &c, &w, &valid);
        hot_u64 pend = __ballot(counted);
        const hot_u64 skip = __ballot(valid && !counted);
        // the wave's total and skipped, once per wave
        const hot_u64 wtot = units ? hot_wave_sum(w) : (hot_u64)__popcll(pend);
        if (lane == 0) {
            if (pend) hot_add_lds(&s_glob[0], wtot);
            if (skip) hot_add_lds(&s_glob[1], (hot_u64)__popcll(skip));
        }
        // merge the wave's lanes per key, one leader each
        bool lead_me = false;
        hot_u64 myw = 0;
        for (int it = 0; it < 64 && pend; it++) {        // wave-uniform: pend is a ballot
            const int lead = __ffsll((long long)pend) - 1;
            const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, lead);
            const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), lead);
            const bool same = counted && k == ((uint64_t)khi << 32 | klo);
            const hot_u64 grp = __ballot(same);          // holds bit `lead`: pend loses a bit every round
            const hot_u64 cnt = (hot_u64)__popcll(grp);
            // cnt == 1: the leader's own weight
            const hot_u64 gw = !units ? cnt : cnt > 1 ? hot_wave_sum(same ? w : 0) : w;
            if ((int)lane == lead) { lead_me = true; myw = gw; }
            pend &= ~grp;
        }
        if (lead_me) {
            uint32_t ls = (uint32_t)(mix64(k) >> 40) & (HOT_LDS_KEYS - 1);
            bool merged = false;
            // LDS slots only go from empty to a key: a key read here is final,
            // an empty slot is settled by the CAS
            for (uint32_t p = 0; p < HOT_LDS_PROBES && !merged; p++, ls = (ls + 1) & (HOT_LDS_KEYS - 1)) {
                hot_u64 cur = __hip_atomic_load(&s_key[ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == EMPTY_KEY) {
                    cur = atomicCAS(&s_key[ls], (hot_u64)EMPTY_KEY, (hot_u64)k);
                    if (cur == EMPTY_KEY) cur = k;
                }
                if (cur == k) {
                    hot_add_lds(&s_w[ls], myw);
                    merged = true;
                }
            }
            if (!merged) hot_sketch_add(sketch, width, k, myw);   // the run is taken: straight to global
        }
    }
    __syncthreads();
    if (tid < HOT_LDS_KEYS && s_key[tid] != EMPTY_KEY && s_w[tid]) hot_sketch_add(sketch, width, s_key[tid], s_w[tid]);
    if (tid < 2 && s_glob[tid]) hot_add(&glob[tid == 0 ? HG_TOTAL : HG_SKIPPED], s_glob[tid]);
}

__global__ __launch_bounds__(HOT_BLOCK) void k_hot_add(uint64_t m, const uint64_t* __restrict__ key,
                                                       const uint32_t* __restrict__ cfg,
                                                       const int64_t* __restrict__ n,
                                                       const uint8_t* __restrict__ dec, uint32_t ncfg, uint32_t units,
                                                       hot_u64* __restrict__ sketch, uint64_t width,
                                                       hot_u64* __restrict__ glob) {
    hot_add_requests(m, HotArrays{key, cfg, n, dec}, ncfg, units, sketch, width, glob);
}

// The adds of a finished routed step on its owner (rl_hot_routed_device):
// request p < min(m_max, *count) of the merged batch, in either form of the
// merge, with the decision of its result record.  The grid is sized for the
// caller's bound, since the host does not know the count; every thread reads
// *count, so the trip count is uniform over the block.  A count above m_max
// re-raises EF_ROUTED_OVER (routed_open's atomicOr, the flag the decide raised
// already); every other store goes to the feature's own memory.
__global__ __launch_bounds__(HOT_BLOCK) void k_hot_add_routed(uint64_t m_max, RoutedIo io, uint32_t ncfg,
                                                              uint32_t units, hot_u64* __restrict__ sketch,
                                                              uint64_t width, hot_u64* __restrict__ glob) {
    const RoutedForm f = routed_open(m_max, io);
    hot_add_requests(f.m, RoutedCount{io, f}, ncfg, units, sketch, width, glob);
}

// key k (hash h = mix64(k)) qualifies: find its record or claim one; without a
// slot, dropped
__device__ inline void hot_claim(HotKey* keys, uint64_t mask, uint64_t probes, hot_u64* glob, uint64_t k, uint64_t h,
                                 uint32_t c) {
    uint64_t s = h & mask;
    for (uint64_t p = 0; p < probes; p++, s = (s + 1) & mask) {
        hot_u64* kp = (hot_u64*)&keys[s].key;
        hot_u64 cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == EMPTY_KEY) {
            cur = atomicCAS(kp, (hot_u64)EMPTY_KEY, (hot_u64)k);
            if (cur == EMPTY_KEY) {
                keys[s].cfg = c;
                hot_add(&glob[HG_KEYS], 1);
                return;
            }
        }
        if (cur == k) return;
    }
    __hip_atomic_store(&glob[HG_DROPPED], (hot_u64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The look at the keys of requests 0 .. m - 1 as `rd` reads them: the text of
// k_hot_pick and k_hot_pick_routed.  m must be uniform over the block.
template <class Read>
__device__ __forceinline__ void hot_pick_requests(uint64_t m, const Read& rd, uint32_t ncfg, uint32_t units,
                                                  const hot_u64* __restrict__ sketch, uint64_t width, hot_u64 hot_min,
                                                  hot_u64* __restrict__ glob, HotKey* __restrict__ keys, uint64_t mask,
                                                  uint64_t probes) {
    const uint32_t lane = threadIdx.x & 63u;
    // block-uniform trip count, as in hot_add_requests
    for (uint64_t base = blockIdx.x * (uint64_t)HOT_BLOCK; base < m; base += (uint64_t)gridDim.x * HOT_BLOCK) {
        uint64_t k;
        uint32_t c;
        hot_u64 w;
        bool valid;
        const bool counted = hot_request(base + threadIdx.x, m, rd, ncfg, units, &k, &c, &w, &valid);
        hot_u64 pend = __ballot(counted);
        bool lead_me = false;
        for (int it = 0; it < 64 && pend; it++) {        // wave-uniform: pend is a ballot
            const int lead = __ffsll((long long)pend) - 1;
            const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, lead);
            const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), lead);
            const hot_u64 grp = __ballot(counted && k == ((uint64_t)khi << 32 | klo));
            if ((int)lane == lead) lead_me = true;
            pend &= ~grp;
        }
        if (lead_me && hot_estimate(sketch, width, k) >= hot_min) hot_claim(keys, mask, probes, glob, k, mix64(k), c);
    }
}

__global__ __launch_bounds__(HOT_BLOCK) void k_hot_pick(uint64_t m, const uint64_t* __restrict__ key,
                                                        const uint32_t* __restrict__ cfg,
                                                        const int64_t* __restrict__ n,
                                                        const uint8_t* __restrict__ dec, uint32_t ncfg, uint32_t units,
                                                        const hot_u64* __restrict__ sketch, uint64_t width,
                                                        hot_u64 hot_min, hot_u64* __restrict__ glob,
                                                        HotKey* __restrict__ keys, uint64_t mask, uint64_t probes) {
    hot_pick_requests(m, HotArrays{key, cfg, n, dec}, ncfg, units, sketch, width, hot_min, glob, keys, mask, probes);
}

// the same over the routed step k_hot_add_routed counted, behind it on the stream
__global__ __launch_bounds__(HOT_BLOCK) void k_hot_pick_routed(uint64_t m_max, RoutedIo io, uint32_t ncfg,
                                                               uint32_t units, const hot_u64* __restrict__ sketch,
                                                               uint64_t width, hot_u64 hot_min,
                                                               hot_u64* __restrict__ glob, HotKey* __restrict__ keys,
                                                               uint64_t mask, uint64_t probes) {
    const RoutedForm f = routed_open(m_max, io);
    hot_pick_requests(f.m, RoutedCount{io, f}, ncfg, units, sketch, width, hot_min, glob, keys, mask, probes);
}

// every candidate's estimate from the sketch as it is now (rl_hot_read)
__global__ __launch_bounds__(256) void k_hot_read(HotKey* __restrict__ keys, uint64_t slots,
                                                  const hot_u64* __restrict__ sketch, uint64_t width) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += stride) {
        const uint64_t k = keys[i].key;
        if (k != EMPTY_KEY) keys[i].est = hot_estimate(sketch, width, k);
    }
}

// every counter 0, every record free (rl_hot_enable, a clearing rl_hot_read)
__global__ __launch_bounds__(256) void k_hot_clear(hot_u64* __restrict__ sketch, uint64_t words,
                                                   HotKey* __restrict__ keys, uint64_t slots,
                                                   hot_u64* __restrict__ glob) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < words; i += stride) sketch[i] = 0;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += stride) keys[i] = HotKey{EMPTY_KEY, 0, 0, 0};
    if (blockIdx.x == 0 && threadIdx.x < HG_WORDS) glob[threadIdx.x] = 0;
}

#endif  // RL_HOT_DEVICE

}  // namespace rl
