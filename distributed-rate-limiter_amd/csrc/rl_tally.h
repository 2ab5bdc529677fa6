// rl_tally.h -- usage tally (rl_tally_*, include/rl_engine.h): what the
// decisions of finished batches were, counted on the device.
//
// k_tally reads one finished batch in the decide layout -- key id, config id,
// n and the decision byte, 21 B per request, one request per thread -- and adds
// to accumulators the engine owns:
//   * per registered config six 64-bit counters: count[decision] for the four
//     decision codes, units[0] = sum of n over denied and units[1] over allowed
//     requests (n > 0 only; the sums wrap modulo 2^64);
//   * global words: requests with an unregistered config id (TG_UNKNOWN) and,
//     among the others, with a decision byte above 3 (TG_BAD) -- such a request
//     adds nothing else;
//   * a fixed-capacity open-addressing table of the keys that had a denied
//     request: {key, denied, units_denied, cfg}.  Home slot mix64(key) & mask,
//     linear probing over at most min(slots, TALLY_PROBES) slots; an empty slot
//     is claimed with one CAS.  Slots are never released before a clear, so a
//     key's probe run only ever fills: the key ends in the same slot every
//     time, or finds its whole run taken by others every time -- it is tracked
//     completely or not at all.  A key without a slot (and the reserved key id,
//     which marks an empty slot) adds to TG_UNTRACKED_REQ / TG_UNTRACKED_UNITS.
//
// Contention.  A hot key can hold a tenth of a batch, all denied: one atomic
// per request on its record would serialize the batch.  Denied lanes are
// merged three times before global memory sees them:
//   1. in the wave: the first pending lane's key is broadcast (readlane of a
//      ballot's first bit), the lanes that hold it drop out, their count is the
//      ballot's popcount and their units a wave sum; at most 64 rounds;
//   2. in the block: the group's leader adds to an LDS table of TALLY_LDS_KEYS
//      keys (linear probing over TALLY_LDS_PROBES slots, an LDS CAS on an empty
//      one; a run taken by other keys sends the group to global memory at
//      once), flushed once when the block ends -- so a key the block sees often
//      costs one global sequence per block, 1024 at most per launch;
//   3. the per-config counters of ids below TALLY_LDS_CFGS accumulate in LDS
//      too (a wave whose lanes all share config and decision adds once), ids
//      above go to the global counters directly.
// Every global add is a no-return atomic.  Nothing waits on another thread;
// every loop is bounded by 64, the probe bound, or m.  The kernel stores to
// the tally's own memory only: it holds no pointer to a state table.
//
// k_tally_routed counts a finished routed step on the key's owner GPU
// (include/rl_route.h rl_tally_routed_device): the same text,
// tally_requests<Read>, reading request p from its 32-byte record and the
// decision from the 32-byte result record at the same receive index.
//
// The kernels are compiled in a translation unit of their own (rl_tally.hip,
// which defines RL_TALLY_DEVICE, with the rl_tally_* entry points): the other
// units include this header through rl_engine_impl.h for the types only and
// gain no device code.
#pragma once

#include <hip/hip_runtime.h>

#include "rl_table.h"
#ifdef RL_TALLY_DEVICE
#include "rl_routed.h"
#endif

namespace rl {

constexpr int TALLY_BLOCK = 256;
// k_tally's grid is min(ceil(m / TALLY_BLOCK), TALLY_GRID) blocks; a larger batch strides
constexpr int TALLY_GRID = 1024;
constexpr uint32_t TALLY_LDS_CFGS = 32;    // config ids below this accumulate in LDS
constexpr uint32_t TALLY_LDS_KEYS = 256;   // denied keys merged per block in LDS ...
constexpr uint32_t TALLY_LDS_PROBES = 8;   // ... linear probing over this many slots
constexpr uint64_t TALLY_PROBES = 64;      // probe bound of the key table (min with its slots)
constexpr int TALLY_CFG_WORDS = 6;         // count[4], units[2]

// global words
constexpr int TG_UNKNOWN = 0, TG_BAD = 1, TG_UNTRACKED_REQ = 2, TG_UNTRACKED_UNITS = 3, TG_KEYS = 4, TG_WORDS = 8;
// ... of the routed form (k_tally_routed): requests looked at, requests dropped at their senders
constexpr int TG_ROUTED_REQ = 5, TG_ROUTED_DROPPED = 6;

struct TallyKey {      // rl_tally_key
    uint64_t key;      // EMPTY_KEY: free
    uint64_t denied;
    uint64_t units;
    uint32_t cfg;      // the config of the denied request that claimed the slot
    uint32_t pad;
};
static_assert(sizeof(TallyKey) == 32, "TallyKey must be 32 bytes");

typedef unsigned long long tally_u64;

#ifdef RL_TALLY_DEVICE

__device__ __forceinline__ void tally_add(tally_u64* p, tally_u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void tally_add_lds(tally_u64* p, tally_u64 v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ tally_u64 tally_wave_sum(tally_u64 v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// `cnt` denied requests of key k (hash h = mix64(k)) with `units` units, of
// config c: find or claim k's record and add; without a slot, the untracked words
__device__ inline void tally_upsert(TallyKey* keys, uint64_t mask, uint64_t probes, tally_u64* glob, uint64_t k,
                                    uint64_t h, uint32_t c, tally_u64 cnt, tally_u64 units) {
    if (k != EMPTY_KEY) {
        uint64_t s = h & mask;
        for (uint64_t p = 0; p < probes; p++, s = (s + 1) & mask) {
            tally_u64* kp = (tally_u64*)&keys[s].key;
            tally_u64 cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == EMPTY_KEY) {
                cur = atomicCAS(kp, (tally_u64)EMPTY_KEY, (tally_u64)k);
                if (cur == EMPTY_KEY) {
                    keys[s].cfg = c;
                    tally_add(&glob[TG_KEYS], 1);
                    cur = k;
                }
            }
            if (cur == k) {
                tally_add((tally_u64*)&keys[s].denied, cnt);
                if (units) tally_add((tally_u64*)&keys[s].units, units);
                return;
            }
        }
    }
    tally_add(&glob[TG_UNTRACKED_REQ], cnt);
    if (units) tally_add(&glob[TG_UNTRACKED_UNITS], units);
}

// request i of a finished batch in the decide layout: the array form's reader
struct TallyArrays {
    const uint64_t* __restrict__ key;
    const uint32_t* __restrict__ cfg;
    const int64_t* __restrict__ n;
    const uint8_t* __restrict__ dec;
    __device__ __forceinline__ void operator()(uint64_t i, bool, uint64_t& k, uint32_t& c, int64_t& nn,
                                               uint32_t& d) const {
        k = key[i];
        c = cfg[i];
        nn = n[i];
        d = dec[i];
    }
};

// The tally of requests 0 .. m - 1 as `rd` reads them: the text of k_tally
// (Read = TallyArrays) and k_tally_routed (Read = RoutedCount, rl_routed.h).
// Only the read differs; the counting rules, the three merges and every atomic
// are this one text.  m must be uniform over the block.
template <class Read>
__device__ __forceinline__ void tally_requests(uint64_t m, const Read& rd, uint32_t ncfg,
                                               tally_u64* __restrict__ cfgc, tally_u64* __restrict__ glob,
                                               TallyKey* __restrict__ keys, uint64_t mask, uint64_t probes) {
    __shared__ tally_u64 s_cfg[TALLY_LDS_CFGS * TALLY_CFG_WORDS];
    __shared__ tally_u64 s_glob[2];                      // TG_UNKNOWN, TG_BAD
    __shared__ tally_u64 s_key[TALLY_LDS_KEYS], s_den[TALLY_LDS_KEYS], s_units[TALLY_LDS_KEYS];
    __shared__ uint32_t s_kcfg[TALLY_LDS_KEYS];
    const uint32_t tid = threadIdx.x;
    if (tid < TALLY_LDS_CFGS * TALLY_CFG_WORDS) s_cfg[tid] = 0;
    if (tid < 2) s_glob[tid] = 0;
    if (tid < TALLY_LDS_KEYS) { s_key[tid] = EMPTY_KEY; s_den[tid] = 0; s_units[tid] = 0; s_kcfg[tid] = 0; }
    __syncthreads();
    const uint32_t lane = tid & 63u;
    // block-uniform trip count: every lane of a wave stays in the loop, so the
    // ballots and shuffles below see all 64 lanes
    for (uint64_t base = blockIdx.x * (uint64_t)TALLY_BLOCK; base < m; base += (uint64_t)gridDim.x * TALLY_BLOCK) {
        const uint64_t i = base + tid;
        const bool valid = i < m;
        uint64_t k = EMPTY_KEY;
        uint32_t c = 0xffffffffu, d = 0xffu;
        tally_u64 u = 0;
        if (valid) {
            int64_t nn;
            rd(i, true, k, c, nn, d);
            u = nn > 0 ? (tally_u64)nn : 0;
        }
        const bool counted = valid && c < ncfg && d <= 3u;
        if (valid && !counted) tally_add_lds(&s_glob[c < ncfg ? 1 : 0], 1);
        if (d > 1u) u = 0;                               // units of denied and allowed requests only
        // --- per-config counters ---
        const uint32_t cd = counted ? (c << 2 | d) : 0xffffffffu;
        const uint32_t cd0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cd);
        if (__ballot(cd == cd0) == ~0ull) {
            if (cd0 != 0xffffffffu) {                    // one config, one decision: the wave adds once
                const tally_u64 us = cd0 & 2u ? 0 : tally_wave_sum(u);
                if (lane == 0) {
                    const uint32_t c0 = cd0 >> 2, d0 = cd0 & 3u;
                    if (c0 < TALLY_LDS_CFGS) {
                        tally_add_lds(&s_cfg[c0 * TALLY_CFG_WORDS + d0], 64);
                        if (us) tally_add_lds(&s_cfg[c0 * TALLY_CFG_WORDS + 4 + d0], us);
                    } else {
                        tally_add(&cfgc[(uint64_t)c0 * TALLY_CFG_WORDS + d0], 64);
                        if (us) tally_add(&cfgc[(uint64_t)c0 * TALLY_CFG_WORDS + 4 + d0], us);
                    }
                }
            }
        } else if (counted) {
            if (c < TALLY_LDS_CFGS) {
                tally_add_lds(&s_cfg[c * TALLY_CFG_WORDS + d], 1);
                if (u) tally_add_lds(&s_cfg[c * TALLY_CFG_WORDS + 4 + d], u);
            } else {
                tally_add(&cfgc[(uint64_t)c * TALLY_CFG_WORDS + d], 1);
                if (u) tally_add(&cfgc[(uint64_t)c * TALLY_CFG_WORDS + 4 + d], u);
            }
        }
        // --- denied keys: merge the wave's lanes per key, one leader each ---
        const bool den = counted && d == 0u;
        tally_u64 pend = __ballot(den);
        tally_u64 mycnt = 0, myunits = 0;
        for (int it = 0; it < 64 && pend; it++) {        // wave-uniform: pend is a ballot
            const int lead = __ffsll((long long)pend) - 1;
            const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)k, lead);
            const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(k >> 32), lead);
            const bool same = den && k == ((uint64_t)khi << 32 | klo);
            const tally_u64 grp = __ballot(same);        // holds bit `lead`: pend loses a bit every round
            const tally_u64 cnt = (tally_u64)__popcll(grp);
            const tally_u64 us = cnt > 1 ? tally_wave_sum(same ? u : 0) : u;   // cnt == 1: the leader's own
            if ((int)lane == lead) { mycnt = cnt; myunits = us; }
            pend &= ~grp;
        }
        if (mycnt) {
            const uint64_t h = mix64(k);
            uint32_t ls = (uint32_t)(h >> 40) & (TALLY_LDS_KEYS - 1);
            bool merged = false;
            // LDS slots only go from empty to a key: a key read here is final,
            // an empty slot is settled by the CAS
            for (uint32_t p = 0; p < TALLY_LDS_PROBES && k != EMPTY_KEY && !merged; p++, ls = (ls + 1) & (TALLY_LDS_KEYS - 1)) {
                tally_u64 cur = __hip_atomic_load(&s_key[ls], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (cur == EMPTY_KEY) {
                    cur = atomicCAS(&s_key[ls], (tally_u64)EMPTY_KEY, (tally_u64)k);
                    if (cur == EMPTY_KEY) {
                        s_kcfg[ls] = c;
                        cur = k;
                    }
                }
                if (cur == k) {
                    tally_add_lds(&s_den[ls], mycnt);
                    if (myunits) tally_add_lds(&s_units[ls], myunits);
                    merged = true;
                }
            }
            if (!merged) tally_upsert(keys, mask, probes, glob, k, h, c, mycnt, myunits);
        }
    }
    __syncthreads();
    if (tid < TALLY_LDS_CFGS * TALLY_CFG_WORDS && tid / TALLY_CFG_WORDS < ncfg && s_cfg[tid]) tally_add(&cfgc[tid], s_cfg[tid]);
    if (tid < 2 && s_glob[tid]) tally_add(&glob[tid == 0 ? TG_UNKNOWN : TG_BAD], s_glob[tid]);
    if (tid < TALLY_LDS_KEYS && s_key[tid] != EMPTY_KEY)
        tally_upsert(keys, mask, probes, glob, s_key[tid], mix64(s_key[tid]), s_kcfg[tid], s_den[tid], s_units[tid]);
}

__global__ __launch_bounds__(TALLY_BLOCK) void k_tally(uint64_t m, const uint64_t* __restrict__ key,
                                                       const uint32_t* __restrict__ cfg,
                                                       const int64_t* __restrict__ n,
                                                       const uint8_t* __restrict__ dec, uint32_t ncfg,
                                                       tally_u64* __restrict__ cfgc, tally_u64* __restrict__ glob,
                                                       TallyKey* __restrict__ keys, uint64_t mask, uint64_t probes) {
    tally_requests(m, TallyArrays{key, cfg, n, dec}, ncfg, cfgc, glob, keys, mask, probes);
}

// The tally of a finished routed step on its owner (rl_tally_routed_device):
// request p < min(m_max, *count) of the merged batch, in either form of the
// merge, with the decision of its result record.  The grid is sized for the
// caller's bound, min(ceil(m_max / TALLY_BLOCK), TALLY_GRID) blocks, since the
// host does not know the count; every thread reads *count, so the trip count
// ceil(min(m_max, *count) / TALLY_BLOCK) rounds of the grid is uniform over the
// block.  A count above m_max re-raises EF_ROUTED_OVER (routed_open's atomicOr,
// the flag the decide raised already); every other store goes to the tally's
// own memory.  One thread adds the step's size to TG_ROUTED_REQ and, with the
// received info rows, the requests the `world` senders dropped for this owner
// (row 3 >> 1 of each source: they never arrived, so nothing else shows them)
// to TG_ROUTED_DROPPED.
__global__ __launch_bounds__(TALLY_BLOCK) void k_tally_routed(uint64_t m_max, RoutedIo io,
                                                              const int64_t* __restrict__ recv_info, uint32_t world,
                                                              uint32_t ncfg, tally_u64* __restrict__ cfgc,
                                                              tally_u64* __restrict__ glob,
                                                              TallyKey* __restrict__ keys, uint64_t mask,
                                                              uint64_t probes) {
    const RoutedForm f = routed_open(m_max, io);
    tally_requests(f.m, RoutedCount{io, f}, ncfg, cfgc, glob, keys, mask, probes);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (f.m) tally_add(&glob[TG_ROUTED_REQ], f.m);
        tally_u64 dropped = 0;
        if (recv_info)
            for (uint32_t s = 0; s < world; s++) dropped += (tally_u64)recv_info[RL_ROUTE_INFO * s + 3] >> 1;
        if (dropped) tally_add(&glob[TG_ROUTED_DROPPED], dropped);
    }
}

// every record free, every counter 0 (rl_tally_enable, a clearing rl_tally_read)
__global__ __launch_bounds__(256) void k_tally_clear(TallyKey* __restrict__ keys, uint64_t slots,
                                                     tally_u64* __restrict__ cfgc, uint64_t cfg_words,
                                                     tally_u64* __restrict__ glob) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < slots; i += stride) keys[i] = TallyKey{EMPTY_KEY, 0, 0, 0, 0};
    for (uint64_t i = blockIdx.x * 256ull + threadIdx.x; i < cfg_words; i += stride) cfgc[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < TG_WORDS) glob[threadIdx.x] = 0;
}

#endif  // RL_TALLY_DEVICE

}  // namespace rl
