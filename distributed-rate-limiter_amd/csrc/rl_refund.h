// rl_refund.h -- Refund: give consumed quota back (rl_refund_batch,
// include/rl_engine.h).  There is no reference script for this verb; the
// contract is DESIGN.md §10i.
//
// A call of m refunds (key, ts, n, cfg, server clock) groups its valid
// requests by target -- the bucket of `key`, or the window counter key
// (key, window_start(ts)) wherever it lives, in peek_wk's search order -- and
// has the effect of ONE script run per target with N = the saturated sum of
// the n of the requests that found the target live at their own store clock:
//   token bucket:  tokens = math.min(capacity, tokens + N), stored through
//                  tostring; last_refill and the TTL stay
//   window:        if count <= N then DEL else DECRBY N (the TTL stays)
// A per-target sum and not m single refunds: %.14g requantises the stored
// tokens, so bucket refunds do not commute, and the sum is the one answer a
// parallel kernel can give whatever its thread order.
//
// Two launches on the replay stream, over scratch the engine owns:
//   loc[R]   the claim word of record r: the target's location code (a table
//            and an index into it; 0 = free), R = 2 * the largest m rounded up
//            to a power of two, so the load never passes 1/2.  An array of its
//            own: with the claim word inside the record, the lookups of a hot
//            target's word shared a cache line with the atomics on its sums,
//            and the one-key case took twice as long
//   rec[R]   {key, ws | TB sentinel with the config, lo, hi}: key and ws by the
//            claiming thread, lo / hi the sums of the low and the high 32 bits
//            of n (2^20 requests overflow neither)
//   list[]   the claimed records, compacted; cnt[2] its length, one word per
//            call parity -- k_refund_add zeroes the other call's word, so no
//            memset runs between calls
// k_refund_add: one request per thread, grid-stride.  Validate, probe_find,
// locate the live target, write the status; merge the wave's lanes per target
// (the ballot rounds of rl_tally.h, at most 64); the group's leader finds or
// claims the record (linear probing from mix64(code), an empty word settled by
// one CAS) and adds with two no-return atomics.  It stores nothing to a state
// table.
// k_refund_apply: one thread per claimed record.  Rebuild N with saturation,
// do the store above -- the only write to table memory -- and free the record.
// k_refund_add_routed: k_refund_add over the merged batch of a routed step
// (rl_routed.h), the same text (refund_requests<RT>); k_refund_apply follows
// it unchanged.
//
// No spin-wait; every loop is bounded by 64, MAX_PROBES, the table masks or
// m; no CAS loop on table words.  A key a later batch's grouping is inserting
// right now (k_probe's CAS, RL_OPT_PIPELINE) reads as an empty slot or as a
// key with the initial, absent state: no live target, RL_REFUND_NOKEY, which
// is the key until that batch's replay runs, after these kernels (rl_reset.h
// makes the same argument).  Every target has one record and one thread of
// k_refund_apply, so its stores race with nothing.
#pragma once

#include "rl_routed.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_window.h"

namespace rl {

constexpr int REFUND_BLOCK = 256;
// both kernels' grids are min(ceil(m / REFUND_BLOCK), REFUND_GRID) blocks; a
// larger call strides
constexpr int REFUND_GRID = 1024;
// the largest call: the sums lo / hi are sized for it
constexpr uint32_t REFUND_MAX = 1u << 20;

// per-request status (RL_REFUND_NOKEY / RL_REFUND_DONE / RL_INVALID, rl_engine.h)
constexpr uint8_t REFUND_NOKEY = 0, REFUND_DONE = 1, REFUND_INVALID = 3;

// location codes: the table in the top two bits, the index below.  0 is no
// location (a free claim word)
constexpr uint64_t RLOC_TB = 1ull << 62, RLOC_WIN = 2ull << 62, RLOC_SPILL = 3ull << 62;
constexpr uint64_t RLOC_INDEX = (1ull << 62) - 1;
// rec.ws of a token-bucket target: the sentinel and the config id below it
// (a window start is a Unix time in seconds, far from INT64_MIN)
constexpr int64_t REFUND_WS_TB = INT64_MIN;

typedef unsigned long long refund_u64;

struct RefundRec {
    uint64_t key;
    int64_t ws;          // window start; REFUND_WS_TB | cfg for a bucket
    refund_u64 lo, hi;   // sum of n & 0xffffffff, sum of n >> 32
};
static_assert(sizeof(RefundRec) == 32, "RefundRec must be 32 bytes");

struct RefundScratch {
    refund_u64* loc;
    RefundRec* rec;
    uint32_t* list;
    uint32_t* cnt;     // [2]
    uint64_t mask;     // records - 1
};

// N of a record: hi * 2^32 + lo, saturated at INT64_MAX
RL_HD inline int64_t refund_total(uint64_t lo, uint64_t hi) {
    const uint64_t h = hi + (lo >> 32);   // both below 2^53: no wrap
    if (h >= (1ull << 31)) return INT64_MAX;
    return (int64_t)(h << 32 | (lo & 0xffffffffull));
}

__device__ __forceinline__ refund_u64 refund_wave_sum(refund_u64 v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the live target of a valid request at its store clock, or 0.  The window
// search is peek_wk's: a dead slot key falls through to the other slot and the
// spill, a dead spill entry ends it
__device__ inline uint64_t refund_locate(uint64_t k, int64_t t, int64_t sms, const CfgDev& C, const TbEntry* tb,
                                         uint64_t tb_mask, const WinEntry* win, uint64_t win_mask, const Spill& spill,
                                         int32_t profile, int64_t& ws) {
    if (C.alg == ALG_TOKEN_BUCKET) {
        const uint32_t s = probe_find(tb, tb_mask, k);
        if (s == NO_SLOT) return 0;
        return key_alive(tb[s].when, sms, profile) ? RLOC_TB | s : 0;
    }
    const uint32_t s = probe_find(win, win_mask, k);
    if (s == NO_SLOT) return 0;
    ws = window_start(t, C);
    const WinEntry e = win[s];   // the 64-byte entry, once
    for (int j = 0; j < 2; j++) {
        if (e.s[j].when == ABSENT || e.s[j].ws != ws) continue;
        if (!key_alive(e.s[j].when, sms, profile)) continue;
        return RLOC_WIN | ((uint64_t)s << 1 | (uint64_t)j);
    }
    const SpillEntry* sp = spill_lookup(spill, k, e.nspill, ws);
    if (!sp) return 0;
    return key_alive(sp->when, sms, profile) ? RLOC_SPILL | (uint64_t)(sp - spill.tab) : 0;
}

// the group's leader: find or claim the record of `code` and add.  At most
// REFUND_MAX targets in 2 * REFUND_MAX records (or the engine's smaller pair):
// a free word is always within the table's length
__device__ inline void refund_upsert(const RefundScratch& S, uint32_t parity, uint64_t code, uint64_t k, int64_t ws,
                                     refund_u64 lo, refund_u64 hi) {
    uint64_t r = mix64(code) & S.mask;
    for (uint64_t p = 0; p <= S.mask; p++, r = (r + 1) & S.mask) {
        refund_u64 cur = __hip_atomic_load(&S.loc[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&S.loc[r], (refund_u64)0, (refund_u64)code);
            if (cur == 0) {   // claimed: the record's identity, and its place in the list
                S.rec[r].key = k;
                S.rec[r].ws = ws;
                const uint32_t at = atomicAdd(&S.cnt[parity], 1u);
                if (at <= S.mask) S.list[at] = (uint32_t)r;
                cur = code;
            }
        }
        if (cur == code) {
            (void)__hip_atomic_fetch_add(&S.rec[r].lo, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (hi) (void)__hip_atomic_fetch_add(&S.rec[r].hi, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
}

// The text of k_refund_add and k_refund_add_routed.  RT selects where a
// request's fields come from and where its status goes; validation, the
// locate, the ballot rounds, the upsert and the parity word are the one text
// between.  RT = false: m refunds as arrays in the caller's order, a status
// byte each (nullable), a nullable store clock.  RT = true: the merged batch of
// a routed step (rl_routed.h) -- m is the bound B = min(m_max, rl_refund_max),
// the size is in device memory, the store clock is the merge's, and the status
// goes out as one rl_route_res {status, 0, 0, 0} at the receive index.
template <bool RT>
__device__ __forceinline__ void refund_requests(uint64_t m, const uint64_t* __restrict__ key,
                                                const int64_t* __restrict__ ts, const int64_t* __restrict__ n,
                                                const uint32_t* __restrict__ cfg, const int64_t* __restrict__ sms,
                                                uint8_t* __restrict__ status, const RoutedIo& io, uint64_t m_max,
                                                const CfgDev* __restrict__ cfgs, uint32_t ncfg, const TbEntry* tb,
                                                uint64_t tb_mask, const WinEntry* win, uint64_t win_mask,
                                                const Spill& spill, int32_t profile, const RefundScratch& S,
                                                uint32_t parity) {
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    // the other call parity's list length: that call's k_refund_apply is done
    if (blockIdx.x == 0 && tid == 0) S.cnt[parity ^ 1u] = 0;
    const uint64_t bound = m;
    RoutedForm f{};
    if (RT) {
        f = routed_open(bound, io);   // a count above B raises EF_ROUTED_OVER
        m = f.m;                      // min(B, *count): the same in every thread
    }
    // block-uniform trip count: every lane of a wave stays in the loop, so the
    // ballots and shuffles below see all 64 lanes
    for (uint64_t base = blockIdx.x * (uint64_t)REFUND_BLOCK; base < m; base += (uint64_t)gridDim.x * REFUND_BLOCK) {
        const uint64_t i = base + tid;
        uint64_t k = 0, code = 0;
        int64_t ws = 0, nn = 0;
        if (i < m) {
            uint32_t c, at = 0;
            int64_t tq = 0, clock = 0;
            if (RT) {
                const rl_route_rec q = routed_request(io, f, i, at, clock);
                k = q.key; nn = q.n; c = q.cfg; tq = q.ts;
            } else {
                k = key[i];
                nn = n[i];
                c = cfg[i];
            }
            uint8_t st = REFUND_INVALID;
            if (c < ncfg && nn > 0 && k != EMPTY_KEY) {
                const int64_t t = RT ? tq : ts[i];
                if (!RT) clock = sms ? sms[i] : floor_div(t, 1000000LL);
                const CfgDev C = cfgs[c];
                ws = C.alg == ALG_TOKEN_BUCKET ? (int64_t)(REFUND_WS_TB | (int64_t)c) : 0;
                code = refund_locate(k, t, clock, C, tb, tb_mask, win, win_mask, spill, profile, ws);
                st = code ? REFUND_DONE : REFUND_NOKEY;
            }
            if (RT) routed_result(io, at, st, 0, 0, 0);
            else if (status) status[i] = st;
        }
        // --- merge the wave's lanes per target, one leader each ---
        const refund_u64 lo = code ? (refund_u64)nn & 0xffffffffull : 0, hi = code ? (refund_u64)nn >> 32 : 0;
        refund_u64 pend = __ballot(code != 0);
        refund_u64 mylo = 0, myhi = 0;
        bool leader = false;
        for (int it = 0; it < 64 && pend; it++) {        // wave-uniform: pend is a ballot
            const int lead = __ffsll((long long)pend) - 1;
            const uint32_t clo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)code, lead);
            const uint32_t chi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(code >> 32), lead);
            const bool same = code == ((uint64_t)chi << 32 | clo);   // the lead's code is not 0
            const refund_u64 grp = __ballot(same);       // holds bit `lead`: pend loses a bit every round
            const bool many = __popcll(grp) > 1;         // one lane: the leader's own n
            const refund_u64 slo = many ? refund_wave_sum(same ? lo : 0) : lo;
            const refund_u64 shi = many ? refund_wave_sum(same ? hi : 0) : hi;
            if ((int)lane == lead) { mylo = slo; myhi = shi; leader = true; }
            pend &= ~grp;
        }
        if (leader) refund_upsert(S, parity, code, k, ws, mylo, myhi);
    }
    if (RT) {
        // the merged requests past B, below the caller's bound: not executed
        const uint64_t cnt = *io.count;
        const uint64_t end = cnt < m_max ? cnt : m_max;
        for (uint64_t p = bound + blockIdx.x * (uint64_t)REFUND_BLOCK + tid; p < end;
             p += (uint64_t)gridDim.x * REFUND_BLOCK)
            routed_result(io, f.ident ? (uint32_t)p : io.order[p], RL_DROPPED, 0, 0, 0);
    }
}

__global__ __launch_bounds__(REFUND_BLOCK) void k_refund_add(uint64_t m, const uint64_t* __restrict__ key,
                                                             const int64_t* __restrict__ ts,
                                                             const int64_t* __restrict__ n,
                                                             const uint32_t* __restrict__ cfg,
                                                             const int64_t* __restrict__ sms,
                                                             uint8_t* __restrict__ status,
                                                             const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                             const TbEntry* tb, uint64_t tb_mask, const WinEntry* win,
                                                             uint64_t win_mask, Spill spill, int32_t profile,
                                                             RefundScratch S, uint32_t parity) {
    refund_requests<false>(m, key, ts, n, cfg, sms, status, RoutedIo{}, 0, cfgs, ncfg, tb, tb_mask, win, win_mask,
                           spill, profile, S, parity);
}

// The refund step of the routed path (rl_refund_routed_device): k_refund_add
// on the merged batch, then k_refund_apply as it is.  The merged batch is ONE
// refund call: all ranks' refunds of one target in the step meet in one record
// and are applied once, whatever the merge order.  The grid is sized for
// B = min(m_max, rl_refund_max), min(ceil(B / REFUND_BLOCK), REFUND_GRID)
// blocks, since the host does not know the count; m = min(B, *count) is the
// same in every thread, so the trip count stays block-uniform.  A count above
// B: one thread raises EF_ROUTED_OVER, and the requests B <= p < min(*count,
// m_max) get {RL_DROPPED, 0, 0, 0} -- not executed, to be resubmitted.
// As the array form: no spin-wait; every loop is bounded by 64, MAX_PROBES,
// the table masks, R or m_max; no CAS loop on table words; nothing is stored
// to a state table here (k_refund_apply makes the only such store); no inline
// assembly.  Its atomics are those of refund_upsert and the one atomicOr.
__global__ __launch_bounds__(REFUND_BLOCK) void k_refund_add_routed(uint64_t bound, uint64_t m_max, RoutedIo io,
                                                                    const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                                    const TbEntry* tb, uint64_t tb_mask,
                                                                    const WinEntry* win, uint64_t win_mask,
                                                                    Spill spill, int32_t profile, RefundScratch S,
                                                                    uint32_t parity) {
    refund_requests<true>(bound, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, io, m_max, cfgs, ncfg, tb,
                          tb_mask, win, win_mask, spill, profile, S, parity);
}

__global__ __launch_bounds__(REFUND_BLOCK) void k_refund_apply(const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                               TbEntry* tb, uint64_t tb_mask, WinEntry* win,
                                                               uint64_t win_mask, Spill spill, int32_t profile,
                                                               RefundScratch S, uint32_t parity) {
    uint64_t count = S.cnt[parity];
    if (count > S.mask + 1) count = S.mask + 1;
    for (uint64_t i = blockIdx.x * (uint64_t)REFUND_BLOCK + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * REFUND_BLOCK) {
        const uint64_t r = S.list[i] & S.mask;
        const uint64_t code = S.loc[r];
        const RefundRec x = S.rec[r];
        // the record is free again for the next call
        S.loc[r] = 0;
        S.rec[r].lo = 0;
        S.rec[r].hi = 0;
        const int64_t N = refund_total(x.lo, x.hi);
        const uint64_t at = code & RLOC_INDEX;
        switch (code & ~RLOC_INDEX) {
        case RLOC_TB: {
            const uint32_t c = (uint32_t)(x.ws & 0xffffffffLL);
            if (at > tb_mask || c >= ncfg) break;
            // tokens = math.min(capacity, tokens + N); HSET tokens tostring(tokens)
            const double cap = cfgs[c].limit_d;
            const double s = tb[at].tok + (double)N;
            tb[at].tok = lua_tostring_roundtrip(s < cap ? s : cap, profile);
            break;
        }
        case RLOC_WIN: {
            if ((at >> 1) > win_mask) break;
            WinSlot* w = &win[at >> 1].s[at & 1];
            // if c <= N then DEL key else DECRBY key N
            const int64_t c = w->cnt;
            if (c <= N) w->when = ABSENT;
            else w->cnt = c - N;
            break;
        }
        case RLOC_SPILL: {
            if (at > spill.mask) break;
            SpillEntry* e = &spill.tab[at];
            const int64_t c = e->cnt;
            if (c <= N) e->when = ABSENT;
            else e->cnt = c - N;
            break;
        }
        default: break;
        }
    }
}

}  // namespace rl
