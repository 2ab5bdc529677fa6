// rl_peek.h -- read-only quota queries (rl_peek_batch, include/rl_engine.h).
//
// A peek is the Result AllowN(key, n) would return at (ts, server clock),
// computed against the table state as it is and changing nothing: no key is
// inserted, no tokens are stored, no INCRBY, no TTL refresh, no lazy-expiry
// deletion, no spill slot claimed.  n == 0 is legal here only: the status
// query ("how much is left"), the same arithmetic with requested = 0.
//
// One request per thread in the caller's order.  Peeks do not interact, so
// there is no sort and duplicate keys simply read the same state.  The token
// bucket runs the script step itself (tb_step, rl_semantics.h) on a local copy
// of the entry that is then dropped.  The window scripts' steps (fw_step /
// sw_step, rl_window.h) write where they read, so their read-only tails are
// restated here: the same lookups without the lazy DEL, the same arithmetic
// without the INCRBY / EXPIRE stores.  Built with -ffp-contract=off like the
// rest of the engine; tests/test_peek_gpu.py pins the restatement against the
// oracle.
//
// No atomic, no spin, no store to table memory; every loop is bounded by
// MAX_PROBES or the table mask (probe_find, spill_lookup).
#pragma once

#include "rl_batch.h"
#include "rl_routed.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_window.h"

namespace rl {

constexpr int PEEK_BLOCK = 256;
// k_peek's grid is min(ceil(m / PEEK_BLOCK), PEEK_GRID) blocks: past
// PEEK_GRID * PEEK_BLOCK requests each thread strides to further ones.
// 1024 blocks of 4 waves are 16 waves per CU on 256 CUs, the random table
// reads of 64 K requests in flight at once.
constexpr int PEEK_GRID = 1024;

// lookupKey of window key `ws` without the lazy DEL of wk_find: the count of
// the live key, or found = false.  Follows wk_find step by step -- a dead slot
// key falls through to the other slot and the spill, a dead spill entry ends
// the search -- so it reads what the script's GET / INCRBY would
__device__ inline int64_t peek_wk(const WinState& w, const Spill& S, int64_t ws, int64_t s_ms, int32_t profile,
                                  bool& found) {
    found = false;
    for (int k = 0; k < 2; k++) {
        if (w.s[k].when == ABSENT || w.s[k].ws != ws) continue;
        if (!key_alive(w.s[k].when, s_ms, profile)) continue;
        found = true;
        return w.s[k].cnt;
    }
    const SpillEntry* e = spill_lookup(S, w.key, w.nspill, ws);
    if (!e) return 0;
    // the entry as one 32-byte copy and the count by a select: with the early
    // return `if (!key_alive(when)) return 0; return cnt;` this toolchain's
    // code dropped the count of every key that has a TTL (tests/test_peek_gpu.py
    // test_spill pins it)
    const SpillEntry x = *e;
    found = key_alive(x.when, s_ms, profile);
    return found ? x.cnt : 0;
}

// fixedWindowScript + AllowN without its writes (fw_step)
__device__ inline Out peek_fw(const WinState& w, const Spill& S, int64_t t, int64_t n, int64_t s_ms,
                              const CfgDev& c, int32_t profile) {
    Out o;
    o.tokens = 0.0;
    const int64_t ws = window_start(t, c);
    o.reset_at = wadd(wmul(ws, NS_PER_S), c.window);
    bool found;
    const int64_t old = peek_wk(w, S, ws, s_ms, profile, found);
    if (incr_overflows(old, n)) {
        o.decision = DEC_ERROR; o.remaining = 0; o.retry = 0;
        return o;
    }
    const int64_t cur = old + n;
    const int64_t count = go_f2i((double)cur);
    const bool allowed = count <= c.limit;
    const int64_t rem = wsub(c.limit, count);
    o.remaining = rem < 0 ? 0 : rem;
    o.decision = allowed ? DEC_ALLOWED : DEC_DENIED;
    o.retry = allowed ? 0 : until_reset(o.reset_at, t);
    return o;
}

// slidingWindowScript + AllowN without its writes (sw_step)
__device__ inline Out peek_sw(const WinState& w, const Spill& S, int64_t t, int64_t n, int64_t s_ms,
                              const CfgDev& c, int32_t profile) {
    Out o;
    o.tokens = 0.0;
    const int64_t ws = window_start(t, c);
    const int64_t pws = ws - c.ttl_c;
    o.reset_at = wadd(wmul(ws, NS_PER_S), c.window);
    bool pfound, cfound;
    const int64_t pcnt = peek_wk(w, S, pws, s_ms, profile, pfound);
    const double prev = pfound ? (double)pcnt : 0.0;
    const int64_t old = peek_wk(w, S, ws, s_ms, profile, cfound);
    if (incr_overflows(old, n)) {
        o.decision = DEC_ERROR; o.remaining = 0; o.retry = 0;
        return o;
    }
    const int64_t cur = old + n;
    const int64_t p = go_f2i(prev);
    const int64_t cc = go_f2i((double)cur);
    // calculateWeightedCount (slidingwindow.go:190-197): two separate roundings
    const int64_t elapsed = wsub(t, wmul(ws, NS_PER_S));
    const double progress = (double)elapsed / (double)c.window;
    double weighted = (double)p * (1.0 - progress);
    weighted = weighted + (double)cc;
    const bool allowed = weighted <= c.limit_d;
    const int64_t rem = wsub(c.limit, go_f2i(weighted));
    o.remaining = rem < 0 ? 0 : rem;
    o.decision = allowed ? DEC_ALLOWED : DEC_DENIED;
    o.retry = allowed ? 0 : until_reset(o.reset_at, t);
    return o;
}

// tokenBucketScript + AllowN without its writes: the script step itself
// (tb_step) on a local copy of the key's entry, which is then dropped.  The
// text k_peek and Charge's ask (rl_charge.h, n = 0) share.
__device__ inline Out peek_tb(const TbEntry* tb, uint64_t tb_mask, uint64_t k, int64_t t, int64_t n, int64_t sms,
                              const CfgDev& C, int32_t profile) {
    const uint32_t s = probe_find(tb, tb_mask, k);
    TbState st{0.0, 0.0, ABSENT};
    if (s != NO_SLOT) {
        const TbEntry e = tb[s];   // the 32-byte entry, once
        st = TbState{e.tok, e.last, e.when};
    }
    return tb_step(st, t, n, sms, C, profile);   // the copy is dropped
}

// One request per thread, grid-stride.  The tables are only read: a key a
// later batch's grouping is inserting right now (k_probe's CAS,
// RL_OPT_PIPELINE) reads either as an empty slot or as a key whose entry
// still holds the initial, absent state -- both are the key without state,
// which is what it is until that batch's replay runs, after this kernel.
//
// RT selects the input form only; the per-request logic below it is the one
// text for both kernels.  RT = false (k_peek): m requests as arrays in the
// caller's order (ReqArgs), results to its arrays.  RT = true (k_peek_routed):
// the merged batch of a routed step (rl_routed.h) -- at most m requests, the
// size in device memory; request p is rec[order[p]] with store clock sms[p],
// or the RL_ORDER_IDENTITY form; its result is one rl_route_res at its receive
// index (no tokens field, as the routed decide).
template <bool RT>
__device__ __forceinline__ void peek_requests(uint64_t m, const ReqArgs& a, const RoutedIo& io,
                                              const CfgDev* __restrict__ cfgs, uint32_t ncfg, const TbEntry* tb,
                                              uint64_t tb_mask, const WinEntry* win, uint64_t win_mask,
                                              const Spill& spill, int32_t profile) {
    RoutedForm f{};
    if (RT) {
        f = routed_open(m, io);
        m = f.m;
    }
    for (uint64_t i = blockIdx.x * (uint64_t)PEEK_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * PEEK_BLOCK) {
        uint64_t k;
        uint32_t c, at = 0;
        int64_t n, t, rsms = 0;
        if (RT) {
            const rl_route_rec q = routed_request(io, f, i, at, rsms);
            k = q.key; c = q.cfg; n = q.n; t = q.ts;
        } else {
            k = a.key[i];
            c = a.cfg[i];
            n = a.n[i];
            t = a.ts[i];
        }
        Out o;
        if (!(c < ncfg && n >= 0 && k != EMPTY_KEY)) {
            o.decision = DEC_INVALID; o.remaining = 0; o.retry = 0; o.reset_at = 0; o.tokens = 0.0;
        } else {
            const int64_t sms = RT ? rsms : a.sms ? a.sms[i] : floor_div(t, 1000000LL);
            const CfgDev C = cfgs[c];
            if (C.alg == ALG_TOKEN_BUCKET) {
                o = peek_tb(tb, tb_mask, k, t, n, sms, C, profile);
            } else {
                const uint32_t s = probe_find(win, win_mask, k);
                WinState w;
                w.key = k;
                w.nspill = 0;
                w.s[0] = w.s[1] = WinSlot{0, 0, ABSENT};
                if (s != NO_SLOT) {
                    const WinEntry e = win[s];   // the 64-byte entry, once
                    w.nspill = e.nspill;
                    w.s[0] = e.s[0];
                    w.s[1] = e.s[1];
                }
                o = C.alg == ALG_FIXED_WINDOW ? peek_fw(w, spill, t, n, sms, C, profile)
                                              : peek_sw(w, spill, t, n, sms, C, profile);
            }
        }
        if (RT) {
            routed_result(io, at, (int64_t)o.decision, o.remaining, o.retry, o.reset_at);
        } else {
            a.dec[i] = o.decision;
            a.rem[i] = o.remaining;
            a.retry[i] = o.retry;
            a.reset[i] = o.reset_at;
            if (a.tok) a.tok[i] = o.tokens;
        }
    }
}

__global__ __launch_bounds__(PEEK_BLOCK) void k_peek(uint64_t m, ReqArgs a, const CfgDev* __restrict__ cfgs,
                                                     uint32_t ncfg, const TbEntry* tb, uint64_t tb_mask,
                                                     const WinEntry* win, uint64_t win_mask, Spill spill,
                                                     int32_t profile) {
    peek_requests<false>(m, a, RoutedIo{}, cfgs, ncfg, tb, tb_mask, win, win_mask, spill, profile);
}

// The peek step of the routed path (rl_peek_routed_device): the grid is sized
// for m_max, min(ceil(m_max / PEEK_BLOCK), PEEK_GRID) blocks, since the host
// does not know the count.  Its one atomic is the atomicOr that reports a
// count above m_max; like k_peek it stores nothing to table memory.
__global__ __launch_bounds__(PEEK_BLOCK) void k_peek_routed(uint64_t m_max, RoutedIo io,
                                                            const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                            const TbEntry* tb, uint64_t tb_mask, const WinEntry* win,
                                                            uint64_t win_mask, Spill spill, int32_t profile) {
    peek_requests<true>(m_max, ReqArgs{}, io, cfgs, ncfg, tb, tb_mask, win, win_mask, spill, profile);
}

}  // namespace rl
