// rl_reset.h -- batched Reset (rl_reset_batch, include/rl_engine.h).
//
// A batch of m resets (key, ts, cfg) has the effect of m rl_reset calls in any
// order: DEL of the token-bucket key, of the fixed window's key of ts, of the
// sliding window's keys of ts and of the window before it -- wherever a window
// key lives (entry slot 0 / 1 or the spill table).
//
// One reset per thread in the caller's order, grid-stride.  The only store to
// table memory is `when = ABSENT` (the store k_reset and wk_delete make): no
// slot is compacted, nspill does not move, no key id is removed, so
//   * the store is idempotent: a duplicate of a reset finds the key deleted
//     (or deletes it a second time with the same word);
//   * deletes commute: a thread reads key ids, nspill, window starts and
//     `when` words, and another thread of the batch changes only `when` words
//     to ABSENT -- a window key that thread was about to delete itself, or one
//     of another window start, which this thread skips either way (wk_delete
//     matches on ws before it looks at `when`; spill_lookup counts an owned
//     entry toward nspill whether it is deleted or not).
// Hence duplicates in one batch and any thread order give one result, that of
// the m single resets.  No atomic, no spin; every loop is bounded by
// MAX_PROBES or the table mask (probe_find, spill_lookup).
#pragma once

#include "rl_routed.h"
#include "rl_table.h"
#include "rl_window.h"

namespace rl {

constexpr int RESET_BLOCK = 256;
// k_reset_batch's grid is min(ceil(m / RESET_BLOCK), RESET_GRID) blocks, as
// k_peek's: past RESET_GRID * RESET_BLOCK resets each thread strides on
constexpr int RESET_GRID = 1024;

// per-request status of a reset batch (RL_RESET_DONE / RL_INVALID, rl_engine.h)
constexpr uint8_t RESET_DONE = 1, RESET_INVALID = 3;

// Reset of one valid request: DEL of the key(s) AllowN would touch at *ts
// (tokenbucket.go:136-144, slidingwindow.go:125-139, fixedwindow.go:118-128).
// *ts is read only where a window start is needed.
__device__ inline void reset_one(uint64_t k, const int64_t* ts, const CfgDev& C, TbEntry* tb, uint64_t tb_mask,
                                 WinEntry* win, uint64_t win_mask, const Spill& spill) {
    if (C.alg == ALG_TOKEN_BUCKET) {
        const uint32_t s = probe_find(tb, tb_mask, k);
        if (s != NO_SLOT) tb[s].when = ABSENT;
        return;
    }
    const uint32_t s = probe_find(win, win_mask, k);
    if (s == NO_SLOT) return;
    const int64_t ws = window_start(*ts, C);
    wk_delete(&win[s], spill, ws);
    if (C.alg == ALG_SLIDING_WINDOW) wk_delete(&win[s], spill, ws - C.ttl_c);
}

// A key a later batch's grouping is inserting right now (k_probe's CAS,
// RL_OPT_PIPELINE) reads either as an empty slot or as a key whose entry holds
// the initial, absent state: nothing to delete in both cases, which is the key
// until that batch's replay runs, after this kernel.
//
// RT selects the input form only; the delete below it is the one text for
// both kernels.  RT = false (k_reset_batch): m resets as arrays in the caller's
// order, a status byte each.  RT = true (k_reset_routed): the merged batch of
// a routed step (rl_routed.h) -- at most m requests, the size in device
// memory; the record's n and its store clock are not used (a DEL has no
// expiry), and the status goes out as one rl_route_res {status, 0, 0, 0} at
// the receive index.
template <bool RT>
__device__ __forceinline__ void reset_requests(uint64_t m, const uint64_t* __restrict__ key,
                                               const int64_t* __restrict__ ts, const uint32_t* __restrict__ cfg,
                                               uint8_t* __restrict__ status, const RoutedIo& io,
                                               const CfgDev* __restrict__ cfgs, uint32_t ncfg, TbEntry* tb,
                                               uint64_t tb_mask, WinEntry* win, uint64_t win_mask,
                                               const Spill& spill) {
    RoutedForm f{};
    if (RT) {
        f = routed_open(m, io);
        m = f.m;
    }
    for (uint64_t i = blockIdx.x * (uint64_t)RESET_BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * RESET_BLOCK) {
        uint64_t k;
        uint32_t c, at = 0;
        int64_t t = 0;   // the arrays' ts[i] is read by reset_one, only where a window start is needed
        if (RT) {
            int64_t sms;   // not used: a DEL does not look at the clock
            const rl_route_rec q = routed_request(io, f, i, at, sms);
            k = q.key; c = q.cfg; t = q.ts;
        } else {
            k = key[i];
            c = cfg[i];
        }
        if (!(c < ncfg && k != EMPTY_KEY)) {
            if (RT) routed_result(io, at, RESET_INVALID, 0, 0, 0);
            else if (status) status[i] = RESET_INVALID;
            continue;
        }
        const CfgDev C = cfgs[c];
        reset_one(k, RT ? &t : &ts[i], C, tb, tb_mask, win, win_mask, spill);
        if (RT) routed_result(io, at, RESET_DONE, 0, 0, 0);
        else if (status) status[i] = RESET_DONE;
    }
}

__global__ __launch_bounds__(RESET_BLOCK) void k_reset_batch(uint64_t m, const uint64_t* __restrict__ key,
                                                             const int64_t* __restrict__ ts,
                                                             const uint32_t* __restrict__ cfg,
                                                             uint8_t* __restrict__ status,
                                                             const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                             TbEntry* tb, uint64_t tb_mask, WinEntry* win,
                                                             uint64_t win_mask, Spill spill) {
    reset_requests<false>(m, key, ts, cfg, status, RoutedIo{}, cfgs, ncfg, tb, tb_mask, win, win_mask, spill);
}

// The reset step of the routed path (rl_reset_routed_device): the grid is
// sized for m_max, min(ceil(m_max / RESET_BLOCK), RESET_GRID) blocks, since the
// host does not know the count.  Its one atomic is the atomicOr that reports a
// count above m_max; its one table store is `when = ABSENT`, as k_reset_batch's.
__global__ __launch_bounds__(RESET_BLOCK) void k_reset_routed(uint64_t m_max, RoutedIo io,
                                                              const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                              TbEntry* tb, uint64_t tb_mask, WinEntry* win,
                                                              uint64_t win_mask, Spill spill) {
    reset_requests<true>(m_max, nullptr, nullptr, nullptr, nullptr, io, cfgs, ncfg, tb, tb_mask, win, win_mask,
                         spill);
}

}  // namespace rl
