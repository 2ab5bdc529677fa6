// rl_routed.h -- the routed record form of a batch (include/rl_route.h) as the
// one-request-per-thread kernels read it: k_peek_routed (rl_peek.h),
// k_reset_routed (rl_reset.h), k_refund_add_routed (rl_refund.h),
// k_charge_ask_routed / k_charge_finish_routed (rl_charge.h), and the counting
// kernels k_tally_routed (rl_tally.h) and k_hot_add_routed / k_hot_pick_routed
// (rl_hot.h), which read a finished step through RoutedCount.
//
// The merge (rl_route_merge) leaves request p at rec[order[p]] with store
// clock sms[p], p < *count -- a size in device memory, so a kernel is launched
// for the caller's bound m_max and reads the actual size itself -- or, for one
// source in time order, only order[0] = RL_ORDER_IDENTITY and sms[0] = the
// store clock of the earlier steps: request p is then rec[p] and its clock
// max(sms[0], floor(ts / 1e6)).  k_probe<.., RT = true> (rl_engine.hip) takes
// the same two forms; routed_open / routed_request restate that reading once
// for the kernels here.  The result of request p is one 32-byte record at its
// receive index, the send layout of the result all-to-all.
#pragma once

#include <stdint.h>

#include "../../include/rl_route.h"
#include "rl_semantics.h"
#include "rl_table.h"

namespace rl {

struct RoutedIo {
    const rl_route_rec* rec;   // 16-byte aligned, as every device allocation is
    const uint32_t* order;
    const uint32_t* count;
    const int64_t* sms;
    rl_route_res* res;         // 16-byte aligned
    uint32_t* eflags;          // the engine's sticky flags (EF_ROUTED_OVER)
};

// what a kernel knows of the batch before its first request
struct RoutedForm {
    uint64_t m;       // requests to execute: min(m_max, *count)
    bool ident;       // received order is decision order
    int64_t clock0;   // ident: the store clock of the earlier steps
};

// Reads *count; a count above the caller's bound is reported by one thread
// (rl_engine_sync: RL_EOVERFLOW), the requests past the bound get no result.
// With no request (the warm-up passes null arrays and a zero count) nothing
// but *count is read.
__device__ inline RoutedForm routed_open(uint64_t m_max, const RoutedIo& io) {
    const uint32_t cnt = *io.count;
    if (cnt > m_max && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(io.eflags, EF_ROUTED_OVER);
    RoutedForm f;
    f.m = m_max < cnt ? m_max : cnt;
    f.ident = f.m && io.order[0] == RL_ORDER_IDENTITY;
    f.clock0 = f.ident ? io.sms[0] : 0;
    return f;
}

struct alignas(16) RoutedHalf {
    int64_t a, b;
};

// request p (p < f.m): its record as two 16-byte loads, its receive index
// and its store clock
__device__ inline rl_route_rec routed_request(const RoutedIo& io, const RoutedForm& f, uint64_t p, uint32_t& at,
                                              int64_t& sms) {
    at = f.ident ? (uint32_t)p : io.order[p];
    const RoutedHalf* q = reinterpret_cast<const RoutedHalf*>(io.rec + at);
    const RoutedHalf lo = q[0], hi = q[1];
    rl_route_rec r;
    r.key = (uint64_t)lo.a;
    r.ts = lo.b;
    r.n = hi.a;
    r.cfg = (uint32_t)((uint64_t)hi.b & 0xffffffffu);
    r.pos = (uint32_t)((uint64_t)hi.b >> 32);
    if (f.ident) {
        const int64_t ms = floor_div(r.ts, 1000000LL);
        sms = ms > f.clock0 ? ms : f.clock0;
    } else {
        sms = io.sms[p];
    }
    return r;
}

// A finished routed step as the counting kernels read it (k_tally_routed,
// rl_tally.h; k_hot_add_routed / k_hot_pick_routed, rl_hot.h): request p < f.m
// is (key, cfg, n) of its record and the decision of the result record at the
// same receive index -- the 16-byte half that holds it; the store clock and
// pos are not used.  The decision is an int64 here: a value outside 0..3,
// negative ones included, reads as the code 0xff, which no counting rule
// accepts.  The reader's call is that of the array forms' readers (TallyArrays,
// HotArrays), so the text after the read is one text.
struct RoutedCount {
    RoutedIo io;
    RoutedForm f;
    __device__ __forceinline__ void operator()(uint64_t p, bool, uint64_t& k, uint32_t& c, int64_t& n,
                                               uint32_t& d) const {
        uint32_t at;
        int64_t sms;
        const rl_route_rec r = routed_request(io, f, p, at, sms);
        const int64_t dec = reinterpret_cast<const RoutedHalf*>(io.res + at)[0].a;
        k = r.key;
        c = r.cfg;
        n = r.n;
        d = (uint64_t)dec <= 3u ? (uint32_t)dec : 0xffu;
    }
};

// the result record at receive index `at`, as two 16-byte stores
__device__ inline void routed_result(const RoutedIo& io, uint32_t at, int64_t decision, int64_t remaining,
                                     int64_t retry, int64_t reset_at) {
    RoutedHalf* q = reinterpret_cast<RoutedHalf*>(io.res + at);
    q[0] = RoutedHalf{decision, remaining};
    q[1] = RoutedHalf{retry, reset_at};
}

}  // namespace rl
