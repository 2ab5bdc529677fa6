// rl_charge.h -- Charge: record usage that is only known after the fact
// (rl_charge_batch, include/rl_engine.h; the contract is DESIGN.md §10m).  The
// verb is a composition, as AllowAll is (rl_allow_all.h): k_charge_ask below
// turns every request's n into the amount n' that can be taken, the unchanged
// decide path runs on n' as one batch, and k_charge_finish turns the ask's and
// the decide's rows into one result row per request.  Nothing here touches a
// state table.
//
// k_charge_ask: one request per thread, grid-stride.  Read-only.
//   invalid (n <= 0, unknown cfg, EMPTY_KEY)   n' = 0, kind CHARGE_INVALID
//   token bucket   n' = min(n, r), r the `remaining` of Peek(key, 0) at the
//                  request's own clocks: peek_tb (rl_peek.h), the text k_peek
//                  runs, with requested = 0.  The row of that tb_step
//                  (reset_at, tokens) is kept for the empty bucket
//   window         n' = n: the scripts INCRBY before they compare
// k_charge_finish: one request per thread, grid-stride; the result rule.
//   bucket, n' >= 1   charged = n' if the decide allowed it, else 0; decision
//                     = ALLOWED if charged == n, DENIED if charged < n, or the
//                     decide's ERROR / INVALID; remaining, reset_at, tokens the
//                     decide's
//   bucket, n' = 0    DENIED, charged 0, remaining 0; reset_at, tokens the ask's
//   window            decision, remaining, reset_at the decide's; tokens 0;
//                     charged = n for ALLOWED or DENIED, else 0
//   invalid           INVALID, zeros
// k_charge_ask_routed / k_charge_finish_routed: the same two kernels over the
// merged batch of a routed step (rl_charge_routed_device, include/rl_route.h;
// DESIGN.md §10n), the same texts (charge_ask_request<RT>, charge_result).  The
// routed decide between them reads n from the records, and recv belongs to the
// pipeline, so the ask writes a normalised copy of the batch -- n = n',
// order2[p] = p, the resolved store clock -- into the engine's scratch
// (ChargeRouted), by merge position; the finish writes one result record
// {decision, remaining, charged, reset_at} per request at its receive index and
// {RL_DROPPED, 0, 0, 0} for the merged requests past the bound B.
// No atomics except, in the routed kernels, the one atomicOr on the sticky
// flags that routed_open does (a count above B); no spin-wait, no LDS, no
// inline assembly, no store to table memory; every loop is bounded by
// MAX_PROBES (probe_find), m, B or m_max; the routed kernels' trip counts are
// uniform over the block.
#pragma once

#include "rl_batch.h"
#include "rl_peek.h"
#include "rl_routed.h"
#include "rl_semantics.h"
#include "rl_table.h"

namespace rl {

constexpr int CHARGE_BLOCK = 256;
// the grid is min(ceil(m / CHARGE_BLOCK), CHARGE_GRID) blocks; a larger call
// strides.  As PEEK_GRID: the ask is a k_peek of token buckets.
constexpr int CHARGE_GRID = 1024;
// the largest call (rl_charge_max = min(max_batch, CHARGE_MAX)): the decide is
// one batch, and the scratch is sized for it
constexpr uint32_t CHARGE_MAX = 1u << 20;

enum : uint8_t { CHARGE_INVALID = 0, CHARGE_BUCKET = 1, CHARGE_WINDOW = 2 };

// The engine's Charge scratch, arrays of rl_charge_max elements in one
// allocation: the ask's outputs (np, kind and the empty bucket's row) and the
// decide's result row.
struct ChargeScratch {
    int64_t* np;          // n': the decide's n
    int64_t* ask_reset;   // token bucket: reset_at of the ask's tb_step
    double* ask_tok;      //               and its tokens
    int64_t *rem, *retry, *reset;   // the decide's row
    double* tok;
    uint8_t* dec;
    uint8_t* kind;        // CHARGE_INVALID / _BUCKET / _WINDOW
};

// The routed charge's scratch (rl_charge_routed_device), arrays of
// rl_charge_max elements in one allocation, indexed by merge position p -- a
// receive index can exceed the bound B.  rec2 / order2 / sms2 are the merged
// batch as the routed decide reads it, normalised: n = n', order2[p] = p (so
// order2[0] = 0 is never RL_ORDER_IDENTITY: both input forms become the
// general one) and the resolved store clock.  res2 is that decide's result;
// row and kind are the ask's.
struct ChargeRouted {
    rl_route_rec* rec2;   // 16-byte aligned
    rl_route_res* res2;   // 16-byte aligned
    RoutedHalf* row;      // {the original n, reset_at of the ask's tb_step}
    int64_t* sms2;
    uint32_t* order2;
    uint8_t* kind;        // CHARGE_INVALID / _BUCKET / _WINDOW
};

// The ask of request i: the text of k_charge_ask and k_charge_ask_routed.  RT
// selects where the request's fields come from and where the ask's row goes;
// validation, the bucket's peek_tb and the clamp are the one text between.
// RT = false: request i of the caller's arrays, a nullable store clock; the
// row goes to S.  RT = true: request i of the merged batch of a routed step
// (rl_routed.h, i < f.m), the merge's store clock; the row and the normalised
// request go to R at merge position i.
template <bool RT>
__device__ __forceinline__ void charge_ask_request(uint64_t i, const uint64_t* __restrict__ key,
                                                   const int64_t* __restrict__ ts, const int64_t* __restrict__ n,
                                                   const uint32_t* __restrict__ cfg,
                                                   const int64_t* __restrict__ sms_in, const RoutedIo& io,
                                                   const RoutedForm& f, const CfgDev* __restrict__ cfgs,
                                                   uint32_t ncfg, const TbEntry* tb, uint64_t tb_mask,
                                                   int32_t profile, const ChargeScratch& S, const ChargeRouted& R) {
    uint64_t k;
    uint32_t c, pos = 0;
    int64_t want, tq = 0, clock = 0;
    if (RT) {
        uint32_t at;
        const rl_route_rec q = routed_request(io, f, i, at, clock);
        k = q.key; c = q.cfg; want = q.n; tq = q.ts; pos = q.pos;
    } else {
        k = key[i];
        c = cfg[i];
        want = n[i];
    }
    int64_t take = 0, reset_at = 0;
    double tokens = 0.0;
    uint8_t kind = CHARGE_INVALID;
    if (c < ncfg && want > 0 && k != EMPTY_KEY) {
        const CfgDev C = cfgs[c];
        if (C.alg == ALG_TOKEN_BUCKET) {
            const int64_t t = RT ? tq : ts[i];
            const int64_t sms = RT ? clock : sms_in ? sms_in[i] : floor_div(t, 1000000LL);
            const Out o = peek_tb(tb, tb_mask, k, t, 0, sms, C, profile);
            kind = CHARGE_BUCKET;
            take = want < o.remaining ? want : o.remaining;
            take = take < 0 ? 0 : take;
            reset_at = o.reset_at;
            tokens = o.tokens;
        } else {
            kind = CHARGE_WINDOW;
            take = want;
        }
    }
    if (RT) {
        // the record with n = n', as two 16-byte stores; the decide reads it
        RoutedHalf* q2 = reinterpret_cast<RoutedHalf*>(R.rec2 + i);
        q2[0] = RoutedHalf{(int64_t)k, tq};
        q2[1] = RoutedHalf{take, (int64_t)((uint64_t)c | (uint64_t)pos << 32)};
        R.order2[i] = (uint32_t)i;
        R.sms2[i] = clock;
        R.row[i] = RoutedHalf{want, reset_at};
        R.kind[i] = kind;
    } else {
        S.np[i] = take;
        S.kind[i] = kind;
        S.ask_reset[i] = reset_at;
        S.ask_tok[i] = tokens;
    }
}

__global__ __launch_bounds__(CHARGE_BLOCK) void k_charge_ask(uint64_t m, const uint64_t* __restrict__ key,
                                                             const int64_t* __restrict__ ts,
                                                             const int64_t* __restrict__ n,
                                                             const uint32_t* __restrict__ cfg,
                                                             const int64_t* __restrict__ sms_in,
                                                             const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                             const TbEntry* tb, uint64_t tb_mask, int32_t profile,
                                                             ChargeScratch S) {
    for (uint64_t i = blockIdx.x * (uint64_t)CHARGE_BLOCK + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * CHARGE_BLOCK)
        charge_ask_request<false>(i, key, ts, n, cfg, sms_in, RoutedIo{}, RoutedForm{}, cfgs, ncfg, tb, tb_mask,
                                  profile, S, ChargeRouted{});
}

// The ask of a routed charge step (rl_charge_routed_device): the grid is sized
// for the bound B = min(m_max, rl_charge_max), min(ceil(B / CHARGE_BLOCK),
// CHARGE_GRID) blocks, since the host does not know the count; a count above B
// raises EF_ROUTED_OVER (routed_open's atomicOr, the kernel's one atomic).  It
// reads the merged batch and the token-bucket table and writes the scratch R
// only: `recv` belongs to the pipeline and is not rewritten.  The loop runs
// ceil(min(B, *count) / CHARGE_BLOCK) rounds of the grid: a trip count uniform
// over the block.
__global__ __launch_bounds__(CHARGE_BLOCK) void k_charge_ask_routed(uint64_t bound, RoutedIo io,
                                                                    const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                                    const TbEntry* tb, uint64_t tb_mask,
                                                                    int32_t profile, ChargeRouted R) {
    const RoutedForm f = routed_open(bound, io);
    for (uint64_t base = blockIdx.x * (uint64_t)CHARGE_BLOCK; base < f.m; base += (uint64_t)gridDim.x * CHARGE_BLOCK) {
        const uint64_t i = base + threadIdx.x;
        if (i < f.m)
            charge_ask_request<true>(i, nullptr, nullptr, nullptr, nullptr, nullptr, io, f, cfgs, ncfg, tb, tb_mask,
                                     profile, ChargeScratch{}, R);
    }
}

// The result rule (the table at the top) of one request: the text of
// k_charge_finish and k_charge_finish_routed.  `src` says where the ask's row
// and the decide's row are read; each is read only on the path that uses it.
template <class Src>
__device__ __forceinline__ void charge_result(uint8_t kind, int64_t want, int64_t take, const Src& src, uint8_t& dec,
                                              int64_t& got, int64_t& rem, int64_t& reset, double& tok) {
    dec = DEC_INVALID;
    got = 0; rem = 0; reset = 0;
    tok = 0.0;
    if (kind == CHARGE_BUCKET && take == 0) {   // an empty bucket: nothing ran
        dec = DEC_DENIED;
        reset = src.ask_reset();
        tok = src.ask_tok();
    } else if (kind != CHARGE_INVALID) {
        const uint8_t d = src.dec();
        rem = src.rem();
        reset = src.reset();
        if (kind == CHARGE_BUCKET) {
            tok = src.tok();
            got = d == DEC_ALLOWED ? take : 0;
            dec = d >= DEC_ERROR ? d : (got == want ? DEC_ALLOWED : DEC_DENIED);
        } else {
            dec = d;
            got = d <= DEC_ALLOWED ? want : 0;
        }
    }
}

// request i's rows in the array form's scratch
struct ChargeRowsAt {
    const ChargeScratch& S;
    uint64_t i;
    __device__ int64_t ask_reset() const { return S.ask_reset[i]; }
    __device__ double ask_tok() const { return S.ask_tok[i]; }
    __device__ uint8_t dec() const { return S.dec[i]; }
    __device__ int64_t rem() const { return S.rem[i]; }
    __device__ int64_t reset() const { return S.reset[i]; }
    __device__ double tok() const { return S.tok[i]; }
};

// the same of a routed step: the ask's reset_at came with `want` (R.row), the
// decide's row is the scratch result record at the merge position, read as two
// 16-byte loads; no tokens, as in every routed result
struct ChargeRowsRouted {
    const RoutedHalf* res2;   // the record of this request
    int64_t reset0;
    __device__ int64_t ask_reset() const { return reset0; }
    __device__ double ask_tok() const { return 0.0; }
    __device__ uint8_t dec() const { return (uint8_t)res2[0].a; }
    __device__ int64_t rem() const { return res2[0].b; }
    __device__ int64_t reset() const { return res2[1].b; }
    __device__ double tok() const { return 0.0; }
};

__global__ __launch_bounds__(CHARGE_BLOCK) void k_charge_finish(uint64_t m, const int64_t* __restrict__ n,
                                                                ChargeScratch S, uint8_t* __restrict__ decision,
                                                                int64_t* __restrict__ charged,
                                                                int64_t* __restrict__ remaining,
                                                                int64_t* __restrict__ reset_at,
                                                                double* __restrict__ tokens) {
    for (uint64_t i = blockIdx.x * (uint64_t)CHARGE_BLOCK + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * CHARGE_BLOCK) {
        const uint8_t kind = S.kind[i];
        const int64_t want = n[i], take = S.np[i];
        uint8_t dec;
        int64_t got, rem, reset;
        double tok;
        charge_result(kind, want, take, ChargeRowsAt{S, i}, dec, got, rem, reset, tok);
        decision[i] = dec;
        charged[i] = got;
        remaining[i] = rem;
        reset_at[i] = reset;
        if (tokens) tokens[i] = tok;
    }
}

// The finish of a routed charge step: for p < min(B, *count) the result rule
// on the ask's row and the decide's record res2[p], written as {decision,
// remaining, charged, reset_at} at the request's receive index -- `charged` in
// the retry_after field, where rl_route_unpack delivers it into the caller's
// retry array.  Then the merged requests past B, below the caller's bound:
// {RL_DROPPED, 0, 0, 0}, grid-stride, bounded by m_max.  It reads `order` and
// the scratch and writes `res` only; routed_open's atomicOr is its one atomic
// (the flag the ask raised already).  Both loops have a trip count uniform
// over the block.
__global__ __launch_bounds__(CHARGE_BLOCK) void k_charge_finish_routed(uint64_t bound, uint64_t m_max, RoutedIo io,
                                                                       ChargeRouted R) {
    const RoutedForm f = routed_open(bound, io);
    const uint64_t stride = (uint64_t)gridDim.x * CHARGE_BLOCK;
    for (uint64_t base = blockIdx.x * (uint64_t)CHARGE_BLOCK; base < f.m; base += stride) {
        const uint64_t p = base + threadIdx.x;
        if (p < f.m) {
            const uint8_t kind = R.kind[p];
            const RoutedHalf row = R.row[p];
            const int64_t take = reinterpret_cast<const RoutedHalf*>(R.rec2 + p)[1].a;
            uint8_t dec;
            int64_t got, rem, reset;
            double tok;
            charge_result(kind, row.a, take, ChargeRowsRouted{reinterpret_cast<const RoutedHalf*>(R.res2 + p), row.b},
                          dec, got, rem, reset, tok);
            routed_result(io, f.ident ? (uint32_t)p : io.order[p], (int64_t)dec, rem, got, reset);
        }
    }
    const uint64_t cnt = *io.count;
    const uint64_t end = cnt < m_max ? cnt : m_max;
    for (uint64_t base = bound + blockIdx.x * (uint64_t)CHARGE_BLOCK; base < end; base += stride) {
        const uint64_t p = base + threadIdx.x;
        if (p < end) routed_result(io, f.ident ? (uint32_t)p : io.order[p], RL_DROPPED, 0, 0, 0);
    }
}

}  // namespace rl
