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
// No atomics, no spin-wait, no LDS, no inline assembly, no store to table
// memory; every loop is bounded by MAX_PROBES (probe_find) or m.
#pragma once

#include "rl_batch.h"
#include "rl_peek.h"
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

__global__ __launch_bounds__(CHARGE_BLOCK) void k_charge_ask(uint64_t m, const uint64_t* __restrict__ key,
                                                             const int64_t* __restrict__ ts,
                                                             const int64_t* __restrict__ n,
                                                             const uint32_t* __restrict__ cfg,
                                                             const int64_t* __restrict__ sms_in,
                                                             const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                             const TbEntry* tb, uint64_t tb_mask, int32_t profile,
                                                             ChargeScratch S) {
    for (uint64_t i = blockIdx.x * (uint64_t)CHARGE_BLOCK + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * CHARGE_BLOCK) {
        const uint64_t k = key[i];
        const uint32_t c = cfg[i];
        const int64_t want = n[i];
        int64_t take = 0, reset_at = 0;
        double tokens = 0.0;
        uint8_t kind = CHARGE_INVALID;
        if (c < ncfg && want > 0 && k != EMPTY_KEY) {
            const CfgDev C = cfgs[c];
            if (C.alg == ALG_TOKEN_BUCKET) {
                const int64_t t = ts[i];
                const int64_t sms = sms_in ? sms_in[i] : floor_div(t, 1000000LL);
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
        S.np[i] = take;
        S.kind[i] = kind;
        S.ask_reset[i] = reset_at;
        S.ask_tok[i] = tokens;
    }
}

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
        uint8_t dec = DEC_INVALID;
        int64_t got = 0, rem = 0, reset = 0;
        double tok = 0.0;
        if (kind == CHARGE_BUCKET && take == 0) {   // an empty bucket: nothing ran
            dec = DEC_DENIED;
            reset = S.ask_reset[i];
            tok = S.ask_tok[i];
        } else if (kind != CHARGE_INVALID) {
            const uint8_t d = S.dec[i];
            rem = S.rem[i];
            reset = S.reset[i];
            if (kind == CHARGE_BUCKET) {
                tok = S.tok[i];
                got = d == DEC_ALLOWED ? take : 0;
                dec = d >= DEC_ERROR ? d : (got == want ? DEC_ALLOWED : DEC_DENIED);
            } else {
                dec = d;
                got = d <= DEC_ALLOWED ? want : 0;
            }
        }
        decision[i] = dec;
        charged[i] = got;
        remaining[i] = rem;
        reset_at[i] = reset;
        if (tokens) tokens[i] = tok;
    }
}

}  // namespace rl
