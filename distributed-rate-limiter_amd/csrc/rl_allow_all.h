// rl_allow_all.h -- AllowAll: one request checked against several limiters,
// all or nothing (rl_allow_all_batch, include/rl_engine.h; the contract is
// DESIGN.md §10k).  The verb is a composition: the decide path runs on the
// members as one batch, k_allow_all_settle below turns the members' decisions
// into one verdict per group and a give-back amount per member, and the refund
// kernels (rl_refund.h) give those amounts back.  Nothing here touches a state
// table.
//
// Groups: member i starts a group when i == 0 or first[i] != 0; a group is a
// maximal run of members, so every byte array is a grouping.  A run of more
// than ALLOW_ALL_MAX_GROUP members is a group whose verdict is DEC_INVALID.
//
// k_allow_all_settle: one member per thread, grid-stride.  Thread i scans back
// at most ALLOW_ALL_MAX_GROUP members for its group's head and from the head
// forward at most ALLOW_ALL_MAX_GROUP members for the end.  In a run of L > 16
// members a member 16 or more past the head finds no head, and one nearer finds
// the head and then no end within 16: every member of the run reaches "too
// long", so the verdict is uniform.  Otherwise the verdict is the most severe
// decision of the span, INVALID > ERROR > DENIED > ALLOWED, and
//   g[i] = n[i]  if the verdict is not ALLOWED and the member took something:
//                a token bucket took when it allowed; a window counter took
//                when it allowed or denied (the script's INCRBY ran either way)
//   g[i] = 0     otherwise (an ERROR or INVALID member stored nothing)
// No atomics, no spin-wait, no LDS, no inline assembly; every loop is bounded
// by ALLOW_ALL_MAX_GROUP or m.  It reads first, cfg, n, decision and the config
// table, and writes verdict and g.
//
// k_allow_all_settle_routed: the same text (allow_all_settle_members<RT>) for
// the sender of a routed AllowAll, with RL_DROPPED in the severity order and a
// selection byte per member; see there.
#pragma once

#include "rl_semantics.h"

namespace rl {

constexpr int ALLOW_ALL_BLOCK = 256;
// the grid is min(ceil(m / ALLOW_ALL_BLOCK), ALLOW_ALL_GRID) blocks; a larger
// call strides
constexpr int ALLOW_ALL_GRID = 1024;
// the largest group (RL_ALLOW_ALL_MAX_GROUP): a stated cap that bounds the
// per-thread scans, not a measured value
constexpr uint32_t ALLOW_ALL_MAX_GROUP = 16;

// severity of a decision code: ALLOWED 0 < DENIED 1 < ERROR 2 < INVALID 3.  The
// map swaps 0 and 1 and is its own inverse; a byte above 3 counts as INVALID
RL_HD inline uint32_t allow_all_severity(uint32_t d) { return d < 2u ? 1u - d : (d < 3u ? d : 3u); }

// The routed settle (rl_allow_all_settle_device, include/rl_route.h; DESIGN.md
// §10l) reads the unpacked results of a routed decide step, where a member may
// be DROPPED (4): never executed, its owner's bucket was full.  Severity there:
// ALLOWED 0 < DENIED 1 < ERROR 2 < DROPPED 3 < INVALID 4 -- a dropped group is
// to be resubmitted whole, an invalid one can never pass; a byte of 5 or more
// counts as INVALID.  The map swaps 0 and 1 and swaps 3 and 4, so it too is
// its own inverse.
RL_HD inline uint32_t allow_all_severity_routed(uint32_t d) {
    return d < 2u ? 1u - d : (d == 2u ? 2u : (d == 4u ? 3u : 4u));
}

// The one text of both settle kernels.  RT = false: §10k's settle.  RT = true:
// the routed severity order, and sel[i] = g[i] > 0 beside g (the selection
// rl_route_pack_sel sends).  A dropped member took nothing: the give-back rule
// needs no case for it.
template <bool RT>
__device__ __forceinline__ void allow_all_settle_members(uint64_t m, const uint8_t* __restrict__ first,
                                                         const uint32_t* __restrict__ cfg,
                                                         const int64_t* __restrict__ n,
                                                         const uint8_t* __restrict__ decision,
                                                         const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                         uint8_t* __restrict__ verdict, int64_t* __restrict__ g,
                                                         uint8_t* __restrict__ sel) {
    for (uint64_t i = blockIdx.x * (uint64_t)ALLOW_ALL_BLOCK + threadIdx.x; i < m;
         i += (uint64_t)gridDim.x * ALLOW_ALL_BLOCK) {
        // the head: the nearest member at or before i that starts a group
        uint64_t head = i;
        bool found = false;
        for (uint32_t d = 0; d < ALLOW_ALL_MAX_GROUP; d++) {
            head = i - d;
            if (head == 0 || first[head] != 0) { found = true; break; }
        }
        // the end (exclusive): the next head, or m
        uint64_t end = head;
        if (found) {
            found = false;
            for (uint32_t d = 1; d <= ALLOW_ALL_MAX_GROUP; d++) {
                end = head + d;
                if (end >= m || first[end] != 0) { found = true; break; }
            }
        }
        uint32_t sev = RT ? 4 : 3;   // a run too long: INVALID
        if (found) {
            sev = 0;
            for (uint64_t j = head; j < end; j++) {   // at most ALLOW_ALL_MAX_GROUP members
                const uint32_t s = RT ? allow_all_severity_routed(decision[j]) : allow_all_severity(decision[j]);
                sev = s > sev ? s : sev;
            }
        }
        const uint8_t v = (uint8_t)(RT ? allow_all_severity_routed(sev) : allow_all_severity(sev));
        const uint8_t dec = decision[i];
        const uint32_t c = cfg[i];
        int64_t back = 0;
        if (v != DEC_ALLOWED && c < ncfg) {
            const bool took =
                cfgs[c].alg == ALG_TOKEN_BUCKET ? dec == DEC_ALLOWED : (dec == DEC_ALLOWED || dec == DEC_DENIED);
            if (took) back = n[i];
        }
        verdict[i] = v;
        g[i] = back;
        if (RT) sel[i] = back > 0;
    }
}

__global__ __launch_bounds__(ALLOW_ALL_BLOCK) void k_allow_all_settle(uint64_t m, const uint8_t* __restrict__ first,
                                                                      const uint32_t* __restrict__ cfg,
                                                                      const int64_t* __restrict__ n,
                                                                      const uint8_t* __restrict__ decision,
                                                                      const CfgDev* __restrict__ cfgs, uint32_t ncfg,
                                                                      uint8_t* __restrict__ verdict,
                                                                      int64_t* __restrict__ g) {
    allow_all_settle_members<false>(m, first, cfg, n, decision, cfgs, ncfg, verdict, g, nullptr);
}

// the sender's settle of a routed AllowAll: decisions may be DROPPED; writes
// the selection too
__global__ __launch_bounds__(ALLOW_ALL_BLOCK) void k_allow_all_settle_routed(
    uint64_t m, const uint8_t* __restrict__ first, const uint32_t* __restrict__ cfg, const int64_t* __restrict__ n,
    const uint8_t* __restrict__ decision, const CfgDev* __restrict__ cfgs, uint32_t ncfg,
    uint8_t* __restrict__ verdict, int64_t* __restrict__ g, uint8_t* __restrict__ sel) {
    allow_all_settle_members<true>(m, first, cfg, n, decision, cfgs, ncfg, verdict, g, sel);
}

}  // namespace rl
