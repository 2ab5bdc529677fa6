// rl_replay.h -- per-key segment replay kernels.
//
// After the sort, the requests of one state-table slot (one user key) form a
// contiguous segment in arrival order.  Replaying a segment applies, request
// by request, exactly what the reference does per call: the Go pre-arithmetic,
// the Lua script against the key's Redis state, and the Go post-arithmetic
// (rl_semantics.h).  State is gathered from the table once per segment, kept in
// registers across the segment, and scattered back once.
//
// Here: the light segments' serial replays (one thread each), the phases
// after the chain (replay_rest) and the kernels: k_tb_chain, k_replay_light
// and the expansion of the chain's committed runs (k_tb_expand,
// k_tb_expand_x).  rl_tb_chain.h has the map of the decision path's headers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_replay_wave.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_tb_chain.h"
#include "rl_tb_stamps.h"
#include "rl_tb_step.h"
#include "rl_tb_window.h"
#include "rl_tb_xdec.h"
#include "rl_window.h"

namespace rl {

// configs cached in LDS per block (when the engine has at most MAX_LCFG)
constexpr int MAX_LCFG = 32;

// fresh: the batch inserted the key (its entry holds the absent state, not read)
__device__ inline void replay_tb_serial(TbEntry* e, uint32_t j0, uint32_t j1, const CfgDev* cfgs,
                                        int32_t profile, const ReqArgs& a, const TbPre& pre, bool fresh = false) {
    double tok = fresh ? 0.0 : e->tok;
    const double add0 = fresh ? __builtin_nan("") : tb_head_add(e, j0, cfgs, profile, a);
    for (uint32_t j = j0; j < j1; j++) {
        const double add = j == j0 ? add0 : pre.add[j];
        const bool alive = add == add;
        Out o = tb_chain_step(tok, alive, alive ? add : 0.0, a.n[j], 0, cfgs[a.cfg[j]], profile);
        write_out_tb(a, j, o.decision, o.tokens);
    }
    tb_store_end(e, tok, j1 - 1, cfgs, profile, a);
}

// fresh: one request on a key the batch inserted -- the absent state, not
// read (one request on two free slots never reaches the spill, which alone
// needs the key)
__device__ inline void replay_win_serial(WinEntry* e, const Spill& S, uint32_t j0, uint32_t j1,
                                         const CfgDev* cfgs, int32_t profile, const ReqArgs& a, uint32_t* eflags,
                                         bool fresh = false) {
    WinState w;
    if (fresh) {
        w.key = EMPTY_KEY;
        w.nspill = 0;
        for (int k = 0; k < 2; k++) w.s[k] = WinSlot{0, 0, ABSENT};
    } else {
        w = win_load(e);
    }
    uint32_t ef = 0;
    replay_win_steps(w, S, j0, j1, cfgs, profile, a, ef);
    win_store(e, w);
    if (ef) atomicOr(eflags, ef);
}

// Outputs of the multi-decade windows' runs (the chain lists them): one wave
// per run, exact_span_x with outputs from the run's exact start, checked
// against the end state the chain resolved.  A kernel of its own: inside
// k_tb_expand its registers halved that kernel's occupancy, which every
// batch's scan of the run starts pays for (mixed: 21 -> 38 us per batch,
// profiles/r5_xdec_ab.txt).
__global__ __launch_bounds__(256) void k_tb_expand_x(TbRuns runs, ReqArgs a, TbPre pre, uint32_t* eflags) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = (gridDim.x * blockDim.x) >> 6;
    const uint32_t n = *runs.xcnt;
    uint32_t iters = 0;
    for (uint32_t i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; i < n; i += nw) {
        const uint32_t p = runs.xlist[i];
        const uint32_t len = runs.len[p];
        const int32_t F = runs.E[p] - XRUN;
        const int64_t D0 = runs.D0[p], D1 = runs.D1[p];
        const XScale xs = xscale(F);
        int64_t Dend = 0;
        const uint32_t brk = exact_span_x<true>(GlobSrc{pre.add, pre.th}, p, len, D0, xs, Dend, a, iters);
        if (lane == 0) {
            if (brk != len || Dend != D1) atomicOr(eflags, EF_INTERNAL);
            runs.len[p] = 0;
        }
    }
}

// Outputs of the committed runs: one wave per run, exact_span with outputs
// from the run's exact start state, checked against the state the chain
// resolved at the run's end.  Waves scan the batch in CH_TILE-position blocks and
// expand the runs that start in their block.
__global__ __launch_bounds__(256) void k_tb_expand(uint32_t m, TbRuns runs, int32_t profile, ReqArgs a, TbPre pre,
                                                   uint32_t* eflags) {
    constexpr int K = CH_K;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nw = (gridDim.x * blockDim.x) >> 6;
    uint32_t iters = 0;
    for (uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; b * CH_TILE < m; b += nw) {
        uint32_t mask = 0;
#pragma unroll
        for (int q = 0; q < K; q++) {
            const uint32_t p = b * CH_TILE + lane * K + q;
            if (p < m && runs.len[p]) mask |= 1u << q;
        }
        for (;;) {
            const uint64_t any = __ballot(mask != 0);
            if (!any) break;
            const uint32_t L = first_lane(any);
            const uint32_t qm = (uint32_t)__builtin_amdgcn_readlane((int)mask, (int)L);
            const uint32_t p = b * CH_TILE + L * K + (uint32_t)__builtin_ctz(qm);
            if (lane == L) mask &= mask - 1u;
            const uint32_t len = runs.len[p];
            const int32_t E = runs.E[p];
            const int64_t D0 = runs.D0[p], D1 = runs.D1[p];
            int64_t Dend = 0;
            uint32_t brk;
            double P, R;
            if (profile == PROFILE_REDIS7 && E >= XRUN - 100) {     // a multi-decade window's: k_tb_expand_x
                continue;
            } else if (profile == PROFILE_REDIS7) {
                mode_scale(QM_DEC, E, P, R);
                brk = exact_span<QM_DEC, true>(GlobSrc{pre.add, pre.th}, p, len, D0, 0, P, R, Dend, a, iters);
            } else {
                mode_scale(QM_BIN, E, P, R);
                brk = exact_span<QM_BIN, true>(GlobSrc{pre.add, pre.th}, p, len, D0, 0, P, R, Dend, a, iters);
            }
            if (lane == 0) {
                if (brk != len || Dend != D1) atomicOr(eflags, EF_INTERNAL);
                runs.len[p] = 0;
            }
        }
    }
}

// Phases 2 and 3 of the replay kernels: heavy token-bucket segments
// (wave_segment) and heavy window segments (wave_win_segment), one per wave,
// then light segments of any algorithm, one per thread, serial
// (replay_*_serial).  nhx: huge token-bucket segments taken here as heavy
// ones, ahead of them (k_replay_light; the chain kernel's phase 1 takes them
// otherwise).  s_u: a __shared__ word of the calling kernel.
__device__ __attribute__((always_inline)) inline void replay_rest(const uint32_t* __restrict__ sk, const SegLists& L,
                                                                 uint32_t* qctr, uint32_t win_base, TbEntry* tb,
                                                                 WinEntry* win, const Spill& spill,
                                                                 const CfgDev* __restrict__ cfgs, int32_t profile,
                                                                 const ReqArgs& a, const TbPre& pre, uint32_t* eflags,
                                                                 uint32_t* dbg, uint32_t& s_u, uint32_t nhx) {
    const uint32_t nheavy = L.count[0], nlight = L.count[1], nwin = L.count[2];
    {
        // heavy segments, HEAVY_G per claim: every wave's claim is an atomic on
        // ONE counter, which sustains only ~88 atomics/us -- with one segment
        // per claim, ten thousand short heavy segments (configs[0]'s keys)
        // spent longer queueing on the counter than replaying
        uint32_t iters = 0;
        ReplayStamps stamps;
        const uint32_t nhw = nhx + nheavy + nwin;
        for (;;) {
            uint32_t u0 = 0;
            if ((threadIdx.x & 63) == 0) u0 = atomicAdd(&qctr[2], (uint32_t)HEAVY_G);
            u0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)u0);
            if (u0 >= nhw) break;
            const uint32_t u1 = min(u0 + (uint32_t)HEAVY_G, nhw);
            for (uint32_t u = u0; u < u1; u++) {
                if (u < nhx + nheavy) {
                    const SegRec sg = u < nhx ? L.list[3][u] : L.list[0][u - nhx];
                    stamps.heavy_begin();
                    wave_segment(&tb[sk[sg.j0]], sg.j0, sg.j0 + sg.len, cfgs, profile, a, pre, eflags, iters);
                    stamps.heavy_end(dbg, sg.len);
                } else {
                    const SegRec sg = L.list[2][u - nhx - nheavy];
                    wave_win_segment(&win[sk[sg.j0] - win_base], spill, sg.j0, sg.j0 + sg.len, cfgs, profile, a,
                                     eflags);
                }
            }
        }
    }
    __syncthreads();
    const uint64_t t_light = __builtin_amdgcn_s_memrealtime();
    ReplayStamps::heavy_phase_end(dbg, t_light);
    for (;;) {
        if (threadIdx.x == 0) s_u = atomicAdd(&qctr[1], (uint32_t)blockDim.x);
        __syncthreads();
        const uint32_t u0 = s_u;
        __syncthreads();
        if (u0 >= nlight) break;
        ReplayStamps::light_claim(dbg);
        const uint32_t u = u0 + threadIdx.x;
        if (u < nlight) {
            const SegRec sg = L.list[1][u];
            const uint32_t k0 = sk[sg.j0];
            // a key the batch inserted, alone in it: the absent state, unread
            const bool fresh = sg.len == 1u && a.fresh && a.fresh[sg.j0];
            if (k0 < win_base) replay_tb_serial(&tb[k0], sg.j0, sg.j0 + sg.len, cfgs, profile, a, pre, fresh);
            else replay_win_serial(&win[k0 - win_base], spill, sg.j0, sg.j0 + sg.len, cfgs, profile, a, eflags, fresh);
        }
    }
    if (threadIdx.x == 0 && dbg) {
        atomicMax(&dbg[DBG_LIGHT_TICKS_MAX], (uint32_t)(__builtin_amdgcn_s_memrealtime() - t_light));
        atomicMax(&dbg[DBG_T_LAST_END], (uint32_t)__builtin_amdgcn_s_memrealtime());
    }
}

// blocks past grid_base join only a batch with a long light phase (many
// distinct keys: every one a serial replay), or with many heavy segments
// (configs[0]'s 10k keys of ~100 requests, one per wave; light_min / 32 =
// m / 128 of them); otherwise they would only take CUs from the next batch's
// grouping, which then bounds the step
__device__ inline bool replay_joins(const SegLists& L, uint32_t grid_base, uint32_t light_min) {
    return blockIdx.x < grid_base || L.count[1] >= light_min || L.count[0] + L.count[2] >= light_min / 32u;
}

// The replay kernel.  Phase 1: huge token-bucket segments, one per block (the
// chain), longest first; then replay_rest.  The hot keys' blocks stay in
// phase 1 while the others drain phases 2-3.  h_huge: a host-mapped word, the
// batch's count of huge segments (the host launches k_replay_light when the
// last replay it saw had none).
template <bool LCFG>
__global__ __launch_bounds__(CH_BLOCK) void k_tb_chain(const uint32_t* __restrict__ sk, SegLists L, uint32_t* qctr,
                                                       uint32_t win_base, TbEntry* tb, WinEntry* win, Spill spill,
                                                       const CfgDev* __restrict__ gcfgs, uint32_t ncfg,
                                                       int32_t profile, ReqArgs a, TbPre pre, uint32_t* eflags,
                                                       uint32_t* dbg, TbRuns runs, uint32_t grid_base,
                                                       uint32_t light_min, uint32_t* h_huge) {
    __shared__ ChainShared sh;
    __shared__ uint32_t s_u;
    __shared__ CfgDev s_cfg[LCFG ? MAX_LCFG : 1];
    if (LCFG) {
        for (uint32_t c = threadIdx.x; c < ncfg; c += blockDim.x) s_cfg[c] = gcfgs[c];
        __syncthreads();
    }
    const CfgDev* cfgs = LCFG ? s_cfg : gcfgs;
    const uint32_t nhuge = L.count[3];
    if (blockIdx.x == 0 && threadIdx.x == 0 && h_huge) *(volatile uint32_t*)h_huge = nhuge;
    if (!replay_joins(L, grid_base, light_min)) return;
    if (threadIdx.x < 2u * CH_NP) (&sh.plan_tag[0][0])[threadIdx.x] = 0u;   // (the claim loop's barrier follows)
    uint32_t plan_seq = 0;   // ch_plan_par numbers (the same in every producer wave)
    // timeline (10 ns ticks, low 32 bits): the first block's start (complemented),
    // the last block's end, the longest segment's start and end
    if (threadIdx.x == 0 && dbg) atomicMax(&dbg[DBG_T_FIRST_START_INV], ~(uint32_t)__builtin_amdgcn_s_memrealtime());
    ReplayStamps::block_start(dbg);
    for (;;) {
        // claim the longest unclaimed huge segment (their list is short:
        // batch / 4096 at most), so the hottest key starts with the first
        // block.  The block reads the whole list at once (one entry per
        // thread, an argmax over the waves): one memory round trip, not one
        // per entry before the hot key's chain can start
        if (threadIdx.x == 0) s_u = atomicAdd(&qctr[0], 1u) < nhuge ? 0u : NO_STOP;
        __syncthreads();
        if (s_u == 0u) {
            __shared__ uint64_t s_best[CH_BLOCK / 64];
            for (;;) {
                uint64_t best = 0;   // (len << 32) | (~k): the longest, ties to the lowest k
                for (uint32_t k = threadIdx.x; k < nhuge; k += blockDim.x) {
                    const uint32_t len = L.list[3][k].len;
                    if (__hip_atomic_load(&L.claim[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
                        const uint64_t c = ((uint64_t)len << 32) | (uint32_t)~k;
                        best = c > best ? c : best;
                    }
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const uint64_t o = __shfl_xor(best, off);
                    best = o > best ? o : best;
                }
                if ((threadIdx.x & 63) == 0) s_best[threadIdx.x >> 6] = best;
                __syncthreads();
                if (threadIdx.x == 0) {
                    uint64_t b = 0;
                    for (int w = 0; w < CH_BLOCK / 64; w++) b = s_best[w] > b ? s_best[w] : b;
                    const uint32_t k = ~(uint32_t)b;
                    s_u = b == 0 ? NO_STOP : (atomicCAS(&L.claim[k], 0u, 1u) == 0u ? k : NO_STOP - 1u);
                }
                __syncthreads();
                if (s_u != NO_STOP - 1u) break;   // claimed one, or none is left; else another block won it: again
                __syncthreads();
            }
        }
        __syncthreads();
        const uint32_t u = s_u;
        __syncthreads();
        if (u == NO_STOP) break;
        const SegRec sg = L.list[3][u];
        const uint64_t t_seg = __builtin_amdgcn_s_memrealtime();
        ch_segment<LCFG>(sh, &tb[sk[sg.j0]], sg.j0, sg.j0 + sg.len, cfgs, profile, a, pre, eflags, dbg, runs,
                         plan_seq);
        __syncthreads();
        if (threadIdx.x == 0 && dbg) {
            const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
            if (atomicMax(&dbg[DBG_SEG_TICKS_MAX], (uint32_t)(t_end - t_seg)) < (uint32_t)(t_end - t_seg)) {
                dbg[DBG_T_SEG_START] = (uint32_t)t_seg;
                dbg[DBG_T_SEG_END] = (uint32_t)t_end;
            }
        }
    }
    replay_rest(sk, L, qctr, win_base, tb, win, spill, cfgs, profile, a, pre, eflags, dbg, s_u, 0u);
}

// The replay kernel of a batch with no huge segment expected (the last
// replay the host saw had none: mixed, uniform and bursty traffic): phases 2-3
// only, in blocks of LT_BLOCK threads -- without the chain's 156 KB of LDS and
// its register budget, a CU holds 12 replay waves instead of 8.  A huge
// segment that arrives anyway is replayed as a heavy one (wave_segment:
// exact, one wave), and the host word makes the next batches take the chain
// kernel again.
#ifndef RL_LT_BLOCK
#define RL_LT_BLOCK 768
#endif
constexpr int LT_BLOCK = RL_LT_BLOCK;
template <bool LCFG>
__global__ __launch_bounds__(LT_BLOCK) void k_replay_light(const uint32_t* __restrict__ sk, SegLists L, uint32_t* qctr,
                                                           uint32_t win_base, TbEntry* tb, WinEntry* win, Spill spill,
                                                           const CfgDev* __restrict__ gcfgs, uint32_t ncfg,
                                                           int32_t profile, ReqArgs a, TbPre pre, uint32_t* eflags,
                                                           uint32_t* dbg, TbRuns runs, uint32_t grid_base,
                                                           uint32_t light_min, uint32_t* h_huge) {
    __shared__ uint32_t s_u;
    __shared__ CfgDev s_cfg[LCFG ? MAX_LCFG : 1];
    if (LCFG) {
        for (uint32_t c = threadIdx.x; c < ncfg; c += blockDim.x) s_cfg[c] = gcfgs[c];
        __syncthreads();
    }
    (void)runs;
    const CfgDev* cfgs = LCFG ? s_cfg : gcfgs;
    const uint32_t nhuge = L.count[3];
    if (blockIdx.x == 0 && threadIdx.x == 0 && h_huge) *(volatile uint32_t*)h_huge = nhuge;
    if (!replay_joins(L, grid_base, light_min)) return;
    if (threadIdx.x == 0 && dbg) atomicMax(&dbg[DBG_T_FIRST_START_INV], ~(uint32_t)__builtin_amdgcn_s_memrealtime());
    replay_rest(sk, L, qctr, win_base, tb, win, spill, cfgs, profile, a, pre, eflags, dbg, s_u, nhuge);
}

}  // namespace rl
