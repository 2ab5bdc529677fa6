// rl_tb_chain.h -- pipelined token-bucket replay of heavy (Zipf hot-key)
// segments: the chain itself (the block-wide replay of one huge segment).
//
// What is replayed: the reference's token-bucket script step
// (tokenbucket.go:23-52 + the Go arithmetic at :114-130), request by request
// in arrival order, on one key.  The carried state is the STORED tokens value,
// which Lua's tostring quantizes (tokenbucket.go:48): under Redis 7 to 14
// significant decimal digits, i.e. an integer D in [1e13, 1e14) in a decade E
// (value = D * 10^(E-13)); under miniredis to the exact double, an integer
// mantissa D in [2^52, 2^53) in a binade E.
//
// Step algebra (u = the unit of D, P = 1/u).  With T = strtod(D*u) and
// sum = RN(T + add), the next stored state is D' = round(sum * P) =
// round(D + add*P + delta) with |delta| <= (D + D') * 2^-53 < 0.0223 (two
// correct roundings of values below 1e14 u).  D is an integer, so whenever
// add*P is farther than TAU_DEC (0.03) from a half-integer (a "far" step),
// D' = D + r with r = rint(add*P) for EVERY predecessor D in the decade: the
// step is an integer add, independent of the state.  Only "near" steps
// (about 6% of them) depend on the exact predecessor.  A step leaves this
// regime when it allows (tokens >= n), clamps (sum >= capacity), leaves the
// decade, or finds the key expired; regime exits are rare for a hot key.
//
// One block replays one segment with three wave roles, in lock-step rounds
// separated by one LDS barrier:
//   producers (CH_NP waves)  summarize the NEXT window of CH_W requests at the
//       current decade: per tile (64 lanes x CH_K requests) the nominal sum of r, bounds of
//       the nominal prefix (decade exit), of the allow/clamp slack, the first
//       expired/huge step, and the tile's near steps compacted into an LDS
//       list -- all state-free, so they run one window ahead of the chain;
//   chain (wave 0)  resolves the window the producers summarized in the
//       previous round: near steps by a wave-wide fixed point on their exact
//       predecessors (64 at a time), then tile by tile either commits the tile
//       as a run {start, length, exact start state, exact end state} or, when
//       the bounds say the tile may leave the regime, replays it exactly
//       (exact_span) to find the first regime exit, which it executes exactly
//       (tb_eval) together with any further out-of-regime steps (serial loop);
//   loader (1 wave)  streams the segment's precomputed inputs (add, th) from
//       HBM into an LDS ring by LDS-DMA, two windows ahead.
// If the chain window ends early (regime exit), the producers' speculative
// window is discarded and the next round re-produces from the exit.
//
// k_tb_expand then replays every committed run exactly and in parallel over
// the whole GPU (one wave per run, exact_span with outputs) and checks that
// each run ends in the state the chain recorded (EF_INTERNAL otherwise).  So
// every result still comes from an exact step on its exact predecessor; the
// bounds above only decide WHERE the chain looks, never a result.
//
// Where the decision path lives (every header includes what it uses):
//   rl_wave.h         DPP scans and reductions, lane reads, the LDS barrier
//   rl_tb_step.h      one script step: TbPre, tb_quant / tb_eval, the exact
//                     fast-mode step (tb_step_d, div_p10), tb_dec_step
//   rl_tb_window.h    the chain's constants and LDS state, the ring and its
//                     loader, exact_span, the producers, the exit guess
//   rl_tb_xdec.h      multi-decade windows: xstep, exact_span_x, the window
//                     plan, their producers
//   rl_tb_serial.h    the serial step loop (serial_steps)
//   rl_tb_stamps.h    the names of the debug words; the diagnostic stamps
//   rl_tb_chain.h     this file: ch_resolve, the out-of-line multi-decade
//                     wrappers, ch_segment (the rounds of the three roles)
//   rl_replay_wave.h  the one-wave segments: wave_segment, wave_win_segment
//   rl_replay.h       the light serial replays, replay_rest, the kernels
//                     k_tb_chain, k_replay_light, k_tb_expand, k_tb_expand_x
//   rl_group.h        grouping and finish: k_segments, k_sort_local,
//                     k_permute, k_unpermute*
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_tb_serial.h"
#include "rl_tb_stamps.h"
#include "rl_tb_step.h"
#include "rl_tb_window.h"
#include "rl_tb_xdec.h"
#include "rl_wave.h"

namespace rl {

// ---------------------------------------------------------------------------
// chain
// ---------------------------------------------------------------------------
enum : uint32_t { CH_FULL = 0, CH_STOP = 1, CH_PARTIAL = 2 };

struct ChOutcome {
    uint32_t kind;
    uint32_t q;        // FULL: window end; STOP: the exiting step; PARTIAL: end of the committed part
    int64_t D;         // exact stored digits before position q
    uint32_t iters;    // ch_resolve_x: the caller's pass count after the call
};

// Resolve the chain window of state s (its tiles are in tile[s.cbuf]).
template <int MODE>
__device__ __attribute__((always_inline)) inline ChOutcome ch_resolve(ChainShared& sh, const ChState& s, double P,
                                                                     double R, const XScale& xs, const ReqArgs& a,
                                                                     const TbRuns& runs, uint32_t* eflags,
                                                                     uint32_t& iters, uint32_t* dbg) {
    const uint32_t lane = threadIdx.x & 63;
    ChResolveStamps stamps;
    stamps.begin(iters);
    const uint32_t cb = s.cbuf;
    const uint32_t nt = (s.ccnt + CH_TILE - 1) / CH_TILE;
    const double LO = MODE == QM_DEC ? (double)DEC_LO : (double)BIN_LO;
    const double HI = MODE == QM_DEC ? (double)DEC_HI : (double)BIN_HI;
    // one lane per tile: lane t < nt holds tile t; tile prefix sums and the
    // near-list prefix (tiles before the first overflowing list) by wave scans
    const bool tv = lane < nt;
    const uint32_t tl = tv ? lane : 0u;
    const ChTile T = sh.tile[cb][tl];
    const uint32_t ovt = min(first_lane(__ballot(tv && T.nc > (uint32_t)CH_NE)), nt);
    const int64_t Sl = tv ? T.S : 0;
    const int64_t TS_t = wave_incl_scan_i64(Sl) - Sl;                 // nominal sum before tile t
    const uint32_t ncl = (tv && lane < ovt) ? T.nc : 0u;
    const uint32_t np1 = wave_scan_u32(ncl, 0u, [](uint32_t x, uint32_t y) { return x + y; });
    const uint32_t np0 = np1 - ncl;                                   // near entries before tile t
    const uint32_t ne = (uint32_t)__builtin_amdgcn_readlane((int)np1, 63);
    uint32_t NPF[CH_NP];                                              // wave-uniform copies
#pragma unroll
    for (int u = 0; u < CH_NP; u++) NPF[u] = (uint32_t)__builtin_amdgcn_readlane((int)np0, u);
    const int64_t tbase_i = s.D + TS_t;                               // nominal start of tile t
    const double tbase = (double)tbase_i;                              // (exact in the one-decade modes)
    uint32_t moff = 0;                                                 // XDEC: max |resolved offset|
    stamps.setup_end(dbg, lane, s);

    // Near steps in sequence order, 64 at a time.  A step's exact result
    // depends on its exact predecessor = nominal + (offset before it); far
    // steps keep the offset, so the offset before step g is the flips (exact
    // result - nominal result) of the earlier near steps.  Wave fixed point:
    // evaluate every step at the current guess, scan the flips, re-guess; when
    // no guess changes before the first step that leaves the regime, the
    // guesses are the true offsets (induction over lanes).
    uint32_t nstop = NO_STOP;
    if constexpr (MODE == QM_XDEC) {
        // The same fixed point on the window's integer states: a guess is the
        // offset (exact - nominal) before the step; an add step reports its
        // flip (exact result - (guessed predecessor + r)), a reset step (a
        // decade up: its result forgets small errors of its predecessor) the
        // offset after it, and a segmented scan turns both into the offset
        // after every step.  No allow / clamp test here (th is not kept):
        // a tile where one is possible never commits (ymin below), and its
        // exact replay finds it.
        constexpr int ITMAX = 16;
        int32_t cbo = 0;
        const uint32_t it_x0 = iters;
        for (uint32_t b = 0; b < ne; b += 64) {
            const uint32_t g = b + lane;
            const bool v = g < ne;
            uint32_t t = 0, base = NPF[0];
#pragma unroll
            for (int u = 1; u < CH_NP; u++) {
                const bool ge = g >= NPF[u];
                t += ge ? 1u : 0u;
                base = ge ? NPF[u] : base;
            }
            const uint32_t k = v ? g - base : 0u;
            const int64_t pn = __shfl(tbase_i, (int)t, 64) + __double_as_longlong(sh.ne_pred[cb][t][k]);
            const double ad = sh.ne_add[cb][t][k];
            const int64_t r = __double_as_longlong(sh.ne_th[cb][t][k]);
            const bool rs = v && ((sh.ne_kind[cb][t] >> k) & 1ull);
            int32_t est = cbo, outv = cbo;
            uint32_t stop_lane = 64;
            for (int it = 0;; it++) {
                const int64_t pred = pn + est;
                int64_t Xn = pred, Xin;
                double tk;
                bool up;
                const bool ok = xstep(pred, xs, ad, __builtin_inf(), Xn, tk, up, Xin);
                // flips from the state the step started from (the guess
                // rounded onto a state), as in the one-decade modes
                const int64_t d64 = rs ? Xn - (pn + r) : Xn - (Xin + r);
                const bool brk = v && (!ok || d64 > 0x3fffffffLL || d64 < -0x3fffffffLL);
                const bool fl = rs && !brk;
                const int64_t incl = seg_incl_scan_i64(fl, (v && !brk) ? d64 : 0, (int64_t)cbo);
                outv = (int32_t)incl;
                const int32_t en = wave_prev_i32(outv, cbo);    // the guess: the offset after the lane before
                iters++;
                if (it + 1 < CH_UNCHECKED) {
                    est = en;
                    continue;
                }
                const uint32_t fb = first_lane(__ballot(brk));
                const uint32_t fc = first_lane(__ballot(v && en != est));
                if (fc >= fb) { stop_lane = fb; break; }
                if (it + 1 == ITMAX) {
                    stop_lane = fc;
                    if (dbg && lane == 0) atomicAdd(&dbg[DBG_X_UNCONVERGED], 1u);
                    break;
                }
                est = en;
            }
            const bool keep = v && lane < stop_lane;
            if (keep) sh.ne_off[g] = outv;
            const uint32_t ao = keep ? (uint32_t)(outv < 0 ? -outv : outv) : 0u;
            moff = max(moff, (uint32_t)__builtin_amdgcn_readlane(
                                 (int)wave_scan_u32(ao, 0u, [](uint32_t x, uint32_t y) { return x > y ? x : y; }), 63));
            if (stop_lane < 64) {
                nstop = b + stop_lane;
                break;
            }
            cbo = __builtin_amdgcn_readlane(outv, 63);
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ne_off visible to this wave
        if (dbg && lane == 0) {
            atomicAdd(&dbg[DBG_X_NEAR_PASSES], iters - it_x0);
            atomicAdd(&dbg[DBG_X_NEAR_ENTRIES], ne);
        }
    } else {
        constexpr int ITMAX = 16;
        int32_t cbo = 0;
        for (uint32_t b = 0; b < ne; b += 64) {
            const uint32_t g = b + lane;
            const bool v = g < ne;
            // the tile t holding near entry g and its first near index NPF[t]
            // (NPF is non-decreasing; selects on wave-uniform values: indexing
            // NPF by a lane-varying t made the compiler spill it to scratch)
            uint32_t t = 0, base = NPF[0];
#pragma unroll
            for (int u = 1; u < CH_NP; u++) {
                const bool ge = g >= NPF[u];
                t += ge ? 1u : 0u;
                base = ge ? NPF[u] : base;
            }
            const uint32_t k = v ? g - base : 0u;
            const double pn = __shfl(tbase, (int)t) + sh.ne_pred[cb][t][k];
            const double ad = sh.ne_add[cb][t][k];
            const double th = sh.ne_th[cb][t][k];
            const double r = rint(ad * P);
            int32_t est = 0, flip = 0;
            uint32_t stop_lane = 64;
            for (int it = 0;; it++) {
                double tk;
                const double pred = pn + (double)(cbo + est);
                const double Dn = tb_step_d<MODE>(pred, P, R, ad, th, tk);
                const bool brk = v && !(Dn == Dn);
                flip = (!v || brk) ? 0 : (int32_t)(Dn - (pred + r));
                const int32_t incl = (int32_t)wave_scan_u32((uint32_t)flip, 0u,
                                                            [](uint32_t x, uint32_t y) { return x + y; });
                const int32_t en = incl - flip;
                iters++;
                // the first CH_UNCHECKED passes skip the convergence test (two
                // ballots, their scalar first-lane searches and a branch: about
                // half of a pass's latency): a pass past the fixed point
                // changes nothing, and most groups need several passes
                if (it + 1 < CH_UNCHECKED) {
                    est = en;
                    continue;
                }
                const uint32_t fb = first_lane(__ballot(brk));
                const uint32_t fc = first_lane(__ballot(v && en != est));
                if (fc >= fb) { stop_lane = fb; break; }             // converged up to the first exit
                if (it + 1 == ITMAX) { stop_lane = fc; break; }      // lanes < fc are exact
                est = en;
            }
            if (v && lane < stop_lane) sh.ne_off[g] = cbo + est + flip;
            if (stop_lane < 64) {
                nstop = b + stop_lane;
                break;
            }
            cbo += __builtin_amdgcn_readlane(est + flip, 63);
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ne_off visible to this wave
    }
    const uint32_t nres = nstop < ne ? nstop : ne;      // ne_off[0, nres) are exact
    stamps.near_end(dbg, lane, s, ne, iters, MODE == QM_XDEC);

    // Tile checks, one lane per tile: a tile whose bounds exclude a regime
    // exit is committed as a run; the first other one is replayed exactly.
    const uint32_t i0 = np0 < nres ? np0 : nres, i1 = np1 < nres ? np1 : nres;
    const int32_t off_in = i0 ? sh.ne_off[i0 - 1] : 0;
    const int32_t off_out = i1 ? sh.ne_off[i1 - 1] : 0;
    const bool forced = tl >= ovt || (nstop != NO_STOP && nstop < np1) || T.ev != NO_STOP;
    const int64_t Dt = s.D + TS_t + off_in;
    const int64_t D1 = Dt + T.S + (off_out - off_in);
    {
        const double dD = (double)Dt, nc = (double)T.nc;
        bool cand;
        if constexpr (MODE == QM_XDEC) {
            // the exact state stays within the producers' classification slack
            // of their estimate V, and below every allow / clamp threshold:
            // |X - V| <= |X_t - V_t| + drift + the tile's offset changes,
            // plus 4096 units for V's own rounding (valid below 2^60, which
            // ch_produce_x enforces: rl_tb_xdec.h)
            const double bound = fabs(dD - T.cmax) + T.cmin + 2.0 * (double)moff + 4096.0;
            cand = forced || !(bound < T.dmax) || !(bound + 2.0 < T.ymin);
        } else {
            cand = forced || !(dD + nc + T.cmax < HI) || !(dD - nc + T.cmin >= LO + 1.0) ||
                   !(dD + nc + 3.0 < T.ymin) || !(dD + nc + fmax(T.cmax, 0.0) <= T.dmax);
        }
        const uint64_t candm = __ballot(tv && cand);
        uint32_t lo = 0;                                   // tiles [lo, c) commit now
        uint32_t c = first_lane(candm);
        const uint32_t pos = s.cfirst + tl * CH_TILE;
        const uint32_t len = (s.ccnt - tl * CH_TILE) < CH_TILE ? (s.ccnt - tl * CH_TILE) : CH_TILE;
        for (;;) {
            if (tv && lane >= lo && lane < c) {
                runs.len[pos] = (uint16_t)len;
                runs.E[pos] = (int16_t)(MODE == QM_XDEC ? s.E + XRUN : s.E);
                runs.D0[pos] = Dt;
                runs.D1[pos] = D1;
            }
            if constexpr (MODE == QM_XDEC) {   // listed for k_tb_expand_x
                const uint64_t cm = __ballot(tv && lane >= lo && lane < c);
                if (cm) {
                    uint32_t b0 = 0;
                    if (lane == 0) b0 = atomicAdd(runs.xcnt, (uint32_t)__popcll(cm));
                    b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
                    if ((cm >> lane) & 1ull) runs.xlist[b0 + (uint32_t)__popcll(cm & ((1ull << lane) - 1ull))] = pos;
                }
            }
            ChOutcome o;
            if (c >= nt) {
                o.kind = CH_FULL;
                o.q = s.cfirst + s.ccnt;
                o.D = readlane_i64(D1, nt - 1);
                return o;
            }
            // exact replay of tile c from its exact start; lane guesses from
            // the resolved near offsets
            const uint32_t cpos = s.cfirst + c * CH_TILE;
            const uint32_t clen = (s.ccnt - c * CH_TILE) < CH_TILE ? (s.ccnt - c * CH_TILE) : CH_TILE;
            const int64_t Dc = readlane_i64(Dt, c);
            const uint32_t cn0 = (uint32_t)__builtin_amdgcn_readlane((int)np0, (int)c);
            const int32_t cin = (int32_t)__builtin_amdgcn_readlane(off_in, (int)c);
            int32_t goff = 0;
            if (MODE != QM_XDEC && c < ovt) {
                const uint32_t gi = cn0 + sh.ne_rank[cb][c][lane];
                const uint32_t gc = gi < nres ? gi : nres;
                goff = (gi > cn0 && gc) ? sh.ne_off[gc - 1] - cin : 0;
            }
            (void)cin;
            int64_t Dq = 0;
            ChResolveStamps tile;
            tile.begin(iters);
            uint32_t brk;
            if constexpr (MODE == QM_XDEC) {
                const uint32_t it_e = iters;
                brk = exact_span_x<false>(RingSrc{sh}, cpos, clen, Dc, xs, Dq, a, iters);
                if (dbg && lane == 0) atomicAdd(&dbg[DBG_X_EXACT_PASSES], iters - it_e);
            }
            else brk = exact_span<MODE, false>(RingSrc{sh}, cpos, clen, Dc, goff, P, R, Dq, a, iters);
            tile.exact_end(dbg, lane, s, iters, MODE == QM_XDEC);
            if (brk > clen) {       // (never) give up on the window: one exact serial step
                if (lane == 0) atomicOr(eflags, EF_INTERNAL);
                brk = 0;
                Dq = Dc;
            }
            if (dbg && lane == 0) atomicAdd(&dbg[MODE == QM_XDEC ? DBG_X_EXACT_TILES : DBG_EXACT_TILES], 1u);
            if (lane == 0 && brk) {
                runs.len[cpos] = (uint16_t)brk;
                runs.E[cpos] = (int16_t)(MODE == QM_XDEC ? s.E + XRUN : s.E);
                runs.D0[cpos] = Dc;
                runs.D1[cpos] = Dq;
                if (MODE == QM_XDEC) runs.xlist[atomicAdd(runs.xcnt, 1u)] = cpos;
            }
            if (brk < clen) {
                o.kind = CH_STOP;
                o.q = cpos + brk;
                o.D = Dq;
                return o;
            }
            const bool agree = Dq == readlane_i64(D1, c);
            const bool fc = __builtin_amdgcn_readlane((int)forced, (int)c) != 0;
            if (fc || !agree) {
                o.kind = c + 1 < nt ? CH_PARTIAL : CH_FULL;
                o.q = cpos + clen;
                o.D = Dq;
                return o;
            }
            lo = c + 1;
            c = first_lane(candm & ~((2ull << c) - 1ull));
        }
    }
}

// the chain's exact state (D, E, mode: its window's representation, or
// stored digits for QM_DEC / QM_NONE) into the representation of window w;
// false when it does not fit (then the state is left as it was)
__device__ inline bool st_convert(ChState& s, const ChWin& w, int32_t profile) {
    if (w.mode == QM_NONE) return false;
    if (w.mode == s.mode && w.E == s.E) return true;
    if (profile != PROFILE_REDIS7 || s.mode == QM_BIN || w.mode == QM_BIN) return false;
    int64_t Dd = s.D;
    int32_t Ed = s.E;
    if (s.mode == QM_XDEC) x_to_dec(s.D, s.E, Dd, Ed);
    int64_t out;
    if (!dec_to_win(Dd, Ed, w.mode, w.E, out)) return false;
    s.D = out;
    s.E = w.E;
    s.mode = w.mode;
    return true;
}

// The multi-decade windows' work out of line (ch_resolve_x, ch_plan_w,
// ch_produce_xw): it is the rarer path, and inlined into the chain kernel its
// registers crowded the one-decade path's -- the 9-wave block (168 VGPRs)
// spilled VGPRs into scratch inside the chain's loops, and an 8-wave block
// cost the heavy / light phases 15 % on FW uniform (profiles/r5_xdec_ab.txt).
// Called with the LDS state as an address-space-3 pointer, so their LDS
// accesses stay ds_* instructions; everything else by value.
typedef ChainShared __attribute__((address_space(3))) ChainLds;

__device__ XDEC_FN ChOutcome ch_resolve_x(ChainLds* shp, ChState s, XScale xs, ReqArgs a,
                                                          TbRuns runs, uint32_t* eflags, uint32_t iters,
                                                          uint32_t* dbg) {
    ChainShared& sh = *(ChainShared*)shp;
    ChOutcome o = ch_resolve<QM_XDEC>(sh, s, xs.P[0], 0.0, xs, a, runs, eflags, iters, dbg);
    o.iters = iters;
    return o;
}

struct XPlanW {
    int32_t mode;
    int32_t E;
    double vt;        // the calling producer's tile start estimate
};
__device__ XDEC_FN XPlanW ch_plan_w(ChainLds* shp, uint32_t first, uint32_t cnt, double v0,
                                                    uint32_t pw, uint32_t seq) {
    ChainShared& sh = *(ChainShared*)shp;
    const XPlan pl = ch_plan_par(sh, first, cnt, v0, pw, seq);
    return XPlanW{pl.mode, pl.E, pick(pl.vt, pw)};
}
__device__ XDEC_FN void ch_produce_xw(ChainLds* shp, uint32_t buf, uint32_t t, uint32_t pfirst,
                                                       uint32_t pcnt, int32_t F, double vt) {
    ChainShared& sh = *(ChainShared*)shp;
    const XScale xs = xscale(F);
    ch_produce_x(sh, buf, t, pfirst, pcnt, xs, vt);
}

// Replay one huge token-bucket segment [j0, j1) with the whole block.
template <bool LCFG>
__device__ __attribute__((always_inline)) inline void ch_segment(ChainShared& sh, TbEntry* e, uint32_t j0, uint32_t j1,
                                                                const CfgDev* __restrict__ cfgs, int32_t profile,
                                                                const ReqArgs& a, const TbPre& pre, uint32_t* eflags,
                                                                uint32_t* dbg, const TbRuns& runs, uint32_t& plan_seq) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t nrounds = 0, iters = 0, par = 0, nserial = 0;
    uint64_t cyc[4] = {0, 0, 0, 0}, t0 = 0, t1 = 0;
    ChStamps stamps;
    (void)t0; (void)t1;
    TbLoader L;
    L.next = j0 / 128u;
    L.issued = 0;
    if (tid == 0) {
        const TbQ q = tb_quant(e->tok, profile);
        ChState s0;
        s0.D = q.D;
        s0.E = q.E;
        s0.mode = fast_mode(q.D, q.E, profile);
        s0.cfirst = j0;
        s0.ccnt = 0;
        s0.pfirst = j0;
        s0.pbuf = 0;
        s0.cbuf = 1;
        s0.hot = j1 - j0 >= 65536u;
        sh.st[0] = s0;
        sh.spec[0].valid = 0u;
    }
    if (wave == (uint32_t)CH_LOADER) {
        ld_until(L, sh, j0, j0 + 2 * CH_W, j1, pre, lane);
        // the head's add comes from the table entry: into the ring and HBM
        // (k_tb_expand reads it there)
        if (lane == 0) {
            const double add0 = tb_head_add(e, j0, cfgs, profile, a);
            pre.add[j0] = add0;
            reinterpret_cast<double*>(&sh.r_add[ring_slot(j0 >> 1)])[j0 & 1u] = add0;
        }
    }
    stamps.segment_begin(sh, tid);
    lds_barrier();
    stamps.first_round();
    const bool xd = CH_XDEC && profile == PROFILE_REDIS7;
    for (;;) {
        ChState s = sh.st[par];
        // A window is resolved in the representation the producers summarized
        // it in (sh.win): the chain's exact state at the window's start is
        // converted into it.  nofit: it did not fit -- at least one exact
        // serial step this round (progress whatever the plans say).
        bool nofit = false;
        {
            const ChSpec sp = sh.spec[par];
            if (sp.valid) {
                ChState t = s;
                if (s.ccnt == 0 && s.pfirst == sp.first &&
                    (xd ? st_convert(t, sh.win[sp.buf], profile) : (s.mode == QM_DEC && s.E == sp.E))) {
                    // the chain's exit ended where the producers guessed: their
                    // window is the next chain window
                    s.D = t.D;
                    s.E = t.E;
                    s.mode = t.mode;
                    s.cfirst = sp.first;
                    s.ccnt = sp.cnt;
                    s.cbuf = sp.buf;
                    s.pbuf = sp.buf ^ 1u;
                    s.pfirst = sp.first + sp.cnt;
                    if (dbg && threadIdx.x == 0) atomicAdd(&dbg[DBG_SPEC_ADOPTED], 1u);
                } else {
                    // the chain went elsewhere: tile[s.cbuf] does not hold its
                    // next window (the state is exact at s.cfirst / s.pfirst)
                    if (s.ccnt > 0) {
                        s.pfirst = s.cfirst;
                        s.ccnt = 0;
                    }
                    if (dbg && threadIdx.x == 0) {
                        atomicAdd(&dbg[DBG_SPEC_REJECTED], 1u);
                        // why: the chain's exit ended 1 or 2-64 steps after the
                        // guess, or anything else
                        const uint32_t dd = s.pfirst - sp.first;
                        atomicAdd(&dbg[s.ccnt > 0 || s.pfirst <= sp.first || dd > 64u ? DBG_SPEC_OTHER
                                       : dd == 1u                                        ? DBG_SPEC_LATE_1
                                                                                         : DBG_SPEC_LATE_64],
                                  1u);
                    }
                }
            } else if (xd && s.ccnt > 0 && !st_convert(s, sh.win[s.cbuf], profile)) {
                s.pfirst = s.cfirst;
                s.ccnt = 0;
                nofit = true;
            }
        }
        if (s.ccnt == 0 && s.pfirst >= j1) break;                 // block-uniform
        const bool fits = s.mode != QM_NONE || (xd && xdec_fit(s.D, s.E));
        const uint32_t pcnt = (fits && !nofit && s.pfirst < j1) ? ((j1 - s.pfirst) < CH_W ? (j1 - s.pfirst) : CH_W)
                                                                 : 0u;
        // the scale (the decimal modes' reciprocal only where the chain
        // resolves a window: a division on every wave's round is ~1 % of the
        // producers' round)
        double P = 1.0, R = 1.0;
        if (s.mode == QM_BIN) mode_scale(s.mode, s.E, P, R);
        else if (s.mode != QM_NONE) P = rlq::pow10_exact(13 - s.E);
        nrounds++;
        CH_T(t0);
        stamps.round_top(t0);
        if (ch_producer_index(wave) >= 0) {
            const uint32_t pw = (uint32_t)ch_producer_index(wave);
            ChSpec sp{0u, 0u, 0u, 0u, 0, 0.0};
            if (s.ccnt > 0 && s.mode == QM_DEC) sp = ch_predict(sh, s, P, R, j1, xd);
            stamps.exit_guess(t0, t1, cyc, sp.valid);
            // the window to summarize and its representation
            ChainLds* const shl = (ChainLds*)&sh;
            XPlanW pl;
            pl.mode = QM_NONE;
            pl.E = 0;
            pl.vt = 0.0;
            uint32_t wf = 0, wc = 0;
            double dmax = (double)DEC_HI;
            if (sp.valid) {
                if (xd) {
                    stamps.plan_call_begin();
                    pl = ch_plan_w(shl, sp.first, sp.cnt, sp.v0, pw, ++plan_seq);
                    stamps.plan_call_end();
                    if (pl.mode == QM_NONE) sp.valid = 0u;
                } else {
                    pl.mode = QM_DEC;
                    pl.E = sp.E;
                }
                wf = sp.first;
                wc = sp.cnt;
            }
            if (!sp.valid && pcnt) {
                wf = s.pfirst;
                wc = pcnt;
                if (s.mode == QM_DEC || s.mode == QM_BIN) {
                    pl.mode = s.mode;
                    pl.E = s.E;
                    if (s.mode == QM_DEC && s.ccnt == CH_W) {
                        // bound on the window's states (the chain verifies it per
                        // tile): from the chain window's base, its nominal growth G
                        // plus the larger of 1.25 G and 1.5 x its peak above its
                        // start.  Round 4 took 2.25 G alone: one hot key's states
                        // climb ~4e-3 tokens per window under a +-2e-3 sawtooth of
                        // last_refill's rounding, which broke the bound in ~40 % of
                        // its tiles -- each then replayed exactly
                        double G = 0.0, pk = 0.0;
#pragma unroll
                        for (int t = 0; t < CH_NP; t++) {
                            pk = fmax(pk, G + sh.tile[s.cbuf][t].cmax);
                            G += sh.tile[s.cbuf][t].Sd;   // exact: |G| < 2^53
                        }
                        const double g = G > 0.0 ? G : 0.0;
                        dmax = fmin(dmax, (double)s.D + g + fmax(1.25 * g, 1.5 * pk) + 0x1p21);
                    }
                } else {
                    // after a multi-decade window or from a state off the fast
                    // decades: plan from the state's estimate at the window start
                    int64_t Xe = s.D;
                    if (s.ccnt > 0) {
                        const uint32_t nt = (s.ccnt + CH_TILE - 1) / CH_TILE;
#pragma unroll
                        for (int t = 0; t < CH_NP; t++) Xe += (uint32_t)t < nt ? sh.tile[s.cbuf][t].S : 0;
                    }
                    stamps.plan_call_begin();
                    // (the round's second plan at most: the call above may have
                    // made one and found no fit, and the round barrier comes
                    // before the next -- the hand-off slots of ch_plan_par,
                    // indexed by the plan number's parity, rely on it)
                    pl = ch_plan_w(shl, wf, wc, st_value(Xe, s.E, s.mode), pw, ++plan_seq);
                    stamps.plan_call_end();
                }
            }
            stamps.plan_end(t1);
            if (pw == 0 && (threadIdx.x & 63) == 0) {
                sp.buf = s.pbuf;
                sh.spec[par ^ 1u] = sp;
                sh.win[s.pbuf] = ChWin{wc ? pl.mode : (int32_t)QM_NONE, pl.E};
                if (dbg && wc) atomicAdd(&dbg[pl.mode == QM_XDEC ? DBG_WIN_SUMMARIZED_X : DBG_WIN_SUMMARIZED_DEC], 1u);
            }
            stamps.produce_begin();
            if (wc && pl.mode == QM_XDEC) {
                ch_produce_xw(shl, s.pbuf, pw, wf, wc, pl.E, pl.vt);
            } else if (wc && pl.mode == QM_DEC) {
                ch_produce<QM_DEC>(sh, s.pbuf, pw, wf, wc, rlq::pow10_exact(13 - pl.E), dmax);
            } else if (wc && pl.mode == QM_BIN) {
                ch_produce<QM_BIN>(sh, s.pbuf, pw, wf, wc, P, (double)BIN_HI);
            }
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            CH_T(t1);
            stamps.produce_end(t1, wc != 0, pl.mode == QM_XDEC);
            cyc[0] += t1 - t0;
        } else if (wave == (uint32_t)CH_LOADER) {
            const uint32_t first = s.ccnt ? s.cfirst : s.pfirst;
            ld_until(L, sh, first, s.pfirst + 2 * CH_W, j1, pre, lane);
            CH_T(t1);
            cyc[0] += t1 - t0;
        } else {
            // ---- chain wave ----
            ChState nx;
            nx.hot = s.hot;
            nx.pbuf = s.pbuf ^ 1u;
            nx.cbuf = s.pbuf;
            ChOutcome o{CH_PARTIAL, s.pfirst, s.D};
            bool restart = true, force = nofit;
            if (s.ccnt > 0) {
                if (s.mode == QM_XDEC) {
                    const XScale xs = xscale(s.E);
                    const uint64_t tx0 = __builtin_amdgcn_s_memtime();
                    o = ch_resolve_x((ChainLds*)&sh, s, xs, a, runs, eflags, iters, dbg);
                    iters = o.iters;
                    if (dbg && lane == 0) {
                        atomicAdd(&dbg[DBG_X_WINDOWS], 1u);
                        atomicAdd(&dbg[DBG_X_FULL], o.kind == CH_FULL ? 1u : 0u);
                        atomicAdd(&dbg[DBG_X_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - tx0) >> 4));
                    }
                } else {
                    XScale xs;
                    xs.F = 0;
                    o = s.mode == QM_DEC ? ch_resolve<QM_DEC>(sh, s, P, 1.0 / P, xs, a, runs, eflags, iters, dbg)
                                         : ch_resolve<QM_BIN>(sh, s, P, R, xs, a, runs, eflags, iters, dbg);
                }
                if (dbg && lane == 0) atomicAdd(&dbg[DBG_WIN_FULL + o.kind], 1u);
                CH_T(t1);
                stamps.resolve_end(t0, t1, s.mode == QM_XDEC);
                cyc[o.kind == CH_FULL ? 0 : 1] += t1 - t0;
                t0 = t1;
                if (o.kind == CH_FULL) {
                    restart = false;
                    nx.D = o.D;                 // exact at s.pfirst (the window's representation)
                } else {
                    force = o.kind == CH_STOP;
                }
            } else if (pcnt) {
                restart = false;                // first window of a run of rounds
                nx.D = s.D;
                if (dbg && lane == 0) atomicAdd(&dbg[DBG_WIN_FIRST], 1u);
            }                                   // else off the fast decades: serial steps from s.pfirst
            if (!restart) {
                nx.E = s.E;
                nx.mode = s.mode;
                nx.cfirst = s.pfirst;
                nx.ccnt = pcnt;
                nx.pfirst = s.pfirst + pcnt;
            } else {
                // exact serial steps: the exiting step, then on while the state
                // fits no window (off the fast decades, and with multi-decade
                // windows also outside theirs) or the last step left the regime
                const uint32_t lim = (j1 - s.pfirst) < CH_W ? j1 : s.pfirst + CH_W;   // resident in the ring
                int64_t Dd = o.D;
                int32_t Ed = s.E;
                if (s.mode == QM_XDEC) x_to_dec(o.D, s.E, Dd, Ed);
                const SerialOut so = serial_steps([&](uint32_t p) { return ring_add(sh, p); },
                                                  [&](uint32_t p) { return ring_th(sh, p); }, o.q, Dd, Ed, force,
                                                  lim, j1, cfgs, profile, a, xd);
                nserial += so.steps;
                CH_T(t1);
                cyc[2] += t1 - t0;
                t0 = t1;
                nx.D = so.D;
                nx.E = so.E;
                nx.mode = so.mode;
                nx.cfirst = so.q;
                nx.ccnt = 0;
                nx.pfirst = so.q;
            }
            if (lane == 0) sh.st[par ^ 1u] = nx;
        }
        par ^= 1u;
        CH_T(t0);
        stamps.round_end(sh, par, t0, ch_producer_index(wave) >= 0 && lane == 0);
        lds_barrier();
        CH_T(t1);
        cyc[3] += t1 - t0;
        stamps.round_barrier_done(sh, par, t1, wave == 0 && lane == 0);
    }
    stamps.flush(dbg, cyc, wave, lane, (uint32_t)CH_LOADER, j1 - j0 >= 65536u);
    if (tid == 0) {
        const ChState s = sh.st[par];
        int64_t Dd = s.D;
        int32_t Ed = s.E;
        if (s.mode == QM_XDEC) x_to_dec(s.D, s.E, Dd, Ed);
        tb_store_end(e, tb_value(Dd, Ed, profile), j1 - 1, cfgs, profile, a);
        if (dbg) {
            atomicAdd(&dbg[DBG_ROUNDS], nrounds);
            atomicAdd(&dbg[DBG_PASSES], iters);
            atomicMax(&dbg[DBG_ROUNDS_MAX], nrounds);
            atomicAdd(&dbg[DBG_SERIAL_STEPS], nserial);
        }
    }
    (void)eflags;
}

}  // namespace rl
