// rl_tb_serial.h -- the serial step loop: exact token-bucket steps by one
// wave wherever a step leaves the fast regime (an allow, a clamp, an expired
// key, a state off the fast decades).  The chain wave (rl_tb_chain.h) and the
// one-wave heavy segment (rl_replay_wave.h) both end their spans with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_semantics.h"
#include "rl_tb_step.h"
#include "rl_tb_xdec.h"
#include "rl_wave.h"

namespace rl {

// Exact serial steps by one wave (every lane computes the same values): from
// the exact stored state (D, E) before position q, the step at q when `force`
// (a step that leaves the regime), then on while the state is off the fast
// decades or the last step left the regime -- at most CH_SERIAL steps and
// never at or past lim.  add_at(p): TbPre::add of p.  Step k's outputs are
// collected in lane k % 64 and stored 64 positions at a time (coalesced),
// not one lane-0 store per step.  Redis 7 steps in decimal mode take
// tb_dec_step; the rest (allows, clamps, expired keys, far decade jumps, the
// binary profile) the general tb_eval.
struct SerialOut {
    uint32_t q;        // next position
    int64_t D;         // exact stored state before it
    int32_t E;
    int32_t mode;
    uint32_t steps;
};

// xd: multi-decade windows are available -- stop after the forced steps
// whenever the state fits one (any state of 1e-9 .. 1e12 tokens, or zero)
__device__ inline bool xdec_fit(int64_t D, int32_t E) { return D == 0 || (E >= XDEC_FMIN && E <= XDEC_FMAX + 4); }

template <typename AddAt, typename ThAt>
__device__ __attribute__((always_inline)) inline SerialOut serial_steps(AddAt add_at, ThAt th_at, uint32_t q, int64_t D, int32_t E,
                                                                       bool force, uint32_t lim, uint32_t j1,
                                                                       const CfgDev* __restrict__ cfgs,
                                                                       int32_t profile, const ReqArgs& a,
                                                                       bool xd = false) {
    const uint32_t lane = threadIdx.x & 63;
    // mode: the callers' fast regime (positive digits only).  emode: how a step
    // is evaluated here -- sign-symmetric, because %.14g / strtod and the
    // binade scaling are: a negative state in a fast decade (the balance a hot
    // key random-walks around zero after an allow, its last_refill rounded to
    // 100 us) steps with the decade arithmetic instead of a full
    // decimal conversion per step
    int32_t mode = fast_mode(D, E, profile);
    int32_t emode = fast_mode(D < 0 ? -D : D, E, profile);
    double Ps = 1.0, Rs = 1.0;
    if (emode != QM_NONE) mode_scale(emode, E, Ps, Rs);
    // the state as a double too (Dd == D while both are live; tb_dec_step
    // updates Dd alone and D follows when the general path needs it)
    double Dd = (double)D;
    bool d_stale = false;
    // add and th = min(capacity, n) of the next 64 positions in one vector load
    // each (lane k holds position q + k; the chain's are in its LDS ring): a
    // step costs its arithmetic, not a dependent memory round trip.  n and the
    // capacity themselves matter only when sum >= th (an allow or a clamp) or
    // the key has expired: below th the step denies without clamping whatever
    // they are, so only those steps load them (from HBM)
    double avec = 0.0, tvec = 0.0;
    double otok = 0.0;
    uint32_t odec = 0;
    uint32_t g0 = q;       // first position of the outputs collected in the lanes
    uint32_t k = 0;
    for (; q < lim && k < (uint32_t)CH_SERIAL && (force || (mode == QM_NONE && !(xd && xdec_fit(xd ? (int64_t)Dd : D, E))));
         k++) {
        const uint32_t kl = k & 63u;
        if (kl == 0) {
            if (k) {   // the previous 64 outputs
                a.tok[g0 + lane] = otok;
                a.dec[g0 + lane] = (uint8_t)odec;
            }
            g0 = q;
            const uint32_t pq = q + lane;
            avec = pq < lim ? add_at(pq) : 0.0;
            tvec = pq < lim ? th_at(pq) : 0.0;
        }
        const double add = __longlong_as_double(readlane_i64(__double_as_longlong(avec), kl));
        const bool alive = add == add;
        const double th = __longlong_as_double(readlane_i64(__double_as_longlong(tvec), kl));
        if (profile == PROFILE_REDIS7 && emode == QM_DEC && alive) {
            double tk;
            if (tb_dec_step(Dd, E, Ps, add, th, tk)) {
                otok = lane == kl ? tk : otok;
                odec = lane == kl ? (uint32_t)DEC_DENIED : odec;
                d_stale = true;
                force = false;
                mode = (Dd >= 1e13) ? QM_DEC : QM_NONE;   // E stays in the fast range
                q++;
                continue;
            }
        }
        if (d_stale) {
            D = (int64_t)Dd;
            d_stale = false;
        }
        TbEval v = tb_eval(emode, D, E, Ps, Rs, alive, alive ? add : 0.0, th, th, profile);
        if (!alive || v.clamped) {      // sum >= th or an expired key: the real n and capacity
            const int64_t nn = a.n[q];
            const double cap = cfgs[a.cfg[q]].limit_d;
            v = tb_eval(emode, D, E, Ps, Rs, alive, alive ? add : 0.0, cap, (double)nn, profile);
        }
        otok = lane == kl ? v.tokens : otok;
        odec = lane == kl ? (uint32_t)(v.allowed ? DEC_ALLOWED : DEC_DENIED) : odec;
        force = !xd && (v.allowed || v.clamped || !alive);
        const bool same = emode != QM_NONE && v.inrange;
        if (same) {
            D = v.Dact;                     // same decade / binade (sign may flip)
        } else {
            // a step out of a fast decade nearly always lands in a neighbouring
            // one: its 14 digits there from one exact scaled rounding (valid in
            // exactly one decade: the exact product >= 1e13 and the rounded
            // digits < 1e14), else the general %.14g decomposition
            bool nb = false;
            if (emode == QM_DEC) {
                const double at = v.tokens < 0.0 ? -v.tokens : v.tokens;
#pragma unroll
                for (int d = -1; d <= 1; d += 2) {
                    const int32_t k2 = 13 - (E + d);
                    if (nb || k2 < 1 || k2 > 22) continue;
                    const double P2 = d < 0 ? Ps * 10.0 : Ps / 10.0;     // exact powers of ten (k2 <= 22)
                    bool ge_lo;
                    const double Dn = round_scaled_Pd(at, P2, ge_lo);
                    if (at > 0.0 && ge_lo && Dn < (double)DEC_HI) {
                        D = v.tokens < 0.0 ? -(int64_t)Dn : (int64_t)Dn;
                        E = E + d;
                        Ps = P2;
                        Rs = 0.0;
                        nb = true;
                    }
                }
            }
            if (!nb) {
                const TbQ nq = tb_quant(v.tokens, profile);
                D = nq.D;
                E = nq.E;
                emode = fast_mode(D < 0 ? -D : D, E, profile);
                if (emode != QM_NONE) mode_scale(emode, E, Ps, Rs);
            }
        }
        Dd = (double)D;
        mode = fast_mode(D, E, profile);
        q++;
    }
    if (d_stale) D = (int64_t)Dd;
    if (k && lane < q - g0) {   // the last (partial) group of outputs
        a.tok[g0 + lane] = otok;
        a.dec[g0 + lane] = (uint8_t)odec;
    }
    return SerialOut{q, D, E, mode, k};
}

}  // namespace rl
