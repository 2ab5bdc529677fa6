// rl_replay_wave.h -- heavy segments replayed by ONE wave: a token-bucket
// segment (wave_segment: exact spans and serial steps, no producers, no
// runs) and a fixed / sliding window segment (wave_win_segment: a prefix sum
// per window run, checked request by request).  replay_rest (rl_replay.h)
// deals them to the waves.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_tb_serial.h"
#include "rl_tb_step.h"
#include "rl_tb_window.h"
#include "rl_tb_xdec.h"
#include "rl_wave.h"
#include "rl_window.h"

namespace rl {

// TbPre::{add, th} from HBM, with the segment head's add computed at replay
struct HeadSrc {
    const double* a;
    const double* t;
    uint32_t j0;
    double add0;
    __device__ double add(uint32_t p) const { return p == j0 ? add0 : a[p]; }
    __device__ double th(uint32_t p) const { return t[p]; }
};

// A multi-decade span of a heavy segment's wave, out of line (as the
// chain's multi-decade work): from the exact stored state (D, E) off the fast
// decades, up to CH_TILE requests at p with outputs, in a window whose floor
// sits four decades below an upper bound of the span's states.  Returns the
// requests replayed (the first one that leaves the regime, or len) and the
// exact state before it in (D, E); 0 when no window fits.
struct XSpan {
    uint32_t brk;
    int32_t E;
    int64_t D;
};
__device__ XDEC_FN XSpan wave_span_x(HeadSrc src, uint32_t p, uint32_t len, int64_t D, int32_t E, ReqArgs a) {
    constexpr int K = CH_K;
    const uint32_t lane = threadIdx.x & 63;
    XSpan o{0u, E, D};
    double sa = 0.0;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const uint32_t i = lane * K + q;
        const double ad = i < len ? src.add(p + i) : 0.0;
        sa += fabs(ad) < 1e300 ? fabs(ad) : 0.0;
    }
    const double x0 = st_value(D, E, QM_NONE);
    const double mx = fabs(x0) + wave_reduce_f64(sa, 0.0, [](double x, double y) { return x + y; });
    if (!(mx < 1e12)) return o;
    const int Et = mx > 0.0 ? (int)floor(log10(mx)) : XDEC_FMIN + 4;
    const int F = max(Et - 4, XDEC_FMIN);
    if (F > XDEC_FMAX) return o;
    int64_t X0;
    if (!dec_to_win(D, E, QM_XDEC, F, X0)) return o;
    const XScale xs = xscale(F);
    int64_t Xe = X0;
    uint32_t iters = 0;
    const uint32_t brk = exact_span_x<true>(src, p, len, X0, xs, Xe, a, iters);
    if (brk > len) return o;   // (never) no convergence: the serial steps take over
    x_to_dec(Xe, F, o.D, o.E);
    o.brk = brk;
    return o;
}

// Replay one heavy (not huge) token-bucket segment [j0, j1) with ONE wave:
// exact_span over CH_TILE requests at a time, writing every result, and exact
// serial steps wherever a step leaves the regime.  No producers, no runs:
// for a few thousand requests this beats a block-wide chain round.
__device__ __attribute__((always_inline)) inline void wave_segment(TbEntry* e, uint32_t j0, uint32_t j1,
                                                                  const CfgDev* __restrict__ cfgs, int32_t profile,
                                                                  const ReqArgs& a, const TbPre& pre,
                                                                  uint32_t* eflags, uint32_t& iters) {
    const TbQ q0 = tb_quant(e->tok, profile);
    const HeadSrc src{pre.add, pre.th, j0, tb_head_add(e, j0, cfgs, profile, a)};
    int64_t D = q0.D;
    int32_t E = q0.E;
    int32_t mode = fast_mode(D, E, profile);
    uint32_t pos = j0;
    const bool xd = CH_XDEC && profile == PROFILE_REDIS7;
    bool exited = false;       // the last span stopped at a step that leaves the regime: a serial step next
    for (uint32_t guard = 0; pos < j1; guard++) {
        if (guard > 2u * (j1 - j0) + 8u) {        // each pass advances pos; never hang on it
            if ((threadIdx.x & 63) == 0) atomicOr(eflags, EF_INTERNAL | 0x100u);
            return;
        }
        if (mode != QM_NONE) {
            double P, R;
            mode_scale(mode, E, P, R);
            const uint32_t len = (j1 - pos) < CH_TILE ? (j1 - pos) : CH_TILE;
            int64_t Dq = D;
            const uint32_t brk = mode == QM_DEC ? exact_span<QM_DEC, true>(src, pos, len, D, 0, P, R, Dq, a, iters)
                                                : exact_span<QM_BIN, true>(src, pos, len, D, 0, P, R, Dq, a, iters);
            if (brk > len) {
                if ((threadIdx.x & 63) == 0) atomicOr(eflags, EF_INTERNAL | 0x200u);
                return;
            }
            D = readfirstlane_i64(Dq);
            pos += (uint32_t)__builtin_amdgcn_readfirstlane((int)brk);
            if (brk == len) continue;
        } else if (xd && !exited && xdec_fit(D, E)) {
            // off the fast decades (after an allow the balance random-walks
            // across zero and decades): a multi-decade span, not serial steps
            const uint32_t len = (j1 - pos) < CH_TILE ? (j1 - pos) : CH_TILE;
            const XSpan xo = wave_span_x(src, pos, len, D, E, a);
            const uint32_t brk = (uint32_t)__builtin_amdgcn_readfirstlane((int)xo.brk);
            if (brk) {
                D = readfirstlane_i64(xo.D);
                E = __builtin_amdgcn_readfirstlane(xo.E);
                mode = fast_mode(D, E, profile);
                pos += brk;
                exited = brk < len;
                continue;
            }
        }
        exited = false;
        const SerialOut so = serial_steps([&](uint32_t p) { return src.add(p); }, [&](uint32_t p) { return src.th(p); },
                                          pos, D, E, true, j1, j1, cfgs,
                                          profile, a, xd);
        // wave-uniform by construction; say so (the loop and its ballots stay uniform)
        pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)so.q);
        D = readfirstlane_i64(so.D);
        E = __builtin_amdgcn_readfirstlane(so.E);
        mode = __builtin_amdgcn_readfirstlane(so.mode);
    }
    if ((threadIdx.x & 63) == 0) tb_store_end(e, tb_value(D, E, profile), j1 - 1, cfgs, profile, a);
}

// window counters: the replay writes the decision and Remaining only (in the
// value slot, as int64 bits); reset_at and retry_after are functions of the
// request's time and config that the finish evaluates (finish_result)
__device__ inline void write_out(const ReqArgs& a, uint32_t i, const Out& o) {
    a.dec[i] = o.decision;
    a.tok[i] = __longlong_as_double(o.remaining);
}

// Replay kernels read the batch in SORTED order: k_permute has copied each
// request's fields to position j of its segment (coalesced loads, one level)
// and results are written at j (coalesced stores); k_unpermute moves them to
// the caller's order.  ReqArgs here always points at the permuted buffers.
struct Req {
    uint32_t c;
    int64_t t, n, sms;
};

__device__ inline Req load_req(const ReqArgs& a, uint32_t j) {
    Req r;
    r.t = a.ts[j];
    r.n = a.n[j];
    r.c = a.cfg[j];
    r.sms = req_server_ms(a, j, r.t);
    return r;
}

// requests [j0, j1) of one window segment, one by one, from state w
__device__ inline void replay_win_steps(WinState& w, const Spill& S, uint32_t j0, uint32_t j1, const CfgDev* cfgs,
                                        int32_t profile, const ReqArgs& a, uint32_t& ef) {
    if (j0 >= j1) return;
    Req cur = load_req(a, j0);
    for (uint32_t j = j0; j < j1; j++) {
        Req nxt = cur;
        if (j + 1 < j1) nxt = load_req(a, j + 1);
        const CfgDev& c = cfgs[cur.c];
        Out o = (c.alg == ALG_SLIDING_WINDOW) ? sw_step(w, S, cur.t, cur.n, cur.sms, c, profile, ef)
                                              : fw_step(w, S, cur.t, cur.n, cur.sms, c, profile, ef);
        write_out(a, j, o);
        cur = nxt;
    }
}

// Replay one heavy fixed / sliding window segment [j0, j1) with ONE wave.
// Within a window run (consecutive requests of one window start ws) the
// reference's state transition is a prefix sum: INCRBY adds n to the current
// window key, whose TTL is set once at creation; SW's previous-window count is
// constant and its key's TTL is refreshed by every request
// (fixedwindow.go:21-27, slidingwindow.go:22-30).  So per run: the first
// request runs exactly (fw_step / sw_step on the exact state: key lookup,
// expiry, slot allocation), the rest are computed in parallel from a prefix
// sum of n and checked request by request against every assumption of that
// shortcut -- the current key alive, no INCRBY overflow, no TTL reset,
// the previous key's refresh chain.  A failed check (or a config change, a
// key in the spill, sub-second windows) continues serially from the first
// request not yet applied, on the exact state reached so far: the first
// request of a run has side effects on the spill table, so nothing is ever
// replayed twice.
__device__ __attribute__((always_inline)) inline void wave_win_segment(WinEntry* e, const Spill& S, uint32_t j0,
                                                                      uint32_t j1, const CfgDev* __restrict__ cfgs,
                                                                      int32_t profile, const ReqArgs& a,
                                                                      uint32_t* eflags) {
    constexpr int K = CH_K;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t c0 = a.cfg[j0];
    const CfgDev& C = cfgs[c0];
    const bool sw = C.alg == ALG_SLIDING_WINDOW;
    WinState w = win_load(e);
    uint32_t ef = 0;
    bool ok = C.ttl_c > 0;
    uint32_t pos = j0;
    while (ok && pos < j1) {
        // first request of the run: exact
        const Req r0 = load_req(a, pos);
        if (r0.c != c0) { ok = false; break; }   // serial from pos
        const Out o0 = sw ? sw_step(w, S, r0.t, r0.n, r0.sms, C, profile, ef)
                          : fw_step(w, S, r0.t, r0.n, r0.sms, C, profile, ef);
        if (lane == 0) write_out(a, pos, o0);
        const int64_t wsn = window_start_ns(r0.t, C);
        const int64_t ws = floor_div(wsn, NS_PER_S), pws = ws - C.ttl_c;
        int ck = -1, pk = -1;
        for (int k = 0; k < 2; k++) {
            if (w.s[k].when == ABSENT) continue;
            if (w.s[k].ws == ws) ck = k;
            else if (sw && w.s[k].ws == pws) pk = k;
        }
        pos++;   // r0 is applied
        if (o0.decision == DEC_ERROR || ck < 0) { ok = false; break; }
        // the run's shortcut keeps the previous window's key in the entry; one
        // in the spill (per-key time went back) takes the serial path
        if (sw && pk < 0 && spill_lookup(S, w.key, w.nspill, pws)) { ok = false; break; }
        const int64_t when_c = w.s[ck].when;
        const int64_t cnt_p = pk >= 0 ? w.s[pk].cnt : 0;
        int64_t c_run = w.s[ck].cnt, sms_prev = r0.sms;
        bool p_alive = pk >= 0;
        bool run_end = false;
        while (ok && !run_end && pos < j1) {
            // K requests per lane; the run ends at the first other window / config
            const uint32_t off = lane * K;
            int64_t t[K], n[K], sm[K];
            bool same[K];
            uint32_t firstx = NO_STOP;
#pragma unroll
            for (int q = 0; q < K; q++) {
                const uint32_t j = pos + off + q;
                const bool v = j < j1;
                t[q] = v ? a.ts[j] : 0;
                n[q] = v ? a.n[j] : 0;
                sm[q] = v ? req_server_ms(a, j, t[q]) : 0;
                // window_start(t) == ws without two 64-bit divisions: W >= 1 s
                // here (ttl_c > 0), so windows whose starts differ also differ
                // in the key's second, and t is in r0's window iff it lies in
                // [wsn, wsn + W)
                same[q] = v && a.cfg[j] == c0 && t[q] >= wsn && t[q] - wsn < C.window;
                if (v && !same[q] && firstx == NO_STOP) firstx = off + q;
            }
            const uint32_t cend = wave_min_u32(firstx);            // run end in this chunk (relative)
            const uint32_t lim = min(min(cend, j1 - pos), (uint32_t)(64 * K));
            run_end = cend != NO_STOP;
            if (lim == 0) break;   // the run was r0 alone: nothing to carry
            // prefix sum of n (int64) inside the run, per-request checks
            int64_t ls = 0;
#pragma unroll
            for (int q = 0; q < K; q++)
                if (off + q < lim) ls += n[q];
            const int64_t li = wave_incl_scan_i64(ls);
            int64_t c = c_run + li - ls;                            // count before my first request
            int64_t sp = __shfl_up(sm[K - 1], 1);                   // server clock of my predecessor
            if (lane == 0) sp = sms_prev;
            bool bad = false, pdead = false;
            uint32_t pdead_at = NO_STOP;
#pragma unroll
            for (int q = 0; q < K; q++) {
                if (off + q >= lim) continue;
                bad |= incr_overflows(c, n[q]);
                const int64_t cur = c + n[q];
                bad |= (double)cur == (double)n[q];                 // would (re)set the TTL
                bad |= !key_alive(when_c, sm[q], profile);          // current key expired mid-run
                if (sw && !pdead && !key_alive(expire_when(C.ttl_p, sp), sm[q], profile)) {
                    pdead = true;
                    pdead_at = off + q;
                }
                sp = sm[q];
                c = cur;
            }
            if (__ballot(bad)) { ok = false; break; }   // serial from pos (this chunk)
            const uint32_t pd = wave_min_u32(pdead_at);             // first request that finds prev dead
            // outputs
            c = c_run + li - ls;
#pragma unroll
            for (int q = 0; q < K; q++) {
                if (off + q >= lim) continue;
                const int64_t cur = c + n[q];
                c = cur;
                Out o;
                o.tokens = 0.0;
                o.reset_at = wadd(wmul(ws, NS_PER_S), C.window);
                int64_t count;
                bool allowed;
                if (sw) {
                    const int64_t p = (p_alive && off + q < pd) ? go_f2i((double)cnt_p) : 0;
                    const int64_t cc = go_f2i((double)cur);
                    const int64_t elapsed = wsub(t[q], wmul(ws, NS_PER_S));
                    const double progress = (double)elapsed / (double)C.window;
                    double weighted = (double)p * (1.0 - progress);
                    weighted = weighted + (double)cc;
                    allowed = weighted <= C.limit_d;
                    count = go_f2i(weighted);
                } else {
                    count = go_f2i((double)cur);
                    allowed = count <= C.limit;
                }
                const int64_t rem = wsub(C.limit, count);
                o.remaining = rem < 0 ? 0 : rem;
                o.decision = allowed ? DEC_ALLOWED : DEC_DENIED;
                o.retry = allowed ? 0 : until_reset(o.reset_at, t[q]);
                write_out(a, pos + off + q, o);
            }
            // carry to the next chunk
            const uint32_t lastl = (lim - 1) / K, lastq = (lim - 1) % K;
            int64_t smv = sm[0];
#pragma unroll
            for (int q = 1; q < K; q++) smv = (uint32_t)q == lastq ? sm[q] : smv;
            sms_prev = readlane_i64(smv, lastl);
            c_run = readlane_i64(c, lastl);
            if (pd != NO_STOP) p_alive = false;
            pos += lim;
        }
        // the state after the run's applied requests
        w.s[ck].cnt = c_run;
        if (pk >= 0) w.s[pk].when = p_alive ? expire_when(C.ttl_p, sms_prev) : ABSENT;
    }
    if (lane == 0) {
        if (!ok) replay_win_steps(w, S, pos, j1, cfgs, profile, a, ef);
        win_store(e, w);
        if (ef) atomicOr(eflags, ef);
    }
}

}  // namespace rl
