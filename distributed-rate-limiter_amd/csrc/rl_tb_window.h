// rl_tb_window.h -- the chain's windows: its shape constants, the block's LDS
// state (ChainShared: the input ring, the tile summaries, the near lists, the
// hand-off of state between the rounds), the loader that fills the ring, the
// exact replay of a span by one wave (exact_span), and the producers that
// summarize a one-decade window (ch_produce) and guess where the chain's
// window will leave the regime (ch_predict).  The algebra and the three wave
// roles are described in rl_tb_chain.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_tb_step.h"
#include "rl_wave.h"

namespace rl {

// 6 producers x 6 requests per lane: 8 waves per block, 2 per SIMD, so a
// wave may hold 256 VGPRs.  With the multi-decade windows' code the 9-wave
// shape (7 x 5, at most 168 VGPRs) spilled inside the chain's loops even with
// that code out of line: configs[1] 2.42 vs 2.80e9, Zipf 1.5 8.6 vs 9.4e8 on
// one box (profiles/r5_xdec_ab.txt)
#ifndef RL_CH_NP
#define RL_CH_NP 6
#endif
#ifndef RL_CH_K
#define RL_CH_K 6
#endif
constexpr int CH_K = RL_CH_K;                          // requests per producer lane
constexpr int CH_NP = RL_CH_NP;                        // producer waves
constexpr uint32_t CH_TILE = 64u * CH_K;               // requests per producer wave
constexpr uint32_t CH_W = (uint32_t)CH_NP * CH_TILE;   // requests per window
constexpr int CH_NE = 64;                              // near-list capacity per tile
// Wave roles.  Waves of a block are dealt to the CU's four SIMDs round-robin
// (wave w on SIMD (w + base) mod 4), so the chain (wave 0) shares its SIMD
// with the mostly idle loader (wave 4) and the producers pair up on the
// other three SIMDs.
constexpr int CH_LOADER = 4;
static_assert(CH_NP + 2 <= 16 && CH_NP >= 3, "wave roles");
__device__ inline int ch_producer_index(uint32_t wave) {
    if (wave == 0 || wave == (uint32_t)CH_LOADER) return -1;
    return (int)wave - (wave < (uint32_t)CH_LOADER ? 1 : 2);
}
constexpr int CH_BLOCK = (CH_NP + 2) * 64;
constexpr int CH_SERIAL = 64;                          // serial exact steps per round at most
#ifndef RL_CH_UNCHECKED
#define RL_CH_UNCHECKED 2
#endif
constexpr int CH_UNCHECKED = RL_CH_UNCHECKED;          // near fixed-point passes before the first convergence test
#ifndef RL_XDEC
#define RL_XDEC 1
#endif
constexpr bool CH_XDEC = RL_XDEC != 0;                 // multi-decade windows (rl_tb_xdec.h), Redis-7 profile
#ifndef RL_HEAVY_G
#define RL_HEAVY_G 2
#endif
constexpr int HEAVY_G = RL_HEAVY_G;                    // heavy segments per wave claim (k_tb_chain phase 2)
// conservative scale of the allow/clamp threshold th*P (covers the rounding of
// th*P and of the bound arithmetic with a wide margin)
constexpr double CH_YSCALE = 1.0 - 0x1p-28;

// LDS ring of the segment's inputs by absolute sorted position, in 16-byte
// granules (two positions).  Granule G lives in slot swz(G mod RING_G): an XOR
// of its column (G mod 16) with bits 4-5, so the 8 lanes of one ds_read_b128
// cycle (lane l reads granule G0 + 4l + j) hit distinct banks, while a row of
// 16 slots still holds 16 consecutive granules (the loader's LDS-DMA writes
// slots lane-linearly and swizzles the SOURCE address instead).
#ifndef RL_RING
#define RL_RING 8192
#endif
constexpr uint32_t RING = RL_RING;               // positions
constexpr uint32_t RING_G = RING / 2;            // granules
__host__ __device__ constexpr uint32_t swz(uint32_t g) { return (g & ~15u) | ((g & 15u) ^ ((g >> 4) & 3u)); }
__host__ __device__ constexpr uint32_t ring_slot(uint32_t granule) { return swz(granule & (RING_G - 1)); }
// the chain window, the producers' window and the loader's next window
static_assert(RING >= 3 * CH_W + 256, "the ring must hold three windows");

struct ChTile {
    int64_t S;          // nominal sum of the tile's increments r
    double Sd;          // S as a double (the producers' state bound sums it every round)
    double ymin;        // min over steps of (th * P * CH_YSCALE - inclusive nominal prefix)
    double cmax, cmin;  // max / min inclusive nominal prefix
    double dmax;        // the near band assumed every state of the tile is <= dmax
    uint32_t ev;        // first expired / huge step (tile-relative) or NO_STOP
    uint32_t nc;        // near steps (> CH_NE: list overflow)
};

struct ChState {
    int64_t D;          // exact stored digits at cfirst (ccnt > 0) or at pfirst (ccnt == 0)
    int32_t E;
    int32_t mode;       // QM_DEC / QM_BIN when (D, E) is in a fast decade, else QM_NONE
    uint32_t cfirst;    // chain window [cfirst, cfirst + ccnt), summarized in tile[cbuf]
    uint32_t ccnt;
    uint32_t pfirst;    // producers' window start (== cfirst + ccnt when ccnt > 0)
    uint32_t pbuf, cbuf;
    uint32_t hot;       // diagnostics: segment of >= 65536 requests
};

// Speculative restart: in a round whose chain window will likely leave the
// regime, the producers predict the exit from nominal states (the exit step q
// and the decade E of its result) and summarize the window from q + 1 at scale
// 10^(13 - E) instead of the window after the chain's.  When the chain's
// exact exit and serial steps end at q + 1 in decade E, the next round
// resolves that window at once -- no producers-only round.
struct ChSpec {
    uint32_t valid;
    uint32_t first, cnt;   // window [first, first + cnt), summarized in tile[buf]
    uint32_t buf;
    int32_t E;             // decimal mode at 10^(13 - E) (without XDEC windows)
    double v0;             // XDEC: the guessed state after the exit (tokens): the window's plan starts there
};

// The window the producers summarized into tile[buf] (its representation:
// the chain converts its exact state into it before resolving the window)
struct ChWin {
    int32_t mode;          // QM_DEC / QM_BIN / QM_XDEC
    int32_t E;             // decade / binade, or the XDEC floor F
};

struct ChainShared {
    double2 r_add[RING_G];       // TbPre::add
    double2 r_th[RING_G];        // TbPre::th
    ChTile tile[2][CH_NP];
    // near steps: tile-relative nominal predecessor (XDEC: int64 bits), add,
    // th (XDEC: the step's nominal increment r, int64 bits)
    double ne_pred[2][CH_NP][CH_NE];
    double ne_add[2][CH_NP][CH_NE];
    double ne_th[2][CH_NP][CH_NE];
    uint64_t ne_kind[2][CH_NP];        // XDEC: bit k = near entry k is a reset step (a decade up)
    uint16_t ne_rank[2][CH_NP][64];    // near steps of the tile before each producer lane
    int32_t ne_off[CH_NP * CH_NE];     // chain: resolved offset after each near step
    ChState st[2];
    ChSpec spec[2];                    // producers' speculative window of the round
    ChWin win[2];                      // the representation of tile[buf]'s window
    // ch_plan_par: each producer wave's tile sums and the plan number they
    // belong to (0 at kernel start), in the slot of the plan number's parity
    double plan_s[2][CH_NP], plan_sp[2][CH_NP];
    uint32_t plan_tag[2][CH_NP];
#ifdef RL_STAMPS
    uint32_t wk[2];                    // the round's longest producer work (cycles / 16)
#endif
};

__device__ inline double ring_add(const ChainShared& sh, uint32_t p) {
    return reinterpret_cast<const double*>(&sh.r_add[ring_slot(p >> 1)])[p & 1u];
}
__device__ inline double ring_th(const ChainShared& sh, uint32_t p) {
    return reinterpret_cast<const double*>(&sh.r_th[ring_slot(p >> 1)])[p & 1u];
}

// ---------------------------------------------------------------------------
// loader: LDS-DMA of TbPre::{add, th} into the ring, 128 positions per chunk
// ---------------------------------------------------------------------------
// A chunk may only overwrite positions no longer needed: chunk c is allowed
// once 128c + 128 <= first + RING, `first` = the oldest position this round
// still reads.  The source arrays carry 128 elements of slack past the batch.
struct TbLoader {
    uint32_t next;       // next chunk to issue
    uint32_t issued;     // chunks issued since the last wait
};

// one 16-byte LDS-DMA per lane into the slots starting at the wave-uniform
// LDS byte address `lds` (issued from asm: hipcc neither counts it nor drains
// it early; ld_until waits for it explicitly)
__device__ __attribute__((always_inline)) inline void glds16(const void* gsrc, uint32_t lds) {
    uint32_t keep;
    __asm__ volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(lds)
                     : "memory");
}

__device__ __attribute__((always_inline)) inline void ld_chunk(ChainShared& sh, uint32_t c, const TbPre& pre,
                                                              uint32_t lane) {
    const uint32_t s0 = (c * 64u) & (RING_G - 1);   // first slot of the chunk (row aligned)
    const uint32_t g = c * 64u + swz(lane);         // granule this lane's slot holds
    const uint32_t la = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&sh.r_add[s0];
    const uint32_t lt = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)&sh.r_th[s0];
    glds16(pre.add + 2u * g, __builtin_amdgcn_readfirstlane(la));
    glds16(pre.th + 2u * g, __builtin_amdgcn_readfirstlane(lt));
}

// issue every chunk the ring can take while `first` is still needed
__device__ __attribute__((always_inline)) inline void ld_issue(TbLoader& L, ChainShared& sh, uint32_t first,
                                                              uint32_t j1, const TbPre& pre, uint32_t lane) {
    const uint32_t lim = (first + RING) / 128u;     // chunks c < lim fit
    const uint32_t endc = (j1 + 127u) / 128u;
    while (L.next < lim && L.next < endc && L.issued < 28u) {   // <= 56 outstanding (vmcnt <= 63)
        ld_chunk(sh, L.next, pre, lane);
        L.next++;
        L.issued++;
    }
}

// at most ~k LDS-DMA ops of this wave still in flight (k rounded down to a
// waitcnt immediate)
__device__ __attribute__((always_inline)) inline void ld_wait_at_most(uint32_t k) {
    if (k >= 48u) __asm__ volatile("s_waitcnt vmcnt(48)" ::: "memory");
    else if (k >= 32u) __asm__ volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else if (k >= 16u) __asm__ volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (k >= 8u) __asm__ volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (k >= 4u) __asm__ volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// make [.., target) resident: issue what is missing (and what the ring can
// take beyond it), then wait for the chunks below target only -- the ones
// issued after them (two LDS-DMA ops per chunk, completed in issue order as
// vmcnt counts them) stay in flight into the next round
__device__ __attribute__((always_inline)) inline void ld_until(TbLoader& L, ChainShared& sh, uint32_t first,
                                                              uint32_t target, uint32_t j1, const TbPre& pre,
                                                              uint32_t lane) {
    const uint32_t need = ((target < j1 ? target : j1) + 127u) / 128u;
    for (;;) {
        ld_issue(L, sh, first, j1, pre, lane);
        if (L.next >= need) {
            const uint32_t extra = L.next - need;      // chunks issued after the last needed one
            ld_wait_at_most(2u * (extra < L.issued ? extra : L.issued));
            L.issued = extra < L.issued ? extra : L.issued;
            break;
        }
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        L.issued = 0;
    }
}

// (TbRuns, the committed runs of the chain: rl_batch.h)

struct RingSrc {
    const ChainShared& sh;
    __device__ double add(uint32_t p) const { return ring_add(sh, p); }
    __device__ double th(uint32_t p) const { return ring_th(sh, p); }
};
struct GlobSrc {
    const double* a;
    const double* t;
    __device__ double add(uint32_t p) const { return a[p]; }
    __device__ double th(uint32_t p) const { return t[p]; }
};

// Exact replay of [p, p + len) (len <= CH_TILE) from the exact stored digits
// D0 by one wave: lane l steps requests [p + K l, p + K l + K) from a guessed
// start (nominal prefix + goff, the caller's guess of the lane's offset); the
// guesses are refined by an exclusive scan of every lane's actual change until
// the first lane whose start changed lies past the first regime exit (by
// induction over lanes, every start up to there is then exact).  Returns the
// relative position of the first step that leaves the regime (len if none)
// and in Dend the exact digits before it (after the span).
// OUT: writes tokens and DENIED for every in-regime step.
template <int MODE, bool OUT, typename Src>
__device__ __attribute__((always_inline)) inline uint32_t exact_span(const Src& src, uint32_t p, uint32_t len,
                                                                     int64_t D0, int32_t goff, double P, double R,
                                                                     int64_t& Dend, const ReqArgs& a,
                                                                     uint32_t& iters) {
    constexpr int K = CH_K;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t off = lane * K;
    const uint32_t nv = off < len ? ((len - off) < (uint32_t)K ? (len - off) : (uint32_t)K) : 0u;
    double add[K], th[K];
    int64_t S = 0;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const bool v = (uint32_t)q < nv;
        add[q] = v ? src.add(p + off + q) : 0.0;
        th[q] = v ? src.th(p + off + q) : __builtin_inf();
        const double pr = add[q] * P;
        if (fabs(pr) < 0x1p49) S += (int64_t)rint(pr);     // NaN / huge: a regime exit anyway
    }
    const int64_t incl = wave_incl_scan_i64(S);
    int64_t st = D0 + incl - S + (lane ? goff : 0);
    const uint32_t last = len ? (len - 1) / K : 0u;
    for (uint32_t it = 0;; it++) {
        if (it > 64u) {            // cannot happen (one more exact lane per pass); never hang on it
            Dend = D0;
            return 0xffffffffu;
        }
        double D = (double)st, Db = 0.0;
        uint32_t bq = NO_STOP;
        // every lane evaluates every step (selects, no branches): a lane past
        // its steps or its first regime exit keeps its state
#pragma unroll
        for (int q = 0; q < K; q++) {
            const bool act = (uint32_t)q < nv && bq == NO_STOP;
            double tk;
            const double Dn = tb_step_d<MODE>(D, P, R, add[q], th[q], tk);
            const bool stop = act && !(Dn == Dn);
            const bool take = act && !stop;
            bq = stop ? (uint32_t)q : bq;
            Db = stop ? D : Db;
            if (OUT && take) {
                a.tok[p + off + q] = tk;
                a.dec[p + off + q] = DEC_DENIED;
            }
            D = take ? Dn : D;
        }
        const bool brk = bq != NO_STOP;
        const int64_t A = brk ? 0 : (int64_t)D - st;
        const int64_t ai = wave_incl_scan_i64(A);
        const int64_t nst = D0 + ai - A;
        const uint32_t fb = first_lane(__ballot(brk));
        const uint32_t fd = first_lane(__ballot(nv > 0 && nst != st));
        iters++;
        if (fb == 64u ? fd == 64u : fd > fb) {
            if (fb < 64u) {
                Dend = (int64_t)readlane_f64(Db, fb);
                return fb * K + (uint32_t)__builtin_amdgcn_readlane((int)bq, (int)fb);
            }
            Dend = (int64_t)readlane_f64(D, last);
            return len;
        }
        st = nst;
    }
}

// ---------------------------------------------------------------------------
// producers
// ---------------------------------------------------------------------------
// a lane's K consecutive adds and thresholds from the ring, positions i0 ..
// i0 + K - 1, in whole 16-byte granules: K / 2 or K / 2 + 1 ds_read_b128 per
// array instead of K ds_read_b64 (i0's parity must be wave-uniform: the
// callers' i0 is a window start plus an even offset)
__device__ __attribute__((always_inline)) inline void ring_read_k(const ChainShared& sh, uint32_t i0,
                                                                 double (&ra)[CH_K], double (&rt)[CH_K]) {
    constexpr int K = CH_K;
    if constexpr (K % 2 == 0) {
        const uint32_t g0 = i0 >> 1;
        if ((i0 & 1u) == 0u) {
#pragma unroll
            for (int j = 0; j < K / 2; j++) {
                const double2 a2 = sh.r_add[ring_slot(g0 + j)], t2 = sh.r_th[ring_slot(g0 + j)];
                ra[2 * j] = a2.x;
                ra[2 * j + 1] = a2.y;
                rt[2 * j] = t2.x;
                rt[2 * j + 1] = t2.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j <= K / 2; j++) {
                const double2 a2 = sh.r_add[ring_slot(g0 + j)], t2 = sh.r_th[ring_slot(g0 + j)];
                if (j > 0) {
                    ra[2 * j - 1] = a2.x;
                    rt[2 * j - 1] = t2.x;
                }
                if (j < K / 2) {
                    ra[2 * j] = a2.y;
                    rt[2 * j] = t2.y;
                }
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < K; q++) {
            ra[q] = ring_add(sh, i0 + q);
            rt[q] = ring_th(sh, i0 + q);
        }
    }
}


// Summary of tile t of the window [pfirst, pfirst + pcnt) at scale P, into
// tile[buf][t], its near list and per-lane near ranks.  State-free except for
// dmax, an estimated bound on the window's states that narrows the near band
// (|delta| <= (|D| + |D'|) 2^-53); the chain checks the bound per tile.
template <int MODE>
__device__ __attribute__((always_inline)) inline void ch_produce(ChainShared& sh, uint32_t buf, uint32_t t,
                                                                uint32_t pfirst, uint32_t pcnt, double P,
                                                                double dmax) {
    constexpr int K = CH_K;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t toff = t * CH_TILE;
    if (toff >= pcnt) return;
    const uint32_t myoff = toff + lane * K;
    const uint32_t nv = myoff < pcnt ? ((pcnt - myoff) < (uint32_t)K ? (pcnt - myoff) : (uint32_t)K) : 0u;
    const uint32_t i0 = pfirst + myoff;
    // near band: a step is far when |frac(add P)| + |delta| < 1/2, with
    // delta = (eta + eps) P the rounding errors of x = strtod(D) and of
    // sum = x + add, |eta|, |eps| <= ulp / 2.  Every state is <= dmax, so x and
    // sum are <= dmax / P = f 2^e (f in [1/2, 1)) and their ulp <= 2^(e - 53):
    // |delta| <= 2^(e - 53) P -- the binade bound, up to 2x tighter than
    // (|D| + |D'|) 2^-53 (which the binary mode keeps)
    double band = 2.0 * dmax * 0x1.0000001p-53;
    if (MODE == QM_DEC) {
        // e: the binade of dmax / P, from the operands' binades and mantissas
        // (no division); the margin only ever picks the binade above
        int ed, ep;
        const double md = frexp(dmax, &ed), mp = frexp(P, &ep);
        const int e = ed - ep + (md * 0x1.00001p+0 >= mp ? 1 : 0);
        band = ldexp(P, e - 53) * 0x1.0000001p+0;
    }
    const double lim = 0.5 - (band + 0x1p-40);
    const double PY = P * CH_YSCALE;
    double add[K], th[K], cb[K];
    double cum = 0.0, ymin = __builtin_inf(), cmax = -__builtin_inf(), cmin = __builtin_inf();
    uint32_t nearm = 0, evq = NO_STOP;
    double ra[K], rt[K];
    ring_read_k(sh, i0, ra, rt);
    // branch-free: every ring slot is readable (positions past the window
    // read stale slots, masked by v), and the bounds use v_max / v_min on
    // values that are never NaN (no canonicalization)
#pragma unroll
    for (int q = 0; q < K; q++) {
        const bool v = (uint32_t)q < nv;
        const double araw = ra[q];
        const double h = rt[q];
        const double a = v ? araw : 0.0;
        add[q] = a;
        th[q] = h;
        cb[q] = cum;
        const double pr = a * P;
        const bool ok = fabs(pr) < 0x1p49;                 // else NaN (expired key) or huge: a stop
        evq = (!ok && evq == NO_STOP) ? (uint32_t)q : evq;
        const double prs = ok ? pr : 0.0;                  // rint on every lane (no branch)
        const double rr = rint(prs);
        if (MODE == QM_DEC) {
            const double fr = (prs - rr) + __builtin_fma(a, P, -pr);  // a*P - rr, one rounding (ok lanes)
            nearm |= (ok && fabs(fr) > lim) ? 1u << q : 0u;
        } else {
            nearm |= (ok && fabs(prs - rr) == 0.5) ? 1u << q : 0u;   // exact tie: parity decides
        }
        cum += rr;                                                    // exact: |cum| < 2^52
        const double mx = vmax_f64(cmax, cum), mn = vmin_f64(cmin, cum), ym = vmin_f64(ymin, h * PY - cum);
        cmax = v ? mx : cmax;
        cmin = v ? mn : cmin;
        ymin = v ? ym : ymin;
    }
    // the tile prefix: in doubles when every lane's sum is below 2^46 (the
    // tile's then below 2^52: exact), else in int64
    double ex, inclD;
    int64_t inclS;    // the exact tile sum (T.S: the nominal tile starts and runs' end states)
    if (__ballot(!(fabs(cum) < 0x1p46)) == 0ull) {
        inclD = wave_incl_scan_f64(cum);
        ex = inclD - cum;
        inclS = (int64_t)inclD;
    } else {
        const int64_t Si = (int64_t)cum;
        const int64_t incl = wave_incl_scan_i64(Si);
        ex = (double)(incl - Si);
        inclD = (double)incl;
        inclS = incl;
    }
    // the tile's bounds: lane 63 holds the reductions (no broadcast)
    const double ymin_t = wave_fold_f64(ymin - ex, __builtin_inf(), [](double x, double y) { return vmin_f64(x, y); });
    const double cmax_t = wave_fold_f64(ex + cmax, -__builtin_inf(), [](double x, double y) { return vmax_f64(x, y); });
    const double cmin_t = wave_fold_f64(ex + cmin, __builtin_inf(), [](double x, double y) { return vmin_f64(x, y); });
    const uint32_t ev_t = wave_scan_u32(evq != NO_STOP ? lane * K + evq : NO_STOP, 0xffffffffu,
                                        [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    const uint32_t ncnt = (uint32_t)__popc(nearm);
    const uint32_t ninc = wave_scan_u32(ncnt, 0u, [](uint32_t x, uint32_t y) { return x + y; });
    sh.ne_rank[buf][t][lane] = (uint16_t)(ninc - ncnt);
    if (nearm) {
        uint32_t k = ninc - ncnt;
#pragma unroll
        for (int q = 0; q < K; q++) {
            if ((nearm >> q) & 1u) {
                if (k < (uint32_t)CH_NE) {
                    sh.ne_pred[buf][t][k] = ex + cb[q];
                    sh.ne_add[buf][t][k] = add[q];
                    sh.ne_th[buf][t][k] = th[q];
                }
                k++;
            }
        }
    }
    if (lane == 63) {
        ChTile& T = sh.tile[buf][t];
        T.S = inclS;
        T.Sd = inclD;
        T.ymin = ymin_t;
        T.cmax = cmax_t;
        T.cmin = cmin_t;
        T.dmax = dmax;
        T.ev = ev_t;
        T.nc = ninc;
    }
}

// The chain window's likely regime exit (decimal mode; every producer wave
// computes the same): the first tile whose bounds admit an exit at the
// nominal state, the first nominal exit in it (nominal digit sums, no %.14g
// steps); the exit step's
// result (sum - th when it allows, else sum), carried on through the serial
// steps that follow an allow or a balance <= 0, decides the decade E.  A
// guess: the chain adopts the window only if its exact replay agrees
// (ch_segment).
// floor(log10 x), out of line.  Inlined into ch_predict, log10's polynomial
// constants were hoisted out of the round loop and held in VGPRs through the
// whole kernel, for a step the guess reaches only when it has found an exit.
// Same function, same result; k_tb_chain's own registers went from 256 to 248
// and configs[1] from 3.22-3.25 to 3.28-3.30e9 (profiles/r7a_ab_log10_ool.txt).
__device__ __attribute__((noinline)) int ch_floor_log10(double x) { return (int)floor(log10(x)); }

__device__ __attribute__((always_inline)) inline ChSpec ch_predict(const ChainShared& sh, const ChState& s, double P,
                                                                  double R, uint32_t j1, bool xd) {
    constexpr int K = CH_K;
    ChSpec sp{0u, 0u, 0u, 0u, 0, 0.0};
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t nt = (s.ccnt + CH_TILE - 1) / CH_TILE;
    const bool tv = lane < nt;
    // (a guess: nominal sums in doubles, exact below 2^53, and only a guess
    // beyond -- the chain adopts the window only if its exact replay agrees)
    const ChTile T = sh.tile[s.cbuf][tv ? lane : 0u];
    const double Sl = tv ? T.Sd : 0.0;
    const double dD = (double)s.D + (wave_incl_scan_f64(Sl) - Sl);   // nominal start of tile t
    const bool cand = tv && (T.ev != NO_STOP || !(dD + T.cmax < (double)DEC_HI) ||
                             !(dD + T.cmin >= (double)DEC_LO + 1.0) || !(dD + 3.0 < T.ymin));
    const uint64_t cm = __ballot(cand);
    if (!cm) return sp;
    const uint32_t c = first_lane(cm);
    const double Dc = readlane_f64(dD, c);
    const uint32_t p0 = s.cfirst + c * CH_TILE;
    const uint32_t clen = (s.ccnt - c * CH_TILE) < CH_TILE ? (s.ccnt - c * CH_TILE) : CH_TILE;
    const uint32_t off = lane * K;
    const uint32_t nv = off < clen ? ((clen - off) < (uint32_t)K ? (clen - off) : (uint32_t)K) : 0u;
    double add[K], th[K];
    ring_read_k(sh, p0 + off, add, th);
    double S = 0.0;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const bool v = (uint32_t)q < nv;
        add[q] = v ? add[q] : 0.0;
        th[q] = v ? th[q] : __builtin_inf();
        const double pr = add[q] * P;
        if (fabs(pr) < 0x1p49) S += rint(pr);
    }
    // nominal states (integer digits, no %.14g step): an exit where the sum
    // reaches th (D + add P >= th P) or the next digits leave the decade
    double D = Dc + (wave_incl_scan_f64(S) - S);
    uint32_t bq = NO_STOP;
    double D_b = 0.0, a_b = 0.0, th_b = 0.0;
#pragma unroll
    for (int q = 0; q < K; q++) {
        const double pr = add[q] * P;
        const double Dn = D + rint(pr);
        const bool stop = (uint32_t)q < nv && bq == NO_STOP &&
                          (!(fabs(pr) < 0x1p49) || !(D + pr < th[q] * P) || !(Dn < (double)DEC_HI) ||
                           !(Dn >= (double)DEC_LO));
        bq = stop ? (uint32_t)q : bq;
        D_b = stop ? D : D_b;
        a_b = stop ? add[q] : a_b;
        th_b = stop ? th[q] : th_b;
        D = Dn;
    }
    const uint32_t fb = first_lane(__ballot(bq != NO_STOP));
    if (fb >= 64u) return sp;
    uint32_t first = p0 + fb * K + (uint32_t)__builtin_amdgcn_readlane((int)bq, (int)fb) + 1u;
    const double sum = readlane_f64(D_b, fb) / P + readlane_f64(a_b, fb), thv = readlane_f64(th_b, fb);
    const bool allow = sum >= thv;
    double post = allow ? sum - thv : sum;
    if (first >= j1 || !(post == post)) return sp;
    if (xd) {
        // multi-decade windows take any state after the exiting step: the
        // window starts right after it, its plan from the guessed state
        sp.valid = 1u;
        sp.first = first;
        sp.cnt = (j1 - first) < CH_W ? (j1 - first) : CH_W;
        sp.v0 = post;
        return sp;
    }
    if (allow || !(post > 0.0)) {
        // the serial steps go on after an allow (the next step too) and while
        // the balance is at or below zero (off the fast decades): they end
        // after the first step that leaves it positive -- the first positive
        // partial sum of the next adds, if no step on the way allows or
        // expires and the serial steps of one round reach it
        const uint32_t p = first + lane;
        const bool ok = p < j1 && lane < (uint32_t)CH_SERIAL - 1u;
        const double ad = ok ? ring_add(sh, p) : 0.0;
        const double tv2 = ok ? ring_th(sh, p) : __builtin_inf();
        double c = ad;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const double u = __shfl_up(c, o, 64);
            c = lane >= (uint32_t)o ? c + u : c;
        }
        const double vsum = post + c;
        const uint32_t fp = first_lane(__ballot(ok && vsum > 0.0));
        const uint32_t fx = first_lane(__ballot(ok && (vsum >= tv2 || !(ad == ad))));
        if (fp >= 64u || fx <= fp) return sp;
        post = readlane_f64(vsum, fp);
        first += fp + 1u;
        if (first >= j1) return sp;
    }
    if (!(post < 1e12)) return sp;
    const int e0 = ch_floor_log10(post);
#pragma unroll
    for (int d = -1; d <= 1; d++) {
        const int e = e0 + d, k = 13 - e;
        if (sp.valid || k < 1 || k > 22) continue;
        bool ge_lo;
        const double Dn = round_scaled_Pd(post, rlq::pow10_exact(k), ge_lo);
        if (ge_lo && Dn < (double)DEC_HI) {
            sp.valid = 1u;
            sp.E = e;
        }
    }
    sp.first = first;
    sp.cnt = (j1 - first) < CH_W ? (j1 - first) : CH_W;
    return sp;
}

}  // namespace rl
