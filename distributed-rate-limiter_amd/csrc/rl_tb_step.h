// rl_tb_step.h -- one token-bucket script step, in every form the replay
// takes it: the state-free inputs of a request (TbPre), the plain step on the
// stored double (tb_chain_step), the stored value as digits in a decade or
// binade (TbQ, tb_quant), the general step from digits (tb_eval), the exact
// step in a fast mode (tb_step_d) and the common Redis-7 serial step
// (tb_dec_step).  Arithmetic on one request only: nothing here knows a wave,
// a window or the chain's shape (rl_tb_chain.h has the map of the headers).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rl_batch.h"
#include "rl_q14.h"
#include "rl_semantics.h"
#include "rl_table.h"

namespace rl {

// State-independent token-bucket quantities of each request (sorted order),
// computed in the permute pass: the previous request of the same key is the
// previous sorted position (or, for a segment head, the table entry).  The
// rest of the script's state-free inputs are computed where they are used:
// reset_at in the finish (tb_result_reset), last_refill and the TTL of a
// segment's last request at its end (tb_store_end).
struct TbPre {
    double* add;       // elapsed * refill_rate (tokenbucket.go:36-37); NaN when HMGET finds
                       // no live key (tokenbucket.go:31-34: tokens = capacity, add = 0).
                       // A segment head's add depends on the table state, so the
                       // replay computes it (tb_head_add); k_permute fills the rest
    double* th;        // min(capacity, float64(n)): the script step allows or clamps
                       // exactly when capacity-free sum >= th (tokenbucket.go:38-43)
};

__device__ inline int64_t req_server_ms(const ReqArgs& a, uint32_t i, int64_t t) {
    return a.sms ? a.sms[i] : floor_div(t, 1000000LL);
}

// the stored state after a token-bucket segment's last request j: HSET
// last_refill = tostring(now) and the EXPIRE (tokenbucket.go:48-49)
__device__ inline void tb_store_end(TbEntry* e, double tok, uint32_t j, const CfgDev* cfgs, int32_t profile,
                                    const ReqArgs& a) {
    const int64_t t = a.ts[j];
    e->tok = tok;
    e->last = lua_tostring_roundtrip((double)t / 1e9, profile);
    e->when = expire_when(cfgs[a.cfg[j]].ttl_tb, req_server_ms(a, j, t));
}

// token bucket: replay writes the decision and the unquantized tokens only;
// remaining/retry_after/reset_at are functions of (decision, tokens, n, time,
// config) that the finish evaluates (tokenbucket.go:114-130,161-165;
// tb_result below)
__device__ inline void write_out_tb(const ReqArgs& a, uint32_t i, uint8_t dec, double tokens) {
    a.dec[i] = dec;
    a.tok[i] = tokens;
}

// one token-bucket script execution on precomputed inputs (tb_step's
// state-dependent part: tokenbucket.go:32-51 + 114-130)
__device__ inline Out tb_chain_step(double& tok, bool alive, double add, int64_t n, int64_t reset_at,
                                    const CfgDev& c, int32_t profile) {
    Out o;
    const double capacity = c.limit_d;
    double tokens = alive ? tok : capacity;
    double sum = tokens + add;
    tokens = (sum < capacity) ? sum : capacity;           // math.min(capacity, sum)
    bool allowed = false;
    if (tokens >= (double)n) { tokens = tokens - (double)n; allowed = true; }
    tok = lua_tostring_roundtrip(tokens, profile);
    int64_t rem = go_f2i(floor(tokens));
    o.tokens = tokens;
    o.decision = allowed ? DEC_ALLOWED : DEC_DENIED;
    o.remaining = rem;
    o.reset_at = reset_at;
    o.retry = 0;
    if (!allowed) {
        int64_t need = wsub(n, rem);
        double w = need == 1 ? c.inv_rate : (double)need / c.rate;   // tokensNeeded / refillRate
        int64_t d = go_f2i(w * 1e9);
        o.retry = d < 0 ? 0 : d;
    }
    return o;
}

// add of a segment head: its predecessor is the table entry (the state after
// the previous batch), read at replay time
__device__ inline double tb_head_add(const TbEntry* e, uint32_t j0, const CfgDev* cfgs, int32_t profile,
                                     const ReqArgs& a) {
    const CfgDev& C = cfgs[a.cfg[j0]];
    const double now = (double)a.ts[j0] / 1e9;
    return key_alive(e->when, req_server_ms(a, j0, a.ts[j0]), profile) ? (now - e->last) * C.rate
                                                                          : __builtin_nan("");
}

struct TbQ {
    int64_t D;
    int32_t E;
};

__device__ inline TbQ tb_quant(double x, int32_t profile) {
    if (x == 0.0 || !(x - x == 0.0)) return TbQ{0, 0};
    if (profile == PROFILE_REDIS7) {
        double ax = x < 0 ? -x : x;
        int64_t D;
        int E;
        if (!rlq::dec14_fast(ax, D, E)) rlq::dec14_slow(ax, D, E);
        return TbQ{x < 0 ? -D : D, E};
    }
    int e;
    double m = frexp(x, &e);
    return TbQ{(int64_t)ldexp(m, 53), e - 53};
}

__device__ inline double tb_value(int64_t D, int32_t E, int32_t profile) {
    if (D == 0) return 0.0;
    if (profile == PROFILE_REDIS7) {
        double v = rlq::dec14_value(D < 0 ? -D : D, E);
        return D < 0 ? -v : v;
    }
    return ldexp((double)D, E);
}

constexpr double TAU_DEC = 0.03;   // > 0.0222: far lanes are exact by the bound

enum : int { QM_NONE = 0, QM_DEC = 1, QM_BIN = 2, QM_XDEC = 3 };   // QM_XDEC: rl_tb_xdec.h

struct TbEval {
    double tokens;
    bool allowed;
    bool clamped;
    bool inrange;   // Dact is the canonical stored representation in this decade
    int64_t Dact;
};

// the script step from a stored state given as digits Dpred in (mode, E)
__device__ inline TbEval tb_eval(int mode, int64_t Dpred, int32_t E, double P, double R, bool alive, double add,
                                 double cap, double nd, int32_t profile) {
    TbEval v;
    double T;
    if (!alive) T = cap;
    // strtod("D e(E-13)"): |D| < 2^47 and 10^k (k <= 22) are exact doubles,
    // so one correctly rounded division is strtod's result (Clinger's fast
    // path); RN is sign-symmetric
    else if (mode == QM_DEC) T = (double)Dpred / P;
    else if (mode == QM_BIN) T = (double)Dpred * R;                      // exact: R = 2^E
    else T = tb_value(Dpred, E, profile);
    const double sum = T + add;
    v.clamped = !(sum < cap);
    double tokens = v.clamped ? cap : sum;                               // math.min(capacity, sum)
    v.allowed = tokens >= nd;
    if (v.allowed) tokens = tokens - nd;
    v.tokens = tokens;
    v.Dact = 0;
    v.inrange = false;
    const double at = tokens < 0.0 ? -tokens : tokens;                   // %.14g is sign-symmetric
    if (mode == QM_DEC) {
        if (at > 0.0 && at * P < 1.4e14) {
            v.Dact = rlq::round_scaled_P(at, P);
            // the exact at*P must not be below 1e13: [1e13 - 0.5, 1e13) rounds to
            // 1e13 here, while %.14g keeps 14 digits of the decade below
            const double p = at * P, err = __builtin_fma(at, P, -p);
            const bool ge_lo = p > 1e13 || (p == 1e13 && err >= 0.0);
            v.inrange = ge_lo && v.Dact < 100000000000000LL;
        }
    } else if (mode == QM_BIN) {
        const double w = at * P;                                         // exact scaling
        if (w >= 4503599627370496.0 && w < 9007199254740992.0) {
            v.Dact = (int64_t)w;
            v.inrange = (double)v.Dact == w;
        }
    }
    if (tokens < 0.0) v.Dact = -v.Dact;
    return v;
}

constexpr int64_t DEC_LO = 10000000000000LL, DEC_HI = 100000000000000LL;
constexpr int64_t BIN_LO = 1LL << 52, BIN_HI = 1LL << 53;
constexpr uint32_t NO_STOP = 0xffffffffu;

// ---------------------------------------------------------------------------
// exact step in a fast mode
// ---------------------------------------------------------------------------
// RNE(x * P) as an exact integer-valued double (x*P < 2^52), P = 10^k exact;
// ge_lo: the exact x*P >= 1e13, i.e. x is not below the decade (a value in
// [1e13 - 0.5, 1e13) units rounds to 1e13 here but %.14g formats it with 14
// digits of the decade below)
__device__ inline double round_scaled_Pd(double x, double P, bool& ge_lo) {
    const double p = x * P;
    const double err = __builtin_fma(x, P, -p);       // x*P == p + err exactly
    ge_lo = (p > (double)DEC_LO) | ((p == (double)DEC_LO) & (err >= 0.0));
    // RNE of p, then the exact product decides a tie of p: p - rint(p) is
    // +-1/2 exactly only when p's fraction is 1/2 (p < 2^52 has ulp <= 1/2),
    // and |err| <= ulp(p)/2 cannot move a non-tie across the half
    double d = rint(p);
    const double h = p - d;                           // exact
    d += ((h == 0.5) & (err > 0.0)) ? 1.0 : 0.0;
    d -= ((h == -0.5) & (err < 0.0)) ? 1.0 : 0.0;
    return d;
}

// x / P correctly rounded (as IEEE division) for an integer-valued |x| < 2^47,
// P = 10^k (1 <= k <= 22, exact) and R within 2^-52 relative of 1/P (RN(1/P),
// or RN(1/10^j) times an exact 10^(j-k), rounded), in five dependent
// operations instead of the division's eleven.  q0 = RN(x R) is within 3 ulp
// of x/P and q1 = q0 + r R (r = x - q0 P, one rounding) within 1/2 ulp +
// 1e-15 ulp; the residual r1 = x - q1 P is then exact (|r1| <= 0.51 ulp(q1) P
// < 2^53 units of ulp(q1) ulp(P), as every 10^k has a mantissa below 2), and
// q1 + r1 R is within 0.51 ulp 2^-52 = 1.1e-16 ulp of x/P.  x/P = x /
// (2^k 5^k) with x an integer below 2^47 is never a rounding midpoint and lies
// at least ulp / (2 5^k) >= 2.1e-16 ulp from one (k <= 22), so the final
// rounding is RN(x/P).
// Checked against IEEE division on 1.3e9 random (x, k), with both reciprocals:
// scripts/div_p10_check.c.
__device__ __attribute__((always_inline)) inline double div_p10(double x, double P, double R) {
    const double q0 = x * R;
    const double q1 = __builtin_fma(__builtin_fma(-q0, P, x), R, q0);
    return __builtin_fma(__builtin_fma(-q1, P, x), R, q1);
}

// The live-key step from stored digits Dpred (exact integer-valued double,
// positive, in the decade/binade of P) in a fast mode: tokens (the
// unquantized double) and the next stored digits D' -- NaN when the step
// leaves the regime: sum >= th (= min(capacity, n): clamp or allow), D' out of
// the decade, or an expired key (add NaN).
template <int MODE>
__device__ inline double tb_step_d(double Dpred, double P, double R, double add, double th, double& tokens) {
    // strtod("D e(E-13)"): D < 2^47 and P = 10^k (k <= 22) are exact doubles,
    // so one correctly rounded division is strtod's result (Clinger's fast
    // path): div_p10 with R = RN(1/P) (mode_scale)
    const double T = MODE == QM_DEC ? div_p10(Dpred, P, R) : Dpred * R;   // binary: exact, R = 2^E
    const double sum = T + add;
    tokens = sum;
    double Dn;
    if (MODE == QM_DEC) {
        bool ge_lo;
        Dn = round_scaled_Pd(sum, P, ge_lo);                        // %.14g of a positive sum
        if (!(ge_lo & (Dn < (double)DEC_HI))) Dn = __builtin_nan("");
    } else {
        Dn = sum * P;                                               // exact scaling
        if (!(Dn >= (double)BIN_LO && Dn < (double)BIN_HI && Dn == floor(Dn))) Dn = __builtin_nan("");
    }
    if (!(sum < th)) Dn = __builtin_nan("");
    return Dn;
}

__device__ inline int32_t fast_mode(int64_t D, int32_t E, int32_t profile) {
    if (profile == PROFILE_REDIS7)
        return (D >= DEC_LO && D < DEC_HI && 13 - E >= 1 && 13 - E <= 22) ? QM_DEC : QM_NONE;
    return (D >= BIN_LO && D < BIN_HI && E > -1000 && E < 900) ? QM_BIN : QM_NONE;
}
__device__ inline void mode_scale(int32_t mode, int32_t E, double& P, double& R) {
    if (mode == QM_DEC || mode == QM_XDEC) {   // XDEC: the window's floor scale 10^(13 - F)
        P = rlq::pow10_exact(13 - E);
        R = 1.0 / P;                       // RN(1/P): the decimal step's div_p10
    } else {
        P = ldexp(1.0, -E);
        R = ldexp(1.0, E);
    }
}

// One Redis-7 script step in decimal mode on the stored state as doubles:
// digits Dd (an integer-valued double, |Dd| in [1e13, 1e14), or 0) at scale
// P = 10^(13 - E), k = 13 - E in [1, 22].  The common serial step -- the key
// alive, the sum below th (no allow, no clamp) -- with %.14g's decade chosen
// on the exact scaled value (as dec14_fast: a >= 10^E and a < 10^(E+1) tested
// on a*P = p + err exactly; digits RNE, a carry to 1e14 moves up a decade) at
// the same, the next or the one after next decade.  False when the step needs
// the general path (tb_eval): sum >= th, or a decade outside k in [1, 22] or
// more than two away.  Sign-symmetric like %.14g and strtod.  The same
// arithmetic as tb_eval(QM_DEC) + its decade search, in about 25 dependent
// double operations instead of the general path's integer conversions,
// table lookups and branches.
__device__ __attribute__((always_inline)) inline bool tb_dec_step(double& Dd, int32_t& E, double& P, double add,
                                                                 double th, double& tokens) {
    const double T = Dd / P;                     // strtod: one correctly rounded division (Clinger)
    const double sum = T + add;
    if (!(sum < th)) return false;               // allow or clamp: n and the capacity decide
    tokens = sum;
    const double a = sum < 0.0 ? -sum : sum;
    if (a == 0.0) {                              // tostring(0) == "0": T = 0 at any scale
        Dd = 0.0;
        return true;
    }
    double Pn = P;
    int32_t En = E;
#pragma unroll
    for (int g = 0; g < 3; g++) {
        const double p = a * Pn, err = __builtin_fma(a, Pn, -p);    // a*Pn == p + err exactly
        const bool lo_ok = (p > 1e13) | ((p == 1e13) & (err >= 0.0));
        const bool hi_ok = (p < 1e14) | ((p == 1e14) & (err < 0.0));
        if (lo_ok & hi_ok) {
            double d = rint(p);                  // RNE of p; the exact product decides a tie of p
            const double h = p - d;
            d += ((h == 0.5) & (err > 0.0)) ? 1.0 : 0.0;
            d -= ((h == -0.5) & (err < 0.0)) ? 1.0 : 0.0;
            if (d == 1e14) {                     // rounding carried into the next decade
                d = 1e13;
                En += 1;
                Pn = Pn / 10.0;                  // exact: a smaller power of ten
            }
            if (En > 12 || En < -9) return false;
            Dd = sum < 0.0 ? -d : d;
            E = En;
            P = Pn;
            return true;
        }
        if (!lo_ok) {
            En -= 1;
            Pn = Pn * 10.0;
        } else {
            En += 1;
            Pn = Pn / 10.0;
        }
        if (En > 12 || En < -9) return false;    // 13 - E outside [1, 22]
    }
    return false;
}

}  // namespace rl
