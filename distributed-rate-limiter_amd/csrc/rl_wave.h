// rl_wave.h -- wave64 helpers of the grouping and replay kernels: the LDS
// barrier, DPP scans and reductions (row shifts and row broadcasts, GFX9
// family), lane reads.  No LDS round trips, no state.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl {

// Barrier for LDS hand-offs only.  __syncthreads() is a workgroup-scope
// fence on gfx950 and waits for every outstanding global store (vmcnt(0));
// the replay rounds scatter results to HBM between barriers and must not wait
// for them.  LDS writes are complete once lgkmcnt reaches 0.
__device__ inline void lds_barrier() {
    __asm__ volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// 64-bit wave64 inclusive scan with DPP row shifts and row broadcasts (GFX9
// family): 6 steps of two v_mov_dpp + a 64-bit add, no LDS round trips.
template <int CTRL, int ROW_MASK>
__device__ inline int64_t dpp_add_step(int64_t inc) {
    uint32_t lo = (uint32_t)inc, hi = (uint32_t)((uint64_t)inc >> 32);
    // old = 0: lanes with no source (or outside ROW_MASK) contribute 0
    uint32_t slo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, CTRL, ROW_MASK, 0xf, false);
    uint32_t shi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, CTRL, ROW_MASK, 0xf, false);
    return inc + (int64_t)(((uint64_t)shi << 32) | slo);
}

__device__ inline int64_t wave_incl_scan_i64(int64_t v) {
    v = dpp_add_step<0x111, 0xf>(v);   // row_shr:1
    v = dpp_add_step<0x112, 0xf>(v);   // row_shr:2
    v = dpp_add_step<0x114, 0xf>(v);   // row_shr:4
    v = dpp_add_step<0x118, 0xf>(v);   // row_shr:8
    v = dpp_add_step<0x142, 0xa>(v);   // row_bcast:15 -> rows 1, 3
    v = dpp_add_step<0x143, 0xc>(v);   // row_bcast:31 -> rows 2, 3
    return v;
}

// generic 32-bit wave64 inclusive scan with DPP; `op(self, earlier)`
template <int CTRL, int RM>
__device__ inline uint32_t dpp32(uint32_t v, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, RM, 0xf, false);
}
template <typename Op>
__device__ inline uint32_t wave_scan_u32(uint32_t v, uint32_t ident, Op op) {
    v = op(v, dpp32<0x111, 0xf>(v, ident));
    v = op(v, dpp32<0x112, 0xf>(v, ident));
    v = op(v, dpp32<0x114, 0xf>(v, ident));
    v = op(v, dpp32<0x118, 0xf>(v, ident));
    v = op(v, dpp32<0x142, 0xa>(v, ident));
    v = op(v, dpp32<0x143, 0xc>(v, ident));
    return v;
}
__device__ inline uint32_t wave_min_u32(uint32_t v) {
    v = wave_scan_u32(v, 0xffffffffu, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ inline int64_t readlane_i64(int64_t v, uint32_t l) {
    uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), (int)l);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// ---------------------------------------------------------------------------
// wave helpers (DPP row shifts / broadcasts, GFX9 family)
// ---------------------------------------------------------------------------
template <int CTRL, int RM>
__device__ inline double dpp_f64(double v, double old) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v), o = __builtin_bit_cast(uint64_t, old);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)o, (int)(uint32_t)b, CTRL, RM, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(o >> 32), (int)(uint32_t)(b >> 32), CTRL,
                                                              RM, 0xf, false);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
__device__ inline double readlane_f64(double v, uint32_t l) {
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), (int)l);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// max / min of two doubles that are never NaN: one v_max_f64 / v_min_f64 (the
// compiler's fmax/fmin canonicalize both inputs first, three instructions)
__device__ inline double vmax_f64(double a, double b) {
    double r;
    __asm__ volatile("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));   // volatile: never sunk into a branch
    return r;
}
__device__ inline double vmin_f64(double a, double b) {
    double r;
    __asm__ volatile("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <typename Op>
__device__ inline double wave_reduce_f64(double v, double ident, Op op) {
    v = op(v, dpp_f64<0x111, 0xf>(v, ident));
    v = op(v, dpp_f64<0x112, 0xf>(v, ident));
    v = op(v, dpp_f64<0x114, 0xf>(v, ident));
    v = op(v, dpp_f64<0x118, 0xf>(v, ident));
    v = op(v, dpp_f64<0x142, 0xa>(v, ident));
    v = op(v, dpp_f64<0x143, 0xc>(v, ident));
    return readlane_f64(v, 63);
}
// inclusive wave scan of doubles (DPP, as wave_incl_scan_i64)
template <int CTRL, int RM>
__device__ inline double dpp_addf_step(double v) {
    return v + dpp_f64<CTRL, RM>(v, 0.0);
}
__device__ inline double wave_incl_scan_f64(double v) {
    v = dpp_addf_step<0x111, 0xf>(v);
    v = dpp_addf_step<0x112, 0xf>(v);
    v = dpp_addf_step<0x114, 0xf>(v);
    v = dpp_addf_step<0x118, 0xf>(v);
    v = dpp_addf_step<0x142, 0xa>(v);
    v = dpp_addf_step<0x143, 0xc>(v);
    return v;
}
// the same reduction, left in lane 63 only (its caller reads it there)
template <typename Op>
__device__ inline double wave_fold_f64(double v, double ident, Op op) {
    v = op(v, dpp_f64<0x111, 0xf>(v, ident));
    v = op(v, dpp_f64<0x112, 0xf>(v, ident));
    v = op(v, dpp_f64<0x114, 0xf>(v, ident));
    v = op(v, dpp_f64<0x118, 0xf>(v, ident));
    v = op(v, dpp_f64<0x142, 0xa>(v, ident));
    v = op(v, dpp_f64<0x143, 0xc>(v, ident));
    return v;
}
__device__ inline int64_t readfirstlane_i64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ inline uint32_t first_lane(uint64_t m) { return m ? (uint32_t)__ffsll((unsigned long long)m) - 1 : 64u; }
// arr[i] of a small register array without dynamic indexing (which would
// place the array in scratch memory)
template <typename T, int N>
__device__ inline T pick(const T (&arr)[N], uint32_t i) {
    T r = arr[0];
#pragma unroll
    for (int u = 1; u < N; u++) r = i == (uint32_t)u ? arr[u] : r;
    return r;
}

}  // namespace rl
