// rl_tb_stamps.h -- the replay kernels' debug words by name, and the
// diagnostic stamps of the stamps build.
//
// The replay kernels count into 88 per-batch debug words (`dbg`, the batch
// set's control words; rl_engine_debug_words copies them out).  DbgWord names
// every word once.  Words marked P are written by the product build; words
// marked S only by the diagnostic build (-DRL_STAMPS, `make stamps`) and are 0
// otherwise.
//
// The stamps themselves -- shader-clock sums per wave role and phase of the
// chain, the chain round's pipeline model, the replay's tail -- live in the
// three objects below, one per scope that keeps stamp state: a wave's
// ch_segment (ChStamps), one ch_resolve (ChResolveStamps), a thread's
// replay_rest (ReplayStamps).  Each method marks one site and is named after
// it.  In the product build the objects are empty and so are their methods:
// the kernels call them unconditionally and carry no #ifdef.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl {

// The numeric values are an interface: bench.py, tests/test_bench_helpers.py,
// tests/test_chain_directed_gpu.py, tests/test_chain_small_segments_gpu.py and
// scripts/hot_allow_stats.py read these words by number.  Never renumber.
// Cycles are shader clocks / 16, ticks the 10 ns realtime counter (low 32
// bits); "hot" means a chain segment of >= 65536 requests.
enum DbgWord : uint32_t {
    DBG_ROUNDS = 0,             // P  chain rounds, summed over the chain segments
    DBG_PASSES = 1,             // P  near fixed-point and exact-span passes of the chain
    DBG_ROUNDS_MAX = 2,         // P  rounds of the chain segment with the most rounds
    DBG_WIN_FULL = 3,           // P  chain windows resolved in full (DBG_WIN_FULL + ChOutcome::kind)
    DBG_WIN_STOP = 4,           // P  chain windows that ended at a regime exit
    DBG_WIN_PARTIAL = 5,        // P  chain windows committed in part
    DBG_WIN_FIRST = 6,          // P  rounds with no window to resolve yet: the first of a run of rounds
    DBG_ST_EXACT_CYC = 7,       // S  cycles in the hot chain's exactly replayed tiles
    DBG_SEG_TICKS_MAX = 8,      // P  the longest chain segment's replay, ticks
    DBG_SPEC_LATE_1 = 9,        // P  guessed windows rejected: the chain's exit ended 1 step after the guess
    DBG_SPEC_LATE_64 = 10,      // P  ... 2 to 64 steps after the guess
    DBG_ST_EXACT_PASSES = 11,   // S  passes of the hot chain's exactly replayed tiles
    DBG_LIGHT_TICKS_MAX = 12,   // P  the longest light phase of a block, ticks
    DBG_T_FIRST_START_INV = 13, // P  the first replay block's start, complemented (atomicMax finds the minimum)
    DBG_T_LAST_END = 14,        // P  the last replay block's end
    DBG_SPEC_OTHER = 15,        // P  guessed windows rejected for any other reason
    DBG_T_SEG_START = 16,       // P  the longest chain segment's start
    DBG_T_SEG_END = 17,         // P  the longest chain segment's end
    DBG_T_STAMP_BEFORE = 18,    // P  RL_STAMP_KERNELS=1: a one-lane kernel just before the replay (rl_engine.hip)
    DBG_T_STAMP_AFTER = 19,     // P  RL_STAMP_KERNELS=1: the same just after the replay
    DBG_EXACT_TILES = 20,       // P  one-decade tiles replayed exactly
    DBG_SERIAL_STEPS = 21,      // P  the chain's serial exact steps
    DBG_SPEC_ADOPTED = 22,      // P  guessed windows adopted as the next chain window
    DBG_SPEC_REJECTED = 23,     // P  guessed windows rejected (= [9] + [10] + [15])
    // S  [24 + 4 * role + k], hot segments: role 0 the chain wave (cycles of
    //    full rounds, stop / partial rounds, serial steps, the barrier), role 1
    //    producer wave 1 (produce, exit guess, windows guessed / 16, the
    //    barrier), role 2 the loader (load, -, -, the barrier)
    DBG_ST_ROLE_CYC = 24,
    DBG_ST_NEAR_CYC = 36,       // S  the hot chain's resolve up to the end of the near fixed point, cycles
    DBG_ST_NEAR_ENTRIES = 37,   // S  near entries of the hot chain's windows
    DBG_ST_NEAR_PASSES = 38,    // S  their fixed-point passes
    DBG_ST_NEAR_SETUP_CYC = 39, // S  the hot chain's resolve before the near fixed point, cycles
    DBG_ST_HW_ID = 40,          // S  [40 + wave] the HW_ID register of each wave of a hot segment's block
    DBG_ST_PLAN_CYC = 48,       // S  producer wave 1's plan (one-decade bound or multi-decade plan), cycles
    DBG_ST_PLAN_CALLS = 49,     // S  its ch_plan_w calls
    DBG_ST_PLAN_CALL_CYC = 50,  // S  cycles inside them
    DBG_ST_T_LAST_START = 51,   // S  the latest replay block start
    DBG_ST_T_HEAVY_END = 53,    // S  the latest end of a block's heavy phase
    DBG_ST_T_LIGHT_CLAIM = 54,  // S  the latest light claim that got work
    DBG_ST_HEAVY_TICKS_MAX = 56,// S  the longest one-wave heavy segment's replay, ticks
    DBG_ST_HEAVY_LEN = 57,      // S  its length
    DBG_X_WINDOWS = 60,         // P  multi-decade windows resolved
    DBG_X_FULL = 61,            // P  of them in full
    DBG_X_NEAR_PASSES = 62,     // P  their near fixed-point passes
    DBG_X_CYC = 63,             // P  the chain wave's cycles in ch_resolve_x
    DBG_WIN_SUMMARIZED_X = 64,  // P  windows the producers summarized multi-decade
    DBG_WIN_SUMMARIZED_DEC = 65,// P  windows the producers summarized one-decade (or binary)
    DBG_X_EXACT_TILES = 66,     // P  multi-decade tiles replayed exactly
    DBG_X_EXACT_PASSES = 67,    // P  their passes
    DBG_X_NEAR_ENTRIES = 68,    // P  near entries of the multi-decade windows
    DBG_X_UNCONVERGED = 69,     // P  multi-decade near groups stopped unconverged
    // S  [70 + k], hot segments: producer wave 1's produce cycles of one-decade /
    //    multi-decade windows (k = 0, 1) and their counts (2, 3); the chain
    //    wave's resolve cycles of one-decade / multi-decade windows (4, 5) and
    //    their counts (6, 7)
    DBG_ST_SPLIT = 70,
    DBG_ST_X_NEAR_CYC = 80,     // S  the multi-decade windows' share of [36]
    DBG_ST_X_EXACT_CYC = 81,    // S  the multi-decade windows' share of [7]
    DBG_ST_MODEL_2BUF = 82,     // S  the pipeline model's finish with two summary buffers, cycles
    DBG_ST_MODEL_3BUF = 83,     // S  ... with three
    DBG_ST_MODEL_MAX = 84,      // S  the rounds' max(producer, chain) work, summed
    DBG_ST_MODEL_CHAIN = 85,    // S  the chain's work, summed over the rounds
    DBG_ST_MODEL_PRODUCER = 86, // S  the slowest producer's work, summed over the rounds
    DBG_ST_ROUND_TOPS = 87,     // S  the chain wave's round tops (barrier exit to the role's work), cycles
};

#define RL_STAMP __device__ __attribute__((always_inline)) inline

#ifdef RL_STAMPS

// the shader clock into v, fenced against the scheduler
#define CH_T(v) do { __builtin_amdgcn_sched_barrier(0); (v) = __builtin_amdgcn_s_memtime(); \
                     __builtin_amdgcn_sched_barrier(0); } while (0)

// One wave's stamps of ch_segment.  Sh is ChainShared, whose wk[2] (the
// round's longest producer work, cycles / 16) exists in this build only.
struct ChStamps {
    // (producer wave 1 / chain wave, hot segments): producer cycles of
    // one-decade / multi-decade windows and their counts, chain resolve cycles
    // of one-decade / multi-decade windows and their counts (DBG_ST_SPLIT)
    uint64_t cx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t cplan = 0;   // producer wave 1: plan cycles
    uint64_t cpcall = 0;  // of which in ch_plan_w calls, npcall of them
    uint32_t npcall = 0;
    // pipeline model (chain wave, lane 0; cycles / 16): the finish times of the
    // producers' and the chain's work per round with two summary buffers (the
    // barrier schedule) and with three (producers one window further ahead)
    // (a wave's round work is measured from the previous barrier's exit, so
    // the round-top code every wave runs is in it)
    uint64_t gP = 0, gC = 0, fP = 0, fC = 0, fC2 = 0, bsum = 0, csum = 0, psum = 0, tr0 = 0, ttop = 0;
    uint64_t tq0 = 0, tp0 = 0;   // the open plan call's / produce's start
    uint32_t wr = 0;             // this wave's work of the round

    template <typename Sh>
    RL_STAMP void segment_begin(Sh& sh, uint32_t tid) {
        if (tid < 2) sh.wk[tid] = 0;
    }
    RL_STAMP void first_round() { CH_T(tr0); }
    // the round top: from the barrier's exit to here
    RL_STAMP void round_top(uint64_t t0) { ttop += t0 - tr0; }
    RL_STAMP void exit_guess(uint64_t t0, uint64_t& t1, uint64_t (&cyc)[4], uint32_t guessed) {
        CH_T(t1);
        cyc[1] += t1 - t0;          // producers: the exit guess
        cyc[2] += guessed;          // producers: windows guessed
    }
    RL_STAMP void plan_call_begin() { CH_T(tq0); }
    RL_STAMP void plan_call_end() {
        uint64_t tq1;
        CH_T(tq1);
        cpcall += tq1 - tq0;
        npcall++;
    }
    // the plan (one-decade bound or multi-decade plan), from the exit guess's end
    RL_STAMP void plan_end(uint64_t t1) {
        uint64_t tpl;
        CH_T(tpl);
        cplan += tpl - t1;
    }
    RL_STAMP void produce_begin() { CH_T(tp0); }
    RL_STAMP void produce_end(uint64_t t1, bool any, bool xdec) {
        if (any) {
            const int xk = xdec ? 1 : 0;
            cx[xk] += t1 - tp0;
            cx[2 + xk] += 1;
        }
    }
    RL_STAMP void resolve_end(uint64_t t0, uint64_t t1, bool xdec) {
        cx[4 + (xdec ? 1 : 0)] += t1 - t0;
        cx[6 + (xdec ? 1 : 0)] += 1;
    }
    // before the round's barrier; producer0: lane 0 of a producer wave
    template <typename Sh>
    RL_STAMP void round_end(Sh& sh, uint32_t par, uint64_t t0, bool producer0) {
        wr = (uint32_t)((t0 - tr0) >> 4);
        if (producer0) atomicMax(&sh.wk[par], wr);
    }
    // after it; chain0: lane 0 of the chain wave
    template <typename Sh>
    RL_STAMP void round_barrier_done(Sh& sh, uint32_t par, uint64_t t1, bool chain0) {
        tr0 = t1;
        if (chain0) {
            // producers of round r summarize window r, the chain of round r
            // resolves window r - 1; a buffer is free once its window is resolved
            const uint64_t pr = sh.wk[par], cr = wr;
            sh.wk[par] = 0;
            const uint64_t nP2 = max(gP, gC) + pr, nC2 = max(gC, gP) + cr;
            gP = nP2;
            gC = nC2;
            const uint64_t nP3 = max(fP, fC2) + pr, nC3 = max(fC, fP) + cr;
            fC2 = fC;
            fP = nP3;
            fC = nC3;
            bsum += max(pr, cr);
            csum += cr;
            psum += pr;
        }
    }
    // the segment's sums into dbg (hot segments; cyc: the product's role cycles)
    RL_STAMP void flush(uint32_t* dbg, const uint64_t (&cyc)[4], uint32_t wave, uint32_t lane, uint32_t loader,
                        bool hot) {
        if (lane == 0 && dbg && hot) {
            dbg[DBG_ST_HW_ID + wave] = __builtin_amdgcn_s_getreg((4) | (0 << 6) | ((32 - 1) << 11));   // HW_ID
            const uint32_t role = wave == 0 ? 0u : wave == 1 ? 1u : wave == loader ? 2u : 3u;
            if (role < 3)
                for (int k = 0; k < 4; k++) atomicAdd(&dbg[DBG_ST_ROLE_CYC + 4 * role + k], (uint32_t)(cyc[k] >> 4));
            if (role == 1) {
                for (int k = 0; k < 4; k++) atomicAdd(&dbg[DBG_ST_SPLIT + k], (uint32_t)(k < 2 ? cx[k] >> 4 : cx[k]));
                atomicAdd(&dbg[DBG_ST_PLAN_CYC], (uint32_t)(cplan >> 4));
                atomicAdd(&dbg[DBG_ST_PLAN_CALLS], npcall);
                atomicAdd(&dbg[DBG_ST_PLAN_CALL_CYC], (uint32_t)(cpcall >> 4));
            }
            if (role == 0) {
                for (int k = 4; k < 8; k++) atomicAdd(&dbg[DBG_ST_SPLIT + k], (uint32_t)(k < 6 ? cx[k] >> 4 : cx[k]));
                atomicAdd(&dbg[DBG_ST_MODEL_2BUF], (uint32_t)max(gP, gC));
                atomicAdd(&dbg[DBG_ST_MODEL_3BUF], (uint32_t)max(fP, fC));
                atomicAdd(&dbg[DBG_ST_MODEL_MAX], (uint32_t)bsum);
                atomicAdd(&dbg[DBG_ST_MODEL_CHAIN], (uint32_t)csum);
                atomicAdd(&dbg[DBG_ST_MODEL_PRODUCER], (uint32_t)psum);
                atomicAdd(&dbg[DBG_ST_ROUND_TOPS], (uint32_t)(ttop >> 4));
            }
        }
    }
};

// A phase of ch_resolve, from begin(): the clock and the pass count there.
// Counted by lane 0 for a hot segment (St is ChState: s.hot).
struct ChResolveStamps {
    uint64_t t0 = 0;
    uint32_t it0 = 0;

    RL_STAMP void begin(uint32_t iters) {
        t0 = __builtin_amdgcn_s_memtime();
        it0 = iters;
    }
    template <typename St>
    RL_STAMP void setup_end(uint32_t* dbg, uint32_t lane, const St& s) {
        if (dbg && lane == 0 && s.hot) atomicAdd(&dbg[DBG_ST_NEAR_SETUP_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - t0) >> 4));
    }
    template <typename St>
    RL_STAMP void near_end(uint32_t* dbg, uint32_t lane, const St& s, uint32_t ne, uint32_t iters, bool xdec) {
        if (dbg && lane == 0 && s.hot) {
            atomicAdd(&dbg[DBG_ST_NEAR_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - t0) >> 4));
            atomicAdd(&dbg[DBG_ST_NEAR_ENTRIES], ne);
            atomicAdd(&dbg[DBG_ST_NEAR_PASSES], iters - it0);
            if (xdec) atomicAdd(&dbg[DBG_ST_X_NEAR_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - t0) >> 4));
        }
    }
    // an exactly replayed tile (an object of its own, begun before the tile)
    template <typename St>
    RL_STAMP void exact_end(uint32_t* dbg, uint32_t lane, const St& s, uint32_t iters, bool xdec) {
        if (dbg && lane == 0 && s.hot) {
            atomicAdd(&dbg[DBG_ST_EXACT_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - t0) >> 4));
            atomicAdd(&dbg[DBG_ST_EXACT_PASSES], iters - it0);
            if (xdec) atomicAdd(&dbg[DBG_ST_X_EXACT_CYC], (uint32_t)((__builtin_amdgcn_s_memtime() - t0) >> 4));
        }
    }
};

// The replay's tail (replay_rest and the chain kernel's block start): realtime
// ticks, low 32 bits.
struct ReplayStamps {
    uint64_t th0 = 0;

    RL_STAMP static void block_start(uint32_t* dbg) {
        if (threadIdx.x == 0 && dbg) atomicMax(&dbg[DBG_ST_T_LAST_START], (uint32_t)__builtin_amdgcn_s_memrealtime());
    }
    RL_STAMP void heavy_begin() { th0 = __builtin_amdgcn_s_memrealtime(); }
    // the longest heavy segment's replay and its length
    RL_STAMP void heavy_end(uint32_t* dbg, uint32_t len) {
        if ((threadIdx.x & 63) == 0 && dbg) {
            const uint32_t dt = (uint32_t)(__builtin_amdgcn_s_memrealtime() - th0);
            if (atomicMax(&dbg[DBG_ST_HEAVY_TICKS_MAX], dt) < dt) dbg[DBG_ST_HEAVY_LEN] = len;
        }
    }
    RL_STAMP static void heavy_phase_end(uint32_t* dbg, uint64_t t_light) {
        if (threadIdx.x == 0 && dbg) atomicMax(&dbg[DBG_ST_T_HEAVY_END], (uint32_t)t_light);
    }
    RL_STAMP static void light_claim(uint32_t* dbg) {
        if (threadIdx.x == 0 && dbg) atomicMax(&dbg[DBG_ST_T_LIGHT_CLAIM], (uint32_t)__builtin_amdgcn_s_memrealtime());
    }
};

#else  // the product build: no stamps

#define CH_T(v) do { } while (0)

struct ChStamps {
    template <typename Sh>
    RL_STAMP void segment_begin(Sh&, uint32_t) {}
    RL_STAMP void first_round() {}
    RL_STAMP void round_top(uint64_t) {}
    RL_STAMP void exit_guess(uint64_t, uint64_t&, uint64_t (&)[4], uint32_t) {}
    RL_STAMP void plan_call_begin() {}
    RL_STAMP void plan_call_end() {}
    RL_STAMP void plan_end(uint64_t) {}
    RL_STAMP void produce_begin() {}
    RL_STAMP void produce_end(uint64_t, bool, bool) {}
    RL_STAMP void resolve_end(uint64_t, uint64_t, bool) {}
    template <typename Sh>
    RL_STAMP void round_end(Sh&, uint32_t, uint64_t, bool) {}
    template <typename Sh>
    RL_STAMP void round_barrier_done(Sh&, uint32_t, uint64_t, bool) {}
    RL_STAMP void flush(uint32_t*, const uint64_t (&)[4], uint32_t, uint32_t, uint32_t, bool) {}
};

struct ChResolveStamps {
    RL_STAMP void begin(uint32_t) {}
    template <typename St>
    RL_STAMP void setup_end(uint32_t*, uint32_t, const St&) {}
    template <typename St>
    RL_STAMP void near_end(uint32_t*, uint32_t, const St&, uint32_t, uint32_t, bool) {}
    template <typename St>
    RL_STAMP void exact_end(uint32_t*, uint32_t, const St&, uint32_t, bool) {}
};

struct ReplayStamps {
    RL_STAMP static void block_start(uint32_t*) {}
    RL_STAMP void heavy_begin() {}
    RL_STAMP void heavy_end(uint32_t*, uint32_t) {}
    RL_STAMP static void heavy_phase_end(uint32_t*, uint64_t) {}
    RL_STAMP static void light_claim(uint32_t*) {}
};

#endif  // RL_STAMPS

}  // namespace rl
