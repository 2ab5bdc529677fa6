// rl_engine_impl.h -- the engine's host state and the helpers that more than
// one translation unit of the library uses.  rl_engine.hip is the decision
// path and the engine's life cycle; rl_ops.hip Peek and Reset; rl_tables.hip
// table maintenance and snapshots; rl_tally.hip the usage tally; rl_hot.hip
// the top keys.  Only rl_engine.hip includes the grouping and the replay
// (rl_group.h, rl_replay.h): nothing here does.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rl_engine.h"
#include "../../include/rl_route.h"
#include "rl_batch.h"
#include "rl_hot.h"
#include "rl_semantics.h"
#include "rl_table.h"
#include "rl_tally.h"

namespace rl {
struct UpRec;   // rl_group.h
}  // namespace rl

constexpr int NSTAGES = 5;
constexpr int NSETS = 3;       // batch buffer sets: grouping b+1 | replay b | finish b-1

// Per-batch device buffers.  A batch runs in three parts on three engine
// streams: grouping (probe, sort, segments, permute) on `front`, the replay
// (k_tb_chain) on `chain`, the finish (run expansion, unpermute) on `tail`.
// The replays are ordered on `chain` (each one reads the table state the
// previous one wrote); nothing else orders batches, so batch b+1's grouping
// and batch b-1's finish overlap batch b's replay.  NSETS buffer sets: set
// b mod NSETS is reused by batch b+NSETS only after batch b's finish.  The
// caller's stream waits for the finish of every batch it enqueued.
struct BatchSet {
    uint32_t *sk0 = nullptr, *sk1 = nullptr, *sv0 = nullptr, *sv1 = nullptr;
    rl::SegRec* list[4] = {nullptr, nullptr, nullptr, nullptr};   // heavy TB, light, heavy window, huge TB
    // requests and results in sorted order (k_permute / k_unpermute)
    int64_t *p_ts = nullptr, *p_n = nullptr, *p_sms = nullptr;
    uint32_t* p_cfg = nullptr;
    void* rec = nullptr;          // requests packed in arrival order (k_probe -> k_permute): ReqRec<XS>
    void* recb = nullptr;         // ReqRec in the MSD pass's bucket order (k_sort_pass -> k_permute)
    // an explicit server clock's record fields that do not fit (rec_pack), by arrival index
    int64_t* side_n = nullptr;
    uint32_t* side_cfg = nullptr;
    int64_t* side_sms = nullptr;
    uint8_t* p_fresh = nullptr;   // sorted order: the request inserted its key (k_permute -> replay phase 3)
    uint8_t* o_dec = nullptr;
    double* o_tok = nullptr;      // tokens (token bucket) / Remaining bits (window): finish_result
    // token-bucket precomputation (k_permute)
    double *q_add = nullptr, *q_th = nullptr;
    rl::TbRuns runs{};            // the chain's committed runs (by start position)
    uint32_t* zero = nullptr;     // ctrl words + look-back status + huge claims (zeroed per batch)
    bool dirty = false;           // a batch began on the set and did not reach its finish's zeroing
    uint32_t* ctrl = nullptr;
    uint32_t* status = nullptr;
    uint32_t* claim = nullptr;
    hipEvent_t front_done = nullptr, chain_done = nullptr, back_done = nullptr;
    uint64_t* kid = nullptr;      // key ids hashed from raw keys (rl_decide_batch_keys_device; lazy)
    rl::UpRec* upb = nullptr;     // results bucketed by arrival index (k_unpermute_bucket)
    bool used = false;
};

struct rl_engine {
    int device = 0;
    int32_t profile = rl::PROFILE_REDIS7;
    uint32_t flags = 0;
    // the engine's stream (host API, device API without a stream, setup) is
    // `tail`: with the caller's stream the engine then uses four streams, one
    // hardware queue each at HIP's default of four queues per process (streams
    // sharing a queue would serialize the replay and the finish)
    hipStream_t stream = nullptr;
    hipStream_t front = nullptr;      // grouping
    hipStream_t chain = nullptr;      // replays, in batch order
    hipStream_t tail = nullptr;       // finishes
    hipEvent_t ev_in = nullptr;       // inputs ready (non-pipelined device API, host API)
    std::string err;

    std::vector<rl::CfgDev> h_cfg;
    rl::CfgDev* d_cfg = nullptr;
    uint32_t cfg_cap = 0;

    rl::TbEntry* d_tb = nullptr;
    uint64_t tb_cap = 0;
    rl::WinEntry* d_win = nullptr;
    uint64_t win_cap = 0;
    rl::SpillEntry* d_spill = nullptr;    // window keys outside their user key's entry (rl_window.h)
    uint64_t spill_cap = 0;
    bool spill_follows = true;        // spill capacity = 2 x window capacity (also after a resize)
    rl::Spill spill() const { return rl::Spill{d_spill, spill_cap - 1}; }
    // what follows the capacities (rl::set_geometry)
    uint32_t win_base = 0, invalid_key = 0;
    int sort_bits = 0, sort_passes = 0;
    uint32_t sort_shifts = 0;   // digit shift of each histogram / pass (8 bits each; sort_shifts())

    uint32_t max_batch = 0;
    uint32_t max_tiles = 0;
    BatchSet set[NSETS];
    // k_small: batches up to small_max run as one workgroup on `chain`; its
    // sorted-order scratch (reused by consecutive small batches, which the
    // chain stream orders)
    uint32_t small_max = 0;
    // batches up to up_max finish through arrival-index buckets, larger ones
    // through k_unpermute / k_unpermute_routed (UP_MAX at creation; RL_UP_MAX
    // lowers it: the buckets and their counters are sized for UP_MAX)
    uint32_t up_max = 0;
    int64_t *s_ts = nullptr, *s_n = nullptr, *s_sms = nullptr;
    uint32_t* s_cfg = nullptr;
    uint8_t* s_dec = nullptr;
    double *s_tok = nullptr, *s_add = nullptr, *s_th = nullptr;
    hipEvent_t ev_small = nullptr;
    hipEvent_t ev_reset = nullptr;    // rl_reset_device: the DEL on `chain` -> the caller's stream
    hipEvent_t ev_peek = nullptr;     // rl_peek_batch_device: k_peek on `chain` -> the caller's stream
    int next_set = 0, last_set = 0;   // set of the next / the last enqueued batch
    size_t zero_bytes = 0;
    int coop_grid = 128;        // k_tb_chain blocks launched (one per CU fits its LDS) ...
    int coop_base = 112;        // ... of which those past 112 of 256 CUs exit at once unless the batch
                                // has at least m / coop_light_div light segments: the other CUs run
                                // the neighbouring batches' grouping and finish (profiles/r3al_ab_replay_grid.txt;
                                // 96 -> 112 with the iterative-ILP build: configs[1] +1.1-1.5 %,
                                // profiles/r6zm_ab_coop_base.txt)
    uint32_t coop_light_div = 4;
    int probe_grid = 1024;      // k_probe blocks at most
    int perm_grid = 1024;       // k_permute / k_unpermute blocks at most
    uint32_t heavy_min = 32;    // segments this long replay cooperatively
    uint32_t huge_min = 4096;   // token-bucket segments this long are dequeued first
    // dynamic LDS that makes a k_tb_chain block fill its CU's LDS: with two
    // batches in flight, the other batches' grouping and finish kernels (each launched with
    // GROUP_LDS bytes at least) then never share a CU with a chain
    size_t chain_pad[2] = {0, 0};
    size_t light_pad[2] = {0, 0};    // k_replay_light: the same one-block-per-CU LDS floor
    uint32_t* h_huge = nullptr;      // mapped host word: huge segments of the last replay seen (k_tb_chain /
    uint32_t* d_huge = nullptr;      //   k_replay_light write it); 0 -> the next batches launch k_replay_light
    bool light_ok = true;            // RL_NO_LIGHT_REPLAY=1: always the chain kernel
    bool force_light = false;        // warm-up: load k_replay_light
    uint32_t* d_eflags = nullptr;
    uint32_t* d_zero = nullptr;       // a device word holding 0 (warm-up of the routed kernels)
    unsigned long long* d_count = nullptr;   // table counts / GC counters (rl_table_info_get, rl_table_gc)
    unsigned long long* h_count = nullptr;   // pinned host copy
    // the grouping sort's last plan (1: every MSD bucket fit LDS), written by
    // the MSD pass into mapped host memory; read when a batch is enqueued
    uint32_t* h_plan = nullptr;
    uint32_t* d_plan = nullptr;   // its device address
    uint32_t* stamp_ring = nullptr;   // RL_STAMP_KERNELS diagnostics

    // host-API staging (device side): rl::stage_in / rl::stage_out
    uint64_t* d_key = nullptr;
    uint64_t* small_kid = nullptr;   // key ids hashed for k_small (rl_decide_batch_keys_device; lazy)
    int64_t *d_ts = nullptr, *d_n = nullptr, *d_sms = nullptr;
    uint32_t* d_cfgid = nullptr;
    uint8_t* d_dec = nullptr;
    int64_t *d_rem = nullptr, *d_retry = nullptr, *d_reset = nullptr;
    double* d_tok = nullptr;

    // timing: front start, after probe, after sort, after segments+permute
    // (front); replay start, end (chain); finish start, end (tail)
    bool timing = false;
    bool timing_all = false;    // level 2: every stage; level 1: the replay only (2 events per batch)
    uint32_t timing_stride = 1; // the replay events on every timing_stride-th batch only (level -k)
    uint64_t timing_seq = 0;
    bool stamps = false;        // RL_STAMP_KERNELS: timestamps around each replay (debug words 18, 19)
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::array<hipEvent_t, 8>> ev_pending;
    double stage_ms[NSTAGES] = {0, 0, 0, 0, 0};
    uint64_t timed_batches = 0;

    rl_stats stats{};

    // usage tally (rl_tally.h): off until rl_tally_enable
    bool tally_on = false;
    rl::TallyKey* d_tally_keys = nullptr;
    uint64_t tally_slots = 0;
    rl::tally_u64* d_tally_cfg = nullptr;     // TALLY_CFG_WORDS per config, tally_cfg_cap rows
    uint32_t tally_cfg_cap = 0;
    rl::tally_u64* d_tally_glob = nullptr;    // TG_WORDS
    uint64_t tally_batches = 0, tally_requests = 0;
    uint64_t tally_routed_steps = 0;          // rl_tally_routed_device calls with m_max > 0

    // top keys (rl_hot.h): off until rl_hot_enable
    bool hot_on = false;
    rl::hot_u64* d_hot_sketch = nullptr;      // HOT_DEPTH rows of hot_width counters
    uint64_t hot_width = 0;
    rl::HotKey* d_hot_keys = nullptr;         // hot_slots candidate records
    uint64_t hot_slots = 0;
    rl::hot_u64* d_hot_glob = nullptr;        // HG_WORDS
    uint64_t hot_min = 0;
    uint32_t hot_weight = 0;
    uint64_t hot_batches = 0, hot_requests = 0;

    // refund scratch (rl_refund.h): one allocation, made and zeroed on `chain`
    // by the first refund; refund_calls picks the list counter of a call
    void* d_refund = nullptr;
    uint64_t refund_records = 0;
    uint64_t refund_calls = 0;
    hipEvent_t ev_refund = nullptr;   // rl_refund_batch_device: k_refund_apply on `chain` -> the caller's stream

    // AllowAll scratch (rl_allow_all.h): one allocation made by the first call,
    // sized for rl_allow_all_max -- the give-back amounts g, then the host
    // form's staging of first, verdict and rollback.  The refund that reads g
    // records ev_refund on `chain`; the next call's settle kernel, on whatever
    // stream, waits for it before it writes g again.  It frees itself with the
    // engine (rl_engine_destroy drains first).
    struct AllowAllScratch {
        void* mem = nullptr;
        ~AllowAllScratch() {
            if (mem) (void)hipFree(mem);
        }
    } allow_all;

    // Charge scratch (rl_charge.h): one allocation made by the first call,
    // sized for rl_charge_max -- n', the ask's row, the decide's row, then the
    // host form's staging of `charged`.  `ev` is the end of the last call's
    // finish kernel on its caller's stream: the next call's ask, on `chain`,
    // waits for it before it writes the scratch again.  It frees itself with
    // the engine (rl_engine_destroy drains first).
    struct ChargeState {
        void* mem = nullptr;
        hipEvent_t ev = nullptr;
        uint64_t calls = 0;
        ~ChargeState() {
            if (mem) (void)hipFree(mem);
            if (ev) (void)hipEventDestroy(ev);
        }
    } charge;

    // The routed charge's scratch (rl_charge.h ChargeRouted): one allocation
    // made by the first rl_charge_routed_device call, sized for rl_charge_max
    // -- the normalised merged batch, the decide's result records and the
    // ask's rows, by merge position.  `ev` is the end of the last call's finish
    // kernel on `tail`: the next call's ask, on `chain`, waits for it before it
    // writes the scratch again.
    ChargeState charge_routed;

    // The tally's and the top keys' kernels run on the caller's stream and read
    // the feature's own memory: the end of the last such call on each stream
    // one was enqueued on is what drain(), rl_tally_read and rl_hot_read wait
    // for (side_record / side_wait).
    std::vector<std::pair<hipStream_t, hipEvent_t>> side_ev;
};

inline int fail(rl_engine* e, int code, const std::string& msg) {
    if (e) e->err = msg;
    return code;
}

#define HIPCHK(e, call)                                                                  \
    do {                                                                                 \
        hipError_t _st = (call);                                                         \
        if (_st != hipSuccess)                                                           \
            return fail((e), RL_EDEVICE, std::string(#call) + ": " + hipGetErrorString(_st)); \
    } while (0)

// versioned output structs (include/rl_engine.h): the caller's struct_size
// bounds what is written, and struct_size comes back as the bytes actually
// filled in (min(caller's, library's)), so a caller built against a newer
// header sees which trailing fields this library knows; a size smaller than
// the header field is rejected
template <class T>
int copy_out(T* dst, T src) {
    if (dst->struct_size < 8) return RL_EINVAL;
    const uint32_t n = (uint32_t)std::min<size_t>(dst->struct_size, sizeof(T));
    src.struct_size = n;
    memcpy(dst, &src, n);
    return RL_OK;
}

// record the end of a tally / top-keys call just enqueued on s
inline int side_record(rl_engine* e, hipStream_t s) {
    hipEvent_t ev = nullptr;
    for (auto& se : e->side_ev)
        if (se.first == s) ev = se.second;
    if (!ev) {
        if (e->side_ev.size() >= 16) {   // streams come and go: keep the list short
            for (auto& se : e->side_ev) {
                HIPCHK(e, hipEventSynchronize(se.second));
                (void)hipEventDestroy(se.second);
            }
            e->side_ev.clear();
        }
        HIPCHK(e, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        e->side_ev.emplace_back(s, ev);
    }
    HIPCHK(e, hipEventRecord(ev, s));
    return RL_OK;
}

// every tally / top-keys call enqueued so far, on any stream, has finished
inline int side_wait(rl_engine* e) {
    for (auto& se : e->side_ev) HIPCHK(e, hipEventSynchronize(se.second));
    return RL_OK;
}

inline uint64_t pow2_at_least(uint64_t v) {
    uint64_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

namespace rl {

// --- rl_engine.hip ---------------------------------------------------------

// every queued kernel of the engine has finished (the engine's streams and,
// through the back_done events, any caller stream a batch was enqueued on)
int drain(rl_engine* e);

// One decide batch of m <= max_batch requests whose inputs are made on the
// device by work queued on s: the grouping waits for s, whatever
// RL_OPT_PIPELINE says of the caller's arrays (Charge's second step,
// rl_ops.hip).  Otherwise rl_decide_batch_device on one chunk.
int decide_after_stream(rl_engine* e, uint32_t m, const ReqArgs& a, hipStream_t s);

// One routed decide batch of bound m <= max_batch (include/rl_route.h: request
// p is rec[order[p]] at store clock sms[p], p < *count; results to
// res[order[p]]) whose inputs are made by work queued on s: the grouping waits
// for s.  The end of its finish, on `tail`, is recorded into `done`; no stream
// is made to wait.  The routed Charge's second step (rl_ops.hip), with s =
// `chain`, where its ask ran.  Otherwise rl_decide_routed_device_ev.
int decide_routed_after_stream(rl_engine* e, uint32_t m, const rl_route_rec* rec, const uint32_t* order,
                               const uint32_t* count, const int64_t* sms, rl_route_res* res, hipStream_t s,
                               hipEvent_t done);

// slot ids (the sort keys) are 31 bits: token-bucket slots, then window slots,
// then invalid_key
inline bool caps_fit(uint64_t tb_cap, uint64_t win_cap) { return tb_cap + win_cap < (1ull << 31); }
// the engine's capacities and everything derived from them: win_base,
// invalid_key, the grouping sort's bits, passes and shifts, and their copy in
// the stats
void set_geometry(rl_engine* e, uint64_t tb_cap, uint64_t win_cap, uint64_t spill_cap);

// Host-API staging of chunk [off, off + c) of the caller's arrays, c <=
// max_batch, on stream s: inputs into d_key, d_ts, d_n, d_cfgid, d_sms;
// results out of d_dec, d_rem, d_retry, d_reset, d_tok.  A null array is not
// staged.
int stage_in(rl_engine* e, size_t off, uint32_t c, const uint64_t* key, const int64_t* ts, const int64_t* n,
             const uint32_t* cfg, const int64_t* sms, hipStream_t s);
int stage_out(rl_engine* e, size_t off, uint32_t c, uint8_t* dec, int64_t* rem, int64_t* retry, int64_t* reset,
              double* tok, hipStream_t s);

// blocks of a grid-stride kernel over m items: min(ceil(m / block), cap)
inline int grid_for(size_t m, int block, int cap) {
    return (int)std::min<size_t>((m + block - 1) / block, (size_t)cap);
}

// One kernel on `chain` between two replays: after the replay of every batch
// (and every chain op) enqueued before, before those enqueued after.  The
// replays -- k_tb_chain, k_replay_light, k_small -- and the DEL of a reset are
// the only writers of entry state, all on `chain`; the grouping reads entry
// keys only and the finish no table state.  Unless the inputs are ready
// (RL_OPT_PIPELINE, or arguments by value), the kernel waits for s.  Its end
// is recorded into `done` when given; else into ev (ev_peek / ev_reset), which
// `so` waits for.  launch(c) enqueues the kernel on c.
template <class Launch>
int chain_op(rl_engine* e, hipStream_t s, bool inputs_ready, hipStream_t so, hipEvent_t ev, hipEvent_t done,
             Launch&& launch) {
    hipStream_t c = e->chain;
    if (!inputs_ready) {
        HIPCHK(e, hipEventRecord(e->ev_in, s));
        HIPCHK(e, hipStreamWaitEvent(c, e->ev_in, 0));
    }
    launch(c);
    HIPCHK(e, hipGetLastError());
    if (done) {
        HIPCHK(e, hipEventRecord(done, c));
        return RL_OK;
    }
    HIPCHK(e, hipEventRecord(ev, c));
    HIPCHK(e, hipStreamWaitEvent(so, ev, 0));
    return RL_OK;
}

// --- rl_ops.hip ------------------------------------------------------------

// the unit's part of the creation warm-up: each of its kernels that a server
// may need at once, launched on an empty or rejected request
int ops_warm_up(rl_engine* e);
// device calls of the q14 slow paths in this unit's kernels (the counter is
// per code object: rl_q14.h)
int ops_q14_slow(rl_engine* e, unsigned long long* out);

// --- rl_tables.hip ---------------------------------------------------------

// fresh tables: every slot never used (enqueued on s)
void tables_init(TbEntry* tb, uint64_t tb_cap, WinEntry* win, uint64_t win_cap, SpillEntry* sp, uint64_t spill_cap,
                 hipStream_t s);
int tables_warm_up(rl_engine* e);

}  // namespace rl
