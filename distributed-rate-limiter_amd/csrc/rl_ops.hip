// rl_ops.hip -- Peek, Reset and Refund (single, batched, routed): the
// kernels of rl_peek.h, rl_reset.h and rl_refund.h and their C entry points.
// Each is one chain op -- one kernel, Refund's two -- on the engine's `chain`
// stream between two replays (chain_op, rl_engine_impl.h).  AllowAll
// (rl_allow_all.h) composes a decide, its settle kernel on the caller's stream
// and a refund; the routed AllowAll's settle (rl_allow_all_settle_device) is
// the second instantiation of that kernel's text.  Charge (rl_charge.h)
// composes its ask as a chain op, a decide and its finish kernel on the
// caller's stream; the routed Charge the same three on the merged batch, its
// decide on the engine's scratch and its finish on `tail`.
// A code object of its own: that of the decision kernels (rl_engine.hip) does
// not change with it.
#include <hip/hip_runtime.h>

#include "../../include/rl_engine.h"
#include "../../include/rl_route.h"
#include "rl_allow_all.h"
#include "rl_charge.h"
#include "rl_engine_impl.h"
#include "rl_peek.h"
#include "rl_refund.h"
#include "rl_reset.h"

using namespace rl;

// Reset of one key (rl_reset_device): the arguments by value, one thread
__global__ void k_reset(uint64_t key, int64_t ts, const CfgDev* cfgs, uint32_t cfg, TbEntry* tb,
                        uint64_t tb_mask, WinEntry* win, uint64_t win_mask, Spill spill) {
    reset_one(key, &ts, cfgs[cfg], tb, tb_mask, win, win_mask, spill);
}

// enqueue one read-only query batch (rl_peek.h) of any size: k_peek as a
// chain op; s waits for it.  No per-batch buffer is involved, and nothing is
// counted in rl_stats.
static int run_peek(rl_engine* e, size_t m, ReqArgs a, hipStream_t s, bool inputs_ready) {
    if (m == 0) return RL_OK;
    return chain_op(e, s, inputs_ready, s, e->ev_peek, nullptr, [&](hipStream_t c) {
        k_peek<<<grid_for(m, PEEK_BLOCK, PEEK_GRID), PEEK_BLOCK, 0, c>>>(
            (uint64_t)m, a, e->d_cfg, (uint32_t)e->h_cfg.size(), e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1,
            e->spill(), e->profile);
    });
}

// enqueue one batch of resets (rl_reset.h) of any size: k_reset_batch as a
// chain op, where rl_reset_device puts its DEL; s waits for it.  Nothing is
// counted in rl_stats and no error flag is raised.
static int run_reset_batch(rl_engine* e, size_t m, const uint64_t* key, const int64_t* ts, const uint32_t* cfg,
                           uint8_t* status, hipStream_t s, bool inputs_ready) {
    if (m == 0) return RL_OK;
    return chain_op(e, s, inputs_ready, s, e->ev_reset, nullptr, [&](hipStream_t c) {
        k_reset_batch<<<grid_for(m, RESET_BLOCK, RESET_GRID), RESET_BLOCK, 0, c>>>(
            (uint64_t)m, key, ts, cfg, status, e->d_cfg, (uint32_t)e->h_cfg.size(), e->d_tb, e->tb_cap - 1, e->d_win,
            e->win_cap - 1, e->spill());
    });
}

// enqueue the peek or the reset step of the routed path (include/rl_route.h):
// k_peek_routed / k_reset_routed as a chain op, ordered like run_peek and
// run_reset_batch.  The kernel always waits for s: the merge produced count,
// order and the store clocks there (RL_OPT_PIPELINE promises the caller's
// arrays, not the router's).  Its end is recorded into `done` when given, else
// so waits for it.  No buffer set is taken, so m_max is not bounded by
// max_batch; nothing is counted in rl_stats; the one flag it can raise is
// EF_ROUTED_OVER.
static int run_routed_op(rl_engine* e, bool reset, size_t m_max, const RoutedIo& io, hipStream_t s, hipStream_t so,
                         hipEvent_t done) {
    const uint32_t ncfg = (uint32_t)e->h_cfg.size();
    return chain_op(e, s, false, so, reset ? e->ev_reset : e->ev_peek, done, [&](hipStream_t c) {
        if (reset)
            k_reset_routed<<<grid_for(m_max, RESET_BLOCK, RESET_GRID), RESET_BLOCK, 0, c>>>(
                (uint64_t)m_max, io, e->d_cfg, ncfg, e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1, e->spill());
        else
            k_peek_routed<<<grid_for(m_max, PEEK_BLOCK, PEEK_GRID), PEEK_BLOCK, 0, c>>>(
                (uint64_t)m_max, io, e->d_cfg, ncfg, e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1, e->spill(),
                e->profile);
    });
}

static int run_refund_routed(rl_engine* e, size_t m_max, const RoutedIo& io, hipStream_t s, hipStream_t so,
                             hipEvent_t done);

static int run_charge_routed(rl_engine* e, size_t m_max, const RoutedIo& io, hipStream_t s, hipStream_t so,
                             hipEvent_t done);

static int allow_all_warm_up(rl_engine* e);
static int charge_warm_up(rl_engine* e);

enum RoutedKind { ROUTED_PEEK, ROUTED_RESET, ROUTED_REFUND, ROUTED_CHARGE };

// the C-ABI of the routed steps: argument checks as rl_decide_routed_device_io
// / _ev, except that m_max is bounded by the 32-bit `order` only
static int routed_op_entry(rl_engine* e, RoutedKind kind, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                           const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                           void* out_stream, void* done_event) {
    if (!e || !count || (m_max && (!recv || !order || !server_ms || !res))) return RL_EINVAL;
    if (m_max > (size_t)UINT32_MAX) return fail(e, RL_EINVAL, "routed batch bound above the 32-bit order index");
    (void)hipSetDevice(e->device);
    hipStream_t s = in_stream ? (hipStream_t)in_stream : e->stream;
    if (!m_max) {   // nothing to run: the event marks the caller's stream
        if (done_event) HIPCHK(e, hipEventRecord((hipEvent_t)done_event, s));
        return RL_OK;
    }
    const RoutedIo io{recv, order, count, server_ms, res, e->d_eflags};
    hipStream_t so = out_stream ? (hipStream_t)out_stream : s;
    if (kind == ROUTED_REFUND) return run_refund_routed(e, m_max, io, s, so, (hipEvent_t)done_event);
    if (kind == ROUTED_CHARGE) return run_charge_routed(e, m_max, io, s, so, (hipEvent_t)done_event);
    return run_routed_op(e, kind == ROUTED_RESET, m_max, io, s, so, (hipEvent_t)done_event);
}

extern "C" int rl_peek_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                     const uint32_t* order, const int64_t* server_ms, rl_route_res* res,
                                     void* in_stream, void* out_stream, void* done_event) {
    return routed_op_entry(e, ROUTED_PEEK, m_max, count, recv, order, server_ms, res, in_stream, out_stream,
                           done_event);
}

extern "C" int rl_reset_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                      const uint32_t* order, const int64_t* server_ms, rl_route_res* res,
                                      void* in_stream, void* out_stream, void* done_event) {
    return routed_op_entry(e, ROUTED_RESET, m_max, count, recv, order, server_ms, res, in_stream, out_stream,
                           done_event);
}

extern "C" int rl_refund_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                       const uint32_t* order, const int64_t* server_ms, rl_route_res* res,
                                       void* in_stream, void* out_stream, void* done_event) {
    return routed_op_entry(e, ROUTED_REFUND, m_max, count, recv, order, server_ms, res, in_stream, out_stream,
                           done_event);
}

extern "C" int rl_charge_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                                       const uint32_t* order, const int64_t* server_ms, rl_route_res* res,
                                       void* in_stream, void* out_stream, void* done_event) {
    return routed_op_entry(e, ROUTED_CHARGE, m_max, count, recv, order, server_ms, res, in_stream, out_stream,
                           done_event);
}

// The routed peek and reset steps on an empty batch (they read the zero count
// and nothing else), then k_peek and k_reset_batch on one request that is
// rejected: no config is registered yet.  The staging arrays hold zeros.
// No refund kernel is launched here, routed or not: the first refund of an
// engine allocates its scratch, and the warm-up allocates nothing.  Last,
// AllowAll's settle kernel on one member, and Charge's two kernels on one
// request and its two routed kernels on an empty batch.
int rl::ops_warm_up(rl_engine* e) {
    hipStream_t s = e->stream;
    const RoutedIo io{nullptr, nullptr, e->d_zero, nullptr, nullptr, e->d_eflags};
    for (const bool reset : {false, true}) {
        const int r = run_routed_op(e, reset, 1, io, s, s, nullptr);
        if (r != RL_OK) return r;
    }
    const ReqArgs a{e->d_key, e->d_ts, e->d_n, e->d_cfgid, nullptr, e->d_dec, e->d_rem, e->d_retry, e->d_reset, e->d_tok};
    const int r = run_peek(e, 1, a, s, false);
    if (r != RL_OK) return r;
    const int rr = run_reset_batch(e, 1, e->d_key, e->d_ts, e->d_cfgid, e->d_dec, s, false);
    if (rr != RL_OK) return rr;
    const int ra = allow_all_warm_up(e);
    if (ra != RL_OK) return ra;
    return charge_warm_up(e);
}

int rl::ops_q14_slow(rl_engine* e, unsigned long long* out) {
    HIPCHK(e, hipMemcpyFromSymbol(out, HIP_SYMBOL(rlq::q14_slow_calls), sizeof *out, 0, hipMemcpyDeviceToHost));
    return RL_OK;
}

// The DEL only writes `when` fields of table entries: a chain op with its
// arguments by value, so nothing to wait for.
extern "C" int rl_reset_device(rl_engine* e, uint32_t cfg_id, uint64_t key_id, int64_t ts_ns, void* stream) {
    if (!e || cfg_id >= e->h_cfg.size() || key_id == EMPTY_KEY) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return chain_op(e, s, true, s, e->ev_reset, nullptr, [&](hipStream_t c) {
        k_reset<<<1, 1, 0, c>>>(key_id, ts_ns, e->d_cfg, cfg_id, e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1,
                                e->spill());
    });
}

extern "C" int rl_reset(rl_engine* e, uint32_t cfg_id, uint64_t key_id, int64_t ts_ns) {
    const int r = rl_reset_device(e, cfg_id, key_id, ts_ns, nullptr);
    if (r != RL_OK) return r;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return RL_OK;
}

// Many resets in one launch (rl_reset.h), ordered as rl_reset_device.  The
// grid strides over any m: no chunking on the device entry point.
extern "C" int rl_reset_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                     const uint32_t* cfg_id, uint8_t* status, void* stream) {
    if (!e || (m && (!key_id || !ts_ns || !cfg_id))) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return run_reset_batch(e, m, key_id, ts_ns, cfg_id, status, s, (e->flags & RL_OPT_PIPELINE) != 0);
}

extern "C" int rl_reset_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                              const uint32_t* cfg_id, uint8_t* status) {
    if (!e || (m && (!key_id || !ts_ns || !cfg_id))) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    // chunks of max_batch: the size of the host API's staging arrays
    for (size_t off = 0; off < m; off += e->max_batch) {
        const uint32_t c = (uint32_t)std::min<size_t>(e->max_batch, m - off);
        int r = stage_in(e, off, c, key_id, ts_ns, nullptr, cfg_id, nullptr, s);
        // the staged inputs arrive on s: the kernel always waits for them
        if (r == RL_OK) r = run_reset_batch(e, c, e->d_key, e->d_ts, e->d_cfgid, status ? e->d_dec : nullptr, s, false);
        if (r == RL_OK) r = stage_out(e, off, c, status, nullptr, nullptr, nullptr, nullptr, s);
        if (r != RL_OK) return r;
        HIPCHK(e, hipStreamSynchronize(s));
    }
    return RL_OK;
}

extern "C" int rl_reset_grid_cap(void) { return RESET_GRID * RESET_BLOCK; }

// Read-only queries (rl_peek.h), ordered as rl_reset_device.  A peek raises no
// error flag, so the sticky status of rl_engine_sync never comes from one.
extern "C" int rl_peek_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                    const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                                    uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                                    int64_t* reset_at_ns, double* tokens, void* stream) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !decision || !remaining || !retry_after_ns || !reset_at_ns)))
        return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    // the grid strides over any m: no chunking
    ReqArgs a{key_id, ts_ns, n, cfg_id, server_ms, decision, remaining, retry_after_ns, reset_at_ns, tokens};
    return run_peek(e, m, a, s, (e->flags & RL_OPT_PIPELINE) != 0);
}

extern "C" int rl_peek_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                             const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* decision,
                             int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns, double* tokens) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !decision || !remaining || !retry_after_ns || !reset_at_ns)))
        return RL_EINVAL;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    // chunks of max_batch: the size of the host API's staging arrays
    for (size_t off = 0; off < m; off += e->max_batch) {
        const uint32_t c = (uint32_t)std::min<size_t>(e->max_batch, m - off);
        int r = stage_in(e, off, c, key_id, ts_ns, n, cfg_id, server_ms, s);
        ReqArgs a{e->d_key, e->d_ts, e->d_n, e->d_cfgid, server_ms ? e->d_sms : nullptr,
                  e->d_dec, e->d_rem, e->d_retry, e->d_reset, tokens ? e->d_tok : nullptr};
        // the staged inputs arrive on s: the kernel always waits for them
        if (r == RL_OK) r = run_peek(e, c, a, s, false);
        if (r == RL_OK) r = stage_out(e, off, c, decision, remaining, retry_after_ns, reset_at_ns, tokens, s);
        if (r != RL_OK) return r;
        HIPCHK(e, hipStreamSynchronize(s));
    }
    return RL_OK;
}

extern "C" int rl_peek_grid_cap(void) { return PEEK_GRID * PEEK_BLOCK; }

// --- Refund (rl_refund.h) ----------------------------------------------------

static uint32_t refund_max(const rl_engine* e) { return std::min<uint32_t>(e->max_batch, REFUND_MAX); }

// the engine's refund scratch, allocated and zeroed in-stream by the first
// call: twice as many records as the largest call has requests, the claim
// words, the records, the list and its two counters in one allocation
static int refund_scratch(rl_engine* e, RefundScratch* out) {
    if (!e->d_refund) {
        const uint64_t R = 2 * pow2_at_least(refund_max(e));
        const size_t bytes = R * (sizeof(refund_u64) + sizeof(RefundRec) + sizeof(uint32_t)) + 2 * sizeof(uint32_t);
        if (!e->ev_refund) HIPCHK(e, hipEventCreateWithFlags(&e->ev_refund, hipEventDisableTiming));
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return fail(e, RL_ENOMEM, "refund scratch: out of device memory");
        if (hipMemsetAsync(p, 0, bytes, e->chain) != hipSuccess) {
            (void)hipFree(p);
            return fail(e, RL_EDEVICE, "refund scratch: memset failed");
        }
        e->d_refund = p;
        e->refund_records = R;
    }
    const uint64_t R = e->refund_records;
    char* p = (char*)e->d_refund;
    out->loc = (refund_u64*)p;
    out->rec = (RefundRec*)(p + R * sizeof(refund_u64));
    out->list = (uint32_t*)(p + R * (sizeof(refund_u64) + sizeof(RefundRec)));
    out->cnt = out->list + R;
    out->mask = R - 1;
    return RL_OK;
}

// enqueue one refund call of m <= refund_max requests: k_refund_add and
// k_refund_apply as one chain op, where rl_reset_batch_device puts its kernel;
// s waits for them.  Nothing is counted in rl_stats and no error flag is raised.
static int run_refund(rl_engine* e, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                      const uint32_t* cfg, const int64_t* sms, uint8_t* status, hipStream_t s, bool inputs_ready) {
    if (m == 0) return RL_OK;
    RefundScratch S;
    const int r = refund_scratch(e, &S);
    if (r != RL_OK) return r;
    const uint32_t parity = (uint32_t)(e->refund_calls++ & 1);
    const uint32_t ncfg = (uint32_t)e->h_cfg.size();
    return chain_op(e, s, inputs_ready, s, e->ev_refund, nullptr, [&](hipStream_t c) {
        const int grid = grid_for(m, REFUND_BLOCK, REFUND_GRID);
        k_refund_add<<<grid, REFUND_BLOCK, 0, c>>>((uint64_t)m, key, ts, n, cfg, sms, status, e->d_cfg, ncfg, e->d_tb,
                                                   e->tb_cap - 1, e->d_win, e->win_cap - 1, e->spill(), e->profile, S,
                                                   parity);
        k_refund_apply<<<grid, REFUND_BLOCK, 0, c>>>(e->d_cfg, ncfg, e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1,
                                                     e->spill(), e->profile, S, parity);
    });
}

// enqueue the refund step of the routed path (include/rl_route.h): the merged
// batch as ONE refund call -- k_refund_add_routed over the first B = min(m_max,
// refund_max) requests, then k_refund_apply, one chain op ordered like
// run_refund.  The kernels always wait for s (count, order and the store clocks
// are the merge's outputs there); their end is recorded into `done` when given,
// else so waits for it.  The scratch and the call parity are the array form's;
// no stream of its own; nothing is counted in rl_stats; the one flag it can
// raise is EF_ROUTED_OVER (a count above B).
static int run_refund_routed(rl_engine* e, size_t m_max, const RoutedIo& io, hipStream_t s, hipStream_t so,
                             hipEvent_t done) {
    RefundScratch S;
    const int r = refund_scratch(e, &S);
    if (r != RL_OK) return r;
    const size_t B = std::min<size_t>(m_max, refund_max(e));
    const uint32_t parity = (uint32_t)(e->refund_calls++ & 1);
    const uint32_t ncfg = (uint32_t)e->h_cfg.size();
    return chain_op(e, s, false, so, e->ev_refund, done, [&](hipStream_t c) {
        const int grid = grid_for(B, REFUND_BLOCK, REFUND_GRID);
        k_refund_add_routed<<<grid, REFUND_BLOCK, 0, c>>>((uint64_t)B, (uint64_t)m_max, io, e->d_cfg, ncfg, e->d_tb,
                                                          e->tb_cap - 1, e->d_win, e->win_cap - 1, e->spill(),
                                                          e->profile, S, parity);
        k_refund_apply<<<grid, REFUND_BLOCK, 0, c>>>(e->d_cfg, ncfg, e->d_tb, e->tb_cap - 1, e->d_win, e->win_cap - 1,
                                                     e->spill(), e->profile, S, parity);
    });
}

extern "C" uint32_t rl_refund_max(rl_engine* e) { return e ? refund_max(e) : 0; }

extern "C" int rl_refund_grid_cap(void) { return REFUND_GRID * REFUND_BLOCK; }

// One refund call (rl_refund.h), ordered as rl_reset_batch_device.  Never
// split: the sum rule holds per call.
extern "C" int rl_refund_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                      const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                                      uint8_t* status, void* stream) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id))) return RL_EINVAL;
    if (m > refund_max(e)) return fail(e, RL_EINVAL, "refund call above rl_refund_max");
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return run_refund(e, m, key_id, ts_ns, n, cfg_id, server_ms, status, s, (e->flags & RL_OPT_PIPELINE) != 0);
}

extern "C" int rl_refund_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                               const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* status) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id))) return RL_EINVAL;
    if (m > refund_max(e)) return fail(e, RL_EINVAL, "refund call above rl_refund_max");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    // one chunk: m <= max_batch, the size of the host API's staging arrays
    int r = stage_in(e, 0, (uint32_t)m, key_id, ts_ns, n, cfg_id, server_ms, s);
    // the staged inputs arrive on s: the kernels always wait for them
    if (r == RL_OK)
        r = run_refund(e, m, e->d_key, e->d_ts, e->d_n, e->d_cfgid, server_ms ? e->d_sms : nullptr,
                       status ? e->d_dec : nullptr, s, false);
    if (r == RL_OK) r = stage_out(e, 0, (uint32_t)m, status, nullptr, nullptr, nullptr, nullptr, s);
    if (r != RL_OK) return r;
    HIPCHK(e, hipStreamSynchronize(s));
    return RL_OK;
}

// --- AllowAll (rl_allow_all.h) -----------------------------------------------

// the engine's AllowAll scratch, allocated by the first call: g, then the
// host form's staging of first, verdict and rollback, rl_allow_all_max each
struct AllowAllBufs {
    int64_t* g;
    uint8_t *first, *verdict, *rollback;
};

static int allow_all_scratch(rl_engine* e, AllowAllBufs* out) {
    auto& A = e->allow_all;
    const size_t M = refund_max(e);
    if (!A.mem && hipMalloc(&A.mem, M * (sizeof(int64_t) + 3)) != hipSuccess) {
        A.mem = nullptr;
        return fail(e, RL_ENOMEM, "AllowAll scratch: out of device memory");
    }
    out->g = (int64_t*)A.mem;
    out->first = (uint8_t*)(out->g + M);
    out->verdict = out->first + M;
    out->rollback = out->verdict + M;
    return RL_OK;
}

static int run_settle(rl_engine* e, size_t m, const uint8_t* first, const uint32_t* cfg, const int64_t* n,
                      const uint8_t* decision, uint8_t* verdict, int64_t* g, hipStream_t s) {
    k_allow_all_settle<<<grid_for(m, ALLOW_ALL_BLOCK, ALLOW_ALL_GRID), ALLOW_ALL_BLOCK, 0, s>>>(
        (uint64_t)m, first, cfg, n, decision, e->d_cfg, (uint32_t)e->h_cfg.size(), verdict, g);
    HIPCHK(e, hipGetLastError());
    return RL_OK;
}

// One AllowAll call of 0 < m <= rl_allow_all_max members with device pointers:
// the decide as one batch (s then sees its results), the settle kernel on s,
// the refund of g as a chain op that always waits for s -- g is made on the
// device, whatever RL_OPT_PIPELINE says of the caller's arrays.
static int run_allow_all(rl_engine* e, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                         const uint32_t* cfg, const int64_t* sms, const uint8_t* first, uint8_t* decision,
                         int64_t* remaining, int64_t* retry, int64_t* reset, double* tokens, uint8_t* verdict,
                         uint8_t* rollback, hipStream_t s) {
    AllowAllBufs B;
    int r = allow_all_scratch(e, &B);
    // the refund's scratch too, before anything is taken: a failed allocation
    // must not leave a decide without its give-back
    RefundScratch S;
    if (r == RL_OK) r = refund_scratch(e, &S);
    if (r == RL_OK) r = rl_decide_batch_device(e, m, key, ts, n, cfg, sms, decision, remaining, retry, reset, tokens, s);
    if (r != RL_OK) return r;
    // the previous call's refund, enqueued from any stream, may still read g:
    // ev_refund is the end of the last refund of any kind on `chain` (a plain
    // refund recorded since only makes the wait later)
    if (e->refund_calls) HIPCHK(e, hipStreamWaitEvent(s, e->ev_refund, 0));
    r = run_settle(e, m, first, cfg, n, decision, verdict, B.g, s);
    if (r == RL_OK) r = run_refund(e, m, key, ts, B.g, cfg, sms, rollback, s, false);
    return r;
}

// the settle kernel on one member read from the staging arrays: no config is
// registered yet, so g = 0; the verdict and g go to staging words.  Nothing is
// allocated.
static int allow_all_warm_up(rl_engine* e) {
    return run_settle(e, 1, e->d_dec, e->d_cfgid, e->d_n, (const uint8_t*)e->d_retry, (uint8_t*)e->d_tok, e->d_rem,
                      e->stream);
}

extern "C" uint32_t rl_allow_all_max(rl_engine* e) { return e ? refund_max(e) : 0; }

extern "C" int rl_allow_all_grid_cap(void) { return ALLOW_ALL_GRID * ALLOW_ALL_BLOCK; }

// The sender's settle of a routed AllowAll (include/rl_route.h): one kernel on
// the caller's stream.  It takes no engine stream, scratch or table, only the
// device config table for `alg`.
extern "C" int rl_allow_all_settle_device(rl_engine* e, size_t m, const uint8_t* first, const uint32_t* cfg_id,
                                          const int64_t* n, const uint8_t* decision, uint8_t* verdict, int64_t* g,
                                          uint8_t* sel, void* stream) {
    if (!e || (m && (!first || !cfg_id || !n || !decision || !verdict || !g || !sel))) return RL_EINVAL;
    if (m > e->max_batch) return fail(e, RL_EINVAL, "routed settle above the engine's max_batch");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    k_allow_all_settle_routed<<<grid_for(m, ALLOW_ALL_BLOCK, ALLOW_ALL_GRID), ALLOW_ALL_BLOCK, 0,
                                (hipStream_t)stream>>>((uint64_t)m, first, cfg_id, n, decision, e->d_cfg,
                                                       (uint32_t)e->h_cfg.size(), verdict, g, sel);
    HIPCHK(e, hipGetLastError());
    return RL_OK;
}

extern "C" int rl_allow_all_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                         const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                                         const uint8_t* first, uint8_t* decision, int64_t* remaining,
                                         int64_t* retry_after_ns, int64_t* reset_at_ns, double* tokens,
                                         uint8_t* verdict, uint8_t* rollback, void* stream) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !first || !decision || !remaining || !retry_after_ns ||
                     !reset_at_ns || !verdict)))
        return RL_EINVAL;
    if (m > refund_max(e)) return fail(e, RL_EINVAL, "AllowAll call above rl_allow_all_max");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return run_allow_all(e, m, key_id, ts_ns, n, cfg_id, server_ms, first, decision, remaining, retry_after_ns,
                         reset_at_ns, tokens, verdict, rollback, s);
}

extern "C" int rl_allow_all_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                  const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                                  const uint8_t* first, uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                                  int64_t* reset_at_ns, double* tokens, uint8_t* verdict, uint8_t* rollback) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !first || !decision || !remaining || !retry_after_ns ||
                     !reset_at_ns || !verdict)))
        return RL_EINVAL;
    if (m > refund_max(e)) return fail(e, RL_EINVAL, "AllowAll call above rl_allow_all_max");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    AllowAllBufs B;
    int r = allow_all_scratch(e, &B);
    if (r != RL_OK) return r;
    HIPCHK(e, hipMemsetAsync(e->d_eflags, 0, 4, s));
    // one chunk: m <= max_batch, the size of the host API's staging arrays
    r = stage_in(e, 0, (uint32_t)m, key_id, ts_ns, n, cfg_id, server_ms, s);
    if (r != RL_OK) return r;
    HIPCHK(e, hipMemcpyAsync(B.first, first, m, hipMemcpyHostToDevice, s));
    // the staged inputs arrive on s; under RL_OPT_PIPELINE the decide's
    // grouping does not wait for s, so they are complete before it is called
    HIPCHK(e, hipStreamSynchronize(s));
    r = run_allow_all(e, m, e->d_key, e->d_ts, e->d_n, e->d_cfgid, server_ms ? e->d_sms : nullptr, B.first, e->d_dec,
                      e->d_rem, e->d_retry, e->d_reset, tokens ? e->d_tok : nullptr, B.verdict,
                      rollback ? B.rollback : nullptr, s);
    if (r == RL_OK) r = stage_out(e, 0, (uint32_t)m, decision, remaining, retry_after_ns, reset_at_ns, tokens, s);
    if (r != RL_OK) return r;
    HIPCHK(e, hipMemcpyAsync(verdict, B.verdict, m, hipMemcpyDeviceToHost, s));
    if (rollback) HIPCHK(e, hipMemcpyAsync(rollback, B.rollback, m, hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    // the sticky device status, as rl_decide_batch returns it (a full table: RL_ENOMEM)
    return rl_engine_sync(e);
}

// --- Charge (rl_charge.h) ----------------------------------------------------

static uint32_t charge_max(const rl_engine* e) { return std::min<uint32_t>(e->max_batch, CHARGE_MAX); }

// the engine's Charge scratch, allocated by the first call: arrays of
// rl_charge_max elements, the 8-byte ones first
static int charge_scratch(rl_engine* e, ChargeScratch* out) {
    auto& A = e->charge;
    const size_t M = charge_max(e);
    if (!A.ev) HIPCHK(e, hipEventCreateWithFlags(&A.ev, hipEventDisableTiming));
    if (!A.mem && hipMalloc(&A.mem, M * (7 * sizeof(int64_t) + 2)) != hipSuccess) {
        A.mem = nullptr;
        return fail(e, RL_ENOMEM, "Charge scratch: out of device memory");
    }
    int64_t* p = (int64_t*)A.mem;
    out->np = p;
    out->ask_reset = p + M;
    out->ask_tok = (double*)(p + 2 * M);
    out->rem = p + 3 * M;
    out->retry = p + 4 * M;
    out->reset = p + 5 * M;
    out->tok = (double*)(p + 6 * M);
    out->dec = (uint8_t*)(p + 7 * M);
    out->kind = out->dec + M;
    return RL_OK;
}

static void launch_charge_ask(rl_engine* e, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                              const uint32_t* cfg, const int64_t* sms, const ChargeScratch& S, hipStream_t c) {
    k_charge_ask<<<grid_for(m, CHARGE_BLOCK, CHARGE_GRID), CHARGE_BLOCK, 0, c>>>(
        (uint64_t)m, key, ts, n, cfg, sms, e->d_cfg, (uint32_t)e->h_cfg.size(), e->d_tb, e->tb_cap - 1, e->profile, S);
}

static int launch_charge_finish(rl_engine* e, size_t m, const int64_t* n, const ChargeScratch& S, uint8_t* decision,
                                int64_t* charged, int64_t* remaining, int64_t* reset, double* tokens, hipStream_t s) {
    k_charge_finish<<<grid_for(m, CHARGE_BLOCK, CHARGE_GRID), CHARGE_BLOCK, 0, s>>>((uint64_t)m, n, S, decision,
                                                                                    charged, remaining, reset, tokens);
    HIPCHK(e, hipGetLastError());
    return RL_OK;
}

// the routed forms: the ask's grid is sized for the bound B, the finish's for
// m_max (it also writes the dropped records past B); both stride
static void launch_charge_ask_routed(rl_engine* e, size_t B, const RoutedIo& io, const ChargeRouted& R,
                                     hipStream_t c) {
    k_charge_ask_routed<<<grid_for(B, CHARGE_BLOCK, CHARGE_GRID), CHARGE_BLOCK, 0, c>>>(
        (uint64_t)B, io, e->d_cfg, (uint32_t)e->h_cfg.size(), e->d_tb, e->tb_cap - 1, e->profile, R);
}

static int launch_charge_finish_routed(rl_engine* e, size_t B, size_t m_max, const RoutedIo& io,
                                       const ChargeRouted& R, hipStream_t s) {
    k_charge_finish_routed<<<grid_for(m_max, CHARGE_BLOCK, CHARGE_GRID), CHARGE_BLOCK, 0, s>>>(
        (uint64_t)B, (uint64_t)m_max, io, R);
    HIPCHK(e, hipGetLastError());
    return RL_OK;
}

// One Charge call of 0 < m <= rl_charge_max requests with device pointers: the
// ask as a chain op ordered like run_peek (s then sees n'), the decide on n' as
// one batch whose grouping always waits for s -- n' is made on the device,
// whatever RL_OPT_PIPELINE says of the caller's arrays -- and the finish kernel
// on s.  The scratch is allocated before anything is enqueued.
static int run_charge(rl_engine* e, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                      const uint32_t* cfg, const int64_t* sms, uint8_t* decision, int64_t* charged,
                      int64_t* remaining, int64_t* reset, double* tokens, hipStream_t s, bool inputs_ready) {
    ChargeScratch S;
    int r = charge_scratch(e, &S);
    if (r != RL_OK) return r;
    // the previous call's finish, enqueued on any stream, may still read the
    // scratch: the ask waits for its end on `chain`, and everything that
    // writes the scratch in this call comes after the ask
    if (e->charge.calls) HIPCHK(e, hipStreamWaitEvent(e->chain, e->charge.ev, 0));
    e->charge.calls++;
    r = chain_op(e, s, inputs_ready, s, e->ev_peek, nullptr,
                 [&](hipStream_t c) { launch_charge_ask(e, m, key, ts, n, cfg, sms, S, c); });
    if (r != RL_OK) return r;
    const ReqArgs a{key, ts, S.np, cfg, sms, S.dec, S.rem, S.retry, S.reset, S.tok};
    r = decide_after_stream(e, (uint32_t)m, a, s);
    if (r == RL_OK) r = launch_charge_finish(e, m, n, S, decision, charged, remaining, reset, tokens, s);
    // recorded also after a failure: whatever was enqueued on s is before it
    HIPCHK(e, hipEventRecord(e->charge.ev, s));
    return r;
}

// both kernels on one request read from the staging arrays: no config is
// registered yet, so the request is invalid and no table is read.  The
// results go to staging words; the scratch stands in the staging arrays too
// (one element each), so nothing is allocated.
static int charge_warm_up(rl_engine* e) {
    const ChargeScratch S{e->d_rem, e->d_reset, e->d_tok, e->d_rem, e->d_retry, e->d_reset, e->d_tok, e->d_dec,
                          (uint8_t*)e->d_sms};
    hipStream_t s = e->stream;
    launch_charge_ask(e, 1, e->d_key, e->d_ts, e->d_n, e->d_cfgid, nullptr, S, s);
    HIPCHK(e, hipGetLastError());
    const int r = launch_charge_finish(e, 1, e->d_n, S, e->d_dec, e->d_retry, e->d_rem, e->d_reset, e->d_tok, s);
    if (r != RL_OK) return r;
    // the routed kernels on an empty batch: they read the zero count and
    // nothing else, so no scratch stands behind the null pointers
    const RoutedIo io{nullptr, nullptr, e->d_zero, nullptr, nullptr, e->d_eflags};
    launch_charge_ask_routed(e, 1, io, ChargeRouted{}, s);
    HIPCHK(e, hipGetLastError());
    return launch_charge_finish_routed(e, 1, 1, io, ChargeRouted{}, s);
}

// the engine's routed Charge scratch, allocated by the first call: arrays of
// rl_charge_max elements by merge position, the widest alignment first
static int charge_routed_scratch(rl_engine* e, ChargeRouted* out) {
    auto& A = e->charge_routed;
    const size_t M = charge_max(e);
    if (!A.ev) HIPCHK(e, hipEventCreateWithFlags(&A.ev, hipEventDisableTiming));
    const size_t each = sizeof(rl_route_rec) + sizeof(rl_route_res) + sizeof(RoutedHalf) + sizeof(int64_t) +
                        sizeof(uint32_t) + sizeof(uint8_t);
    if (!A.mem && hipMalloc(&A.mem, M * each) != hipSuccess) {
        A.mem = nullptr;
        return fail(e, RL_ENOMEM, "routed Charge scratch: out of device memory");
    }
    out->rec2 = (rl_route_rec*)A.mem;
    out->res2 = (rl_route_res*)(out->rec2 + M);
    out->row = (RoutedHalf*)(out->res2 + M);
    out->sms2 = (int64_t*)(out->row + M);
    out->order2 = (uint32_t*)(out->sms2 + M);
    out->kind = (uint8_t*)(out->order2 + M);
    return RL_OK;
}

// enqueue the charge step of the routed path (include/rl_route.h): the merged
// batch as ONE Charge call of bound B = min(m_max, rl_charge_max).
//   ask      k_charge_ask_routed as a chain op ordered like run_routed_op's
//            peek.  It always waits for s: count, order and the store clocks
//            are the merge's outputs there.  It writes the normalised batch
//            (n = n', order2[p] = p, the resolved clocks) and its rows into
//            the engine's scratch; recv is not written.
//   decide   the unchanged routed decide on the scratch, bound B, the caller's
//            own count word.  Its grouping waits for `chain`, where the ask
//            ran, not for a caller's stream; its results are scratch too.
//   finish   k_charge_finish_routed on `tail`, in stream order behind the
//            decide's finish: the result records at the receive indices, and
//            RL_DROPPED past B.
// The end of the finish is recorded into `done` when given, else so waits for
// it.  No stream is added, the host waits for nothing and reads nothing.  The
// scratch is allocated before anything is enqueued; the next routed charge's
// ask waits for this call's finish (charge_routed.ev) before it writes the
// scratch again.  rl_stats moves as for a routed decide of bound B; the flags
// the call can raise are the decide's own and EF_ROUTED_OVER (a count above B).
static int run_charge_routed(rl_engine* e, size_t m_max, const RoutedIo& io, hipStream_t s, hipStream_t so,
                             hipEvent_t done) {
    ChargeRouted R;
    int r = charge_routed_scratch(e, &R);
    if (r != RL_OK) return r;
    auto& A = e->charge_routed;
    const size_t B = std::min<size_t>(m_max, charge_max(e));
    if (A.calls) HIPCHK(e, hipStreamWaitEvent(e->chain, A.ev, 0));
    A.calls++;
    // ev_peek is recorded behind the ask like a peek's; nothing waits for it
    r = chain_op(e, s, false, nullptr, nullptr, e->ev_peek,
                 [&](hipStream_t c) { launch_charge_ask_routed(e, B, io, R, c); });
    if (r != RL_OK) return r;
    r = decide_routed_after_stream(e, (uint32_t)B, R.rec2, R.order2, io.count, R.sms2, R.res2, e->chain, A.ev);
    if (r == RL_OK) r = launch_charge_finish_routed(e, B, m_max, io, R, e->tail);
    // recorded also after a failure: whatever was enqueued on `tail` is before it
    HIPCHK(e, hipEventRecord(A.ev, e->tail));
    if (r != RL_OK) return r;
    if (done) HIPCHK(e, hipEventRecord(done, e->tail));
    else HIPCHK(e, hipStreamWaitEvent(so, A.ev, 0));
    return RL_OK;
}

extern "C" uint32_t rl_charge_max(rl_engine* e) { return e ? charge_max(e) : 0; }

extern "C" int rl_charge_grid_cap(void) { return CHARGE_GRID * CHARGE_BLOCK; }

extern "C" int rl_charge_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                      const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                                      uint8_t* decision, int64_t* charged, int64_t* remaining, int64_t* reset_at_ns,
                                      double* tokens, void* stream) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !decision || !charged || !remaining || !reset_at_ns)))
        return RL_EINVAL;
    if (m > charge_max(e)) return fail(e, RL_EINVAL, "Charge call above rl_charge_max");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = stream ? (hipStream_t)stream : e->stream;
    return run_charge(e, m, key_id, ts_ns, n, cfg_id, server_ms, decision, charged, remaining, reset_at_ns, tokens, s,
                      (e->flags & RL_OPT_PIPELINE) != 0);
}

extern "C" int rl_charge_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                               const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* decision, int64_t* charged,
                               int64_t* remaining, int64_t* reset_at_ns, double* tokens) {
    if (!e || (m && (!key_id || !ts_ns || !n || !cfg_id || !decision || !charged || !remaining || !reset_at_ns)))
        return RL_EINVAL;
    if (m > charge_max(e)) return fail(e, RL_EINVAL, "Charge call above rl_charge_max");
    if (m == 0) return RL_OK;
    (void)hipSetDevice(e->device);
    hipStream_t s = e->stream;
    HIPCHK(e, hipMemsetAsync(e->d_eflags, 0, 4, s));
    // one chunk: m <= max_batch, the size of the host API's staging arrays
    int r = stage_in(e, 0, (uint32_t)m, key_id, ts_ns, n, cfg_id, server_ms, s);
    // the staged inputs arrive on s: the ask always waits for them.  `charged`
    // is staged through the array a decide stages retry_after_ns through
    if (r == RL_OK)
        r = run_charge(e, m, e->d_key, e->d_ts, e->d_n, e->d_cfgid, server_ms ? e->d_sms : nullptr, e->d_dec,
                       e->d_retry, e->d_rem, e->d_reset, tokens ? e->d_tok : nullptr, s, false);
    if (r == RL_OK) r = stage_out(e, 0, (uint32_t)m, decision, remaining, charged, reset_at_ns, tokens, s);
    if (r != RL_OK) return r;
    HIPCHK(e, hipStreamSynchronize(s));
    // the sticky device status, as rl_decide_batch returns it (a full table: RL_ENOMEM)
    return rl_engine_sync(e);
}
