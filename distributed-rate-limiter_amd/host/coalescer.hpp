// coalescer.hpp -- request coalescer in front of the decision engine
// (include/rl_coalescer.h has the policy, ordering and context contract).
//
// The reference's Limiter.AllowN is one Redis EVAL per call
// (tokenbucket.go:172, slidingwindow.go:164, fixedwindow.go:152); the north
// star's BatchAllow path gathers concurrent calls into GPU batches
// (SURVEY.md §8b, §8f rank 1).  Threads: callers submit and wait; one
// submitter thread forms batches and launches them (and runs the ordered
// table operations); one completer thread waits for each launch in order and
// hands results back.
#pragma once

#include <stdint.h>
#include <string.h>

#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/rl_coalescer.h"
#include "../../include/rl_snapshot.h"

namespace rlc {

enum Op : uint8_t { OP_REQ, OP_RESET, OP_PEEK, OP_REFUND, OP_ALLOW_ALL, OP_CHARGE, OP_INFO, OP_GC, OP_SNAPSHOT, OP_RESTORE, OP_TALLY, OP_HOT, OP_COUNT };

// the coalescer's counters and a host backend's functions: the C structs of
// include/rl_coalescer.h with their trailing Charge members, laid out as
// rl_coalescer_stats_charge / rl_coalescer_backend_charge
struct Counters : rl_coalescer_stats {
    uint64_t charge_launches = 0;
};
static_assert(sizeof(Counters) == sizeof(rl_coalescer_stats_charge), "Counters is rl_coalescer_stats_charge");
struct BackendFns : rl_coalescer_backend {
    rl_charge_fn charge = nullptr;
};
static_assert(sizeof(BackendFns) == sizeof(rl_coalescer_backend_charge), "BackendFns is rl_coalescer_backend_charge");

// What the queue, the launch and the counters do with a submission of each
// operation: stated once here and read everywhere else (a `switch (op)` stays
// only where the action itself differs: which backend call runs).
using StatField = uint64_t Counters::*;
struct OpTraits {
    // carries requests through a launch slot (Submit); the others are single
    // table operations, run synchronously on the submitter thread (SubmitOp)
    bool batched;
    bool reads_n;          // `n` is an input (a reset has none)
    // dec, rem, retry and reset come back; else only a per-request status in
    // `dec`, which is copied back -- and its RL_RESET_DONE / RL_REFUND_DONE
    // (one code) counted into `completed` -- only when the launch succeeded
    bool results;
    bool merges;           // the run of adjacent same-op submissions at the queue head is one launch
    bool splits;           // taken in parts of up to max_batch (else whole: m > max_batch is RL_EINVAL)
    bool queue_cap;        // a full queue refuses it
    // a decision: the automatic GC budgets it before its launch, the linger
    // waits for more of it, it counts in submitted / cancelled / expired
    bool decides;
    bool counts_batch;     // its launch counts in `batches` ...
    bool counts_max;       // ... and in `max_batch_seen`
    StatField launches;    // its own launch counter, if any
    StatField completed;   // at completion: += m (results), or += the statuses that say done
    bool keeps_gc_count;   // a table operation that touches no table: the automatic GC's count still holds
    // its requests come in groups: `first` goes in with them, `verdict` comes
    // back with the results, and the groups launched count in allow_all_groups
    bool grouped;
};
constexpr StatField NO_STAT = nullptr;
using St = Counters;
constexpr OpTraits OPS[OP_COUNT] = {
    //              batched reads_n results merges splits q_cap  decides batch  max    launches                 completed      keeps_gc grouped
    /* REQ       */ {true,  true,   true,   true,  true,  true,  true,   true,  true,  NO_STAT,                 &St::decided,  false,   false},
    /* RESET     */ {true,  false,  false,  true,  true,  false, false,  true,  false, &St::reset_launches,     &St::resets,   false,   false},
    /* PEEK      */ {true,  true,   true,   false, true,  true,  false,  false, false, NO_STAT,                 &St::peeked,   false,   false},
    /* REFUND    */ {true,  true,   false,  false, false, true,  false,  false, false, &St::refund_launches,    &St::refunds,  false,   false},
    /* ALLOW_ALL */ {true,  true,   true,   false, false, true,  true,   false, false, &St::allow_all_launches, &St::decided,  false,   true},
    /* CHARGE    */ {true,  true,   true,   false, false, true,  true,   false, false, &St::charge_launches,    &St::decided,  false,   false},
    /* INFO      */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       false,   false},
    /* GC        */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       false,   false},
    /* SNAPSHOT  */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       false,   false},
    /* RESTORE   */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       false,   false},
    /* TALLY     */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       true,    false},
    /* HOT       */ {false, false,  false,  false, false, false, false,  false, false, NO_STAT,                 NO_STAT,       true,    false},
};

// the SoA arrays of one block of requests and results
struct Arrays {
    uint64_t* key = nullptr;
    int64_t* ts = nullptr;
    int64_t* n = nullptr;
    uint32_t* cfg = nullptr;
    uint8_t* dec = nullptr;
    int64_t* rem = nullptr;
    int64_t* retry = nullptr;
    int64_t* reset = nullptr;
    uint8_t* head = nullptr;      // a grouped operation's group heads, `first` of the C-ABI (in) ...
    uint8_t* verdict = nullptr;   // ... and its per-member group verdict (out)
};
// The one layout of such a block -- a slot's pinned host block, its device
// block, a host backend's heap block, a submission's buffer --, by capacity:
// key ts n | cfg | rem retry reset | dec | head | verdict, the result area
// 64-byte aligned (the device path needs that).  block_bytes(cap) holds it.
// head and verdict, which only a grouped operation uses, come last: the
// offsets of the others, and the plain path's copies, do not depend on them.
constexpr size_t block_bytes(size_t cap) { return cap * 63 + 64; }
inline void carve(uint8_t* p, size_t cap, Arrays& a) {
    a.key = reinterpret_cast<uint64_t*>(p);
    a.ts = reinterpret_cast<int64_t*>(p + 8 * cap);
    a.n = reinterpret_cast<int64_t*>(p + 16 * cap);
    a.cfg = reinterpret_cast<uint32_t*>(p + 24 * cap);
    uint8_t* q = p + ((28 * cap + 63) & ~size_t(63));
    a.rem = reinterpret_cast<int64_t*>(q);
    a.retry = reinterpret_cast<int64_t*>(q + 8 * cap);
    a.reset = reinterpret_cast<int64_t*>(q + 16 * cap);
    a.dec = q + 24 * cap;
    a.head = q + 25 * cap;
    a.verdict = q + 26 * cap;
}

// one launch's staging buffers (host side; pinned for the GPU backend)
struct Slot : Arrays {
    size_t m = 0;
    Op op = OP_REQ;   // of the submissions it was formed from: one operation per launch
    int status = RL_OK;
    int64_t t_form = 0, t_h2d = 0, t_launched = 0;   // steady ns (batch trace)
    struct Part {
        struct Sub* sub;
        size_t off, count, at;   // sub[off, off+count) <-> slot[at, at+count)
    };
    std::vector<Part> parts;
};

// OP_TALLY arguments (rl_tally_read's): the caller's buffers (it blocks until
// the operation is done)
struct TallyArgs {
    rl_tally_cfg* cfg_out = nullptr;
    size_t cfg_cap = 0;
    uint32_t* ncfg = nullptr;
    rl_tally_key* key_out = nullptr;
    size_t key_cap = 0;
    uint64_t* keys_tracked = nullptr;
    rl_tally_info* info = nullptr;
    int clear = 0;
};

// OP_HOT arguments (rl_hot_read's), as TallyArgs
struct HotArgs {
    rl_hot_key* key_out = nullptr;
    size_t key_cap = 0;
    uint64_t* keys_tracked = nullptr;
    rl_hot_info* info = nullptr;
    int clear = 0;
};

// OP_SNAPSHOT / OP_RESTORE arguments: the caller's buffers (it blocks until
// the operation is done)
struct SnapArgs {
    void* buf = nullptr;              // OP_SNAPSHOT: written; OP_RESTORE: read
    size_t len = 0;
    uint32_t world = 1, rank = 0;
    rl_snapshot_info* out = nullptr;  // OP_SNAPSHOT
};

// one table operation's arguments (SubmitOp); each operation reads its own
struct OpArgs {
    int64_t now_ms = 0;                 // OP_INFO, OP_GC, OP_SNAPSHOT, OP_RESTORE
    uint64_t cap_tb = 0, cap_win = 0;   // OP_GC, OP_RESTORE
    SnapArgs snap;                      // OP_SNAPSHOT, OP_RESTORE
    TallyArgs tally;                    // OP_TALLY
    HotArgs hot;                        // OP_HOT
};

// Hand a versioned struct (its first field: uint32_t struct_size) to a caller
// that may have been compiled with a shorter one: the bytes the caller's
// struct_size covers, with struct_size = the bytes filled in.
template <class T>
inline void copy_out_sized(T* out, T v) {
    v.struct_size = (uint32_t)(out->struct_size < sizeof v ? out->struct_size : sizeof v);
    memcpy(out, &v, v.struct_size);
}

// where batches go: the GPU engine, or synchronous host functions (tests)
class Backend {
public:
    virtual ~Backend() = default;
    // usage tally (rl_coalescer_opts.tally_key_slots): once enabled, launch()
    // counts every OP_REQ batch behind its decisions, before wait(slot) returns
    virtual int tally_enable(uint32_t key_slots) = 0;
    // rl_tally_read: every batch launched so far is counted (synchronous)
    virtual int tally_read(const TallyArgs& a) = 0;
    // top keys (rl_coalescer_opts.hot_min): once enabled, launch() counts every
    // OP_REQ batch behind its decisions (and behind its tally), as one rl_hot_batch call
    virtual int hot_enable(const rl_hot_opts& o) = 0;
    // rl_hot_read: every batch launched so far is counted (synchronous)
    virtual int hot_read(const HotArgs& a) = 0;
    virtual int init(int nslots, size_t max_batch, std::vector<Slot>* slots) = 0;
    // The slot's s.m requests of operation s.op, asynchronous: after every
    // launch before it and before every later one, completed through
    // wait(slot).  OP_REQ: decisions (rl_decide_batch_device); OP_PEEK:
    // read-only queries (rl_peek_batch_device); OP_RESET: resets (key, ts, cfg;
    // rl_reset_batch_device) and OP_REFUND: one refund call
    // (rl_refund_batch_device), both with the per-request status into s.dec;
    // OP_ALLOW_ALL: one AllowAll call (rl_allow_all_batch_device), s.head in,
    // s.verdict out beside the decide's results; OP_CHARGE: one Charge call
    // (rl_charge_batch_device), `charged` where a decide's retry_after_ns goes
    virtual int launch(int slot, Slot& s) = 0;
    virtual int wait(int slot, Slot& s) = 0;     // until launch `slot` completed
    // synchronous table operations (the GPU engine drains its batches first)
    virtual int table_info(int64_t now_ms, rl_table_info* out) = 0;
    virtual int gc(int64_t now_ms, uint64_t tb_cap, uint64_t win_cap, rl_table_info* out) = 0;
    // state snapshots (include/rl_snapshot.h): the GPU engine only
    virtual int snapshot(int64_t now_ms, uint32_t world, uint32_t rank, void* buf, size_t cap,
                         rl_snapshot_info* out) {
        (void)now_ms, (void)world, (void)rank, (void)buf, (void)cap, (void)out;
        return RL_EINVAL;
    }
    virtual int restore(const void* buf, size_t len, int64_t now_ms, uint64_t tb_cap, uint64_t win_cap,
                        rl_table_info* out) {
        (void)buf, (void)len, (void)now_ms, (void)tb_cap, (void)win_cap, (void)out;
        return RL_EINVAL;
    }
    // the table a config's keys live in (0 token bucket, 1 window), or -1
    // when unknown (the automatic GC then counts the request against both)
    virtual int table_of(uint32_t cfg) { (void)cfg; return -1; }
};

std::unique_ptr<Backend> make_gpu_backend(rl_engine* e);
std::unique_ptr<Backend> make_fn_backend(const BackendFns& b);

// one submission: its requests (copied) and results, or one table operation
struct Sub : Arrays {
    uint64_t first = 0;
    size_t m = 0, taken = 0, left = 0;
    int status = RL_OK;
    Op op = OP_REQ;
    int64_t deadline = 0;         // steady ns; 0 = none
    bool done = false;
    bool waiting = false;         // a caller blocks on cv (else completion skips the wake)
    bool cancelled = false;       // rl_coalescer_cancel before completion
    bool dropped = false;         // completed unapplied (deadline / cancel before launch)
    bool truncated = false;       // launched in part; the rest dropped (deadline / cancel): no results
    bool in_queue = false;        // queue_ still holds it (the submitter pops it)
    bool waited = false;          // the caller released its ticket
    uint32_t inflight = 0;        // slot parts launched, not completed
    int64_t done_ns = 0;          // steady clock at completion
    int64_t submit_ns = 0;        // steady clock at Submit (batch trace)
    void* tag = nullptr;          // the caller's completion tag (SetNotify)
    OpArgs args;                  // a table operation's arguments ...
    rl_table_info info{};         // ... and the result of OP_INFO / OP_GC / OP_RESTORE
    std::condition_variable cv;
    std::unique_ptr<uint8_t[]> mem;
    size_t cap = 0;               // requests the buffer holds (pooled Subs are reused)
    explicit Sub(size_t m);
    void renew(size_t m);         // reset for a new submission of m <= cap requests
};

int64_t steady_ns();

// One launched batch, for stall attribution (RL_COALESCER_TRACE=<ring size>):
// steady-clock ns of the oldest request's Submit, the batch taken from the
// queue, inputs on the device (H2D done), the engine call returned, the
// completer starting to wait, and the results back on the host.
struct BatchTrace {
    uint64_t seq;
    uint64_t m;
    int64_t t_submit, t_form, t_h2d, t_launched, t_wait, t_done;
};

class Coalescer {
public:
    Coalescer(std::unique_ptr<Backend> be, const rl_coalescer_opts& o);
    ~Coalescer();
    int start();
    // tag: with SetNotify, the completion callback receives it
    // op: one with OPS[op].batched.  OP_REQ, or OP_PEEK -- read-only queries,
    // queued in sequence order like a Reset and launched on their own (not
    // merged with requests or with other peeks); not counted in submitted /
    // decided --, or OP_RESET: m resets (n is not read), merged with the reset
    // submissions next to it in the queue into one launch; Wait's `dec`
    // receives their status; or OP_REFUND: one refund call of m <= max_batch
    // requests, launched whole and on its own; Wait's `dec` receives the status;
    // or OP_ALLOW_ALL: one AllowAll call of m <= max_batch members in the
    // groups `first` marks, launched whole and on its own, counted like
    // requests; Wait's `verdict` receives each member's group verdict; or
    // OP_CHARGE: one Charge call of m <= max_batch requests, launched whole and
    // on its own, counted like requests; Wait's `retry` receives `charged`
    int Submit(size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n, const uint32_t* cfg,
               uint64_t* ticket, int64_t deadline = 0, void* tag = nullptr, Op op = OP_REQ,
               const uint8_t* first = nullptr);
    // one table operation (an op without OPS[op].batched: table count, table
    // GC, snapshot, restore, tally read, top-keys read), queued in sequence
    // order; never refused by a full queue
    int SubmitOp(Op op, const OpArgs& a, uint64_t* ticket, void* tag = nullptr);
    // rl_coalescer_opts.tally_key_slots != 0
    bool TallyOn() const { return o_.tally_key_slots != 0; }
    // rl_coalescer_opts.hot_min != 0
    bool HotOn() const { return o_.hot_min != 0; }
    // the largest launch: a refund submission above it is refused
    size_t MaxBatch() const { return o_.max_batch; }
    // Completion callback for submissions made with a tag: fn(user, ticket,
    // tag) runs once when the submission is done (applied, failed, or dropped
    // unapplied), on a coalescer thread (or the thread of a Cancel / Wait that
    // dropped it) WITH THE COALESCER LOCK HELD: it must only hand the ticket
    // to its owner (an event loop then collects it with Wait(ticket, 0, ...))
    // and never call back into the coalescer.  Set before the first tagged
    // submission.
    using NotifyFn = void (*)(void* user, uint64_t ticket, void* tag);
    void SetNotify(NotifyFn fn, void* user);
    int Cancel(uint64_t ticket);
    // done_ns (optional): steady-clock completion time of the submission;
    // info (optional): an OP_INFO / OP_GC result
    int Wait(uint64_t ticket, int64_t timeout_ns, uint8_t* dec, int64_t* rem, int64_t* retry, int64_t* reset,
             int64_t* done_ns = nullptr, rl_table_info* info = nullptr, uint8_t* verdict = nullptr);
    Counters Stats();
    void Shutdown();
    // the trace ring, oldest first (empty unless RL_COALESCER_TRACE is set)
    std::vector<BatchTrace> Trace();

private:
    void submitter();
    void completer();
    // queue `s`, filled in but for its ticket, as `m` pending requests (a
    // table operation: 1); refused -- and released -- when the coalescer is
    // closed or, for an operation a full queue refuses, the queue is full
    int enqueue(Sub* s, size_t m, uint64_t* ticket);
    // The part of `s` not launched yet ends with `code` (its deadline passed,
    // or it was cancelled) and is never applied.  Nothing launched: the
    // submission is dropped, done.  A submission split across launches, partly
    // launched (applied, as an EVAL already sent): that part completes as
    // usual, and the submitter pops the submission when it reaches the head
    // of the queue (taken = m stops it)
    void end_unlaunched_locked(Sub* s, int code);
    // a submission became done at `now` (lock held): its waiter and the completion callback
    void finish_locked(Sub* s, int64_t now) {
        s->done = true;
        s->done_ns = now;
        if (s->waiting) s->cv.notify_all();
        notify_locked(s);
    }
    void notify_locked(Sub* s) {
        if (notify_ && s->tag) notify_(notify_user_, s->first, s->tag);
    }
    NotifyFn notify_ = nullptr;
    void* notify_user_ = nullptr;
    // the submitter takes the queue's first submission off it (lock held)
    Sub* pop_front_locked() {
        Sub* s = queue_.front();
        queue_.pop_front();
        s->in_queue = false;
        return s;
    }
    // free a submission no one references any more (queue, slots, caller)
    void maybe_free_locked(Sub* s);
    // automatic GC before launching `s` (submitter thread, lock not held)
    void auto_gc(const Slot& s);
    // run a synchronous table operation (submitter thread, lock not held)
    int run_table_op(Sub* op);
    // pooled submissions: no heap allocation (and no mmap / page faults for
    // large ones) per Submit in steady state
    Sub* get_sub(size_t m);
    void put_sub(Sub* s);
    std::mutex pool_mu_;
    std::vector<Sub*> pool_;

    std::unique_ptr<Backend> be_;
    rl_coalescer_opts o_;
    std::vector<Slot> slots_;
    std::mutex mu_;
    std::condition_variable cv_sub_, cv_done_, cv_space_;
    std::deque<Sub*> queue_;                       // submissions with requests not yet launched
    std::unordered_map<uint64_t, Sub*> subs_;      // by ticket, until waited for
    std::deque<int> launched_;                     // slots on the device, in launch order
    uint64_t next_seq_ = 0, pending_ = 0;
    int inflight_ = 0, next_slot_ = 0;
    bool stop_ = false, sub_exited_ = false;
    bool sub_idle_ = false;        // the submitter sleeps on cv_sub_ (submit wakes it only then)
    Counters st_{};
    std::vector<BatchTrace> trace_;   // ring of trace_cap_ batches
    size_t trace_cap_ = 0;
    uint64_t done_batches_ = 0;
    // automatic GC (submitter thread only)
    int64_t gc_last_check_ = 0;       // steady ns
    // requests launched since the last count that may insert into the
    // token-bucket table [0] / the window and spill tables [1], and how many
    // cannot fill them past gc_high_pct
    uint64_t gc_launched_[2] = {0, 0};
    uint64_t gc_budget_[2] = {0, 0};
    bool gc_counted_ = false;         // a first count was taken
    std::thread t_sub_, t_done_;
};

// the C++ object behind a C-ABI handle (bench_e2e reads completion times)
Coalescer* unwrap(rl_coalescer* c);

}  // namespace rlc
