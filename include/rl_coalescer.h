/*
 * rl_coalescer.h -- request coalescing in front of the decision engine.
 *
 * The reference decides one request per Redis round trip: every
 * Limiter.Allow/AllowN (tokenbucket.go:90-133, slidingwindow.go:68-122,
 * fixedwindow.go:65-115) is one client.Eval.  The north star's BatchAllow path
 * (internal/ratelimiter + cmd/server; the planned
 * gRPC service of docs/ARCHITECTURE.md:287-304) instead gathers concurrent
 * calls into GPU batches.  This is that coalescer, as a C-ABI a cgo layer can
 * call from many goroutines (no callbacks into the caller, no caller pointers
 * retained after a call returns).
 *
 * Policy: one submitter thread owns the engine.  Whenever fewer than
 * `max_in_flight` batches are on the GPU and requests are pending, it takes up
 * to `max_batch` of them (after lingering up to `linger_ns` for more when the
 * GPU is idle) and launches them as one batch.  Light load therefore sees
 * batches of one or a few requests and the latency of one launch sequence;
 * under heavy load the queue grows while the GPU works and batches grow to
 * `max_batch`.
 *
 * Order: every submitted request gets a global sequence number under the
 * queue lock; batches take requests in sequence order and the engine replays
 * batches in launch order, so the decisions are those of the reference
 * limiter receiving the requests one by one in sequence order.  A ticket is
 * the sequence number of the first request of its submission.  Reset, table
 * GC and table counts are queued like requests and take effect exactly
 * between the requests submitted before and after them.
 *
 * Contexts ("All methods should respect context cancellation and deadlines",
 * interface.go:75).  A submission may carry a deadline, and may be cancelled
 * (ctx.Done()).  go-redis checks the context before it sends a command and
 * returns ctx.Err() while it waits for the reply; the limiter then takes its
 * error branch, fail-open or fail-closed (tokenbucket.go:100-112,
 * slidingwindow.go:84-96, fixedwindow.go:80-92).  The coalescer does the same:
 *   - a submission none of whose requests has been launched when its deadline
 *     passes or when it is cancelled is dropped: it never reaches the state
 *     table (an EVAL never sent);
 *   - one already (partly) launched is applied in full (an EVAL already sent),
 *     but its waiter returns at the deadline / on cancellation all the same;
 *   - the wait returns RL_EDEADLINE (context.DeadlineExceeded) or
 *     RL_ECANCELED (context.Canceled); the caller maps it to the fail-open or
 *     fail-closed result exactly as for any other storage error.
 * Deadlines are on the clock rl_coalescer_now_ns() reads (CLOCK_MONOTONIC);
 * a Go caller converts with deadline_ns = rl_coalescer_now_ns() +
 * time.Until(d).
 *
 * ABI: every struct below starts with `struct_size`, which the caller sets to
 * sizeof the struct it was compiled with.  Inputs of an unknown size are
 * rejected with RL_EINVAL; outputs are written up to the caller's size.
 */
#ifndef RL_COALESCER_H
#define RL_COALESCER_H

#include <stddef.h>
#include <stdint.h>

#include "rl_engine.h"
#include "rl_snapshot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RL_EAGAIN     (-11)   /* queue full (rl_coalescer_opts.queue_cap) */
#define RL_ECLOSED    (-32)   /* coalescer destroyed / shutting down */
#define RL_EDEADLINE  (-62)   /* the submission's deadline passed (context.DeadlineExceeded) */
#define RL_ECANCELED (-125)   /* the submission was cancelled (context.Canceled) */

typedef struct rl_coalescer rl_coalescer;

typedef struct rl_coalescer_opts {
    uint32_t struct_size;    /* sizeof(rl_coalescer_opts) */
    uint32_t max_batch;      /* requests per launch (<= the engine's max_batch); 0 = 65536 */
    uint32_t max_in_flight;  /* batches on the GPU at once, 1..3; 0 = 3 */
    uint32_t gc_high_pct;    /* automatic GC: collect when a table's used slots pass this % (0 = 50) */
    int64_t  linger_ns;      /* with the GPU idle, wait this long for more requests (0 = launch at once) */
    uint64_t queue_cap;      /* pending requests beyond which submit returns RL_EAGAIN; 0 = 1 << 24 */
    /* Automatic table GC (Redis's active expiry; the TTLs of tokenbucket.go:170,
     * fixedwindow.go:151, slidingwindow.go:161-162).  0 = off.  Otherwise the
     * submitter counts the tables' slots (rl_table_info_get) at least every
     * gc_interval_ns, and sooner when the requests launched since the last count
     * could have filled the headroom to gc_high_pct; a table past gc_high_pct is
     * collected (rl_table_gc) at server clock floor(t / 1e6) - gc_margin_ms, t =
     * the time of the last request launched, and doubled first (up to the
     * gc_max_* capacities) when its live keys fill more than half of
     * gc_high_pct.  Exact while no later request carries a time more than
     * gc_margin_ms older than an earlier one. */
    int64_t  gc_interval_ns;
    int64_t  gc_margin_ms;         /* 0 = 1000 */
    uint64_t gc_max_tb_capacity;   /* growth limits (0 = no limit but the engine's) */
    uint64_t gc_max_win_capacity;
    /* Usage tally (rl_tally_*, rl_engine.h): 0 = off; otherwise the records of
     * the throttled-key table (rounded up to a power of 2, 16 .. 1<<24), and
     * every launched batch of requests is counted behind its decisions (a
     * caller compiled before this field passes the shorter struct_size: off) */
    uint32_t tally_key_slots;
    /* Top keys (rl_hot_*, rl_engine.h): hot_min == 0 = off; otherwise
     * rl_hot_opts' width, key_slots, weight and hot_min, and every launched
     * batch of requests is counted behind its decisions, after the tally when
     * both are on (a caller compiled before these fields passes a shorter
     * struct_size: off) */
    uint32_t hot_width;
    uint32_t hot_key_slots;
    uint32_t hot_weight;
    uint64_t hot_min;
} rl_coalescer_opts;

typedef struct rl_coalescer_stats {
    uint32_t struct_size;    /* sizeof(rl_coalescer_stats) */
    uint32_t pad_;
    uint64_t submitted;      /* requests accepted */
    uint64_t decided;        /* requests completed (applied, or failed by the engine) */
    uint64_t batches;        /* launches */
    uint64_t max_batch_seen; /* largest launch */
    uint64_t pending;        /* requests queued, not yet launched */
    uint64_t expired;        /* requests dropped unapplied: deadline passed before launch */
    uint64_t cancelled;      /* requests dropped unapplied: cancelled before launch */
    uint64_t gc_runs;        /* table GCs (automatic and rl_coalescer_gc) */
    uint64_t gc_checks;      /* automatic occupancy counts */
    uint64_t gc_failures;    /* GCs that returned an error (the old tables stay) */
    uint64_t peeked;         /* read-only queries completed (rl_coalescer_peek); not in submitted / decided */
    uint64_t resets;         /* resets executed (rl_coalescer_reset / _reset_batch); not in submitted / decided */
    uint64_t reset_launches; /* launches they took: a run of adjacent reset submissions is one launch */
    uint64_t refunds;        /* refund requests that contributed (RL_REFUND_DONE; rl_coalescer_refund); not in
                                submitted / decided */
    uint64_t refund_launches; /* refund submissions launched: one launch each, never merged */
    uint64_t allow_all_groups;   /* groups of the AllowAll submissions launched (rl_coalescer_allow_all); their
                                    members count in submitted / decided */
    uint64_t allow_all_launches; /* AllowAll submissions launched: one launch each, never merged; not in batches */
} rl_coalescer_stats;

/* rl_coalescer_stats with Charge's trailing counter, filled in by
 * rl_coalescer_get_stats_charge: the caller sets s.struct_size to sizeof the
 * whole struct.  rl_coalescer_get_stats keeps writing rl_coalescer_stats as it
 * stands above and no more, whatever size a caller passes: callers compiled
 * against it rely on the size it reports. */
typedef struct rl_coalescer_stats_charge {
    rl_coalescer_stats s;
    uint64_t charge_launches;    /* Charge submissions launched (rl_coalescer_charge): one launch each, never
                                    merged; not in batches.  Their requests count in submitted / decided */
} rl_coalescer_stats_charge;

/* Signature of rl_decide_batch (host arrays, synchronous).  A backend of this
 * type replaces the GPU in rl_coalescer_create_with_backend: the CPU tests
 * use it to check the batching and ordering logic on hosts without a GPU. */
typedef int (*rl_batch_fn)(void* user, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                           const int64_t* n, const uint32_t* cfg_id, uint8_t* decision, int64_t* remaining,
                           int64_t* retry_after_ns, int64_t* reset_at_ns);
/* Reset(ctx, key) for the test seam's host backend (rl_reset's signature) */
typedef int (*rl_reset_fn)(void* user, uint32_t cfg_id, uint64_t key_id, int64_t ts_ns);
/* rl_reset_batch's signature: m resets, per-request status (RL_RESET_DONE / RL_INVALID; never null here) */
typedef int (*rl_reset_batch_fn)(void* user, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                 const uint32_t* cfg_id, uint8_t* status);
/* rl_refund_batch's signature without the store clock (floor(ts_ns / 1e6)): one refund call, per-request
 * status (RL_REFUND_DONE / RL_REFUND_NOKEY / RL_INVALID; never null here) */
typedef int (*rl_refund_fn)(void* user, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                            const uint32_t* cfg_id, uint8_t* status);
/* rl_allow_all_batch's signature without the store clock, the tokens and the rollback: one AllowAll call
 * (decide, settle, refund) */
typedef int (*rl_allow_all_fn)(void* user, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                               const uint32_t* cfg_id, const uint8_t* first, uint8_t* decision, int64_t* remaining,
                               int64_t* retry_after_ns, int64_t* reset_at_ns, uint8_t* verdict);
/* rl_charge_batch's signature without the store clock and the tokens: one Charge call (ask, decide, result) */
typedef int (*rl_charge_fn)(void* user, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                            const uint32_t* cfg_id, uint8_t* decision, int64_t* charged, int64_t* remaining,
                            int64_t* reset_at_ns);
/* table counts / GC for the host backend (rl_table_info_get / rl_table_gc) */
typedef int (*rl_info_fn)(void* user, int64_t now_ms, rl_table_info* out);
typedef int (*rl_gc_fn)(void* user, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity,
                        rl_table_info* out);

/* A host backend (test seam): batch is required, the rest nullable (the
 * matching operation then fails with RL_EINVAL). */
typedef struct rl_coalescer_backend {
    uint32_t struct_size;    /* sizeof(rl_coalescer_backend) */
    rl_batch_fn batch;
    rl_reset_fn reset;
    rl_info_fn table_info;
    rl_gc_fn gc;
    void* user;
    rl_batch_fn peek;        /* rl_peek_batch: must leave the backend's state unchanged (a caller compiled
                                before this field passes the shorter struct_size: no peek) */
    rl_reset_batch_fn reset_batch; /* nullable (and absent from a shorter struct): resets then go through
                                      `reset`, one call per key; its RL_EINVAL is that request's RL_INVALID */
    rl_refund_fn refund;     /* nullable (and absent from a shorter struct): rl_coalescer_refund is then
                                RL_EINVAL */
    rl_allow_all_fn allow_all; /* nullable (and absent from a shorter struct): rl_coalescer_allow_all is then
                                  RL_EINVAL */
} rl_coalescer_backend;

/* rl_coalescer_backend with Charge's trailing function: pass &x.b with
 * x.b.struct_size = sizeof x.  rl_coalescer_backend above is the struct up to
 * allow_all, as a caller compiled before Charge passes it. */
typedef struct rl_coalescer_backend_charge {
    rl_coalescer_backend b;
    rl_charge_fn charge;     /* nullable (and absent from a shorter struct): rl_coalescer_charge is then
                                RL_EINVAL */
} rl_coalescer_backend_charge;

/* Coalescer over a GPU engine, on the device current on the calling thread
 * (the engine's: rl_engine_create makes it current).  The engine should be created with
 * RL_OPT_PIPELINE (batch b+1's grouping then overlaps batch b's replay) and
 * must not be used by anyone else while the coalescer lives. */
int rl_coalescer_create(rl_engine* e, const rl_coalescer_opts* opts, rl_coalescer** out);
/* Test seam: the same coalescer over a synchronous host backend. */
int rl_coalescer_create_with_host_backend(const rl_coalescer_backend* be, const rl_coalescer_opts* opts,
                                          rl_coalescer** out);
/* shorthands of the above: batch only / batch + reset */
int rl_coalescer_create_with_backend(rl_batch_fn fn, void* user, const rl_coalescer_opts* opts,
                                     rl_coalescer** out);
int rl_coalescer_create_with_backends(rl_batch_fn fn, rl_reset_fn reset_fn, void* user,
                                      const rl_coalescer_opts* opts, rl_coalescer** out);
/* Completes the queued requests, then stops the threads and frees every
 * submission not yet waited for.  No rl_coalescer_wait may be in progress. */
int rl_coalescer_destroy(rl_coalescer* c);

/* the clock deadlines are measured on (CLOCK_MONOTONIC, ns) */
int64_t rl_coalescer_now_ns(void);

/* Enqueue m requests (copied; thread-safe, never blocks on the GPU).
 * *ticket = sequence number of the first request. */
int rl_coalescer_submit(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                        const int64_t* n, const uint32_t* cfg_id, uint64_t* ticket);
/* ... with a deadline (rl_coalescer_now_ns clock; 0 = none): see Contexts above */
int rl_coalescer_submit_deadline(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                 const int64_t* n, const uint32_t* cfg_id, int64_t deadline_ns,
                                 uint64_t* ticket);
/* ctx.Done(): a submission not launched yet is dropped unapplied; a launched
 * one is applied and its results discarded.  Its wait (in progress or later)
 * returns RL_ECANCELED at once; the ticket is still waited for exactly once.
 * No effect on a submission already complete.  RL_EINVAL: unknown ticket. */
int rl_coalescer_cancel(rl_coalescer* c, uint64_t ticket);
/* Block until the submission `ticket` is decided (timeout_ns < 0: no limit)
 * and copy its results out (in submission order).  Each ticket is waited for
 * exactly once.  Returns the engine status of its batch(es); RL_EDEADLINE /
 * RL_ECANCELED (ticket released, outputs untouched); RL_ETIMEOUT when
 * timeout_ns ran out first (the ticket stays valid: wait again); RL_EINVAL for
 * an unknown ticket. */
int rl_coalescer_wait(rl_coalescer* c, uint64_t ticket, int64_t timeout_ns, uint8_t* decision,
                      int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns);
/* submit(1) + wait: what one Limiter.AllowN call does */
int rl_coalescer_decide(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, int64_t n, uint32_t cfg_id,
                        uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns);
/* ... with a deadline (AllowN(ctx, ...) with ctx.Deadline()) */
int rl_coalescer_decide_deadline(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, int64_t n, uint32_t cfg_id,
                                 int64_t deadline_ns, uint8_t* decision, int64_t* remaining,
                                 int64_t* retry_after_ns, int64_t* reset_at_ns);
/* Reset(ctx, key) at ts_ns (rl_reset_device, include/rl_engine.h;
 * tokenbucket.go:136-144, slidingwindow.go:125-139, fixedwindow.go:118-128) in
 * sequence order: after every request submitted before it, before every
 * request submitted after it.  Blocks until applied.  The DEL is enqueued on
 * the engine's replay stream like a batch: the pipeline is not drained. */
int rl_coalescer_reset(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, uint32_t cfg_id);
/* m resets (rl_reset_batch_device) as one submission in sequence order; blocks
 * until applied.  `status` (nullable): RL_RESET_DONE, or RL_INVALID for an
 * unknown config or the reserved key -- the rest is applied and the call
 * returns RL_OK.  One larger than max_batch is split across launches.  The
 * submitter merges a run of adjacent reset submissions at the head of the
 * queue -- these and single rl_coalescer_reset calls alike -- into one launch
 * of up to max_batch; a single reset that was invalid still returns RL_EINVAL
 * to its own caller only.  Resets count toward neither submitted / decided nor
 * the automatic GC's insert budgets (stats.resets, stats.reset_launches). */
int rl_coalescer_reset_batch(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                             const uint32_t* cfg_id, uint8_t* status);
/* One refund call (rl_refund_batch_device, include/rl_engine.h; the store
 * clock of a request is floor(ts_ns / 1e6)) as one submission in sequence
 * order: after every request submitted before it, before every request
 * submitted after it, on the engine's replay stream -- the pipeline is not
 * drained.  Blocks until applied.  `status` (nullable): RL_REFUND_DONE,
 * RL_REFUND_NOKEY or RL_INVALID per request.  A submission is one launch and
 * one engine call: it is never split (larger than max_batch, or than the
 * engine's rl_refund_max: RL_EINVAL) and never merged with another refund
 * submission, since the engine sums the refunds of one call per target; the
 * submissions apply in sequence order, so a caller who wants refunds applied
 * one by one sends one per call.  Counted in stats.refunds /
 * .refund_launches only; no part in the automatic GC's insert budgets.
 * RL_EINVAL over a host backend without `refund`. */
int rl_coalescer_refund(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                        const uint32_t* cfg_id, uint8_t* status);
/* One AllowAll call (rl_allow_all_batch_device, include/rl_engine.h; the store
 * clock of a member is floor(ts_ns / 1e6)): m members in groups -- member i
 * starts a group when i == 0 or first[i] != 0 --, all or nothing per group, as
 * one submission in sequence order.  Blocks until applied.  Every member gets
 * its own decision, remaining, retry_after_ns and reset_at_ns (the decide's,
 * before any give-back) and `verdict`, its group's verdict.  A submission is
 * one launch and one engine call: never split (above max_batch, or above the
 * engine's rl_allow_all_max: RL_EINVAL) and never merged with another -- merging
 * would make the denials on a rolled-back group's transient take, and the
 * refund sums of a bucket, depend on the timing of the queue.  A full queue
 * refuses it (RL_EAGAIN).  Its members insert keys: they count in the automatic
 * GC's insert budgets and in stats.submitted / .decided; its groups and launch
 * count in stats.allow_all_groups / .allow_all_launches.  deadline_ns (0 =
 * none) and cancellation behave as for a decide submission: one whose deadline
 * passed before its launch is dropped unapplied (RL_EDEADLINE).  With the
 * usage tally or the top keys on, the members are counted with their own
 * decisions -- what each limiter's script did --, as a decide batch is; the
 * give-backs are not in the tally, as a refund's are not.  RL_EINVAL over a
 * host backend without `allow_all`. */
int rl_coalescer_allow_all(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                           const uint32_t* cfg_id, const uint8_t* first, int64_t deadline_ns, uint8_t* decision,
                           int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns, uint8_t* verdict);
/* One Charge call (rl_charge_batch_device, include/rl_engine.h; the store clock
 * of a request is floor(ts_ns / 1e6)): usage recorded after the fact, as one
 * submission in sequence order.  Blocks until applied.  Every request gets its
 * decision, charged, remaining and reset_at_ns as the engine call gives them.
 * A submission is one launch and one engine call: never split (above
 * max_batch, or above the engine's rl_charge_max: RL_EINVAL) and never merged
 * with another -- merging makes duplicates, whose asks all read the state before
 * the launch, so the results would depend on the timing of the queue.  A full
 * queue refuses it (RL_EAGAIN).  Its requests insert keys: they count in the
 * automatic GC's insert budgets and in stats.submitted / .decided; its launch
 * counts in rl_coalescer_stats_charge.charge_launches.  deadline_ns (0 = none)
 * and cancellation behave as for a decide submission.  With the usage tally or
 * the top keys on, the requests are counted behind the launch as a decide
 * batch's are, with the asked n and the verb's own decision.  RL_EINVAL over a
 * host backend without `charge`. */
int rl_coalescer_charge(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                        const uint32_t* cfg_id, int64_t deadline_ns, uint8_t* decision, int64_t* charged,
                        int64_t* remaining, int64_t* reset_at_ns);
/* Read-only queries (rl_peek_batch_device, include/rl_engine.h): for each
 * request the Result AllowN would return, against the state left by every
 * request submitted before the call and none submitted after it; nothing is
 * changed, n == 0 asks how much is left.  Queued in sequence order like Reset,
 * on the engine's replay stream: the pipeline is not drained.  Blocks until
 * done.  Not counted in submitted / decided (stats.peeked) nor in the
 * automatic GC's insert budgets.  RL_EINVAL over a host backend without
 * `peek`. */
int rl_coalescer_peek(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                      const int64_t* n, const uint32_t* cfg_id, uint8_t* decision, int64_t* remaining,
                      int64_t* retry_after_ns, int64_t* reset_at_ns);
/* rl_table_info_get / rl_table_gc in sequence order (both drain the
 * engine's in-flight batches first).  Block until done. */
int rl_coalescer_table_info(rl_coalescer* c, int64_t now_ms, rl_table_info* out);
int rl_coalescer_gc(rl_coalescer* c, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity,
                    rl_table_info* out);
/* rl_snapshot_export / rl_snapshot_import (include/rl_snapshot.h) in sequence
 * order: a snapshot sees every request submitted before it and none submitted
 * after; a restore lands between the same two.  Block until done.  A restore
 * counts as a GC run in the stats (it is one).  Engine-backed coalescers only:
 * over a host backend both return RL_EINVAL. */
int rl_coalescer_snapshot(rl_coalescer* c, int64_t now_ms, uint32_t world, uint32_t rank,
                          void* buf, size_t cap, rl_snapshot_info* out);
int rl_coalescer_restore(rl_coalescer* c, const void* buf, size_t len, int64_t now_ms,
                         uint64_t tb_capacity, uint64_t win_capacity, rl_table_info* out);
int rl_coalescer_get_stats(rl_coalescer* c, rl_coalescer_stats* out);
/* the same counters and, behind them, charge_launches; struct_size comes back
 * as the bytes filled in */
int rl_coalescer_get_stats_charge(rl_coalescer* c, rl_coalescer_stats_charge* out);
/* The usage tally (rl_tally_read's arguments, rl_engine.h) in sequence order
 * like rl_coalescer_table_info: it has counted every request submitted before
 * the call and none submitted after; nothing is drained.  With
 * tally_key_slots the submitter enqueues rl_tally_batch_device behind every
 * batch of requests, on that batch's stream (its buffers are not reused before
 * the tally has run).  Peeks and resets are not counted, nor are requests
 * dropped unapplied (deadline, cancel).  Blocks until done.  RL_EINVAL when
 * tally_key_slots was 0.
 * Over a host backend the coalescer keeps the same tally itself, on the host:
 * the same table rule and probe bound.  A host backend registers no configs,
 * so there a config id is known from the first request of it that the backend
 * decides (any decision but RL_INVALID); an RL_INVALID request of a config id
 * not known yet adds to unknown_cfg. */
int rl_coalescer_tally(rl_coalescer* c, rl_tally_cfg* cfg_out, size_t cfg_cap, uint32_t* ncfg,
                       rl_tally_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                       rl_tally_info* info, int clear);
/* The top keys (rl_hot_read's arguments, rl_engine.h) in sequence order like
 * rl_coalescer_tally: it has counted every request submitted before the call
 * and none submitted after; nothing is drained.  With hot_min the submitter
 * enqueues rl_hot_batch_device behind every batch of requests, on that batch's
 * stream and arrays (behind the tally's, when that is on too; the slot's
 * buffers are not reused before it has run): one rl_hot_batch call per launched
 * batch.  Peeks and resets are not counted, nor are requests dropped unapplied
 * (deadline, cancel).  Blocks until done.  RL_EINVAL when hot_min was 0.
 * Over a host backend the coalescer keeps the same sketch and candidate table
 * itself, on the host: per backend batch all the adds, then the look at the
 * batch's keys.  A config id counts as known by the tally's host rule. */
int rl_coalescer_hot(rl_coalescer* c, rl_hot_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                     rl_hot_info* info, int clear);

#ifdef __cplusplus
}
#endif
#endif
