/*
 * rl_engine.h -- C-ABI of the MI355X batched rate-limit decision engine.
 *
 * This is the drop-in boundary that replaces the reference's storage seam:
 * every decision the reference makes with one go-redis EVAL round trip
 *   tokenbucket.go:172   client.Eval(ctx, tokenBucketScript, ...)
 *   slidingwindow.go:164 client.Eval(ctx, slidingWindowScript, ...)
 *   fixedwindow.go:152   client.Eval(ctx, fixedWindowScript, ...)
 * plus the Go arithmetic around it (AllowN, tokenbucket.go:90-133,
 * slidingwindow.go:68-122, fixedwindow.go:65-115) is made here, for a whole
 * batch, by HIP kernels over an HBM-resident state table.  Reset's DEL
 * (tokenbucket.go:139, slidingwindow.go:134, fixedwindow.go:123) maps to
 * rl_reset.  A cgo binding is shown in INTEGRATION.md.
 *
 * Conventions: plain C types only; arrays are caller-owned and only accessed
 * during the call (the *_device entry point: until the stream reaches it); the
 * engine owns all device memory.  Calls on one engine are not re-entrant.
 * Every function returns RL_OK (0) or a negative RL_E* status.
 * Every struct starts with `struct_size`, which the caller sets to sizeof the
 * struct it was compiled with: inputs of a size the library does not know are
 * rejected with RL_EINVAL, outputs are written up to the caller's size.
 */
#ifndef RL_ENGINE_H
#define RL_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define RL_OK          0
#define RL_EINVAL    (-22)  /* bad argument / config fails Validate (config.go:16-50) */
#define RL_ENOMEM    (-12)  /* device allocation failed or state table full */
#define RL_EDEVICE    (-5)  /* HIP runtime error (text in rl_last_error) */
#define RL_ETIMEOUT (-110)  /* a device-side bounded wait expired */
#define RL_EORDER    (-34)  /* reserved: no longer returned (window keys of any age are kept) */
#define RL_EEXIST (-17)  /* rl_snapshot_import: a key of the snapshot is already in the engine */

/* algorithms (interface.go:11-23) */
#define RL_ALG_TOKEN_BUCKET   1
#define RL_ALG_SLIDING_WINDOW 2
#define RL_ALG_FIXED_WINDOW   3

/* backend semantics profile */
#define RL_PROFILE_REDIS7    0  /* real Redis 7: Lua tostring "%.14g", expiry now > when */
#define RL_PROFILE_MINIREDIS 1  /* miniredis + gopher-lua (the reference tests) */

/* per-request decision codes */
#define RL_DENIED  0
#define RL_ALLOWED 1
#define RL_ERROR   2  /* the script failed (INCRBY overflow): Go sees err != nil */
#define RL_INVALID 3  /* n <= 0, unknown cfg id or reserved key id: not executed */

/* reserved key id (marks an empty table slot) */
#define RL_KEY_RESERVED UINT64_MAX

typedef struct rl_engine rl_engine;

typedef struct rl_opts {
    uint32_t struct_size;   /* sizeof(rl_opts) */
    int32_t  device;        /* HIP device ordinal */
    int32_t  profile;       /* RL_PROFILE_* */
    uint64_t tb_capacity;   /* token-bucket table slots; rounded up to a power of 2 */
    uint64_t win_capacity;  /* window-counter table slots; rounded up to a power of 2 */
    uint32_t max_batch;     /* largest batch one launch sequence handles (<= 2^28) */
    uint32_t flags;         /* RL_OPT_* */
    uint64_t spill_capacity; /* window keys kept outside their user key's table entry (a live key
                                evicted by a newer window, or created out of order); rounded up to a
                                power of 2; 0 = 2 x win_capacity (a sliding window key holds ~2) */
} rl_opts;

/* rl_opts.flags: the device-API input arrays of every rl_decide_batch_device
 * call are complete when the call is made (not produced by work still queued
 * on `stream`).  The engine then runs each batch in three parts on three
 * internal streams -- grouping (hash, sort, permute), replay, finish -- so
 * that batch b+1's grouping and batch b-1's finish overlap batch b's replay
 * (three batches in flight, three internal buffer sets).  Replays stay in
 * call order; results are identical.  `stream` still orders the results:
 * work queued on it after the call sees them.  The inputs must stay
 * unmodified until then. */
#define RL_OPT_PIPELINE 1u

typedef struct rl_stats {
    uint32_t struct_size;     /* sizeof(rl_stats) */
    uint32_t pad_;
    uint64_t batches;
    uint64_t decisions;
    uint64_t last_segments;   /* distinct keys in the last batch */
    uint64_t last_heavy;      /* segments replayed cooperatively in the last batch */
    uint64_t last_coop_rounds; /* cooperative rounds of the last batch (all heavy segments) */
    uint64_t last_coop_iters;  /* offset fixed-point iterations of the last batch (all heavy segments) */
    uint32_t sort_bits;
    uint32_t sort_passes;
    uint64_t stamp_cycles[7];  /* replay timers of the last batch (10 ns ticks): [0] longest huge segment,
                                  [2] max per-block light phase, [4] first block start to last block end,
                                  [6] max rounds of one segment; [1] [3] [5] unused (0) */
    uint64_t coop_ends[4];     /* how the last batch's cooperative rounds ended: [0] window done,
                                  [1] stop request (allow / clamp / decade / expiry), [2] boundary
                                  (exact-pass mismatch safety net), [3] offset iteration cap */
    uint64_t sort_predicted;   /* batches whose grouping sort was launched as k_sort_local only (every
                                  MSD bucket predicted to fit LDS: no LSD passes, no k_segments) */
    uint64_t light_batches;    /* batches replayed by the light replay kernel (no huge segment expected) */
    uint64_t plain_finish_batches; /* batches above the bucketed finish's limit (2^21 requests, or RL_UP_MAX
                                      when lower): results scattered by arrival index (k_unpermute, or
                                      k_unpermute_routed on the routed path) */
} rl_stats;

/* replaces redis.NewClient + NewTokenBucket/NewSlidingWindow/NewFixedWindow's
 * storage (tokenbucket.go:63-81 etc.) */
int rl_engine_create(const rl_opts* opts, rl_engine** out);
int rl_engine_destroy(rl_engine* e);

/* Register one limiter config (Config, interface.go:46-70; Validate config.go:16-50).
 * State is keyed by key_id only: callers give each (config, formatted key)
 * its own id, as FormatKey(key) is unique per prefix (config.go:81-87). */
int rl_config_register(rl_engine* e, uint8_t alg, int64_t limit, int64_t window_ns,
                       uint32_t* cfg_id);
/* The state table a config's keys live in: 0 the token-bucket table, 1 the
 * window table (whose keys may also move window keys to the spill table);
 * RL_EINVAL for an unknown id.  The coalescer's automatic GC budgets each
 * table by the requests that can insert into it. */
int rl_config_table(rl_engine* e, uint32_t cfg_id);

/* One batch in arrival order (array index = seq).  Host arrays; synchronous.
 *   ts_ns      request time, Unix ns (stands for time.Now() in AllowN)
 *   n          AllowN count (Allow = 1); n <= 0 yields RL_INVALID
 *   server_ms  Redis clock per request (nullable: floor(ts_ns / 1e6))
 * Outputs per request: decision (RL_DENIED/ALLOWED/ERROR/INVALID), remaining,
 * retry_after_ns, reset_at_ns (Unix ns; also valid for RL_ERROR, for the
 * fail-open Result), tokens (nullable; token-bucket only: the Lua `tokens`
 * value at the end of the script, bit-exact). */
int rl_decide_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                    const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                    uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                    int64_t* reset_at_ns, double* tokens);

/* Same, with device pointers, enqueued on `stream` (a hipStream_t; NULL = the
 * engine's stream).  Asynchronous: check errors with rl_engine_sync. */
int rl_decide_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                           const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                           uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                           int64_t* reset_at_ns, double* tokens, void* stream);

/* wait for queued work; returns the sticky device status (RL_ENOMEM if the
 * table filled, RL_EORDER, RL_ETIMEOUT) and clears it */
int rl_engine_sync(rl_engine* e);

/* Reset(ctx, key) at time ts_ns: DEL of the key(s) AllowN would touch at ts_ns
 * (tokenbucket.go:136-144, slidingwindow.go:125-139, fixedwindow.go:118-128).
 * Synchronous. */
int rl_reset(rl_engine* e, uint32_t cfg_id, uint64_t key_id, int64_t ts_ns);
/* The same DEL enqueued in batch order: after every batch enqueued before the
 * call, before every batch enqueued after it (it runs on the engine's replay
 * stream, nothing is drained); `stream` (a hipStream_t, NULL = the engine's
 * stream) waits for it. */
int rl_reset_device(rl_engine* e, uint32_t cfg_id, uint64_t key_id, int64_t ts_ns, void* stream);

/* Many resets in one launch.  A batch of m resets (key_id[i], ts_ns[i],
 * cfg_id[i]) has the effect of m rl_reset calls in any order (the deletes are
 * idempotent and commute, so duplicates are fine).  A request with an unknown
 * cfg_id or RL_KEY_RESERVED is not executed: its status is RL_INVALID, the
 * rest of the batch is applied and the call still returns RL_OK, as a decide
 * batch does for invalid requests.  Executed requests get RL_RESET_DONE.
 * `status` is nullable.  rl_stats.batches / .decisions and the sticky status
 * of rl_engine_sync are untouched.  m == 0 is RL_OK without a launch; null
 * input arrays with m > 0 are RL_EINVAL.
 * Host arrays; synchronous; m may exceed max_batch (staged in chunks). */
#define RL_RESET_DONE 1
int rl_reset_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                   const uint32_t* cfg_id, uint8_t* status);
/* Same, with device pointers, ordered as rl_reset_device: one kernel on the
 * engine's replay stream, after every batch enqueued before the call and
 * before every batch enqueued after it, nothing drained; `stream` (a
 * hipStream_t, NULL = the engine's stream) waits for it.  Without
 * RL_OPT_PIPELINE the kernel first waits for the work queued on `stream` (the
 * inputs); with it the inputs are complete at call time.  m may exceed
 * max_batch. */
int rl_reset_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                          const uint32_t* cfg_id, uint8_t* status, void* stream);
/* resets one rl_reset_batch launch covers with one reset per thread (grid cap
 * x block size); a larger batch strides */
int rl_reset_grid_cap(void);

/* Refund: give consumed quota back.  A request is (key_id, ts_ns, n, cfg_id,
 * server_ms): ts_ns selects the window (a window limiter refunds the counter
 * key of window_start(ts_ns); a sliding window only that one, the previous
 * window's count is history), server_ms (nullable: floor(ts_ns / 1e6)) is the
 * store clock that decides whether the target is live.  One call groups its
 * valid requests by target -- the bucket of key_id, or the window counter key
 * wherever it lives -- and has the effect of one script run per target, with N
 * the sum (saturated at INT64_MAX) of the n of the requests whose target is
 * live at their own store clock in the state left by every batch enqueued
 * before the call:
 *   token bucket:  tokens = math.min(capacity, tokens + N), stored through
 *                  tostring (%.14g under RL_PROFILE_REDIS7); last_refill and
 *                  the TTL are untouched
 *   window:        if count <= N then DEL key else DECRBY key N (TTL kept)
 * The sum and not m single refunds: for a bucket %.14g requantises the stored
 * count, so single refunds do not commute; a caller who needs them one by one
 * sends one refund per call.  Per-request status (nullable), from the state
 * before the call only:
 *   RL_REFUND_DONE   the request contributed
 *   RL_REFUND_NOKEY  valid, but its target has no live state (a fresh key is
 *                    full anyway); nothing is stored for it: no insert and no
 *                    lazy-expiry delete
 *   RL_INVALID       n <= 0, unknown cfg_id or RL_KEY_RESERVED; the rest of the
 *                    call is applied and the call returns RL_OK
 * Two configs refunding one bucket id in one call use the capacity of one of
 * them, unspecified.  m <= rl_refund_max(e) = min(max_batch, 1 << 20), else
 * RL_EINVAL: a call is never split (the sum rule).  m == 0 is RL_OK without a
 * launch; null input arrays with m > 0 are RL_EINVAL.  rl_stats.batches /
 * .decisions, the sticky status of rl_engine_sync, the tally and the top keys
 * are untouched.  Host arrays; synchronous. */
#define RL_REFUND_NOKEY 0
#define RL_REFUND_DONE  1
int rl_refund_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                    const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* status);
/* Same, with device pointers, ordered exactly as rl_reset_batch_device: two
 * kernels on the engine's replay stream, after every batch enqueued before the
 * call and before every batch enqueued after it, nothing drained; `stream`
 * waits for them.  The first refund of an engine allocates its scratch. */
int rl_refund_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                           const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* status,
                           void* stream);
/* the largest refund call */
uint32_t rl_refund_max(rl_engine* e);
/* refunds one launch covers with one request per thread (grid cap x block
 * size); a larger call strides */
int rl_refund_grid_cap(void);

/* AllowAll: check one request against several limiters, all or nothing.  A
 * call carries m member requests (key_id, ts_ns, n, cfg_id, server_ms) as a
 * decide batch does, and a byte array first[m]: member i starts a new group
 * when i == 0 or first[i] != 0, and a group is a maximal run of members (every
 * byte array is a grouping).  A group has at most RL_ALLOW_ALL_MAX_GROUP
 * members; a longer run is one group whose verdict is RL_INVALID.  The call has
 * exactly the effect of three steps, placed between the batches enqueued before
 * and after it:
 *   1. decide   rl_decide_batch_device on the m members as one batch in array
 *               order: decision, remaining, retry_after_ns, reset_at_ns and
 *               tokens of every member exactly as that call gives them
 *   2. settle   verdict[i], the same for every member of a group: the most
 *               severe decision of the group, RL_INVALID > RL_ERROR > RL_DENIED
 *               > RL_ALLOWED.  The give-back g[i] is n[i] when the verdict is
 *               not RL_ALLOWED and the member took something -- a token bucket
 *               that allowed; a window limiter that allowed or denied (a denied
 *               window request still ran INCRBY, fixedwindow.go:22,
 *               slidingwindow.go:24) -- and 0 otherwise (an RL_ERROR or
 *               RL_INVALID member stored nothing)
 *   3. refund   one rl_refund_batch_device call over the same (key_id, ts_ns,
 *               cfg_id, server_ms) with n = g, with exactly that call's
 *               semantics: per-target sums, the %.14g store, DEL at zero,
 *               nothing stored for RL_REFUND_NOKEY.  Its status comes back as
 *               rollback[i] (nullable): RL_REFUND_DONE the amount was given
 *               back, RL_REFUND_NOKEY there was no live target (a window under
 *               one second, whose TTL is 0), RL_INVALID nothing was asked back
 * A failed check therefore takes nothing from any limiter, up to Refund's
 * limits: a bucket's last_refill and the TTLs are not rolled back, and %.14g
 * requantises the stored tokens.  The verb is conservative: within one call a
 * later group sees the quota an earlier group took before that group is rolled
 * back, so it may be denied where a strictly sequential all-or-nothing would
 * admit it; it is never admitted on quota a sequential run would not have.  A
 * member's `remaining` is the decide's value, taken before any give-back.  A
 * one-member group is AllowN, plus the give-back of a denied window member's
 * INCRBY.
 * m <= rl_allow_all_max(e) = rl_refund_max(e), else RL_EINVAL: a call is never
 * split (the refund's sum rule).  m == 0 is RL_OK without a launch; null input
 * arrays (or a null verdict) with m > 0 are RL_EINVAL.  rl_stats moves as for
 * the decide; the tally and the top keys are not touched.  The first call
 * allocates the engine's scratch for g.  Host arrays; synchronous; returns the
 * sticky device status as rl_decide_batch does (RL_ENOMEM: the table filled and
 * some members were rejected).  "A failed check takes nothing" is a statement
 * about verdicts, not about return codes: a non-RL_OK return after the decide
 * was enqueued (a HIP runtime error in the event wait, the settle launch or the
 * refund: RL_EDEVICE) leaves the members' takes in place and gives nothing
 * back.  That is a device-error path only; argument errors and failed
 * allocations return before anything is taken. */
#define RL_ALLOW_ALL_MAX_GROUP 16
int rl_allow_all_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                       const uint32_t* cfg_id, const int64_t* server_ms, const uint8_t* first,
                       uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns,
                       double* tokens, uint8_t* verdict, uint8_t* rollback);
/* Same, with device pointers: the decide enqueued on `stream` as
 * rl_decide_batch_device does, the settle kernel on `stream` behind it, then
 * the refund on the engine's replay stream, ordered as rl_refund_batch_device;
 * `stream` waits for it.  The give-backs are made on the device, so the refund
 * always waits for `stream`, whatever RL_OPT_PIPELINE says: under that flag
 * this call holds the next batch's replay until this batch's finish has run.
 * That is the price of the verb; plain batches pay nothing for it.  Calls may
 * come from different streams: each call's settle kernel waits for the previous
 * call's refund before it writes the scratch again. */
int rl_allow_all_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                              const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                              const uint8_t* first, uint8_t* decision, int64_t* remaining,
                              int64_t* retry_after_ns, int64_t* reset_at_ns, double* tokens, uint8_t* verdict,
                              uint8_t* rollback, void* stream);
/* the largest AllowAll call: rl_refund_max(e) */
uint32_t rl_allow_all_max(rl_engine* e);
/* members one settle launch covers with one member per thread (grid cap x
 * block size); a larger call strides */
int rl_allow_all_grid_cap(void);

/* Charge: record usage that is only known after the fact.  A call carries m
 * requests (key_id, ts_ns, n, cfg_id, server_ms) as a decide batch does and has
 * exactly the effect of three steps, placed between the batches enqueued before
 * and after it:
 *   1. ask      read-only.  A request with n <= 0, an unknown cfg_id or
 *               RL_KEY_RESERVED is RL_INVALID and its n' is 0.  A token-bucket
 *               request gets n' = min(n, r), r the `remaining` rl_peek_batch
 *               returns for (key_id, n = 0) at the request's own ts_ns /
 *               server_ms in the state left by every batch enqueued before the
 *               call.  A window request (fixed or sliding) gets n' = n
 *   2. decide   rl_decide_batch_device on (key_id, ts_ns, n', cfg_id,
 *               server_ms) as one batch in array order; the requests with
 *               n' = 0 are that batch's RL_INVALID requests and are not
 *               executed.  Inserts, refill, expiry, spill and %.14g are that
 *               call's
 *   3. result   one row per request:
 *               bucket, n' >= 1   charged = n' if the decide allowed it, else 0;
 *                                 decision = RL_ALLOWED if charged == n,
 *                                 RL_DENIED if charged < n, or the decide's
 *                                 RL_ERROR / RL_INVALID; remaining, reset_at_ns
 *                                 and tokens are the decide's
 *               bucket, n' = 0    (an empty bucket) nothing ran and nothing is
 *                                 stored: RL_DENIED, charged = 0, remaining = 0;
 *                                 reset_at_ns and tokens are those of the ask
 *               window            decision, remaining, reset_at_ns are the
 *                                 decide's, tokens = 0; charged = n for
 *                                 RL_ALLOWED or RL_DENIED, else 0.  RL_DENIED
 *                                 means the whole n was recorded and the count is
 *                                 now above the limit: the scripts INCRBY before
 *                                 they compare (fixedwindow.go:22,
 *                                 slidingwindow.go:24)
 *               invalid           RL_INVALID, zeros
 * There is no retry-after: nothing is being retried.  n - charged is what the
 * bucket could not cover.
 * For buckets that appear once in a call the verb is exact: Peek's parity with
 * AllowN guarantees that the decide allows n'.  The verb is conservative about
 * duplicates: the second request for a bucket has asked min(n, r) with r read
 * before the first request's take, so the decide can deny it; its row then says
 * RL_DENIED, charged = 0 and `remaining` as the decide read it, and the caller
 * charges again.  In a call with one time stamp a bucket that refused any ask
 * therefore ends with fewer whole tokens than that ask.  The exact sequential
 * form is not offered.
 * m <= rl_charge_max(e) = min(max_batch, 1 << 20), else RL_EINVAL: a call is
 * never split.  m == 0 is RL_OK without a launch; null arrays with m > 0 are
 * RL_EINVAL, except server_ms and tokens, which are nullable.  rl_stats moves as
 * for the decide, and so does the sticky status; a full table rejects whole keys
 * as the decide does, and those rows carry the decide's code and charged = 0.
 * The first call allocates the engine's scratch, before anything is enqueued.
 * Host arrays; synchronous; returns the sticky device status as rl_decide_batch
 * does. */
int rl_charge_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                    const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* decision, int64_t* charged,
                    int64_t* remaining, int64_t* reset_at_ns, double* tokens);
/* Same, with device pointers: the ask is one kernel on the engine's replay
 * stream, ordered as rl_peek_batch_device, and `stream` waits for it; the
 * decide follows as rl_decide_batch_device enqueues it, except that n' is made
 * on the device, so its grouping always waits for `stream`, whatever
 * RL_OPT_PIPELINE says; the finish kernel runs on `stream` behind the decide.
 * Calls may come from different streams: each call's ask waits for the previous
 * call's finish before it writes the scratch again. */
int rl_charge_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns, const int64_t* n,
                           const uint32_t* cfg_id, const int64_t* server_ms, uint8_t* decision, int64_t* charged,
                           int64_t* remaining, int64_t* reset_at_ns, double* tokens, void* stream);
/* the largest Charge call */
uint32_t rl_charge_max(rl_engine* e);
/* requests one launch of the ask or the finish covers with one request per
 * thread (grid cap x block size); a larger call strides */
int rl_charge_grid_cap(void);

/* Peek: read-only quota queries.  For each request, the outputs
 * rl_decide_batch would give for it at (ts_ns, server_ms) against the state
 * left by every batch enqueued before the call -- and nothing changes: no key
 * is inserted, no tokens stored, no INCRBY, no TTL refresh, no lazy-expiry
 * deletion, no spill slot claimed; rl_stats.batches / .decisions and the
 * sticky status of rl_engine_sync are untouched.  Requests of one call do not
 * see each other.  n == 0 is legal here only, the status query: a token bucket
 * answers RL_ALLOWED with remaining = floor(tokens after refill) (unless ts_ns
 * lies so far before its last refill that the refill leaves tokens < 0), a window
 * limiter with remaining = max(limit - count, 0).  n < 0, an unknown cfg_id and
 * RL_KEY_RESERVED yield RL_INVALID; a window count whose INCRBY would overflow
 * RL_ERROR with reset_at_ns, as in rl_decide_batch.  A key without state (never
 * seen, expired, or in a table too full to take it) answers as a fresh key.
 * m may exceed max_batch. */
int rl_peek_batch(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                  const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                  uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                  int64_t* reset_at_ns, double* tokens);
/* Same, with device pointers, ordered as rl_reset_device: after every batch
 * enqueued before the call, before every batch enqueued after it (one kernel
 * on the engine's replay stream, nothing is drained); `stream` (a hipStream_t,
 * NULL = the engine's stream) waits for the results.  Without RL_OPT_PIPELINE
 * the kernel first waits for the work queued on `stream` (the inputs). */
int rl_peek_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                         const int64_t* n, const uint32_t* cfg_id, const int64_t* server_ms,
                         uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                         int64_t* reset_at_ns, double* tokens, void* stream);
/* requests one rl_peek_batch launch covers with one request per thread (grid
 * cap x block size); a larger batch strides */
int rl_peek_grid_cap(void);

int rl_engine_stats(rl_engine* e, rl_stats* out);

/* State-table occupancy.  A key is live at server clock now_ms when its Redis
 * TTL has not expired (a window entry: either of its two counter keys). */
typedef struct rl_table_info {
    uint32_t struct_size;     /* sizeof(rl_table_info) */
    uint32_t pad_;
    uint64_t tb_capacity, tb_used, tb_live;
    uint64_t win_capacity, win_used, win_live;
    uint64_t spill_capacity, spill_used, spill_live;   /* spill slots ever claimed / live window keys */
} rl_table_info;
int rl_table_info_get(rl_engine* e, int64_t now_ms, rl_table_info* out);

/* Redis KEYS: every key live at server clock now_ms, as (key id, kind,
 * window start).  A token-bucket key is the hash FormatKey(key)
 * (tokenbucket.go:95); a window key is FormatKey(key):ws (fixedwindow.go:139-141,
 * slidingwindow.go:150-152).  Writes up to `cap` records (any order);
 * *count = how many keys are live.  Synchronous, waits for queued batches; a
 * diagnostic (the reference's tests list keys with miniredis Keys()). */
#define RL_KIND_HASH   0
#define RL_KIND_WINDOW 1
typedef struct rl_key_rec {
    uint64_t key_id;
    int64_t window_start;   /* Unix seconds (RL_KIND_WINDOW); 0 for a hash */
    uint32_t kind;          /* RL_KIND_* */
    uint32_t pad_;
} rl_key_rec;
int rl_table_keys(rl_engine* e, int64_t now_ms, rl_key_rec* out, size_t cap, uint64_t* count);

/* Table GC (the TTLs of tokenbucket.go:170,
 * slidingwindow.go:161-162, fixedwindow.go:151): drop every key expired at
 * server clock now_ms -- Redis's active expiry -- and optionally resize the
 * tables (0 = keep the capacity; the spill table follows win_capacity when
 * rl_opts.spill_capacity was 0, else keeps its capacity).  Keys are only ever inserted by the decision
 * path, so this is what keeps a long-running table from filling.  Decisions
 * are unchanged provided no later request carries a server clock below
 * now_ms (lazy expiry would see those keys as absent anyway).  Synchronous;
 * waits for queued batches.  RL_ENOMEM (old tables kept) when the live keys do
 * not fit the requested capacity.  `out` (nullable): the tables afterwards. */
int rl_table_gc(rl_engine* e, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity, rl_table_info* out);

/* per-stage device time (ms) accumulated since the last call, measured with
 * HIP events on the stream the kernels run on; stages: 0 probe, 1 sort,
 * 2 segments + permute, 3 replay (k_tb_chain), 4 finish (run expansion +
 * unpermute).  rl_engine_set_timing(e, on): 0 off, 1 the replay only (two
 * events per batch on its stream), 2 every stage, -k (k >= 2) the replay
 * only on every k-th batch (the event pair costs the replay stream ~10 us per
 * batch; a timed benchmark samples).  *batches counts the batches timed. */
int rl_engine_set_timing(rl_engine* e, int on);
int rl_engine_stage_times(rl_engine* e, double* ms, int nstages, uint64_t* batches);
/* diagnostic: the last batch's replay debug counters (up to 88 words; layout in rl_engine.hip CTRL_DBG) */
int rl_engine_debug_words(rl_engine* e, uint32_t* out, size_t n);

int rl_last_error(rl_engine* e, char* buf, size_t len);

/* self-test hooks: exact tonumber(tostring(x)) of Redis Lua ("%.14g"),
 * host instantiation and device instantiation of the same code */
int rl_selftest_q14_host(const double* in, double* out, size_t n);
int rl_selftest_q14_device(rl_engine* e, const double* in, double* out, size_t n);

/* Usage tally: what the decisions were, counted on the device -- per config
 * the requests by decision code and the units granted and denied, and the keys
 * that are being throttled.  Off until rl_tally_enable; it reads result arrays
 * only and never touches the state tables, rl_stats or the sticky status of
 * rl_engine_sync.  Every rl_tally_* call before rl_tally_enable is RL_EINVAL.
 *
 * Per request (key_id, cfg_id, n, decision): an unregistered cfg_id adds one to
 * unknown_cfg and nothing else; otherwise a decision byte above 3 adds one to
 * bad_codes and nothing else; otherwise count[decision] of the config grows by
 * one and, for RL_DENIED / RL_ALLOWED with n > 0, units[decision] by n (modulo
 * 2^64).  Every key with a denied request is recorded in a table of key_slots
 * records (open addressing from mix64(key_id) & (key_slots - 1), at most
 * min(key_slots, 64) probes): its denied requests and their units.  The table
 * only fills until the next clear, so a key is tracked completely or not at
 * all; the denied requests of keys without a slot (and of RL_KEY_RESERVED) are
 * summed in untracked_requests / untracked_units. */
typedef struct rl_tally_opts {
    uint32_t struct_size;   /* sizeof(rl_tally_opts) */
    uint32_t key_slots;     /* rounded up to a power of 2, 16 .. 1<<24; 0 = 65536 */
} rl_tally_opts;
typedef struct rl_tally_cfg {
    uint64_t count[4];      /* by decision code: RL_DENIED, RL_ALLOWED, RL_ERROR, RL_INVALID */
    uint64_t units[2];      /* sum of n: [0] denied, [1] allowed */
} rl_tally_cfg;
typedef struct rl_tally_key {
    uint64_t key_id, denied, units_denied;
    uint32_t cfg_id, pad_;  /* cfg_id: the config of one of the key's denied requests */
} rl_tally_key;
typedef struct rl_tally_info {
    uint32_t struct_size, pad_;   /* sizeof(rl_tally_info) */
    uint64_t key_slots, keys_tracked, untracked_requests, untracked_units, unknown_cfg, bad_codes;
    uint64_t batches, requests;   /* rl_tally_batch(_device) calls with m > 0 / their requests */
} rl_tally_info;
/* allocates the accumulators; a second call is RL_EINVAL.  A config registered
 * later gets a zero row. */
int rl_tally_enable(rl_engine* e, const rl_tally_opts* opts);
/* Count one finished batch in the decide layout (device pointers), on `stream`
 * (a hipStream_t; NULL = the engine's stream): queued after
 * rl_decide_batch_device on the same stream it sees that batch's results.  The
 * arrays must stay unmodified until the stream has passed the call.  m may
 * exceed max_batch; m == 0 is RL_OK without a launch; null arrays with m > 0
 * are RL_EINVAL. */
int rl_tally_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                          const int64_t* n, const uint8_t* decision, void* stream);
/* the same with host arrays; synchronous */
int rl_tally_batch(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                   const int64_t* n, const uint8_t* decision);
/* Synchronous: waits for every tally call made before it, on any stream.
 * Writes the rows of configs 0 .. min(cfg_cap, *ncfg) - 1 (*ncfg: the configs
 * registered) and the key_cap tracked keys with the most denied requests,
 * ordered by denied descending, then key_id ascending (fewer when fewer are
 * tracked; *keys_tracked: how many are).  Every output is nullable.  With
 * clear != 0 everything is zeroed after the copy, before any later tally
 * call. */
int rl_tally_read(rl_engine* e, rl_tally_cfg* cfg_out, size_t cfg_cap, uint32_t* ncfg,
                  rl_tally_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                  rl_tally_info* info, int clear);
/* requests one k_tally launch covers with one request per thread (grid cap x
 * block size); a larger batch strides */
int rl_tally_grid_cap(void);

/* Top keys: which keys carry the traffic, over all decisions -- a count-min
 * sketch of RL_HOT_DEPTH rows by `width` 64-bit counters, plus a table of
 * key_slots candidate keys.  A sibling of the tally: off until rl_hot_enable,
 * it reads finished batches' arrays only and never touches the state tables,
 * rl_stats, the sticky status of rl_engine_sync or the tally.  Every rl_hot_*
 * call before rl_hot_enable is RL_EINVAL.
 *
 * A request (key_id, cfg_id, n, decision) counts iff cfg_id is registered,
 * decision <= RL_ERROR (denied, allowed or error: the limiter executed it),
 * key_id != RL_KEY_RESERVED and, with RL_HOT_UNITS, n > 0.  Its weight is 1
 * (RL_HOT_REQUESTS) or (uint64_t)n (RL_HOT_UNITS); sums are modulo 2^64.
 * Every other request adds 1 to `skipped` and nothing else.  `total` is the
 * sum of the counted weights.
 *
 * The column of key k in row r (0 .. 3) is mix64(k ^ mix64(r + 1)) & (width - 1),
 * mix64 as in the state tables (csrc/rl_table.h).  One rl_hot_batch(_device)
 * call has exactly this effect:
 *   (A) every counted request adds its weight to its four counters;
 *   (B) once all of the call's adds are in, every key with a counted request
 *       in this call is looked at: its estimate is the minimum of its four
 *       counters, and if that is at least hot_min the key is inserted into the
 *       candidate table.
 * The candidate table follows the tally's rule: home slot mix64(k) &
 * (key_slots - 1), linear probing over at most min(key_slots, 64) slots, an
 * empty slot claimed with one CAS, the record keeps the cfg_id of one of the
 * key's requests, and records are never released before a clear -- a key finds
 * its record every time or finds its run taken every time.  A qualifying key
 * without a slot makes `dropped` non-zero: it is non-zero exactly when that has
 * happened since the last clear, its value is otherwise unspecified.
 *
 * Adds commute, so the sketch after a call is a function of the multiset of
 * requests counted so far and, unless the table overflows, so is the candidate
 * set: every key k for which some call held a counted request of k and left
 * k's estimate at or above hot_min.  A count-min sketch never underestimates:
 * every key whose true weight reaches hot_min is a candidate from the call in
 * which it gets there.  Keys whose counters collide with heavier ones may be
 * candidates too (false positives), with the overestimate they had.
 *
 * Error bound (documented, not tested): under the usual hashing assumption,
 * estimate - true weight <= e * total / width for one key with probability at
 * least 1 - e^-4. */
#define RL_HOT_DEPTH 4
#define RL_HOT_REQUESTS 0u
#define RL_HOT_UNITS 1u
typedef struct rl_hot_opts {
    uint32_t struct_size;   /* sizeof(rl_hot_opts) */
    uint32_t width;         /* rounded up to a power of 2, 16 .. 1<<24; 0 = 1<<18 */
    uint32_t key_slots;     /* rounded up to a power of 2, 16 .. 1<<24; 0 = 65536 */
    uint32_t weight;        /* RL_HOT_REQUESTS | RL_HOT_UNITS */
    uint64_t hot_min;       /* >= 1, else RL_EINVAL */
} rl_hot_opts;
typedef struct rl_hot_key {
    uint64_t key_id, estimate;
    uint32_t cfg_id, pad_;  /* cfg_id: the config of one of the key's counted requests */
} rl_hot_key;
typedef struct rl_hot_info {
    uint32_t struct_size, pad_;   /* sizeof(rl_hot_info) */
    uint64_t width, depth, key_slots, hot_min, weight;
    uint64_t keys_tracked, dropped, total, skipped;
    uint64_t batches, requests;   /* rl_hot_batch(_device) calls with m > 0 / their requests */
} rl_hot_info;
/* allocates and zeroes the sketch and the table; a second call is RL_EINVAL.
 * A config registered later counts from then on. */
int rl_hot_enable(rl_engine* e, const rl_hot_opts* opts);
/* Count one finished batch in the decide layout (device pointers), on `stream`
 * (a hipStream_t; NULL = the engine's stream): two launches, the adds and then
 * the look at the call's keys.  Queued after rl_decide_batch_device on the same
 * stream it sees that batch's results.  The arrays must stay unmodified until
 * the stream has passed the call.  m may exceed max_batch; m == 0 is RL_OK
 * without a launch; null arrays with m > 0 are RL_EINVAL.  Calls on different
 * streams may run at once; (B) of a call then sees what has been added by then. */
int rl_hot_batch_device(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                        const int64_t* n, const uint8_t* decision, void* stream);
/* the same with host arrays; synchronous */
int rl_hot_batch(rl_engine* e, size_t m, const uint64_t* key_id, const uint32_t* cfg_id,
                 const int64_t* n, const uint8_t* decision);
/* Synchronous: waits for every rl_hot_* call made before it, on any stream.
 * Each candidate's estimate is read from the sketch as it is now (a kernel over
 * the candidate records; the sketch is not copied to the host).  Writes the
 * key_cap candidates with the largest estimates, ordered by estimate
 * descending, then key_id ascending (fewer when fewer are tracked;
 * *keys_tracked: how many are).  Every output is nullable.  With clear != 0 the
 * sketch, the candidates and the counters are zeroed before any later call. */
int rl_hot_read(rl_engine* e, rl_hot_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                rl_hot_info* info, int clear);
/* requests one k_hot_add / k_hot_pick launch covers with one request per thread
 * (grid cap x block size); a larger batch strides */
int rl_hot_grid_cap(void);

#ifdef __cplusplus
}
#endif
#endif
