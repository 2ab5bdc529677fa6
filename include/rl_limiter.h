/*
 * rl_limiter.h -- C-ABI of the host mirror of the reference's Go API
 * (internal/ratelimiter: Config, RateLimiter.Allow/AllowN/Reset/Close), built
 * over include/rl_engine.h.  This is what a non-C++ host (Go via cgo, Python
 * via ctypes) binds when it wants the reference's per-call semantics instead
 * of raw batches; see INTEGRATION.md.
 *
 * Reference anchors: interface.go:26-145, config.go:16-87, errors.go:5-20,
 * tokenbucket.go:63-152, slidingwindow.go:41-147, fixedwindow.go:38-136.
 */
#ifndef RL_LIMITER_H
#define RL_LIMITER_H

#include <stddef.h>
#include <stdint.h>

#include "rl_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* return codes: which Go error value the reference would return */
#define RLL_OK           0  /* err == nil, *out is the Result */
#define RLL_ERR_INVALID_N 1  /* ErrInvalidN, Result nil (tokenbucket.go:91-93) */
#define RLL_ERR_FAILED   2  /* fmt.Errorf("failed to check rate limit: %w"), Result nil */
#define RLL_ERR_CONFIG   3  /* constructor error ("config cannot be nil", "invalid config: ...") */
#define RLL_ERR_RESET    4  /* fmt.Errorf("failed to reset rate limit: %w") */
#define RLL_ERR_ARG      5  /* bad C argument */
#define RLL_ERR_REFUND   6  /* fmt.Errorf("failed to refund rate limit: %w"), in Reset's style */
#define RLL_ERR_CHARGE   7  /* fmt.Errorf("failed to charge rate limit: %w") */

#define RLL_NOW_WALL   INT64_MIN  /* now_ns: read the wall clock (time.Now()) */
#define RLL_SMS_DEFAULT INT64_MIN /* server_ms: Redis clock = floor(now_ns / 1e6) */

typedef struct rll_engine rll_engine;    /* rl_engine + key interner */
typedef struct rll_limiter rll_limiter;

typedef struct rll_result {
    uint8_t allowed;
    int64_t limit;
    int64_t remaining;
    int64_t retry_after_ns;
    int64_t reset_at_ns;
} rll_result;

#define RLL_TIME_ZERO INT64_MIN   /* reset_at_ns of time.Time{} */

/* Result constructors (result.go:5-50): NewAllowedResult, NewDeniedResult,
 * NewFailOpenResult, NewFailClosedResult */
int rll_new_allowed_result(int64_t limit, int64_t remaining, int64_t reset_at_ns, rll_result* out);
int rll_new_denied_result(int64_t limit, int64_t retry_after_ns, int64_t reset_at_ns, rll_result* out);
int rll_new_fail_open_result(rll_result* out);
int rll_new_fail_closed_result(rll_result* out);

int rll_engine_new(const rl_opts* opts, rll_engine** out, char* err, size_t errlen);
int rll_engine_free(rll_engine* e);
rl_engine* rll_engine_raw(rll_engine* e);
/* test hook (miniredis FastForward replay): fixed Redis clock for every call;
 * RLL_SMS_DEFAULT restores the default */
int rll_engine_set_server_ms(rll_engine* e, int64_t server_ms);

/* Redis KEYS (what the reference's tests read with miniredis Keys()): the
 * live keys' names at Redis clock server_ms, sorted, one per line
 * ("prefix:key" for a token bucket, "prefix:key:ws" for a window counter).
 * Writes what fits in buf (NUL-terminated); returns the full length, or a
 * negative RLL_ERR_* code. */
int rll_keys(rll_engine* e, int64_t server_ms, char* buf, size_t len);

/* Config.Validate() (config.go:16-50); algorithm NULL means a nil *Config */
int rll_config_validate(const char* algorithm, int64_t limit, int64_t window_ns, char* err, size_t errlen);
/* Config.FormatKey(key) (config.go:81-87) for a config with this Prefix
 * (prefix NULL means a nil *Config); returns the length written */
int rll_format_key(const char* prefix, const char* key, char* out, size_t len);
/* Go time.Duration.String() */
int rll_duration_string(int64_t d, char* out, size_t len);

/* New{TokenBucket,SlidingWindow,FixedWindow} by algorithm name.  prefix NULL
 * == "" (defaults to "ratelimit" via WithDefaults).  config_nil != 0 models a
 * nil *Config. */
int rll_new(rll_engine* e, const char* algorithm, int64_t limit, int64_t window_ns,
            const char* prefix, int fail_open, int config_nil, rll_limiter** out, char* err,
            size_t errlen);

/* AllowN(ctx, key, n); Allow == n = 1.  ctx_cancelled != 0 models a cancelled
 * context. */
int rll_allow_n(rll_limiter* l, const char* key, size_t keylen, int64_t n, int64_t now_ns,
                int ctx_cancelled, rll_result* out, char* err, size_t errlen);

/* Peek: the Result AllowN(ctx, key, n) would return, with nothing changed
 * (rl_peek_batch, include/rl_engine.h).  As rll_allow_n, except that n == 0 is
 * accepted (how much is left) and only n < 0 is RLL_ERR_INVALID_N.  A key the
 * interner has never seen is not interned; the metrics and logging decorators
 * forward a peek unrecorded. */
int rll_peek_n(rll_limiter* l, const char* key, size_t keylen, int64_t n, int64_t now_ns,
               int ctx_cancelled, rll_result* out, char* err, size_t errlen);

/* BatchAllow: m requests in one engine launch; per-request code in codes[] */
int rll_allow_batch(rll_limiter* l, size_t m, const char* const* keys, const size_t* keylens,
                    const int64_t* n, const int64_t* now_ns, rll_result* out, int32_t* codes);

/* Observability decorators (docs/ADR/003-decorator-pattern-for-observability.md):
 * wrap the limiter in place; every later call goes through them.
 * rll_metrics_expose writes the Prometheus text exposition
 * (rate_limiter_requests_total{algorithm,allowed,error},
 * rate_limiter_decision_seconds histogram) and returns its full length. */
int rll_add_metrics(rll_limiter* l);
int rll_metrics_expose(rll_limiter* l, char* buf, size_t len);
/* LoggingDecorator: records go to a bounded in-library queue that the
 * caller drains (pull style -- the library never calls back into Go; a full
 * queue drops its oldest record).  rll_log_drain writes whole records as
 * text lines "<level>\t<msg>\t<fields>\n" (level: 0 debug, 1 info, 2 warn,
 * 3 error; fields "k=v k=v") while they fit in buf (NUL-terminated), removes
 * them from the queue and returns how many it wrote; *dropped (nullable) =
 * records lost to overflow so far. */
int rll_add_logging(rll_limiter* l, size_t capacity);
int rll_log_drain(rll_limiter* l, char* buf, size_t len, uint64_t* dropped);

int rll_reset(rll_limiter* l, const char* key, size_t keylen, int64_t now_ns, char* err, size_t errlen);
/* ResetMany: observably m rll_reset calls in order (a key string never seen
 * is interned as rll_reset interns it; a closed limiter fails with the same
 * text and interns nothing), as one rl_reset_batch underneath.  RLL_OK, or
 * RLL_ERR_RESET with the message of the failure. */
int rll_reset_many(rll_limiter* l, size_t m, const char* const* keys, const size_t* keylens, int64_t now_ns,
                   char* err, size_t errlen);
/* Refund: give n units back to `key` (rl_refund_batch, include/rl_engine.h):
 * a bucket gains min(capacity, tokens + n), a window counter loses n and is
 * deleted at zero.  now_ns is the store clock (RLL_NOW_WALL: the wall clock);
 * at_ns picks the window a window limiter refunds -- the time of the request
 * being refunded, or any time inside its window; 0 = now_ns.  *applied
 * (nullable): 1 when the key had live state, 0 when it had none (never seen,
 * expired, or that window holds nothing: a fresh key is full anyway, and
 * nothing is stored or interned for it).  n <= 0 is RLL_ERR_INVALID_N with
 * ErrInvalidN's text, before any I/O.  A storage error (a closed limiter, an
 * engine failure) is RLL_ERR_REFUND with its message -- never a fail-open
 * result, as Reset.  The metrics decorator counts refunds and refunded units
 * (rate_limiter_refunds_total{algorithm,applied},
 * rate_limiter_refunded_units_total{algorithm}; exposed once a refund was
 * made); the logging decorator logs a refund at debug and its failure at
 * error level. */
int rll_refund_n(rll_limiter* l, const char* key, size_t keylen, int64_t n, int64_t now_ns, int64_t at_ns,
                 uint8_t* applied, char* err, size_t errlen);
/* RefundMany: m refunds as ONE engine call -- refunds of one key (and window)
 * are summed and returned in one step, which for a token bucket under
 * RL_PROFILE_REDIS7 can differ in the last digit from m rll_refund_n calls
 * (%.14g requantises the stored count after each).  at_ns nullable (all 0).
 * Any n <= 0 fails the whole call with RLL_ERR_INVALID_N, nothing applied. */
int rll_refund_many(rll_limiter* l, size_t m, const char* const* keys, const size_t* keylens, const int64_t* n,
                    const int64_t* at_ns, int64_t now_ns, uint8_t* applied, char* err, size_t errlen);
/* Charge: record usage that is only known after the fact (rl_charge_batch,
 * include/rl_engine.h).  A token bucket gives up min(n, what it holds) and
 * never goes below zero; a window counter records the whole n, over its limit
 * or not (its script runs INCRBY before it compares).  *out: charged, short_by
 * = n - charged, remaining, reset_at_unix_ns, and over_limit -- less than n was
 * charged, or the window's count is now above its limit.  now_ns is the time of
 * the request (RLL_NOW_WALL: the wall clock).  n <= 0 is RLL_ERR_INVALID_N
 * before any I/O.  The key is interned as rll_allow_n interns it.  On a storage
 * error (a closed limiter, a cancelled context, an engine failure, a request
 * the engine could not execute) a fail-open limiter answers RLL_OK with
 * charged = 0 and over_limit = 0 -- the usage is not recorded and nobody is
 * held up --, a fail-closed one RLL_ERR_CHARGE with the message.  The metrics
 * decorator counts rate_limiter_charged_units_total{algorithm} and
 * rate_limiter_charge_short_units_total{algorithm}, exposed once the verb was
 * used; the logging decorator logs a short charge at debug and a failed call
 * at error level. */
typedef struct rll_charge {
    int64_t charged;
    int64_t short_by;
    int64_t remaining;
    int64_t reset_at_unix_ns;
    uint8_t over_limit;
    uint8_t pad_[7];
} rll_charge;
int rll_charge_n(rll_limiter* l, const char* key, size_t keylen, int64_t n, int64_t now_ns, int ctx_cancelled,
                 rll_charge* out, char* err, size_t errlen);
/* m charges in ONE engine call, all at now_ns.  Within the call a later request
 * for the same bucket asks against the state before the call: it can charge 0
 * (over_limit = 1) where a call of its own would charge what is left, and the
 * caller charges again.  Any n <= 0 fails the whole call with
 * RLL_ERR_INVALID_N, nothing applied.  A fail-closed limiter fails the whole
 * call on the first request the engine could not execute. */
int rll_charge_many(rll_limiter* l, size_t m, const char* const* keys, const size_t* keylens, const int64_t* n,
                    int64_t now_ns, int ctx_cancelled, rll_charge* out /* m */, char* err, size_t errlen);
/* AllowAll: check one request against k limiters, 1 <= k <= 16, all on one
 * rll_engine (else RLL_ERR_ARG), all or nothing (rl_allow_all_batch,
 * include/rl_engine.h): one group of one engine call.  Quota stays taken only
 * if every member was allowed; otherwise every member that took something gets
 * it back, a denied window member's count included, up to Refund's limits.
 * out[j] is limiter j's Result as rll_allow_n would build it (its remaining is
 * the value before any give-back); *allowed (nullable) is 1 iff every member
 * was allowed; *denied_by (nullable) the index of the first member that was
 * not, or -1.  Any n <= 0 is RLL_ERR_INVALID_N before any I/O.  A key never
 * seen is interned exactly as rll_allow_n interns it.  A storage error (a
 * closed limiter, a cancelled context, an engine failure) is handled per
 * limiter: a fail-open limiter contributes its fail-open Result and is not
 * sent to the engine, a fail-closed one fails the call with RLL_ERR_FAILED as
 * rll_allow_n does -- before anything is sent when the error is known then.
 * A member the engine could not execute (RL_ERROR: INCRBY overflow) is
 * RLL_ERR_FAILED with that limiter's message; its group was rolled back.  The
 * metrics decorator of each member counts the group
 * (rate_limiter_allow_all_total{allowed}) and the units of its own take that
 * were given back (rate_limiter_allow_all_rolled_back_units_total{algorithm}),
 * exposed once the verb was used; the logging decorator logs a denied group at
 * debug and a failed call at error level. */
int rll_allow_all(rll_limiter* const* ls, size_t k, const char* const* keys, const size_t* keylens,
                  const int64_t* n, int64_t now_ns, int ctx_cancelled, rll_result* out /* k */, uint8_t* allowed,
                  int32_t* denied_by, char* err, size_t errlen);
int rll_close(rll_limiter* l);   /* Close(): later calls take the storage-error path */
int rll_free(rll_limiter* l);

#ifdef __cplusplus
}
#endif
#endif
