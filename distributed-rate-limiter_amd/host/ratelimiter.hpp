// ratelimiter.hpp -- host-side mirror of the reference's Go package
// `internal/ratelimiter` over the MI355X engine (include/rl_engine.h).
//
// Same names, argument meaning and error behaviour as the reference:
//   Algorithm / Config / Result        interface.go:8-70
//   Config::Validate / WithDefaults /
//   KeyPrefix / FormatKey              config.go:16-87 (identical messages)
//   RateLimiter::Allow/AllowN/Reset/
//   Close                              interface.go:76-145
//   NewTokenBucket / NewSlidingWindow /
//   NewFixedWindow                     tokenbucket.go:63-81, slidingwindow.go:41-59,
//                                      fixedwindow.go:38-56
//   ErrInvalidN etc.                   errors.go:5-20
// The storage client argument (`*redis.Client`) becomes an `Engine*`; all
// decisions go through one GPU launch sequence (single call or batch).
// Go is not available in this build image; this C++ layer is the executable
// specification of the thin Go/cgo layer shown in INTEGRATION.md.
#pragma once

#include <stdint.h>

#include <atomic>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rl_engine.h"

namespace ratelimiter {

using Algorithm = std::string;
extern const Algorithm TokenBucket;    // "token_bucket"
extern const Algorithm SlidingWindow;  // "sliding_window"
extern const Algorithm FixedWindow;    // "fixed_window"
extern const char* const DefaultPrefix;  // "ratelimit"

constexpr int64_t Nanosecond = 1, Microsecond = 1000, Millisecond = 1000000, Second = 1000000000,
                  Minute = 60 * Second, Hour = 60 * Minute;

// Go's time.Duration.String()
std::string DurationString(int64_t d);

// Go-style error value: empty = nil.  `is` tags sentinel identity (errors.Is).
struct Error {
    enum Kind { None = 0, InvalidN, InvalidConfig, StorageUnavailable, InvalidKey, Closed, Other };
    Kind is = None;
    std::string msg;
    explicit operator bool() const { return is != None; }
    static Error New(Kind k, std::string m) { return Error{k, std::move(m)}; }
};
extern const Error ErrInvalidConfig, ErrStorageUnavailable, ErrInvalidKey, ErrInvalidN, ErrClosed;

struct Result {
    bool Allowed = false;
    int64_t Limit = 0;
    int64_t Remaining = 0;
    int64_t RetryAfter = 0;  // time.Duration (ns)
    int64_t ResetAt = 0;     // time.Time as Unix ns
};

// time.Time{} (the zero Time) as a ResetAt value
constexpr int64_t ZeroTime = INT64_MIN;

// Result constructors (result.go:5-50)
Result NewAllowedResult(int64_t limit, int64_t remaining, int64_t reset_at);
Result NewDeniedResult(int64_t limit, int64_t retry_after, int64_t reset_at);
Result NewFailOpenResult();
Result NewFailClosedResult();

struct Config {
    Algorithm algorithm;
    int64_t Limit = 0;
    int64_t Window = 0;  // time.Duration (ns)
    std::string Prefix;
    bool FailOpen = false;

    Config WithDefaults() const;
    std::string KeyPrefix() const { return Prefix; }
    std::string FormatKey(const std::string& key) const;
};
// nil-receiver forms (config.go:17-19, :55-57, :72-74)
Error Validate(const Config* c);
std::string KeyPrefix(const Config* c);
std::string FormatKey(const Config* c, const std::string& key);

// context.Context subset: cancellation + deadline (Unix ns, 0 = none)
struct Context {
    std::atomic<bool> cancelled{false};
    int64_t deadline_ns = 0;
    Context() = default;
    Context(const Context& o) : cancelled(o.cancelled.load()), deadline_ns(o.deadline_ns) {}
    static const Context& Background();
};

// Unix-ns clock standing for time.Now(); replaceable for deterministic tests.
using Clock = std::function<int64_t()>;
int64_t WallClockNs();

// One GPU engine plus the key-id interner: the "storage" all limiters share,
// as one Redis.  A key's identity is its formatted name (FormatKey,
// config.go:81-87) and nothing else, so limiters with one Prefix share state
// exactly as they share Redis keys.
class Engine {
public:
    static Error Create(const rl_opts& opts, std::unique_ptr<Engine>* out);
    explicit Engine(rl_engine* e) : e_(e) {}
    ~Engine();
    rl_engine* raw() { return e_; }
    uint64_t Intern(const std::string& formatted_key);
    // lookup only: false (and nothing interned) for a name never seen
    bool Lookup(const std::string& formatted_key, uint64_t* id);
    // the formatted key of an interned id ("" if unknown)
    std::string Name(uint64_t id);
    std::mutex& mu() { return mu_; }
    Clock clock = WallClockNs;
    // test hook: when >= 0, every call passes this Redis clock (ms)
    int64_t server_ms_override = INT64_MIN;

private:
    rl_engine* e_;
    std::mutex mu_;
    std::mutex intern_mu_;
    std::unordered_map<std::string, uint64_t> ids_;
    std::vector<std::string> names_;   // by id
};

struct BatchRequest {
    std::string key;
    int64_t n = 1;
    int64_t now_ns = INT64_MIN;  // INT64_MIN: read the engine clock
};
struct BatchOutcome {
    Error err;
    Result result;
    bool has_result = false;
};

// one refund: n units back to `key`; at_ns picks the window (a window limiter
// refunds the counter of the window at_ns lies in; 0 = the call's time)
struct RefundRequest {
    std::string key;
    int64_t n = 1;
    int64_t at_ns = 0;
};

// one charge: n units of usage, known after the fact, recorded against `key`
struct ChargeRequest {
    std::string key;
    int64_t n = 1;
};
// what became of it: `charged` units were recorded (a bucket gives up what it
// holds, a window counter records all of n); `over_limit`: less than n was
// charged, or the window's count is now above its limit
struct ChargeOutcome {
    int64_t charged = 0;
    bool over_limit = false;
    int64_t remaining = 0;
    int64_t reset_at = 0;        // Unix ns
};

class Engine;
// a limiter's member of an AllowAll group (RateLimiter::AllowAllMemberOf)
struct AllowAllMember {
    Engine* engine = nullptr;
    bool closed = false;          // Close() was called: the storage-error path
    bool fail_open = false;
    int64_t limit = 0;
    int32_t alg = 0;              // RL_ALG_*
    uint32_t cfg_id = 0;
    uint64_t key_id = 0;
    int64_t ts = 0, sms = 0;
    int64_t fail_open_reset_at = 0;
};
// one member's view of a finished AllowAll call (RateLimiter::ObserveAllowAll)
struct AllowAllEvent {
    std::string key;
    int64_t n = 0;
    int32_t index = 0;            // of this member in its group
    size_t members = 0;
    bool allowed = false;         // the group
    int32_t denied_by = -1;
    uint64_t rolled_back_units = 0;   // of this member: n when its take was given back
    std::string error;            // not empty: the call failed with it
};

class RateLimiter {
public:
    virtual ~RateLimiter() = default;
    virtual Error Allow(const Context& ctx, const std::string& key, Result* out) = 0;
    virtual Error AllowN(const Context& ctx, const std::string& key, int64_t n, Result* out) = 0;
    virtual Error Reset(const Context& ctx, const std::string& key) = 0;
    // Reset as if called at Unix time t (deterministic replay)
    virtual Error ResetAt(const Context& ctx, const std::string& key, int64_t t) = 0;
    // ResetMany (new; rl_reset_batch): Reset of every key, in one engine
    // launch.  t = INT64_MIN reads the engine clock once per key, as that
    // many Reset calls would.
    virtual Error ResetManyAt(const Context& ctx, const std::vector<std::string>& keys, int64_t t) = 0;
    virtual Error Close() = 0;
    // Peek (new; rl_peek_batch): the Result AllowN(key, n) would return at
    // now_ns (INT64_MIN: the engine clock), changing nothing.  n == 0 asks how
    // much is left; n < 0 is ErrInvalidN.  A key never seen is not interned.
    virtual Error PeekN(const Context& ctx, const std::string& key, int64_t n, int64_t now_ns, Result* out) = 0;
    // Refund (new; rl_refund_batch): give back quota an admitted request did
    // not use, as ONE engine call -- per key (and window) the sum of the n is
    // returned in one step: a bucket gains min(capacity, tokens + N), a window
    // counter loses N (deleted at zero).  now_ns (INT64_MIN: the engine clock)
    // is the store clock.  Any n <= 0 is ErrInvalidN before any I/O.  A
    // storage error is returned as an error, never a fail-open Result, as
    // Reset does.  applied[i] (nullable): the key had live state to refund to
    // (a fresh key is full anyway).  A key never seen is not interned.
    virtual Error RefundMany(const Context& ctx, const std::vector<RefundRequest>& reqs, int64_t now_ns,
                             std::vector<uint8_t>* applied) = 0;
    // one refund (a call of one)
    Error RefundN(const Context& ctx, const std::string& key, int64_t n, int64_t now_ns, int64_t at_ns,
                  bool* applied) {
        std::vector<uint8_t> a;
        Error e = RefundMany(ctx, {RefundRequest{key, n, at_ns}}, now_ns, &a);
        if (!e && applied) *applied = a[0] != 0;
        return e;
    }
    // Charge (new; rl_charge_batch): record usage that is only known after
    // the fact, every request of the call in ONE engine call.  A token bucket
    // gives up min(n, what it holds) and never goes below zero; a window
    // counter records the whole n, over its limit or not.  Within one call a
    // later request for the same bucket asks against the state before the
    // call, so it can charge 0 where a call of its own would charge the rest:
    // its outcome says so, and the caller charges again.  now_ns (INT64_MIN:
    // the engine clock) is the time of every request.  Any n <= 0 is
    // ErrInvalidN before any I/O.  A storage error (closed limiter, cancelled
    // context, engine failure, a request the engine could not execute): a
    // fail-open limiter answers charged = 0 with no error -- the usage is not
    // recorded and the caller is not held up --, a fail-closed one returns
    // "failed to charge rate limit: ...".
    virtual Error ChargeMany(const Context& ctx, const std::vector<ChargeRequest>& reqs, int64_t now_ns,
                             std::vector<ChargeOutcome>* out) = 0;
    // one charge (a call of one)
    Error ChargeN(const Context& ctx, const std::string& key, int64_t n, int64_t now_ns, ChargeOutcome* out) {
        std::vector<ChargeOutcome> o;
        Error e = ChargeMany(ctx, {ChargeRequest{key, n}}, now_ns, &o);
        if (!e && out) *out = o[0];
        return e;
    }
    // AllowAll (new; ratelimiter::AllowAll below): this limiter's member of a
    // group check.  With intern == false only the engine, `closed` and the
    // config fields are filled in; with intern == true also the key id (the
    // key is interned exactly as AllowN interns it) and the clocks of now_ns
    // (INT64_MIN: the engine clock).  false: this limiter cannot take part.
    // A decorator forwards to the limiter it wraps.
    virtual bool AllowAllMemberOf(const std::string& key, int64_t now_ns, bool intern, AllowAllMember* m) {
        (void)key, (void)now_ns, (void)intern, (void)m;
        return false;
    }
    // what became of a group this limiter was a member of: a decorator counts
    // or logs it and forwards it to the limiter it wraps
    virtual void ObserveAllowAll(const AllowAllEvent& ev) { (void)ev; }
    // request-coalescing path (new): one engine launch for many requests
    virtual void BatchAllow(const Context& ctx, const std::vector<BatchRequest>& reqs,
                            std::vector<BatchOutcome>* out) = 0;
    virtual const Config& config() const = 0;
};

// AllowAll (new; rl_allow_all_batch): check one request against k limiters of
// one engine, 1 <= k <= 16, all or nothing: quota stays taken only if every
// member was allowed; otherwise every member that took something gets it back
// (a denied window member's INCRBY included), up to Refund's limits.
// (*out)[j] is limiter j's Result as AllowN would build it; *allowed: every
// member was allowed; *denied_by: the first member that was not, or -1.  Any
// n <= 0 is ErrInvalidN before any I/O.  A storage error (closed limiter,
// cancelled context, engine failure) is handled per limiter: a fail-open
// limiter contributes its fail-open Result (and is not sent to the engine), a
// fail-closed one fails the call with "failed to check rate limit: ...".  A
// member the engine could not execute (RL_ERROR, RL_INVALID) fails the call
// with that limiter's message, fail-open or not: its group was rolled back, so
// nothing was admitted.  *bad_arg: k out of range, a null limiter, or
// limiters of different engines (nothing ran).
Error AllowAll(const Context& ctx, const std::vector<RateLimiter*>& ls, const std::vector<std::string>& keys,
               const std::vector<int64_t>& n, int64_t now_ns, std::vector<Result>* out, bool* allowed,
               int32_t* denied_by, bool* bad_arg);

Error NewTokenBucket(Engine* engine, const Config* config, std::unique_ptr<RateLimiter>* out);
Error NewSlidingWindow(Engine* engine, const Config* config, std::unique_ptr<RateLimiter>* out);
Error NewFixedWindow(Engine* engine, const Config* config, std::unique_ptr<RateLimiter>* out);
// dispatch on config->algorithm
Error New(Engine* engine, const Config* config, std::unique_ptr<RateLimiter>* out);

}  // namespace ratelimiter
