// decorators.cpp -- see decorators.hpp (ADR-003 decorator pattern).
#include "decorators.hpp"

#include <stdio.h>

namespace ratelimiter {

const char* ErrorType(const Error& e) {
    switch (e.is) {
        case Error::None: return "none";
        case Error::InvalidN: return "invalid_n";
        case Error::InvalidConfig: return "invalid_config";
        case Error::StorageUnavailable: return "storage_unavailable";
        case Error::InvalidKey: return "invalid_key";
        case Error::Closed: return "closed";
        default: return "other";
    }
}

const std::array<double, 12> MetricsDecorator::kBuckets = {1e-5, 2.5e-5, 5e-5, 1e-4, 2.5e-4, 5e-4,
                                                          1e-3, 2.5e-3, 5e-3, 1e-2, 1e-1, 1.0};

MetricsDecorator::MetricsDecorator(std::unique_ptr<RateLimiter> inner, Clock clock)
    : inner_(std::move(inner)), clock_(std::move(clock)) {}

void MetricsDecorator::record(const Error& e, const Result* r, int64_t n_decisions, int64_t elapsed_ns) {
    const double s = (double)elapsed_ns / 1e9;
    size_t b = 0;
    while (b < kBuckets.size() && s > kBuckets[b]) b++;
    std::lock_guard<std::mutex> g(mu_);
    requests_[{!e && r && r->Allowed, ErrorType(e)}] += 1;
    hist_[b] += (uint64_t)n_decisions;
    sum_s_ += s * (double)n_decisions;
    observations_ += (uint64_t)n_decisions;
}

Error MetricsDecorator::Allow(const Context& ctx, const std::string& key, Result* out) {
    return AllowN(ctx, key, 1, out);
}

Error MetricsDecorator::AllowN(const Context& ctx, const std::string& key, int64_t n, Result* out) {
    const int64_t t0 = clock_();
    Result r;
    Error e = inner_->AllowN(ctx, key, n, &r);
    record(e, &r, 1, clock_() - t0);
    if (!e && out) *out = r;
    return e;
}

Error MetricsDecorator::Reset(const Context& ctx, const std::string& key) { return inner_->Reset(ctx, key); }
Error MetricsDecorator::ResetAt(const Context& ctx, const std::string& key, int64_t t) {
    return inner_->ResetAt(ctx, key, t);
}

void MetricsDecorator::BatchAllow(const Context& ctx, const std::vector<BatchRequest>& reqs,
                                  std::vector<BatchOutcome>* out) {
    const int64_t t0 = clock_();
    inner_->BatchAllow(ctx, reqs, out);
    const int64_t dt = clock_() - t0;
    // every request of the batch waited for the whole batch
    for (const auto& o : *out) record(o.err, o.has_result ? &o.result : nullptr, 1, dt);
}

Error MetricsDecorator::RefundMany(const Context& ctx, const std::vector<RefundRequest>& reqs, int64_t now_ns,
                                   std::vector<uint8_t>* applied) {
    std::vector<uint8_t> a;
    Error e = inner_->RefundMany(ctx, reqs, now_ns, &a);
    if (!e) {
        std::lock_guard<std::mutex> g(mu_);
        for (size_t i = 0; i < reqs.size(); i++) {
            refunds_[a[i] ? 1 : 0]++;
            if (a[i]) {
                const uint64_t u = (uint64_t)reqs[i].n;
                refunded_units_ = refunded_units_ + u < refunded_units_ ? UINT64_MAX : refunded_units_ + u;
            }
        }
        if (applied) *applied = a;
    }
    return e;
}

static uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? UINT64_MAX : a + b; }

Error MetricsDecorator::ChargeMany(const Context& ctx, const std::vector<ChargeRequest>& reqs, int64_t now_ns,
                                   std::vector<ChargeOutcome>* out) {
    std::vector<ChargeOutcome> o;
    Error e = inner_->ChargeMany(ctx, reqs, now_ns, &o);
    if (e.is != Error::InvalidN) {
        std::lock_guard<std::mutex> g(mu_);
        charge_used_ = true;
        if (!e)
            for (size_t i = 0; i < reqs.size(); i++) {
                charged_units_ = sat_add(charged_units_, (uint64_t)o[i].charged);
                charge_short_units_ = sat_add(charge_short_units_, (uint64_t)(reqs[i].n - o[i].charged));
            }
    }
    if (!e && out) *out = o;
    return e;
}

uint64_t MetricsDecorator::ChargedUnits() const {
    std::lock_guard<std::mutex> g(mu_);
    return charged_units_;
}

uint64_t MetricsDecorator::ChargeShortUnits() const {
    std::lock_guard<std::mutex> g(mu_);
    return charge_short_units_;
}

void MetricsDecorator::ObserveAllowAll(const AllowAllEvent& ev) {
    {
        std::lock_guard<std::mutex> g(mu_);
        allow_all_used_ = true;
        allow_alls_[ev.error.empty() && ev.allowed ? 1 : 0]++;
        const uint64_t u = ev.rolled_back_units;
        rolled_back_units_ = rolled_back_units_ + u < rolled_back_units_ ? UINT64_MAX : rolled_back_units_ + u;
    }
    inner_->ObserveAllowAll(ev);
}

uint64_t MetricsDecorator::AllowAlls(bool allowed) const {
    std::lock_guard<std::mutex> g(mu_);
    return allow_alls_[allowed ? 1 : 0];
}

uint64_t MetricsDecorator::RolledBackUnits() const {
    std::lock_guard<std::mutex> g(mu_);
    return rolled_back_units_;
}

uint64_t MetricsDecorator::Refunds(bool applied) const {
    std::lock_guard<std::mutex> g(mu_);
    return refunds_[applied ? 1 : 0];
}

uint64_t MetricsDecorator::RefundedUnits() const {
    std::lock_guard<std::mutex> g(mu_);
    return refunded_units_;
}

uint64_t MetricsDecorator::Count(bool allowed, const std::string& error) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = requests_.find({allowed, error});
    return it == requests_.end() ? 0 : it->second;
}

std::string MetricsDecorator::Expose() const {
    std::lock_guard<std::mutex> g(mu_);
    const std::string alg = inner_->config().algorithm;
    std::string s = "# HELP rate_limiter_requests_total Rate limit decisions by outcome.\n"
                    "# TYPE rate_limiter_requests_total counter\n";
    char line[256];
    for (const auto& kv : requests_) {
        snprintf(line, sizeof line, "rate_limiter_requests_total{algorithm=\"%s\",allowed=\"%s\",error=\"%s\"} %llu\n",
                 alg.c_str(), kv.first.first ? "true" : "false", kv.first.second.c_str(),
                 (unsigned long long)kv.second);
        s += line;
    }
    s += "# HELP rate_limiter_decision_seconds Decision latency.\n"
         "# TYPE rate_limiter_decision_seconds histogram\n";
    uint64_t acc = 0;
    for (size_t b = 0; b <= kBuckets.size(); b++) {
        acc += hist_[b];
        if (b < kBuckets.size())
            snprintf(line, sizeof line, "rate_limiter_decision_seconds_bucket{algorithm=\"%s\",le=\"%g\"} %llu\n",
                     alg.c_str(), kBuckets[b], (unsigned long long)acc);
        else
            snprintf(line, sizeof line, "rate_limiter_decision_seconds_bucket{algorithm=\"%s\",le=\"+Inf\"} %llu\n",
                     alg.c_str(), (unsigned long long)acc);
        s += line;
    }
    snprintf(line, sizeof line, "rate_limiter_decision_seconds_sum{algorithm=\"%s\"} %.9g\n", alg.c_str(), sum_s_);
    s += line;
    snprintf(line, sizeof line, "rate_limiter_decision_seconds_count{algorithm=\"%s\"} %llu\n", alg.c_str(),
             (unsigned long long)observations_);
    s += line;
    if (refunds_[0] || refunds_[1]) {
        s += "# HELP rate_limiter_refunds_total Refund requests by whether the key had live state.\n"
             "# TYPE rate_limiter_refunds_total counter\n";
        for (int a = 0; a < 2; a++) {
            snprintf(line, sizeof line, "rate_limiter_refunds_total{algorithm=\"%s\",applied=\"%s\"} %llu\n", alg.c_str(),
                     a ? "true" : "false", (unsigned long long)refunds_[a]);
            s += line;
        }
        s += "# HELP rate_limiter_refunded_units_total Units given back by applied refunds.\n"
             "# TYPE rate_limiter_refunded_units_total counter\n";
        snprintf(line, sizeof line, "rate_limiter_refunded_units_total{algorithm=\"%s\"} %llu\n", alg.c_str(),
                 (unsigned long long)refunded_units_);
        s += line;
    }
    if (allow_all_used_) {
        s += "# HELP rate_limiter_allow_all_total All-or-nothing group checks this limiter was a member of.\n"
             "# TYPE rate_limiter_allow_all_total counter\n";
        for (int a = 0; a < 2; a++) {
            snprintf(line, sizeof line, "rate_limiter_allow_all_total{allowed=\"%s\"} %llu\n", a ? "true" : "false",
                     (unsigned long long)allow_alls_[a]);
            s += line;
        }
        s += "# HELP rate_limiter_allow_all_rolled_back_units_total Units taken by this limiter in a failed group "
             "and given back.\n"
             "# TYPE rate_limiter_allow_all_rolled_back_units_total counter\n";
        snprintf(line, sizeof line, "rate_limiter_allow_all_rolled_back_units_total{algorithm=\"%s\"} %llu\n",
                 alg.c_str(), (unsigned long long)rolled_back_units_);
        s += line;
    }
    if (charge_used_) {
        s += "# HELP rate_limiter_charged_units_total Units of usage recorded after the fact.\n"
             "# TYPE rate_limiter_charged_units_total counter\n";
        snprintf(line, sizeof line, "rate_limiter_charged_units_total{algorithm=\"%s\"} %llu\n", alg.c_str(),
                 (unsigned long long)charged_units_);
        s += line;
        s += "# HELP rate_limiter_charge_short_units_total Units a charge asked for and the limiter could not cover.\n"
             "# TYPE rate_limiter_charge_short_units_total counter\n";
        snprintf(line, sizeof line, "rate_limiter_charge_short_units_total{algorithm=\"%s\"} %llu\n", alg.c_str(),
                 (unsigned long long)charge_short_units_);
        s += line;
    }
    return s;
}

LoggingDecorator::LoggingDecorator(std::unique_ptr<RateLimiter> inner, LogSink sink)
    : inner_(std::move(inner)), sink_(std::move(sink)) {}

void LoggingDecorator::log_outcome(const std::string& key, const Error& e, const Result* r) {
    if (e) {
        sink_(LogLevel::Error, "rate limiter error", {{"key", key}, {"error", e.msg}});
    } else if (r && !r->Allowed) {
        sink_(LogLevel::Debug, "request denied", {{"key", key}, {"limit", std::to_string(r->Limit)}});
    }
}

Error LoggingDecorator::Allow(const Context& ctx, const std::string& key, Result* out) {
    return AllowN(ctx, key, 1, out);
}

Error LoggingDecorator::AllowN(const Context& ctx, const std::string& key, int64_t n, Result* out) {
    Result r;
    Error e = inner_->AllowN(ctx, key, n, &r);
    log_outcome(key, e, e ? nullptr : &r);
    if (!e && out) *out = r;
    return e;
}

Error LoggingDecorator::Reset(const Context& ctx, const std::string& key) {
    Error e = inner_->Reset(ctx, key);
    if (e) sink_(LogLevel::Error, "rate limiter reset error", {{"key", key}, {"error", e.msg}});
    return e;
}

Error LoggingDecorator::ResetAt(const Context& ctx, const std::string& key, int64_t t) {
    Error e = inner_->ResetAt(ctx, key, t);
    if (e) sink_(LogLevel::Error, "rate limiter reset error", {{"key", key}, {"error", e.msg}});
    return e;
}

Error LoggingDecorator::ResetManyAt(const Context& ctx, const std::vector<std::string>& keys, int64_t t) {
    Error e = inner_->ResetManyAt(ctx, keys, t);
    if (e) sink_(LogLevel::Error, "rate limiter reset error", {{"keys", std::to_string(keys.size())}, {"error", e.msg}});
    return e;
}

void LoggingDecorator::ObserveAllowAll(const AllowAllEvent& ev) {
    if (!ev.error.empty())
        sink_(LogLevel::Error, "rate limiter allow-all error",
              {{"key", ev.key}, {"members", std::to_string(ev.members)}, {"error", ev.error}});
    else if (!ev.allowed)
        sink_(LogLevel::Debug, "allow-all denied",
              {{"key", ev.key}, {"n", std::to_string(ev.n)}, {"member", std::to_string(ev.index)},
               {"denied_by", std::to_string(ev.denied_by)},
               {"rolled_back_units", std::to_string(ev.rolled_back_units)}});
    inner_->ObserveAllowAll(ev);
}

Error LoggingDecorator::RefundMany(const Context& ctx, const std::vector<RefundRequest>& reqs, int64_t now_ns,
                                   std::vector<uint8_t>* applied) {
    std::vector<uint8_t> a;
    Error e = inner_->RefundMany(ctx, reqs, now_ns, &a);
    if (e) {
        sink_(LogLevel::Error, "rate limiter refund error",
              {{"keys", std::to_string(reqs.size())}, {"error", e.msg}});
        return e;
    }
    for (size_t i = 0; i < reqs.size(); i++)
        sink_(LogLevel::Debug, "quota refunded",
              {{"key", reqs[i].key}, {"n", std::to_string(reqs[i].n)}, {"applied", a[i] ? "true" : "false"}});
    if (applied) *applied = a;
    return e;
}

Error LoggingDecorator::ChargeMany(const Context& ctx, const std::vector<ChargeRequest>& reqs, int64_t now_ns,
                                   std::vector<ChargeOutcome>* out) {
    std::vector<ChargeOutcome> o;
    Error e = inner_->ChargeMany(ctx, reqs, now_ns, &o);
    if (e) {
        sink_(LogLevel::Error, "rate limiter charge error", {{"keys", std::to_string(reqs.size())}, {"error", e.msg}});
        return e;
    }
    for (size_t i = 0; i < reqs.size(); i++)
        if (o[i].charged < reqs[i].n)
            sink_(LogLevel::Debug, "charge short",
                  {{"key", reqs[i].key}, {"n", std::to_string(reqs[i].n)}, {"charged", std::to_string(o[i].charged)}});
    if (out) *out = o;
    return e;
}

void LoggingDecorator::BatchAllow(const Context& ctx, const std::vector<BatchRequest>& reqs,
                                  std::vector<BatchOutcome>* out) {
    inner_->BatchAllow(ctx, reqs, out);
    for (size_t i = 0; i < out->size(); i++)
        log_outcome(reqs[i].key, (*out)[i].err, (*out)[i].has_result ? &(*out)[i].result : nullptr);
}

}  // namespace ratelimiter
