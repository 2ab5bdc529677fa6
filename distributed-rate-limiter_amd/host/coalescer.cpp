// coalescer.cpp -- see coalescer.hpp / include/rl_coalescer.h.
#include "coalescer.hpp"

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <chrono>

#include "../csrc/rl_table.h"   // rl::mix64

namespace rlc {

int64_t steady_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

Sub::Sub(size_t m_) : mem(new uint8_t[block_bytes(m_ ? m_ : 1)]), cap(m_ ? m_ : 1) {
    // layout by capacity, so a reused buffer keeps its arrays in place
    carve(mem.get(), cap, *this);
    renew(m_);
}

void Sub::renew(size_t m_) {
    first = 0;
    m = m_;
    taken = 0;
    left = m_;
    status = RL_OK;
    op = OP_REQ;
    deadline = 0;
    done = waiting = cancelled = dropped = truncated = in_queue = waited = false;
    inflight = 0;
    done_ns = submit_ns = 0;
    tag = nullptr;
    args = OpArgs{};
    info = rl_table_info{};
}

// Completion waits: the runtime's (default), or polling the event
// (RL_COALESCER_POLL=1, one busy core per waiting thread).  The A/B in
// DESIGN.md (configs[4] tail) found the same rare stalls either way.
static bool poll_waits() {
    static const bool p = getenv("RL_COALESCER_POLL") != nullptr;
    return p;
}
static hipError_t await_event(hipEvent_t ev) {
    if (!poll_waits()) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t r = hipEventQuery(ev);
        if (r != hipErrorNotReady) return r;
        for (int i = 0; i < 32; i++) __builtin_ia32_pause();
    }
}

// ---------------------------------------------------------------------------
// GPU backend: pinned staging per slot, one H2D copy stream, results come back
// on an output stream that the engine orders behind each batch's finish.
// Inputs are complete when rl_decide_batch_device is called (the H2D copy is
// waited for on the submitter thread), so an engine created with
// RL_OPT_PIPELINE overlaps batch b+1's grouping with batch b's replay.
// ---------------------------------------------------------------------------
class GpuBackend : public Backend {
public:
    explicit GpuBackend(rl_engine* e) : e_(e) { (void)hipGetDevice(&dev_id_); }
    ~GpuBackend() override {
        for (auto& d : dev_) {
            (void)hipFree(d.key);
            if (d.ev) (void)hipEventDestroy(d.ev);
            if (d.ev_in) (void)hipEventDestroy(d.ev_in);
        }
        for (void* h : host_) (void)hipHostFree(h);
        if (cs_) (void)hipStreamDestroy(cs_);
        if (os_) (void)hipStreamDestroy(os_);
    }
    int init(int nslots, size_t M, std::vector<Slot>* slots) override {
        (void)hipSetDevice(dev_id_);
        if (hipStreamCreateWithFlags(&cs_, hipStreamNonBlocking) != hipSuccess) return RL_EDEVICE;
        if (hipStreamCreateWithFlags(&os_, hipStreamNonBlocking) != hipSuccess) return RL_EDEVICE;
        slots->resize(nslots);
        dev_.resize(nslots);
        for (int i = 0; i < nslots; i++) {
            // inputs first (one H2D block), then outputs
            void* h = nullptr;
            if (hipHostMalloc(&h, block_bytes(M), hipHostMallocDefault) != hipSuccess) return RL_ENOMEM;
            host_.push_back(h);
            carve(static_cast<uint8_t*>(h), M, (*slots)[i]);
            Dev& d = dev_[i];
            uint8_t* dp = nullptr;
            if (hipMalloc(&dp, block_bytes(M)) != hipSuccess) return RL_ENOMEM;
            d.key = dp;
            if (hipEventCreateWithFlags(&d.ev, hipEventDisableTiming) != hipSuccess) return RL_EDEVICE;
            if (hipEventCreateWithFlags(&d.ev_in, hipEventDisableTiming) != hipSuccess) return RL_EDEVICE;
        }
        M_ = M;
        return RL_OK;
    }
    int tally_enable(uint32_t key_slots) override {
        (void)hipSetDevice(dev_id_);
        rl_tally_opts o{sizeof(rl_tally_opts), key_slots};
        const int rc = rl_tally_enable(e_, &o);
        tally_ = rc == RL_OK;
        return rc;
    }
    // the tallies were enqueued on os_ behind their batches: rl_tally_read
    // waits for the last of them -- which is behind the finish of every batch
    // launched so far -- and copies on the engine's stream, where those
    // finishes ran; batches submitted after this call are not launched yet
    int tally_read(const TallyArgs& a) override {
        (void)hipSetDevice(dev_id_);
        return rl_tally_read(e_, a.cfg_out, a.cfg_cap, a.ncfg, a.key_out, a.key_cap, a.keys_tracked, a.info, a.clear);
    }
    int hot_enable(const rl_hot_opts& o) override {
        (void)hipSetDevice(dev_id_);
        const int rc = rl_hot_enable(e_, &o);
        hot_ = rc == RL_OK;
        return rc;
    }
    // as tally_read: rl_hot_read waits for the last call enqueued on os_
    int hot_read(const HotArgs& a) override {
        (void)hipSetDevice(dev_id_);
        return rl_hot_read(e_, a.key_out, a.key_cap, a.keys_tracked, a.info, a.clear);
    }
    // The one staging routine.  A batch of up to zero_copy_max_ requests runs
    // zero-copy: the kernels read the requests from, and write the results
    // into, the pinned slot itself (host memory the device maps).  No
    // hipMemcpyAsync on the submit path: the configs[4] stalls were the
    // submitter blocked ~8 ms inside those calls with the device idle
    // (profiles/r3d_stall_trace.json).  A larger one is staged: the inputs
    // the operation reads go to the slot's device block on cs_ and are waited
    // for here, and what it returns comes back on os_ behind the engine's
    // work.  Either way the slot's completion event is recorded on os_ last,
    // so the slot is not reused before everything enqueued for it has run.
    int launch(int i, Slot& s) override {
        (void)hipSetDevice(dev_id_);   // the submitter thread
        Dev& d = dev_[i];
        const OpTraits& t = OPS[s.op];
        const size_t m = s.m;
        const bool staged = m > zero_copy_max_;
        Arrays a = s;   // the arrays the engine works on
        if (staged) {
            carve(d.key, M_, a);
            bool ok = hipMemcpyAsync(a.key, s.key, 8 * m, hipMemcpyHostToDevice, cs_) == hipSuccess;
            ok &= hipMemcpyAsync(a.ts, s.ts, 8 * m, hipMemcpyHostToDevice, cs_) == hipSuccess;
            if (t.reads_n) ok &= hipMemcpyAsync(a.n, s.n, 8 * m, hipMemcpyHostToDevice, cs_) == hipSuccess;
            ok &= hipMemcpyAsync(a.cfg, s.cfg, 4 * m, hipMemcpyHostToDevice, cs_) == hipSuccess;
            if (t.grouped) ok &= hipMemcpyAsync(a.head, s.head, m, hipMemcpyHostToDevice, cs_) == hipSuccess;
            ok &= hipEventRecord(d.ev_in, cs_) == hipSuccess;
            ok &= await_event(d.ev_in) == hipSuccess;
            if (!ok) return RL_EDEVICE;
        }
        s.t_h2d = steady_ns();
        const int rc = engine_call(s.op, m, a);
        if (rc != RL_OK) return rc;
        bool ok = true;
        if (staged) {
            ok = hipMemcpyAsync(s.dec, a.dec, m, hipMemcpyDeviceToHost, os_) == hipSuccess;
            if (t.results) {
                ok &= hipMemcpyAsync(s.rem, a.rem, 8 * m, hipMemcpyDeviceToHost, os_) == hipSuccess;
                ok &= hipMemcpyAsync(s.retry, a.retry, 8 * m, hipMemcpyDeviceToHost, os_) == hipSuccess;
                ok &= hipMemcpyAsync(s.reset, a.reset, 8 * m, hipMemcpyDeviceToHost, os_) == hipSuccess;
            }
            if (t.grouped) ok &= hipMemcpyAsync(s.verdict, a.verdict, m, hipMemcpyDeviceToHost, os_) == hipSuccess;
        }
        ok &= hipEventRecord(d.ev, os_) == hipSuccess;
        return ok ? RL_OK : RL_EDEVICE;
    }
    // The engine's work for one launch, enqueued so that os_ (and with it the
    // slot's completion event) waits for it.  A reset or a refund is one or
    // two kernels on the engine's replay stream between two batches.  Behind
    // a successful decide, the tally and then the top keys count the batch on
    // os_, on the arrays the decide used; behind an AllowAll call they count
    // its members the same way, with the members' own decisions, and behind a
    // Charge call its requests, with the asked n and the verb's decisions.
    int engine_call(Op op, size_t m, const Arrays& a) {
        switch (op) {
            case OP_REQ: {
                int rc = rl_decide_batch_device(e_, m, a.key, a.ts, a.n, a.cfg, nullptr, a.dec, a.rem, a.retry, a.reset,
                                                nullptr, os_);
                if (rc == RL_OK && tally_) rc = rl_tally_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                if (rc == RL_OK && hot_) rc = rl_hot_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                return rc;
            }
            case OP_PEEK:
                return rl_peek_batch_device(e_, m, a.key, a.ts, a.n, a.cfg, nullptr, a.dec, a.rem, a.retry, a.reset, nullptr,
                                            os_);
            case OP_RESET: return rl_reset_batch_device(e_, m, a.key, a.ts, a.cfg, a.dec, os_);
            case OP_REFUND: return rl_refund_batch_device(e_, m, a.key, a.ts, a.n, a.cfg, nullptr, a.dec, os_);
            case OP_ALLOW_ALL: {
                int rc = rl_allow_all_batch_device(e_, m, a.key, a.ts, a.n, a.cfg, nullptr, a.head, a.dec, a.rem, a.retry,
                                                   a.reset, nullptr, a.verdict, nullptr, os_);
                if (rc == RL_OK && tally_) rc = rl_tally_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                if (rc == RL_OK && hot_) rc = rl_hot_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                return rc;
            }
            case OP_CHARGE: {
                int rc = rl_charge_batch_device(e_, m, a.key, a.ts, a.n, a.cfg, nullptr, a.dec, a.retry, a.rem, a.reset,
                                                nullptr, os_);
                if (rc == RL_OK && tally_) rc = rl_tally_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                if (rc == RL_OK && hot_) rc = rl_hot_batch_device(e_, m, a.key, a.cfg, a.n, a.dec, os_);
                return rc;
            }
            default: return RL_EINVAL;
        }
    }
    int wait(int i, Slot&) override {
        (void)hipSetDevice(dev_id_);   // the completer thread
        return await_event(dev_[i].ev) == hipSuccess ? RL_OK : RL_EDEVICE;
    }
    int table_info(int64_t now_ms, rl_table_info* out) override {
        (void)hipSetDevice(dev_id_);
        return rl_table_info_get(e_, now_ms, out);
    }
    int gc(int64_t now_ms, uint64_t tb_cap, uint64_t win_cap, rl_table_info* out) override {
        (void)hipSetDevice(dev_id_);
        return rl_table_gc(e_, now_ms, tb_cap, win_cap, out);
    }
    int snapshot(int64_t now_ms, uint32_t world, uint32_t rank, void* buf, size_t cap,
                 rl_snapshot_info* out) override {
        (void)hipSetDevice(dev_id_);
        return rl_snapshot_export(e_, now_ms, world, rank, buf, cap, out);
    }
    int restore(const void* buf, size_t len, int64_t now_ms, uint64_t tb_cap, uint64_t win_cap,
                rl_table_info* out) override {
        (void)hipSetDevice(dev_id_);
        return rl_snapshot_import(e_, buf, len, now_ms, tb_cap, win_cap, out);
    }
    int table_of(uint32_t cfg) override {
        if (cfg >= table_.size()) {      // configs registered since: look them up once
            for (uint32_t c = (uint32_t)table_.size();; c++) {
                const int t = rl_config_table(e_, c);
                if (t < 0) break;
                table_.push_back((int8_t)t);
            }
        }
        return cfg < table_.size() ? table_[cfg] : -1;
    }

private:
    struct Dev {
        uint8_t* key = nullptr;   // base of the slot's device block
        hipEvent_t ev = nullptr;       // results back on the host
        hipEvent_t ev_in = nullptr;    // inputs on the device
    };
    rl_engine* e_;
    bool tally_ = false;         // tally_enable succeeded: launch() counts its batches
    bool hot_ = false;           // hot_enable succeeded: the same for the top keys
    std::vector<int8_t> table_;  // table_of per config id (submitter thread)
    int dev_id_ = 0;             // the engine's device: current when the coalescer is created
    // batches up to this size run zero-copy on the pinned slot (larger ones:
    // one H2D copy, device-resident inputs for the grouping's several reads)
    size_t zero_copy_max_ = getenv("RL_COALESCER_ZC_MAX") ? strtoull(getenv("RL_COALESCER_ZC_MAX"), nullptr, 10)
                                                          : (size_t)65536;
    hipStream_t cs_ = nullptr, os_ = nullptr;
    std::vector<void*> host_;
    std::vector<Dev> dev_;
    size_t M_ = 0;
};

// What the usage tally and the top keys over a host backend share.
//
// A host backend registers no configs: a config id is known from the first
// request of it the backend decided (any decision but RL_INVALID), up to
// MAX_CFGS ids.
struct KnownCfgs {
    static constexpr uint32_t MAX_CFGS = 1u << 16;   // one request's config id sizes the tally's rows: 3 MiB at most
    uint32_t n = 0;
    // request (config c, decision d) is of a known config (which it may make known)
    bool admit(uint32_t c, uint32_t d) {
        if (c >= n) {
            if (d >= RL_INVALID || c >= MAX_CFGS) return false;
            n = c + 1;
        }
        return true;
    }
};

// The key table of csrc/rl_tally.h and csrc/rl_hot.h in plain C++: rows with a
// key_id and a cfg_id, home slot mix64(key) & mask, linear probing over
// min(slots, 64) slots, a slot never released before a clear.
template <class Row>
struct KeyTable {
    static constexpr uint64_t PROBES = 64;
    std::vector<Row> rows;
    void assign(uint64_t slots) {   // all free: enable, and clear
        Row free{};
        free.key_id = RL_KEY_RESERVED;
        rows.assign(slots, free);
    }
    // the key's row, claimed on the way (and counted in *tracked) when it had
    // none; null: no room within the probes
    Row* find_or_claim(uint64_t k, uint32_t c, uint64_t* tracked) {
        const uint64_t mask = rows.size() - 1, probes = std::min<uint64_t>(rows.size(), PROBES);
        uint64_t s = rl::mix64(k) & mask;
        for (uint64_t p = 0; p < probes; p++, s = (s + 1) & mask) {
            Row& r = rows[s];
            if (r.key_id == RL_KEY_RESERVED) {
                r.key_id = k;
                r.cfg_id = c;
                (*tracked)++;
            }
            if (r.key_id == k) return &r;
        }
        return nullptr;
    }
    // the `cap` rows in use with the largest `by` (ties: the smaller key id
    // first), in that order
    void top(Row* out, size_t cap, uint64_t Row::*by) const {
        if (!out || !cap) return;
        std::vector<Row> tab;
        for (const Row& r : rows)
            if (r.key_id != RL_KEY_RESERVED) tab.push_back(r);
        const size_t want = std::min(cap, tab.size());
        std::partial_sort(tab.begin(), tab.begin() + want, tab.end(), [by](const Row& x, const Row& y) {
            return x.*by != y.*by ? x.*by > y.*by : x.key_id < y.key_id;
        });
        memcpy(out, tab.data(), sizeof(Row) * want);
    }
};

// The usage tally over a host backend: k_tally's sums (csrc/rl_tally.h) one
// request at a time -- the same per-config counters, the same key table.
class HostTally {
public:
    int enable(uint32_t key_slots) {
        if (key_slots > (1u << 24)) return RL_EINVAL;
        uint64_t slots = 16;
        while (slots < (key_slots ? key_slots : 65536u)) slots *= 2;
        keys_.assign(slots);
        return RL_OK;
    }
    void add(size_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n, const uint8_t* dec) {
        info_.batches++;
        info_.requests += m;
        for (size_t i = 0; i < m; i++) {
            const uint32_t c = cfg[i], d = dec[i];
            if (!known_.admit(c, d)) { info_.unknown_cfg++; continue; }
            if (known_.n > rows_.size()) rows_.resize(known_.n, rl_tally_cfg{});
            if (d > 3) { info_.bad_codes++; continue; }
            const uint64_t u = n[i] > 0 ? (uint64_t)n[i] : 0;
            rows_[c].count[d]++;
            if (d <= RL_ALLOWED) rows_[c].units[d] += u;
            if (d == RL_DENIED) denied(key[i], c, u);
        }
    }
    int read(const TallyArgs& a) {
        const size_t rows = a.cfg_out ? std::min(a.cfg_cap, rows_.size()) : 0;
        if (rows) memcpy(a.cfg_out, rows_.data(), sizeof(rl_tally_cfg) * rows);
        if (a.ncfg) *a.ncfg = (uint32_t)rows_.size();
        keys_.top(a.key_out, a.key_cap, &rl_tally_key::denied);
        if (a.keys_tracked) *a.keys_tracked = info_.keys_tracked;
        if (a.info) {
            if (a.info->struct_size < 8) return RL_EINVAL;
            rl_tally_info I = info_;
            I.key_slots = keys_.rows.size();
            copy_out_sized(a.info, I);
        }
        if (a.clear) {
            // the config ids seen stay known: their rows are zero
            std::fill(rows_.begin(), rows_.end(), rl_tally_cfg{});
            keys_.assign(keys_.rows.size());
            info_ = rl_tally_info{};
        }
        return RL_OK;
    }

private:
    void denied(uint64_t k, uint32_t c, uint64_t u) {
        rl_tally_key* r = k != RL_KEY_RESERVED ? keys_.find_or_claim(k, c, &info_.keys_tracked) : nullptr;
        if (r) {
            r->denied++;
            r->units_denied += u;
        } else {
            info_.untracked_requests++;
            info_.untracked_units += u;
        }
    }
    KnownCfgs known_;
    std::vector<rl_tally_cfg> rows_;
    KeyTable<rl_tally_key> keys_;
    rl_tally_info info_{};
};

// The top keys over a host backend: the sketch and candidate table of
// csrc/rl_hot.h in plain C++ -- per backend batch every counted request's adds
// (A), then the look at the batch's keys (B): estimate = the minimum of the
// key's four counters; at or above hot_min the key is looked up in the table
// and inserted when absent.
class HostHot {
public:
    int enable(const rl_hot_opts& o) {
        if (o.struct_size != sizeof(rl_hot_opts) || o.width > (1u << 24) || o.key_slots > (1u << 24) ||
            o.weight > RL_HOT_UNITS || o.hot_min < 1)
            return RL_EINVAL;
        uint64_t width = 16, slots = 16;
        while (width < (o.width ? o.width : 1u << 18)) width *= 2;
        while (slots < (o.key_slots ? o.key_slots : 65536u)) slots *= 2;
        width_ = width;
        units_ = o.weight == RL_HOT_UNITS;
        hot_min_ = o.hot_min;
        sketch_.assign(RL_HOT_DEPTH * width, 0);
        keys_.assign(slots);
        for (int r = 0; r < RL_HOT_DEPTH; r++) salt_[r] = rl::mix64((uint64_t)r + 1);
        return RL_OK;
    }
    void add(size_t m, const uint64_t* key, const uint32_t* cfg, const int64_t* n, const uint8_t* dec) {
        info_.batches++;
        info_.requests += m;
        counted_.assign(m, 0);
        for (size_t i = 0; i < m; i++) {                         // (A)
            const uint32_t c = cfg[i], d = dec[i];
            if (!known_.admit(c, d) || d > RL_ERROR || key[i] == RL_KEY_RESERVED || (units_ && n[i] <= 0)) {
                info_.skipped++;
                continue;
            }
            const uint64_t w = units_ ? (uint64_t)n[i] : 1;
            counted_[i] = 1;
            info_.total += w;
            for (int r = 0; r < RL_HOT_DEPTH; r++) sketch_[r * width_ + col(key[i], r)] += w;
        }
        for (size_t i = 0; i < m; i++)                            // (B)
            if (counted_[i] && estimate(key[i]) >= hot_min_ && !keys_.find_or_claim(key[i], cfg[i], &info_.keys_tracked))
                info_.dropped = 1;
    }
    int read(const HotArgs& a) {
        if (a.key_out && a.key_cap) {
            // a row's estimate is looked up when it is read (a free row's stays 0)
            for (rl_hot_key& r : keys_.rows)
                if (r.key_id != RL_KEY_RESERVED) r.estimate = estimate(r.key_id);
            keys_.top(a.key_out, a.key_cap, &rl_hot_key::estimate);
        }
        if (a.keys_tracked) *a.keys_tracked = info_.keys_tracked;
        if (a.info) {
            if (a.info->struct_size < 8) return RL_EINVAL;
            rl_hot_info I = info_;
            I.width = width_;
            I.depth = RL_HOT_DEPTH;
            I.key_slots = keys_.rows.size();
            I.hot_min = hot_min_;
            I.weight = units_ ? RL_HOT_UNITS : RL_HOT_REQUESTS;
            copy_out_sized(a.info, I);
        }
        if (a.clear) {
            // the config ids seen stay known
            std::fill(sketch_.begin(), sketch_.end(), 0);
            keys_.assign(keys_.rows.size());
            info_ = rl_hot_info{};
        }
        return RL_OK;
    }

private:
    uint64_t col(uint64_t k, int r) const { return rl::mix64(k ^ salt_[r]) & (width_ - 1); }
    uint64_t estimate(uint64_t k) const {
        uint64_t est = ~0ull;
        for (int r = 0; r < RL_HOT_DEPTH; r++) est = std::min(est, sketch_[r * width_ + col(k, r)]);
        return est;
    }
    KnownCfgs known_;
    std::vector<uint64_t> sketch_;
    KeyTable<rl_hot_key> keys_;
    std::vector<uint8_t> counted_;
    uint64_t salt_[RL_HOT_DEPTH] = {};
    uint64_t width_ = 0, hot_min_ = 0;
    bool units_ = false;
    rl_hot_info info_{};
};

// synchronous host functions (the CPU tests plug the oracle in here)
class FnBackend : public Backend {
public:
    explicit FnBackend(const BackendFns& b) : b_(b) {}
    int tally_enable(uint32_t key_slots) override {
        const int rc = tally_.enable(key_slots);
        tally_on_ = rc == RL_OK;
        return rc;
    }
    int tally_read(const TallyArgs& a) override { return tally_on_ ? tally_.read(a) : RL_EINVAL; }
    int hot_enable(const rl_hot_opts& o) override {
        const int rc = hot_.enable(o);
        hot_on_ = rc == RL_OK;
        return rc;
    }
    int hot_read(const HotArgs& a) override { return hot_on_ ? hot_.read(a) : RL_EINVAL; }
    int init(int nslots, size_t M, std::vector<Slot>* slots) override {
        slots->resize(nslots);
        mem_.resize(nslots);
        for (int i = 0; i < nslots; i++) {
            mem_[i].reset(new uint8_t[block_bytes(M)]);
            carve(mem_[i].get(), M, (*slots)[i]);
        }
        return RL_OK;
    }
    int launch(int, Slot& s) override {
        s.t_h2d = steady_ns();
        switch (s.op) {
            case OP_REQ: {
                const int rc = b_.batch(b_.user, s.m, s.key, s.ts, s.n, s.cfg, s.dec, s.rem, s.retry, s.reset);
                // launch() and tally_read() both run on the submitter thread
                if (rc == RL_OK && tally_on_) tally_.add(s.m, s.key, s.cfg, s.n, s.dec);
                if (rc == RL_OK && hot_on_) hot_.add(s.m, s.key, s.cfg, s.n, s.dec);
                return rc;
            }
            case OP_PEEK:
                return b_.peek ? b_.peek(b_.user, s.m, s.key, s.ts, s.n, s.cfg, s.dec, s.rem, s.retry, s.reset) : RL_EINVAL;
            case OP_REFUND: return b_.refund ? b_.refund(b_.user, s.m, s.key, s.ts, s.n, s.cfg, s.dec) : RL_EINVAL;
            case OP_ALLOW_ALL: {
                if (!b_.allow_all) return RL_EINVAL;
                const int rc = b_.allow_all(b_.user, s.m, s.key, s.ts, s.n, s.cfg, s.head, s.dec, s.rem, s.retry, s.reset,
                                            s.verdict);
                if (rc == RL_OK && tally_on_) tally_.add(s.m, s.key, s.cfg, s.n, s.dec);
                if (rc == RL_OK && hot_on_) hot_.add(s.m, s.key, s.cfg, s.n, s.dec);
                return rc;
            }
            case OP_CHARGE: {
                if (!b_.charge) return RL_EINVAL;
                const int rc = b_.charge(b_.user, s.m, s.key, s.ts, s.n, s.cfg, s.dec, s.retry, s.rem, s.reset);
                if (rc == RL_OK && tally_on_) tally_.add(s.m, s.key, s.cfg, s.n, s.dec);
                if (rc == RL_OK && hot_on_) hot_.add(s.m, s.key, s.cfg, s.n, s.dec);
                return rc;
            }
            case OP_RESET: return reset_batch(s);
            default: return RL_EINVAL;
        }
    }
    int wait(int, Slot&) override { return RL_OK; }
    int table_info(int64_t now_ms, rl_table_info* out) override {
        return b_.table_info ? b_.table_info(b_.user, now_ms, out) : RL_EINVAL;
    }
    int gc(int64_t now_ms, uint64_t tb_cap, uint64_t win_cap, rl_table_info* out) override {
        return b_.gc ? b_.gc(b_.user, now_ms, tb_cap, win_cap, out) : RL_EINVAL;
    }

private:
    int reset_batch(Slot& s) {
        if (b_.reset_batch) return b_.reset_batch(b_.user, s.m, s.key, s.ts, s.cfg, s.dec);
        if (!b_.reset) return RL_EINVAL;
        // a backend without reset_batch: one reset call per key, in order; its
        // RL_EINVAL (unknown config, reserved key) is that request's status
        for (size_t i = 0; i < s.m; i++) {
            const int rc = b_.reset(b_.user, s.cfg[i], s.key[i], s.ts[i]);
            if (rc != RL_OK && rc != RL_EINVAL) return rc;
            s.dec[i] = rc == RL_OK ? RL_RESET_DONE : RL_INVALID;
        }
        return RL_OK;
    }
    BackendFns b_;
    HostTally tally_;
    bool tally_on_ = false;
    HostHot hot_;
    bool hot_on_ = false;
    std::vector<std::unique_ptr<uint8_t[]>> mem_;
};

std::unique_ptr<Backend> make_gpu_backend(rl_engine* e) { return std::unique_ptr<Backend>(new GpuBackend(e)); }
std::unique_ptr<Backend> make_fn_backend(const BackendFns& b) {
    return std::unique_ptr<Backend>(new FnBackend(b));
}

// ---------------------------------------------------------------------------


Coalescer::Coalescer(std::unique_ptr<Backend> be, const rl_coalescer_opts& o) : be_(std::move(be)), o_(o) {
    if (o_.max_batch == 0) o_.max_batch = 65536;
    if (o_.max_in_flight == 0) o_.max_in_flight = 3;
    if (o_.max_in_flight > 3) o_.max_in_flight = 3;
    if (o_.queue_cap == 0) o_.queue_cap = 1ull << 24;
    if (o_.linger_ns < 0) o_.linger_ns = 0;
    if (o_.gc_high_pct == 0 || o_.gc_high_pct > 95) o_.gc_high_pct = 50;
    if (o_.gc_margin_ms <= 0) o_.gc_margin_ms = 1000;
    if (o_.gc_interval_ns < 0) o_.gc_interval_ns = 0;
    if (const char* v = getenv("RL_COALESCER_TRACE")) trace_cap_ = (size_t)strtoull(v, nullptr, 10);
    st_.struct_size = sizeof(rl_coalescer_stats);
}

int Coalescer::start() {
    int rc = be_->init((int)o_.max_in_flight, o_.max_batch, &slots_);
    if (rc != RL_OK) return rc;
    if (o_.tally_key_slots) {
        rc = be_->tally_enable(o_.tally_key_slots);
        if (rc != RL_OK) return rc;
    }
    if (o_.hot_min) {
        rl_hot_opts h{sizeof(rl_hot_opts), o_.hot_width, o_.hot_key_slots, o_.hot_weight, o_.hot_min};
        rc = be_->hot_enable(h);
        if (rc != RL_OK) return rc;
    }
    t_sub_ = std::thread([this] { submitter(); });
    t_done_ = std::thread([this] { completer(); });
    return RL_OK;
}

Coalescer::~Coalescer() {
    Shutdown();
    for (auto& kv : subs_) delete kv.second;
    for (Sub* s : pool_) delete s;
}

void Coalescer::Shutdown() {
    {
        std::lock_guard<std::mutex> g(mu_);
        if (stop_) return;
        stop_ = true;
    }
    cv_sub_.notify_all();
    cv_done_.notify_all();
    if (t_sub_.joinable()) t_sub_.join();
    if (t_done_.joinable()) t_done_.join();
    // anything never launched (backend failure) is released as closed
    std::lock_guard<std::mutex> g(mu_);
    for (auto& kv : subs_) {
        Sub* s = kv.second;
        if (!s->done) {
            s->done = true;
            s->status = RL_ECLOSED;
            s->cv.notify_all();
            notify_locked(s);
        }
    }
}

void Coalescer::SetNotify(NotifyFn fn, void* user) {
    std::lock_guard<std::mutex> g(mu_);
    notify_ = fn;
    notify_user_ = user;
}

int Coalescer::Submit(size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n, const uint32_t* cfg,
                      uint64_t* ticket, int64_t deadline, void* tag, Op op, const uint8_t* first) {
    if (op >= OP_COUNT || !OPS[op].batched) return RL_EINVAL;
    const OpTraits& t = OPS[op];
    if (!ticket || (m && (!key || !ts || !cfg || (!n && t.reads_n) || (!first && t.grouped))) || deadline < 0)
        return RL_EINVAL;
    // a submission that is not split is one launch (a refund: the engine's sum rule)
    if (!t.splits && m > o_.max_batch) return RL_EINVAL;
    Sub* s = get_sub(m);
    s->op = op;
    s->deadline = deadline;
    s->tag = tag;
    if (trace_cap_) s->submit_ns = steady_ns();
    memcpy(s->key, key, 8 * m);
    memcpy(s->ts, ts, 8 * m);
    if (n) memcpy(s->n, n, 8 * m);
    memcpy(s->cfg, cfg, 4 * m);
    if (t.grouped) memcpy(s->head, first, m);
    return enqueue(s, m, ticket);
}

int Coalescer::SubmitOp(Op op, const OpArgs& a, uint64_t* ticket, void* tag) {
    if (op >= OP_COUNT || OPS[op].batched || !ticket) return RL_EINVAL;
    Sub* s = get_sub(1);
    s->op = op;
    s->tag = tag;
    s->args = a;
    if (trace_cap_) s->submit_ns = steady_ns();
    return enqueue(s, 1, ticket);
}

int Coalescer::enqueue(Sub* s, size_t m, uint64_t* ticket) {
    {
        std::lock_guard<std::mutex> g(mu_);
        if (stop_ || (pending_ + m > o_.queue_cap && OPS[s->op].queue_cap)) {
            const int rc = stop_ ? RL_ECLOSED : RL_EAGAIN;
            put_sub(s);
            return rc;
        }
        s->first = next_seq_;
        // an empty submission is done at once; its ticket must still be unique
        next_seq_ += m ? m : 1;
        subs_[s->first] = s;
        if (OPS[s->op].decides) st_.submitted += m;
        if (m) {
            queue_.push_back(s);
            s->in_queue = true;
            pending_ += m;
        } else {
            finish_locked(s, steady_ns());
        }
        *ticket = s->first;
        // wake the submitter only when it sleeps: at millions of submissions
        // per second an unconditional notify is a futex call per submission
        if (!m || !sub_idle_) return RL_OK;
    }
    cv_sub_.notify_one();
    return RL_OK;
}

void Coalescer::end_unlaunched_locked(Sub* s, int code) {
    const size_t rest = s->m - s->taken;
    if (rest == 0) return;
    pending_ -= rest;
    if (OPS[s->op].decides) (code == RL_ECANCELED ? st_.cancelled : st_.expired) += rest;
    // the outcome is the context's error, whoever completes it: the results
    // of a launched part are discarded and the rest never ran (its result
    // arrays hold whatever a pooled Sub held before)
    s->status = code;
    if (s->taken == 0) {
        s->dropped = true;
    } else {
        s->truncated = true;
        s->taken = s->m;
    }
    s->left -= rest;
    if (s->left == 0 && !s->done) finish_locked(s, steady_ns());
}

void Coalescer::maybe_free_locked(Sub* s) {
    if (s->waited && !s->in_queue && s->inflight == 0) put_sub(s);
}

int Coalescer::Cancel(uint64_t ticket) {
    std::lock_guard<std::mutex> g(mu_);
    auto it = subs_.find(ticket);
    if (it == subs_.end()) return RL_EINVAL;
    Sub* s = it->second;
    if (s->done) return RL_OK;
    s->cancelled = true;
    end_unlaunched_locked(s, RL_ECANCELED);
    if (s->waiting) s->cv.notify_all();   // a waiter whose launched part is still out sees `cancelled`
    return RL_OK;
}

int Coalescer::Wait(uint64_t ticket, int64_t timeout_ns, uint8_t* dec, int64_t* rem, int64_t* retry,
                    int64_t* reset, int64_t* done_ns, rl_table_info* info, uint8_t* verdict) {
    std::unique_lock<std::mutex> lk(mu_);
    auto it = subs_.find(ticket);
    if (it == subs_.end()) return RL_EINVAL;
    Sub* s = it->second;
    const int64_t t_end = timeout_ns < 0 ? INT64_MAX : steady_ns() + timeout_ns;
    int code = RL_OK;   // != RL_OK: the ticket ends without results
    for (;;) {
        if (s->cancelled) { code = RL_ECANCELED; break; }
        if (s->done) {
            if (s->dropped || s->truncated) code = s->status;
            break;
        }
        const int64_t now = steady_ns();
        if (s->deadline && now >= s->deadline) {
            // not launched: never applied; launched: applied, results discarded,
            // and what was not launched yet never will be
            end_unlaunched_locked(s, RL_EDEADLINE);
            code = RL_EDEADLINE;
            break;
        }
        if (now >= t_end) {
            s->waiting = false;
            return RL_ETIMEOUT;
        }
        s->waiting = true;
        const int64_t until = s->deadline ? std::min(t_end, s->deadline) : t_end;
        if (until == INT64_MAX) s->cv.wait(lk);
        else s->cv.wait_for(lk, std::chrono::nanoseconds(until - now));
    }
    s->waiting = false;
    subs_.erase(it);
    if (code != RL_OK) {
        if (done_ns) *done_ns = steady_ns();
        s->waited = true;
        maybe_free_locked(s);
        return code;
    }
    // done and applied: no slot or queue references it any more
    lk.unlock();
    const size_t m = s->m;
    if (OPS[s->op].batched) {
        if (dec) memcpy(dec, s->dec, m);   // the decision, or the per-request status
    }
    if (OPS[s->op].results) {
        if (rem) memcpy(rem, s->rem, 8 * m);
        if (retry) memcpy(retry, s->retry, 8 * m);
        if (reset) memcpy(reset, s->reset, 8 * m);
    }
    if (OPS[s->op].grouped && verdict) memcpy(verdict, s->verdict, m);
    if (info) *info = s->info;
    if (done_ns) *done_ns = s->done_ns;
    int st = s->status;
    put_sub(s);
    return st;
}

Sub* Coalescer::get_sub(size_t m) {
    {
        std::lock_guard<std::mutex> g(pool_mu_);
        for (size_t i = pool_.size(); i-- > 0;) {
            Sub* s = pool_[i];
            if (s->cap >= m && s->cap <= 4 * m + 4096) {   // fits, and not far too big
                pool_[i] = pool_.back();
                pool_.pop_back();
                s->renew(m);
                return s;
            }
        }
    }
    return new Sub(m);
}

void Coalescer::put_sub(Sub* s) {
    {
        std::lock_guard<std::mutex> g(pool_mu_);
        if (pool_.size() < 256 && s->cap <= (1u << 20)) {
            pool_.push_back(s);
            return;
        }
    }
    delete s;
}

std::vector<BatchTrace> Coalescer::Trace() {
    std::lock_guard<std::mutex> g(mu_);
    std::vector<BatchTrace> out;
    if (trace_cap_ == 0 || trace_.size() < trace_cap_) return trace_;
    const size_t h = done_batches_ % trace_cap_;
    out.insert(out.end(), trace_.begin() + h, trace_.end());
    out.insert(out.end(), trace_.begin(), trace_.begin() + h);
    return out;
}

Counters Coalescer::Stats() {
    std::lock_guard<std::mutex> g(mu_);
    Counters r = st_;
    r.pending = pending_;
    return r;
}

int Coalescer::run_table_op(Sub* op) {
    const OpArgs& a = op->args;
    rl_table_info info{};
    info.struct_size = sizeof info;
    int st;
    switch (op->op) {
        case OP_INFO: st = be_->table_info(a.now_ms, &info); break;
        // every batch before it is launched, its tally enqueued behind it
        case OP_TALLY: st = be_->tally_read(a.tally); break;
        case OP_HOT: st = be_->hot_read(a.hot); break;
        case OP_SNAPSHOT:
            st = be_->snapshot(a.now_ms, a.snap.world, a.snap.rank, a.snap.buf, a.snap.len, a.snap.out);
            break;
        default: {   // OP_GC, OP_RESTORE: a restore is a GC that also merges a snapshot
            st = op->op == OP_RESTORE ? be_->restore(a.snap.buf, a.snap.len, a.now_ms, a.cap_tb, a.cap_win, &info)
                                      : be_->gc(a.now_ms, a.cap_tb, a.cap_win, &info);
            std::lock_guard<std::mutex> g(mu_);
            st_.gc_runs++;
            if (st != RL_OK) st_.gc_failures++;
        }
    }
    op->info = info;
    return st;
}

// Automatic GC (include/rl_coalescer.h, rl_coalescer_opts.gc_*): every request
// inserts at most one entry into one table (a window request may also move one
// window key to the spill table), so after a count with `budget` free slots
// below the high-water mark of the fullest table, that many requests cannot
// push any table past it.  Runs before launching `s`, so a GC lands between
// the batches launched before and `s`.
void Coalescer::auto_gc(const Slot& s) {
    if (o_.gc_interval_ns <= 0 || s.m == 0) return;
    const int64_t now = steady_ns();
    // the batch's requests per table: a token-bucket request can insert one
    // entry into the token-bucket table, a window request one into the window
    // table and one into the spill table; a request of an unknown config counts
    // for both
    uint64_t mt[2] = {0, 0};
    for (size_t i = 0; i < s.m; i++) {
        const int t = be_->table_of(s.cfg[i]);
        if (t != 1) mt[0]++;
        if (t != 0) mt[1]++;
    }
    if (gc_counted_ && gc_launched_[0] + mt[0] <= gc_budget_[0] && gc_launched_[1] + mt[1] <= gc_budget_[1] &&
        now - gc_last_check_ < o_.gc_interval_ns) {
        gc_launched_[0] += mt[0];
        gc_launched_[1] += mt[1];
        return;
    }
    // server clock of the GC: no later request may carry an older one (the
    // engine's clock is floor(ts / 1e6)); requests come in near time order,
    // within gc_margin_ms of each other
    int64_t min_ts = INT64_MAX;
    for (size_t i = 0; i < s.m; i++) min_ts = std::min(min_ts, s.ts[i]);
    const int64_t now_ms = (min_ts >= 0 ? min_ts / 1000000 : -((-min_ts + 999999) / 1000000)) - o_.gc_margin_ms;
    rl_table_info in{};
    in.struct_size = sizeof in;
    if (be_->table_info(now_ms, &in) != RL_OK) {
        gc_counted_ = true;
        gc_budget_[0] = gc_budget_[1] = 0;
        gc_last_check_ = now;
        gc_launched_[0] = mt[0];
        gc_launched_[1] = mt[1];
        return;
    }
    const double hi = o_.gc_high_pct / 100.0;
    auto high = [&](uint64_t cap) { return (uint64_t)(hi * (double)cap); };
    auto full = [&](uint64_t used, uint64_t cap, uint64_t m) { return used + m > high(cap); };
    {
        std::lock_guard<std::mutex> g(mu_);
        st_.gc_checks++;
    }
    if (full(in.tb_used, in.tb_capacity, mt[0]) || full(in.win_used, in.win_capacity, mt[1]) ||
        full(in.spill_used, in.spill_capacity, mt[1])) {
        // grow a table whose live keys alone fill half its headroom
        auto grow = [&](uint64_t live, uint64_t cap, uint64_t lim) -> uint64_t {
            if (live <= high(cap) / 2) return 0;
            if (lim && 2 * cap > lim) return 0;
            return 2 * cap;
        };
        const uint64_t ntb = grow(in.tb_live, in.tb_capacity, o_.gc_max_tb_capacity);
        uint64_t nwin = grow(in.win_live, in.win_capacity, o_.gc_max_win_capacity);
        if (!nwin && in.spill_live > high(in.spill_capacity) / 2 &&
            !(o_.gc_max_win_capacity && 2 * in.win_capacity > o_.gc_max_win_capacity))
            nwin = 2 * in.win_capacity;   // the spill table follows the window table
        rl_table_info out{};
        out.struct_size = sizeof out;
        int st = be_->gc(now_ms, ntb, nwin, &out);
        bool ok = st == RL_OK;
        if (!ok && (ntb || nwin)) ok = be_->gc(now_ms, 0, 0, &out) == RL_OK;   // no room to grow: in place
        {
            std::lock_guard<std::mutex> g(mu_);
            st_.gc_runs++;
            if (!ok) st_.gc_failures++;
        }
        if (ok) in = out;
    }
    auto room = [&](uint64_t used, uint64_t cap) -> uint64_t { return used < high(cap) ? high(cap) - used : 0; };
    gc_budget_[0] = room(in.tb_used, in.tb_capacity);
    gc_budget_[1] = std::min(room(in.win_used, in.win_capacity), room(in.spill_used, in.spill_capacity));
    gc_counted_ = true;
    gc_last_check_ = now;
    gc_launched_[0] = mt[0];      // this batch launches after the count
    gc_launched_[1] = mt[1];
}

void Coalescer::submitter() {
    for (;;) {
        std::unique_lock<std::mutex> lk(mu_);
        sub_idle_ = true;
        cv_sub_.wait(lk, [&] { return (stop_ && pending_ == 0) || (pending_ > 0 && inflight_ < (int)o_.max_in_flight); });
        sub_idle_ = false;
        if (pending_ == 0) break;   // stop_ with nothing left
        // submissions dropped while queued (deadline, cancel) leave the queue here
        auto pop_dropped = [&] {
            while (!queue_.empty() && queue_.front()->dropped) maybe_free_locked(pop_front_locked());
        };
        pop_dropped();
        if (o_.linger_ns > 0 && inflight_ == 0 && pending_ < o_.max_batch && !stop_ && OPS[queue_.front()->op].decides) {
            const auto until = std::chrono::steady_clock::now() + std::chrono::nanoseconds(o_.linger_ns);
            sub_idle_ = true;
            cv_sub_.wait_until(lk, until, [&] { return stop_ || pending_ >= o_.max_batch; });
            sub_idle_ = false;
            pop_dropped();
            if (pending_ == 0) continue;
        }
        Sub* f = queue_.front();
        const OpTraits& t = OPS[f->op];
        if (!t.batched) {
            // a table operation: synchronous, on this thread: every batch
            // before it is launched and the backend drains them; nothing after
            // it is launched yet
            pop_front_locked();
            pending_ -= 1;
            f->taken = 1;
            lk.unlock();
            const int st = run_table_op(f);
            lk.lock();
            f->status = st;
            f->left = 0;
            finish_locked(f, steady_ns());
            maybe_free_locked(f);
            // a manual GC invalidates the automatic GC's count
            if (!t.keeps_gc_count) gc_counted_ = false;
            continue;
        }
        const int si = next_slot_;
        Slot& s = slots_[si];
        s.parts.clear();
        s.op = f->op;
        size_t m = 0;
        const int64_t now = steady_ns();
        while (m < o_.max_batch && !queue_.empty()) {
            Sub* sub = queue_.front();
            if (sub->dropped) {
                maybe_free_locked(pop_front_locked());
                continue;
            }
            // requests merge, and so do resets: the run of adjacent ones at
            // the queue head is one launch, enqueued between the batches
            // around it; a peek submission is launched on its own, and so is
            // a refund submission (one engine call: the engine sums the
            // refunds of a call per target) and an AllowAll submission (its
            // groups' transient takes must not depend on the queue's timing)
            if (sub->op != f->op || (!t.merges && sub != f)) break;
            // its context ended before (the rest of) it was sent: that part is never applied
            if (sub->taken < sub->m && (sub->cancelled || (sub->deadline && sub->deadline <= now)))
                end_unlaunched_locked(sub, sub->cancelled ? RL_ECANCELED : RL_EDEADLINE);
            if (sub->dropped || sub->taken == sub->m) {
                // dropped, or the rest of a split submission truncated: nothing left to launch
                maybe_free_locked(pop_front_locked());
                continue;
            }
            const size_t take = std::min(sub->m - sub->taken, (size_t)o_.max_batch - m);
            s.parts.push_back({sub, sub->taken, take, m});
            sub->taken += take;
            sub->inflight++;
            m += take;
            if (sub->taken == sub->m) pop_front_locked();
        }
        if (m == 0) continue;   // everything at the head was dropped
        pending_ -= m;
        next_slot_ = (next_slot_ + 1) % (int)o_.max_in_flight;
        inflight_++;
        lk.unlock();
        if (trace_cap_) s.t_form = steady_ns();
        // the submissions' inputs are immutable after Submit: copy unlocked
        for (const auto& p : s.parts) {
            memcpy(s.key + p.at, p.sub->key + p.off, 8 * p.count);
            memcpy(s.ts + p.at, p.sub->ts + p.off, 8 * p.count);
            if (t.reads_n) memcpy(s.n + p.at, p.sub->n + p.off, 8 * p.count);
            memcpy(s.cfg + p.at, p.sub->cfg + p.off, 4 * p.count);
            if (t.grouped) memcpy(s.head + p.at, p.sub->head + p.off, p.count);
        }
        s.m = m;
        // only a decision inserts: the others have no part in the automatic GC's budgets
        if (t.decides) auto_gc(s);
        s.status = be_->launch(si, s);
        if (trace_cap_) s.t_launched = steady_ns();
        lk.lock();
        if (t.counts_batch) st_.batches++;   // a reset launch too, though it is no request batch: max_batch_seen stays
        if (t.counts_max) st_.max_batch_seen = std::max<uint64_t>(st_.max_batch_seen, m);
        if (t.launches) (st_.*t.launches)++;
        launched_.push_back(si);
        lk.unlock();
        cv_done_.notify_one();
    }
    std::lock_guard<std::mutex> g(mu_);
    // only dropped submissions can be left in the queue
    while (!queue_.empty()) maybe_free_locked(pop_front_locked());
    sub_exited_ = true;
    cv_done_.notify_all();
}

void Coalescer::completer() {
    for (;;) {
        int si;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_done_.wait(lk, [&] { return !launched_.empty() || sub_exited_; });
            if (launched_.empty()) break;
            si = launched_.front();
        }
        Slot& s = slots_[si];
        const OpTraits& t = OPS[s.op];
        const int64_t t_wait = trace_cap_ ? steady_ns() : 0;
        int st = s.status == RL_OK ? be_->wait(si, s) : s.status;
        uint64_t completed = s.m;
        if (t.results) {
            for (const auto& p : s.parts) {
                memcpy(p.sub->dec + p.off, s.dec + p.at, p.count);
                memcpy(p.sub->rem + p.off, s.rem + p.at, 8 * p.count);
                memcpy(p.sub->retry + p.off, s.retry + p.at, 8 * p.count);
                memcpy(p.sub->reset + p.off, s.reset + p.at, 8 * p.count);
                if (t.grouped) memcpy(p.sub->verdict + p.off, s.verdict + p.at, p.count);
            }
        } else {
            // a status: meaningful only when the launch succeeded; RL_RESET_DONE
            // and RL_REFUND_DONE are the same code
            completed = 0;
            if (st == RL_OK) {
                for (const auto& p : s.parts) memcpy(p.sub->dec + p.off, s.dec + p.at, p.count);
                for (size_t i = 0; i < s.m; i++) completed += s.dec[i] == RL_RESET_DONE;
            }
        }
        // the groups of a launch that ran: never merged, so member 0 starts one
        uint64_t groups = 0;
        if (t.grouped && st == RL_OK)
            for (size_t i = 0; i < s.m; i++) groups += i == 0 || s.head[i] != 0;
        const int64_t now = steady_ns();
        bool wake;
        {
            std::lock_guard<std::mutex> g(mu_);
            wake = sub_idle_;
            st_.allow_all_groups += groups;
            launched_.pop_front();
            inflight_--;
            if (trace_cap_) {
                BatchTrace bt{done_batches_, s.m, 0, s.t_form, s.t_h2d, s.t_launched, t_wait, now};
                bt.t_submit = s.parts.empty() ? s.t_form : s.parts[0].sub->submit_ns;   // the oldest request
                if (trace_.size() < trace_cap_) trace_.push_back(bt);
                else trace_[done_batches_ % trace_cap_] = bt;
            }
            done_batches_++;
            st_.*t.completed += completed;
            for (const auto& p : s.parts) {
                Sub* sub = p.sub;
                if (st != RL_OK && !sub->truncated) sub->status = st;
                sub->left -= p.count;
                sub->inflight--;
                if (sub->left == 0 && !sub->done) finish_locked(sub, now);
                maybe_free_locked(sub);   // orphaned (its waiter gave up) and now complete
            }
        }
        if (wake) cv_sub_.notify_one();
    }
}

}  // namespace rlc

// ---------------------------------------------------------------------------
// C-ABI
// ---------------------------------------------------------------------------

struct rl_coalescer {
    rlc::Coalescer* c;
};

rlc::Coalescer* rlc::unwrap(rl_coalescer* c) { return c ? c->c : nullptr; }

static int create(std::unique_ptr<rlc::Backend> be, const rl_coalescer_opts* opts, rl_coalescer** out) {
    if (!out) return RL_EINVAL;
    rl_coalescer_opts o{};
    o.struct_size = sizeof o;
    if (opts) {
        // a caller compiled before a trailing field was added passes a shorter
        // struct: any size from the first such field's offset up to ours (what
        // it does not cover stays 0, off)
        if (opts->struct_size < offsetof(rl_coalescer_opts, tally_key_slots) ||
            opts->struct_size > sizeof(rl_coalescer_opts))
            return RL_EINVAL;
        memcpy(&o, opts, opts->struct_size);
        o.struct_size = sizeof o;
        // the top keys' options count only from a struct that holds all four
        if (opts->struct_size < sizeof(rl_coalescer_opts)) o.hot_width = o.hot_key_slots = o.hot_weight = 0, o.hot_min = 0;
    }
    auto* c = new rlc::Coalescer(std::move(be), o);
    int rc = c->start();
    if (rc != RL_OK) {
        delete c;
        return rc;
    }
    *out = new rl_coalescer{c};
    return RL_OK;
}

extern "C" int rl_coalescer_create(rl_engine* e, const rl_coalescer_opts* opts, rl_coalescer** out) {
    if (!e || !out) return RL_EINVAL;
    return create(rlc::make_gpu_backend(e), opts, out);
}

extern "C" int rl_coalescer_create_with_host_backend(const rl_coalescer_backend* be, const rl_coalescer_opts* opts,
                                                     rl_coalescer** out) {
    // a caller compiled before `peek` / `reset_batch` / `refund` / `allow_all` / `charge` were added passes the
    // shorter struct; one with `charge` passes rl_coalescer_backend_charge's size
    if (!be || !out ||
        (be->struct_size != sizeof(rl_coalescer_backend_charge) && be->struct_size != sizeof(rl_coalescer_backend) && be->struct_size != offsetof(rl_coalescer_backend, peek) &&
         be->struct_size != offsetof(rl_coalescer_backend, reset_batch) &&
         be->struct_size != offsetof(rl_coalescer_backend, refund) &&
         be->struct_size != offsetof(rl_coalescer_backend, allow_all)))
        return RL_EINVAL;
    rlc::BackendFns b{};
    memcpy(static_cast<rl_coalescer_backend*>(&b), be, std::min<size_t>(be->struct_size, sizeof(rl_coalescer_backend)));
    if (be->struct_size == sizeof(rl_coalescer_backend_charge))
        b.charge = reinterpret_cast<const rl_coalescer_backend_charge*>(be)->charge;
    b.struct_size = sizeof b;
    if (!b.batch) return RL_EINVAL;
    return create(rlc::make_fn_backend(b), opts, out);
}

extern "C" int rl_coalescer_create_with_backend(rl_batch_fn fn, void* user, const rl_coalescer_opts* opts,
                                                rl_coalescer** out) {
    return rl_coalescer_create_with_backends(fn, nullptr, user, opts, out);
}

extern "C" int rl_coalescer_create_with_backends(rl_batch_fn fn, rl_reset_fn reset_fn, void* user,
                                                 const rl_coalescer_opts* opts, rl_coalescer** out) {
    rl_coalescer_backend b{sizeof(rl_coalescer_backend), fn, reset_fn, nullptr, nullptr, user, nullptr, nullptr, nullptr,
                           nullptr};
    return rl_coalescer_create_with_host_backend(&b, opts, out);
}

extern "C" int rl_coalescer_destroy(rl_coalescer* c) {
    if (!c) return RL_EINVAL;
    delete c->c;
    delete c;
    return RL_OK;
}

extern "C" int64_t rl_coalescer_now_ns(void) { return rlc::steady_ns(); }

extern "C" int rl_coalescer_submit(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                   const int64_t* n, const uint32_t* cfg_id, uint64_t* ticket) {
    if (!c) return RL_EINVAL;
    return c->c->Submit(m, key_id, ts_ns, n, cfg_id, ticket);
}

extern "C" int rl_coalescer_submit_deadline(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                            const int64_t* n, const uint32_t* cfg_id, int64_t deadline_ns,
                                            uint64_t* ticket) {
    if (!c) return RL_EINVAL;
    return c->c->Submit(m, key_id, ts_ns, n, cfg_id, ticket, deadline_ns);
}

extern "C" int rl_coalescer_cancel(rl_coalescer* c, uint64_t ticket) {
    if (!c) return RL_EINVAL;
    return c->c->Cancel(ticket);
}

extern "C" int rl_coalescer_wait(rl_coalescer* c, uint64_t ticket, int64_t timeout_ns, uint8_t* decision,
                                 int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns) {
    if (!c) return RL_EINVAL;
    return c->c->Wait(ticket, timeout_ns, decision, remaining, retry_after_ns, reset_at_ns);
}

extern "C" int rl_coalescer_decide(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, int64_t n, uint32_t cfg_id,
                                   uint8_t* decision, int64_t* remaining, int64_t* retry_after_ns,
                                   int64_t* reset_at_ns) {
    return rl_coalescer_decide_deadline(c, key_id, ts_ns, n, cfg_id, 0, decision, remaining, retry_after_ns,
                                        reset_at_ns);
}

extern "C" int rl_coalescer_decide_deadline(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, int64_t n,
                                            uint32_t cfg_id, int64_t deadline_ns, uint8_t* decision,
                                            int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns) {
    if (!c) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(1, &key_id, &ts_ns, &n, &cfg_id, &t, deadline_ns);
    if (rc != RL_OK) return rc;
    return c->c->Wait(t, -1, decision, remaining, retry_after_ns, reset_at_ns);
}

extern "C" int rl_coalescer_reset(rl_coalescer* c, uint64_t key_id, int64_t ts_ns, uint32_t cfg_id) {
    if (!c) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(1, &key_id, &ts_ns, nullptr, &cfg_id, &t, 0, nullptr, rlc::OP_RESET);
    if (rc != RL_OK) return rc;
    // merged with the resets queued next to it: its own status tells whether it ran
    uint8_t status = RL_RESET_DONE;
    rc = c->c->Wait(t, -1, &status, nullptr, nullptr, nullptr);
    return rc == RL_OK && status != RL_RESET_DONE ? RL_EINVAL : rc;
}

extern "C" int rl_coalescer_reset_batch(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                        const uint32_t* cfg_id, uint8_t* status) {
    if (!c) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(m, key_id, ts_ns, nullptr, cfg_id, &t, 0, nullptr, rlc::OP_RESET);
    if (rc != RL_OK) return rc;
    return c->c->Wait(t, -1, status, nullptr, nullptr, nullptr);
}

extern "C" int rl_coalescer_refund(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                   const int64_t* n, const uint32_t* cfg_id, uint8_t* status) {
    if (!c) return RL_EINVAL;
    // one submission is one launch: a larger one is not split (the sum rule)
    if (m > c->c->MaxBatch()) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(m, key_id, ts_ns, n, cfg_id, &t, 0, nullptr, rlc::OP_REFUND);
    if (rc != RL_OK) return rc;
    return c->c->Wait(t, -1, status, nullptr, nullptr, nullptr);
}

extern "C" int rl_coalescer_allow_all(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                      const int64_t* n, const uint32_t* cfg_id, const uint8_t* first,
                                      int64_t deadline_ns, uint8_t* decision, int64_t* remaining,
                                      int64_t* retry_after_ns, int64_t* reset_at_ns, uint8_t* verdict) {
    if (!c) return RL_EINVAL;
    // one submission is one launch: a larger one is not split (the refund's sum rule)
    if (m > c->c->MaxBatch()) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(m, key_id, ts_ns, n, cfg_id, &t, deadline_ns, nullptr, rlc::OP_ALLOW_ALL, first);
    if (rc != RL_OK) return rc;
    return c->c->Wait(t, -1, decision, remaining, retry_after_ns, reset_at_ns, nullptr, nullptr, verdict);
}

extern "C" int rl_coalescer_charge(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                   const int64_t* n, const uint32_t* cfg_id, int64_t deadline_ns, uint8_t* decision,
                                   int64_t* charged, int64_t* remaining, int64_t* reset_at_ns) {
    if (!c) return RL_EINVAL;
    // one submission is one launch: a larger one is not split (its duplicates would ask against another state)
    if (m > c->c->MaxBatch()) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(m, key_id, ts_ns, n, cfg_id, &t, deadline_ns, nullptr, rlc::OP_CHARGE);
    if (rc != RL_OK) return rc;
    // `charged` travels where a decide's retry_after_ns does
    return c->c->Wait(t, -1, decision, remaining, charged, reset_at_ns);
}

extern "C" int rl_coalescer_peek(rl_coalescer* c, size_t m, const uint64_t* key_id, const int64_t* ts_ns,
                                 const int64_t* n, const uint32_t* cfg_id, uint8_t* decision, int64_t* remaining,
                                 int64_t* retry_after_ns, int64_t* reset_at_ns) {
    if (!c) return RL_EINVAL;
    uint64_t t;
    int rc = c->c->Submit(m, key_id, ts_ns, n, cfg_id, &t, 0, nullptr, rlc::OP_PEEK);
    if (rc != RL_OK) return rc;
    return c->c->Wait(t, -1, decision, remaining, retry_after_ns, reset_at_ns);
}

static int table_op(rl_coalescer* c, rlc::Op op, const rlc::OpArgs& a, rl_table_info* out = nullptr) {
    uint64_t t;
    int rc = c->c->SubmitOp(op, a, &t);
    if (rc != RL_OK) return rc;
    rl_table_info info{};
    rc = c->c->Wait(t, -1, nullptr, nullptr, nullptr, nullptr, nullptr, &info);
    if (out && rc == RL_OK) rlc::copy_out_sized(out, info);
    return rc;
}

extern "C" int rl_coalescer_table_info(rl_coalescer* c, int64_t now_ms, rl_table_info* out) {
    if (!c || !out || out->struct_size < 8) return RL_EINVAL;
    rlc::OpArgs a;
    a.now_ms = now_ms;
    return table_op(c, rlc::OP_INFO, a, out);
}

extern "C" int rl_coalescer_gc(rl_coalescer* c, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity,
                               rl_table_info* out) {
    if (!c || (out && out->struct_size < 8)) return RL_EINVAL;
    rlc::OpArgs a;
    a.now_ms = now_ms;
    a.cap_tb = tb_capacity;
    a.cap_win = win_capacity;
    return table_op(c, rlc::OP_GC, a, out);
}

extern "C" int rl_coalescer_snapshot(rl_coalescer* c, int64_t now_ms, uint32_t world, uint32_t rank, void* buf,
                                     size_t cap, rl_snapshot_info* out) {
    if (!c || !out || out->struct_size < 8) return RL_EINVAL;
    rlc::OpArgs a;
    a.now_ms = now_ms;
    a.snap = {buf, cap, world, rank, out};
    return table_op(c, rlc::OP_SNAPSHOT, a);
}

extern "C" int rl_coalescer_restore(rl_coalescer* c, const void* buf, size_t len, int64_t now_ms,
                                    uint64_t tb_capacity, uint64_t win_capacity, rl_table_info* out) {
    if (!c || (out && out->struct_size < 8)) return RL_EINVAL;
    rlc::OpArgs a;
    a.now_ms = now_ms;
    a.cap_tb = tb_capacity;
    a.cap_win = win_capacity;
    a.snap.buf = const_cast<void*>(buf);
    a.snap.len = len;
    return table_op(c, rlc::OP_RESTORE, a, out);
}

extern "C" int rl_coalescer_tally(rl_coalescer* c, rl_tally_cfg* cfg_out, size_t cfg_cap, uint32_t* ncfg,
                                  rl_tally_key* key_out, size_t key_cap, uint64_t* keys_tracked, rl_tally_info* info,
                                  int clear) {
    if (!c || !c->c->TallyOn() || (info && info->struct_size < 8)) return RL_EINVAL;
    rlc::OpArgs a;
    a.tally = {cfg_out, cfg_cap, ncfg, key_out, key_cap, keys_tracked, info, clear};
    return table_op(c, rlc::OP_TALLY, a);
}

extern "C" int rl_coalescer_hot(rl_coalescer* c, rl_hot_key* key_out, size_t key_cap, uint64_t* keys_tracked,
                                rl_hot_info* info, int clear) {
    if (!c || !c->c->HotOn() || (info && info->struct_size < 8)) return RL_EINVAL;
    rlc::OpArgs a;
    a.hot = {key_out, key_cap, keys_tracked, info, clear};
    return table_op(c, rlc::OP_HOT, a);
}

extern "C" int rl_coalescer_get_stats(rl_coalescer* c, rl_coalescer_stats* out) {
    if (!c || !out || out->struct_size < 8) return RL_EINVAL;
    // the struct of before Charge, whatever the caller's size: rl_coalescer_get_stats_charge has the rest
    const rl_coalescer_stats v = c->c->Stats();
    rlc::copy_out_sized(out, v);
    return RL_OK;
}

extern "C" int rl_coalescer_get_stats_charge(rl_coalescer* c, rl_coalescer_stats_charge* out) {
    if (!c || !out || out->s.struct_size < 8) return RL_EINVAL;
    rlc::Counters v = c->c->Stats();
    v.struct_size = (uint32_t)std::min<size_t>(out->s.struct_size, sizeof v);
    memcpy(out, &v, v.struct_size);
    return RL_OK;
}
