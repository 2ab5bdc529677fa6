// reset_storm -- 64 threads x 256 single Resets through the coalescer while 4
// threads decide one request at a time (scripts/reset_batch_timing.py --mode
// storm, without an interpreter lock between the client threads).  Only calls
// the C-ABI had before rl_coalescer_reset_batch, so one binary runs against
// the library of either tree:
//   LD_LIBRARY_PATH=<tree>/distributed-rate-limiter_amd/lib ./reset_storm <label>
// Prints the wall time of the resets, the launches, and p50 / p99 / max of the
// decide calls made during the storm.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../include/rl_coalescer.h"

static double now_us() {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
    const char* label = argc > 1 ? argv[1] : "this tree";
    const int nthreads = 64, per = 256, nload = 4;
    const int64_t T0 = 1760000000000000000LL;
    rl_opts o{};
    o.struct_size = sizeof o;
    o.profile = RL_PROFILE_REDIS7;
    o.tb_capacity = 1 << 18;
    o.win_capacity = 1 << 12;
    o.max_batch = 1 << 16;
    o.flags = RL_OPT_PIPELINE;
    rl_engine* e = nullptr;
    if (rl_engine_create(&o, &e) != RL_OK) return 1;
    uint32_t c = 0;
    if (rl_config_register(e, RL_ALG_TOKEN_BUCKET, 20, 12000000000LL, &c) != RL_OK) return 1;
    rl_coalescer_opts co{};
    co.struct_size = sizeof co;
    co.max_batch = 1 << 16;
    rl_coalescer* q = nullptr;
    if (rl_coalescer_create(e, &co, &q) != RL_OK) return 1;
    const size_t nk = (size_t)nthreads * per;
    {   // every key the storm resets exists
        std::vector<uint64_t> key(nk);
        std::vector<int64_t> ts(nk, T0), n(nk, 1), r(nk);
        std::vector<uint32_t> cfg(nk, c);
        std::vector<uint8_t> d(nk);
        for (size_t i = 0; i < nk; i++) key[i] = i;
        uint64_t t = 0;
        if (rl_coalescer_submit(q, nk, key.data(), ts.data(), n.data(), cfg.data(), &t) != RL_OK) return 1;
        if (rl_coalescer_wait(q, t, -1, d.data(), r.data(), r.data(), r.data()) != RL_OK) return 1;
    }
    std::atomic<bool> stop{false}, storm{false};
    std::atomic<int> bad{0};
    std::vector<std::vector<double>> lat(nload);
    std::vector<std::thread> loaders, resetters;
    for (int i = 0; i < nload; i++)
        loaders.emplace_back([&, i] {
            for (int64_t j = 0; !stop.load(); j++) {
                uint8_t d;
                int64_t a, b, r;
                const double t = now_us();
                if (rl_coalescer_decide(q, 1000000 + i, T0 + j, 1, c, &d, &a, &b, &r) != RL_OK) bad++;
                const double dt = now_us() - t;
                if (storm.load()) lat[i].push_back(dt);
            }
        });
    std::this_thread::sleep_for(std::chrono::milliseconds(200));   // the steady load alone
    rl_coalescer_stats s0{}, s1{};
    s0.struct_size = s1.struct_size = sizeof s0;
    rl_coalescer_get_stats(q, &s0);
    storm.store(true);
    const double t0 = now_us();
    for (int i = 0; i < nthreads; i++)
        resetters.emplace_back([&, i] {
            for (int j = 0; j < per; j++)
                if (rl_coalescer_reset(q, (uint64_t)i * per + j, T0, c) != RL_OK) bad++;
        });
    for (auto& t : resetters) t.join();
    const double wall = now_us() - t0;
    storm.store(false);
    rl_coalescer_get_stats(q, &s1);
    stop.store(true);
    for (auto& t : loaders) t.join();
    rl_coalescer_destroy(q);
    const int sync = rl_engine_sync(e);
    rl_engine_destroy(e);
    std::vector<double> d;
    for (auto& v : lat) d.insert(d.end(), v.begin(), v.end());
    std::sort(d.begin(), d.end());
    if (bad.load() || sync != RL_OK || d.empty()) {
        fprintf(stderr, "reset_storm: %d failed calls, sync %d\n", bad.load(), sync);
        return 1;
    }
    printf("storm (%s): %d threads x %d single Resets through the coalescer, %d decide threads (C++ clients)\n", label,
           nthreads, per, nload);
    printf("  resets: wall %9.1f ms (%6.1f us per reset)   launches of all kinds %llu   reset_launches ", wall / 1e3,
           wall / nk, (unsigned long long)(s1.batches - s0.batches));
    // a library older than the field fills in fewer bytes and says so in struct_size
    if (s1.struct_size >= offsetof(rl_coalescer_stats, reset_launches) + sizeof(uint64_t))
        printf("%llu\n", (unsigned long long)(s1.reset_launches - s0.reset_launches));
    else
        printf("n/a (one per reset)\n");
    printf("  decide calls during the storm: %zu   p50 %8.1f us   p99 %8.1f us   max %8.1f us\n", d.size(),
           d[d.size() / 2], d[(size_t)(d.size() * 0.99)], d.back());
    return 0;
}
