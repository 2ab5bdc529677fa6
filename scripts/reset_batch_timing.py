#!/usr/bin/env python3
"""Timings of batched Reset (rl_reset_batch_device, k_reset_batch) on an MI355X.

  --mode kernels  k_reset_batch against k_peek at 1M requests, same session,
                  same tables, same request arrays: configs[1]'s token-bucket
                  table (2^21 slots, Zipf 1.1 keys) and an 8M-key fixed-window
                  table (2^24 slots, uniform keys).  HIP events on the caller's
                  stream around one call (kernel plus two event hand-offs
                  between streams).  A decide of the same batch runs before
                  every timed reset, so each reset deletes live keys.
  --mode calls    4096 resets: one rl_reset_batch_device call against 4096
                  rl_reset_device calls, wall time from the first call to the
                  end of the stream sync.
  --mode storm    through the coalescer: 64 threads x 256 single Resets while
                  4 threads decide one request at a time (C++ clients,
                  scripts/micro/reset_storm.cpp); wall time of the resets,
                  stats.reset_launches, and the p99 of the decide calls made
                  during the storm.  The binary uses only calls the parent
                  commit has, so `--tree <parent checkout>` runs the same
                  storm against that checkout's library.

  python scripts/reset_batch_timing.py --mode all [--out profiles/reset_batch_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--mode", choices=["kernels", "calls", "storm", "all"], default="all")
ap.add_argument("--out", default=None, help="append the lines to this file")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--tree", default=None, help="storm: the checkout whose library to run against")
ap.add_argument("--label", default="this tree")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the engine library: tests/conftest.py says why)

import rl_amd  # noqa: E402
import traces  # noqa: E402

NS = 1_000_000_000
M = 1_000_000
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def dev_arrays(key, ts, n, cfg, dev):
    ins = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                            np.ascontiguousarray(x)).to(dev) for x in (key, ts, n, cfg.view(np.int32))]
    m = key.size
    outs = ([torch.empty(m, dtype=torch.uint8, device=dev)] +
            [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(m, dtype=torch.float64, device=dev)])
    return ins, outs


def timed(fn, repeats, before=None):
    """ms between two events on the current stream around fn(); before() runs
    untimed ahead of every call"""
    t = []
    for i in range(repeats + 1):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            t.append(a.elapsed_time(b))
    return statistics.median(t), min(t)


def kernels_scenario(name, eng, warm, batch, repeats):
    dev = torch.device("cuda", 0)
    for b in warm:
        eng.decide(*b, want_tokens=False)
    ins, outs = dev_arrays(*batch, dev)
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = [x.data_ptr() for x in ins]
    dargs = (M, p[0], p[1], p[2], p[3], None, *[x.data_ptr() for x in outs], stream)
    decide = lambda: eng.decide_device(*dargs)
    decide()
    t_peek = timed(lambda: eng.peek_device(*dargs), repeats)
    t_reset = timed(lambda: eng.reset_batch_device(M, p[0], p[1], p[3], status.data_ptr(), stream), repeats,
                    before=decide)
    t_again = timed(lambda: eng.reset_batch_device(M, p[0], p[1], p[3], status.data_ptr(), stream), repeats)
    torch.cuda.synchronize()
    assert eng.sync() == 0 and bool((status == rl_amd.RESET_DONE).all())
    info = eng.table_info(int(batch[1][-1]) // 1_000_000)
    emit(f"{name}: {M} requests, tables {info.tb_capacity} + {info.win_capacity} slots, "
         f"{info.tb_used + info.win_used} keys present")
    emit(f"  k_peek                        median {t_peek[0]:7.3f} ms   min {t_peek[1]:7.3f} ms")
    emit(f"  k_reset_batch (live keys)     median {t_reset[0]:7.3f} ms   min {t_reset[1]:7.3f} ms   "
         f"{M / t_reset[1] / 1e3:7.1f} M resets/s   k_reset_batch / k_peek {t_reset[1] / t_peek[1]:5.2f}x")
    emit(f"  k_reset_batch (already reset) median {t_again[0]:7.3f} ms   min {t_again[1]:7.3f} ms")


def mode_kernels():
    emit(f"kernels, --repeats {args.repeats}: device ms between two events on the caller's stream")
    g = traces.TokenBucketZipf(batch=M)
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1024, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE)
    for a, L, W in g.configs:
        eng.register(a, L, W)
    warm = [g.next_batch() for _ in range(4)]
    kernels_scenario("tb_zipf", eng, warm, g.next_batch(), args.repeats)
    eng.close()
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1024, win_capacity=1 << 24, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE, spill_capacity=1024)
    eng.register(rl_amd.FIXED_WINDOW, 100, 3600 * NS)
    rng = np.random.default_rng(7)
    nkeys, t0 = 8 * M, traces.T0
    warm = [(np.arange(i * M, (i + 1) * M, dtype=np.uint64), np.full(M, t0 + i, np.int64), np.ones(M, np.int64),
             np.zeros(M, np.uint32)) for i in range(nkeys // M)]
    batch = (rng.integers(0, nkeys, M).astype(np.uint64), np.full(M, t0 + 1000, np.int64), np.ones(M, np.int64),
             np.zeros(M, np.uint32))
    kernels_scenario("fw_8M", eng, warm, batch, args.repeats)
    eng.close()


def mode_calls():
    K = 4096
    dev = torch.device("cuda", 0)
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 16, win_capacity=1 << 16, max_batch=1 << 16,
                        flags=rl_amd.OPT_PIPELINE)
    cfg_tb = eng.register(rl_amd.TOKEN_BUCKET, 20, 12 * NS)
    key = np.arange(K, dtype=np.uint64)
    ts = np.full(K, traces.T0, np.int64)
    cfg = np.full(K, cfg_tb, np.uint32)
    warm = lambda: eng.decide(key, ts, np.ones(K, np.int64), cfg, want_tokens=False)
    dk, dt, dc = (torch.from_numpy(x).to(dev) for x in (key.view(np.int64), ts, cfg.view(np.int32)))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    one, many = [], []
    for i in range(args.repeats + 1):
        warm()
        t = time.perf_counter()
        eng.reset_batch_device(K, dk.data_ptr(), dt.data_ptr(), dc.data_ptr(), None, stream)
        torch.cuda.synchronize()
        one.append((time.perf_counter() - t) * 1e3)
        warm()
        t = time.perf_counter()
        for k in range(K):
            rl_amd.lib.rl_reset_device(eng.h, cfg_tb, k, traces.T0, stream)
        torch.cuda.synchronize()
        many.append((time.perf_counter() - t) * 1e3)
    assert eng.sync() == 0
    eng.close()
    one, many = one[1:], many[1:]
    emit(f"calls, --repeats {args.repeats}: {K} resets, wall ms from the first call to the end of the sync")
    emit(f"  1 x rl_reset_batch_device      median {statistics.median(one):9.3f} ms   min {min(one):9.3f} ms")
    emit(f"  {K} x rl_reset_device        median {statistics.median(many):9.3f} ms   min {min(many):9.3f} ms   "
         f"({min(many) / K * 1e3:.1f} us per call)   ratio {min(many) / min(one):7.1f}x")


def mode_storm():
    """scripts/micro/reset_storm (C++ client threads: no interpreter lock
    between them) against the library of --tree, or of this tree"""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "micro", "reset_storm")
    if not os.path.exists(exe):
        sys.exit(f"{exe} is not built: make -C scripts/micro reset_storm")
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "distributed-rate-limiter_amd", "lib") + os.pathsep +
               os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe, args.label], env=env, check=True, capture_output=True, text=True).stdout
    for line in out.splitlines():
        emit(line)


for mode, fn in (("kernels", mode_kernels), ("calls", mode_calls), ("storm", mode_storm)):
    if args.mode in (mode, "all"):
        fn()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
