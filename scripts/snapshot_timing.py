#!/usr/bin/env python3
"""Wall time of engine snapshots (include/rl_snapshot.h) on an MI355X, next to
the table operations that do the same passes without the snapshot's extra work:

  snapshot   Engine.snapshot: size query (the counting launch of
             k_snapshot_export) + staging + the writing launch + the
             device-to-host copy of the blob, against
  table_info rl_table_info_get: the same read pass over the three tables with
             no writes (three k_table_count launches);
  restore    Engine.restore into a fresh engine of the same capacity: upload +
             rebuild from the dense records, against
  table_gc   rl_table_gc at the same capacity: the same rebuild from a table.

Scenarios: 1M and 16M live keys, token bucket only and mixed (1/2 token
bucket, 1/4 fixed window, 1/4 sliding window), tables at load factor <= 1/2.
Every figure is the median (and the minimum) of --repeats timed calls after one
untimed call; each call ends in a device synchronise inside the library.

The kernels' own device times come from a run of this script under
`rocprofv3 --kernel-trace --stats` with `--scenario` naming one scenario (the
per-kernel MinNs of that run), never from this script's clocks.

  python scripts/snapshot_timing.py [--out profiles/snapshot_timing.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402

try:
    import torch  # noqa: E402,F401  (before the engine library: tests/conftest.py says why)
except ImportError:
    pass
import rl_amd  # noqa: E402

NS = 1_000_000_000
T0 = 1_760_000_000_000_000_000
# an hour-long window: every key stays live for the whole run
CONFIGS = [(rl_amd.TOKEN_BUCKET, 20, 3600 * NS), (rl_amd.FIXED_WINDOW, 100, 3600 * NS),
           (rl_amd.SLIDING_WINDOW, 100, 3600 * NS)]
BATCH = 1 << 20


def pow2_at_least(x):
    return 1 << max(10, (int(x) - 1).bit_length())


def new_engine(tb_cap, win_cap):
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=tb_cap, win_capacity=win_cap, max_batch=BATCH)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    return eng


def fill(eng, nkeys, mixed):
    """nkeys distinct keys, one request each, in batches of 1M"""
    for lo in range(0, nkeys, BATCH):
        key = np.arange(lo, min(lo + BATCH, nkeys), dtype=np.uint64)
        cfg = np.zeros(key.size, np.uint32)
        if mixed:
            cfg = np.where(key % 4 < 2, 0, np.where(key % 4 == 2, 1, 2)).astype(np.uint32)
        eng.decide(key, np.full(key.size, T0 + lo, np.int64), np.ones(key.size, np.int64), cfg, want_tokens=False)


def timed(fn, repeats):
    fn()                                      # warm-up: code objects, staging allocations
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def scenario(name, nkeys, mixed, repeats, emit):
    ntb = nkeys if not mixed else nkeys // 2
    tb_cap = pow2_at_least(2 * ntb)
    win_cap = pow2_at_least(2 * (nkeys - ntb)) if mixed else 1024
    now_ms = (T0 + nkeys) // 1_000_000 + 1
    eng = new_engine(tb_cap, win_cap)
    fill(eng, nkeys, mixed)
    info = eng.table_info(now_ms)
    assert info.tb_live + info.win_live == nkeys, (info.tb_live, info.win_live)
    table_mb = (32 * info.tb_capacity + 64 * info.win_capacity + 32 * info.spill_capacity) / 1e6

    blob = eng.snapshot(now_ms)
    sinfo = rl_amd.rl_snapshot_info()
    t_info = timed(lambda: eng.table_info(now_ms), repeats)
    t_size = timed(lambda: rl_amd.lib.rl_snapshot_export(eng.h, now_ms, 1, 0, None, 0, ctypes.byref(sinfo)), repeats)
    t_snap = timed(lambda: eng.snapshot(now_ms), repeats)
    t_gc = timed(lambda: eng.table_gc(now_ms, tb_cap, win_cap), repeats)

    def restore():
        fresh = new_engine(tb_cap, win_cap)
        t0 = time.perf_counter()
        fresh.restore(blob, now_ms)
        dt = (time.perf_counter() - t0) * 1e3
        fresh.close()
        return dt
    restore()
    r = [restore() for _ in range(repeats)]
    t_restore = (statistics.median(r), min(r))
    eng.close()

    emit(f"{name}: {nkeys} live keys ({info.tb_live} token bucket, {info.win_live} window), tables "
         f"{info.tb_capacity} + {info.win_capacity} + {info.spill_capacity} slots = {table_mb:.0f} MB, "
         f"blob {blob.size / 1e6:.1f} MB")
    for what, (med, lo) in [("table_info", t_info), ("snapshot size query", t_size), ("snapshot", t_snap),
                            ("table_gc", t_gc), ("restore", t_restore)]:
        emit(f"  {what:<20s} median {med:9.3f} ms   min {lo:9.3f} ms")
    emit(f"  snapshot / table_info {t_snap[0] / t_info[0]:6.2f}x    size query / table_info "
         f"{t_size[0] / t_info[0]:5.2f}x    restore / table_gc {t_restore[0] / t_gc[0]:5.2f}x    "
         f"snapshot {blob.size / 1e6 / t_snap[0]:.2f} GB/s")


SCENARIOS = {"1M_tb": (1_000_000, False), "1M_mixed": (1_000_000, True),
             "16M_tb": (16_000_000, False), "16M_mixed": (16_000_000, True)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scenario", choices=sorted(SCENARIOS), action="append",
                    help="only these scenarios (default: all four)")
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"scripts/snapshot_timing.py --repeats {args.repeats}: wall ms per call (host clock around a synchronous "
         "call)")
    for name in args.scenario or SCENARIOS:
        scenario(name, *SCENARIOS[name], args.repeats, emit)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
