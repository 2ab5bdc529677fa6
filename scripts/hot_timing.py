#!/usr/bin/env python3
"""Timing of the top keys' kernels (k_hot_add + k_hot_pick, csrc/rl_hot.h) on an
MI355X, against k_tally on the same batches in the same run.

Three 1M-request batches: configs[1] (token bucket, Zipf 1.1 keys: the hot key
holds ~12 % of the batch) and a uniform fixed-window batch, each decided on a
warm engine first, and one key holding the whole batch.  HIP events on the
caller's stream around one rl_hot_batch_device call (both launches) and around
one rl_tally_batch_device call; state is cleared before every timed call; the
minimum and the median of --repeats.  The one-key batch is not decided: the top
keys count it as allowed, the tally gets an all-denied copy of the decisions
(its worst case: every request of the key reaches the key table).

  python scripts/hot_timing.py [--out profiles/hot_timing.txt]
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=None, help="append the lines to this file")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--width", type=int, default=0, help="counters per sketch row (0: the default, 1 << 18)")
ap.add_argument("--hot-min", type=int, default=1000)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the engine library: tests/conftest.py says why)

import rl_amd  # noqa: E402
import traces  # noqa: E402

M = 1_000_000
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(call, clear):
    t = []
    for i in range(args.repeats + 1):
        clear()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if i:
            t.append(a.elapsed_time(b) * 1e3)
    return min(t), statistics.median(t)


def scenario(name, gen, tb, win, one_key=False):
    dev = torch.device("cuda", 0)
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=tb, win_capacity=win, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE)
    for a, L, W in gen.configs:
        eng.register(a, L, W)
    eng.tally_enable()
    eng.hot_enable(args.hot_min, width=args.width)
    for _ in range(4):
        eng.decide(*gen.next_batch(), want_tokens=False)
    key, ts, n, cfg = gen.next_batch()
    if one_key:
        key = np.full(M, key[0], np.uint64)
        cfg = np.full(M, cfg[0], np.uint32)
        dec_hot, dec_tally = np.ones(M, np.uint8), np.zeros(M, np.uint8)
    else:
        dec_hot = dec_tally = eng.decide(key, ts, n, cfg, want_tokens=False).decision
    dk, dn, dc, dh, dt = (torch.from_numpy(x).to(dev) for x in (key.view(np.int64), n, cfg.view(np.int32), dec_hot,
                                                              dec_tally))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    hot = timed(lambda: eng.hot_batch_device(M, dk.data_ptr(), dc.data_ptr(), dn.data_ptr(), dh.data_ptr(), stream),
                lambda: eng.hot_read(clear=True))
    tally = timed(lambda: eng.tally_device(M, dk.data_ptr(), dc.data_ptr(), dn.data_ptr(), dt.data_ptr(), stream),
                  lambda: eng.tally_read(clear=True))
    h = eng.hot_read(top=3)
    counted = (dec_hot <= 2) & (cfg < len(gen.configs))
    ids, cnt = np.unique(key[counted], return_counts=True)
    assert h.info.total == int(counted.sum()) and h.info.total + h.info.skipped == M
    assert not h.keys.size or int(h.keys[0]["estimate"]) >= int(cnt.max())
    denied = int((dec_tally == rl_amd.DENIED).sum())
    emit(f"{name}: {M} requests, {int(counted.sum())} counted on {ids.size} distinct keys "
         f"(heaviest key: {int(cnt.max())} requests); {denied} denied")
    emit(f"  k_hot_add + k_hot_pick   min {hot[0]:8.1f} us   median {hot[1]:8.1f} us   of {args.repeats}")
    emit(f"  k_tally                  min {tally[0]:8.1f} us   median {tally[1]:8.1f} us   of {args.repeats}")
    emit(f"  ratio of the minima {hot[0] / tally[0]:.2f}, of the medians {hot[1] / tally[1]:.2f}")
    emit(f"  sketch {h.info.depth} x {h.info.width}, hot_min {h.info.hot_min}: {h.info.keys_tracked} candidates of "
         f"{int((cnt >= h.info.hot_min).sum())} keys at or above it, dropped {h.info.dropped}" +
         (f"; top key: id {int(h.keys[0]['key_id'])}, estimate {int(h.keys[0]['estimate'])}" if h.keys.size else ""))
    eng.close()


emit(f"k_hot_add + k_hot_pick and k_tally, --repeats {args.repeats}: device us between two events on the caller's "
     "stream, one call each")
scenario("tb_zipf (configs[1])", traces.TokenBucketZipf(batch=M), 1 << 21, 1024)
scenario("fw_uniform", traces.FixedWindowUniform(batch=M), 1024, 1 << 21)
scenario("one key", traces.TokenBucketZipf(batch=M), 1 << 21, 1024, one_key=True)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
