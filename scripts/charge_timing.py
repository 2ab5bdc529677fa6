#!/usr/bin/env python3
"""Timings of Charge (rl_charge_batch_device: k_charge_ask, the decide and
k_charge_finish) on an MI355X, at M = 1048575 requests in one call.

The requests are distinct keys in thirds: a token bucket, a fixed window and a
sliding window (key id mod 3).  A bucket request is short when it asks for more
than the bucket holds: it is clamped to what is there and takes it.  The share
of short bucket requests is 0 %, 10 % and 100 %; every repeat runs one
millisecond later, so a bucket emptied by the repeat before holds something
again.  Beside it, in the same session and on the same arrays: a plain decide
and a plain peek of the same M.  HIP events on the caller's stream around one
call, median of --repeats.

  python scripts/charge_timing.py [--out profiles/charge_timing.txt]
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--out", default=None, help="append the lines to this file")
ap.add_argument("--repeats", type=int, default=9)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the engine library: tests/conftest.py says why)

import rl_amd  # noqa: E402

NS = 1_000_000_000
T0 = 1_760_000_000 * NS
M = (1 << 20) - 1
LIMIT = 1 << 50
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, repeats, before=None):
    """ms between two events on the current stream around fn(); before() runs
    ahead of each call, outside the events"""
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


dev = torch.device("cuda", 0)
eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1 << 22, max_batch=1 << 20,
                    flags=rl_amd.OPT_PIPELINE)
assert eng.charge_max() == 1 << 20
for alg in (rl_amd.TOKEN_BUCKET, rl_amd.FIXED_WINDOW, rl_amd.SLIDING_WINDOW):
    eng.register(alg, LIMIT, 3600 * NS)
key = np.arange(M, dtype=np.uint64)
cfg = (key % np.uint64(3)).astype(np.uint32)
buckets = np.nonzero(cfg == 0)[0]
rng = np.random.default_rng(5)
to_dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                    x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)
d_key, d_cfg = to_dev(key), to_dev(cfg)
d_ts = torch.full((M,), T0 + 1000, dtype=torch.int64, device=dev)
outs = ([torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev) for _ in range(3)] +
        [torch.empty(M, dtype=torch.float64, device=dev)])
stream = torch.cuda.current_stream(dev).cuda_stream
p = lambda t: t.data_ptr()
later = lambda: d_ts.add_(1_000_000)

emit(f"--repeats {args.repeats}: device ms between two events on the caller's stream; M = {M} requests on distinct "
     f"keys (a third each TB, FW, SW), tables of 2^21 / 2^22 slots")
# every key exists and holds taken units before anything is timed
eng.decide(key, np.full(M, T0, np.int64), np.full(M, 1 << 30, np.int64), cfg, want_tokens=False)
for share in (0.0, 0.1, 1.0):
    n = np.ones(M, np.int64)
    short = buckets[rng.random(buckets.size) < share]
    n[short] = LIMIT + 1                          # more than a bucket ever holds
    d_n = to_dev(n)
    torch.cuda.synchronize()
    t = timed(lambda: eng.charge_device(M, p(d_key), p(d_ts), p(d_n), p(d_cfg), None, *[p(x) for x in outs], stream),
              args.repeats, later)
    torch.cuda.synchronize()
    assert eng.sync() == 0
    dec, charged = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    is_short = np.zeros(M, bool)
    is_short[short] = True
    assert (dec[~is_short] == rl_amd.ALLOWED).all() and (charged[~is_short] == 1).all()
    assert (dec[is_short] == rl_amd.DENIED).all() and (charged[is_short] > 0).all()
    emit(f"  Charge, {100 * share:5.1f} % of the bucket requests short   median {t[0]:7.3f} ms   min {t[1]:7.3f} ms   "
         f"{M / t[1] / 1e3:7.1f} M requests/s   {short.size} short")
d_one = torch.ones(M, dtype=torch.int64, device=dev)
t = timed(lambda: eng.decide_device(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), None, p(outs[0]), p(outs[2]), p(outs[1]),
                                    p(outs[3]), p(outs[4]), stream), args.repeats, later)
emit(f"  plain decide of the same M                    median {t[0]:7.3f} ms   min {t[1]:7.3f} ms")
t = timed(lambda: eng.peek_device(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), None, p(outs[0]), p(outs[2]), p(outs[1]),
                                  p(outs[3]), p(outs[4]), stream), args.repeats, later)
torch.cuda.synchronize()
assert eng.sync() == 0
emit(f"  plain peek of the same M                      median {t[0]:7.3f} ms   min {t[1]:7.3f} ms")
eng.close()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
