#!/usr/bin/env python3
"""Timings of Refund (rl_refund_batch_device: k_refund_add + k_refund_apply)
on an MI355X, at m = 2^20 requests in one call.

Three key shapes over 2^20 live keys -- all distinct, Zipf 1.1, one key --
on a token-bucket table and on a fixed-window table (2^22 slots each), and
k_reset_batch at the same m on the same request arrays, in the same session,
as the yardstick.  HIP events on the caller's stream around one call: the
kernels plus two event hand-offs between streams.  The refunds are n = 1
against counters warmed far above what the repeats take back, so every
request of every repeat contributes; the resets run last (they delete).

  python scripts/refund_timing.py [--out profiles/refund_timing.txt]
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
M = 1 << 20
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, repeats):
    """ms between two events on the current stream around fn()"""
    t = []
    for i in range(repeats + 1):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            t.append(a.elapsed_time(b))
    return statistics.median(t), min(t)


def scenario(alg_name, alg, repeats):
    dev = torch.device("cuda", 0)
    tb = alg == rl_amd.TOKEN_BUCKET
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 22 if tb else 1024,
                        win_capacity=1024 if tb else 1 << 22, max_batch=M, flags=rl_amd.OPT_PIPELINE,
                        spill_capacity=1024)
    assert eng.refund_max() == M
    eng.register(alg, 1 << 50, 3600 * NS)
    ids = np.arange(M, dtype=np.uint64)
    # every key holds 2^40 taken units: (repeats + 1) * 2^20 refunds of 1 on one key leave it far from empty
    eng.decide(ids, np.full(M, T0, np.int64), np.full(M, 1 << 40, np.int64), np.zeros(M, np.uint32), want_tokens=False)
    rng = np.random.default_rng(11)
    shapes = [("all distinct", rng.permutation(M).astype(np.uint64)),
              ("Zipf 1.1", ((rng.zipf(1.1, M) - 1) % M).astype(np.uint64)),
              ("one key", np.full(M, 12345, np.uint64))]
    ts = torch.full((M,), T0 + 1000, dtype=torch.int64, device=dev)
    n = torch.ones(M, dtype=torch.int64, device=dev)
    cfg = torch.zeros(M, dtype=torch.int32, device=dev)
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    emit(f"{alg_name}: m = {M} per call, {M} live keys, table of {1 << 22} slots")
    base = None
    keys = {}
    for name, k in shapes:
        dk = torch.from_numpy(k.view(np.int64)).to(dev)
        keys[name] = dk
        torch.cuda.synchronize()
        t = timed(lambda: eng.refund_device(M, dk.data_ptr(), ts.data_ptr(), n.data_ptr(), cfg.data_ptr(), None,
                                            status.data_ptr(), stream), repeats)
        torch.cuda.synchronize()
        assert eng.sync() == 0 and bool((status == rl_amd.REFUND_DONE).all())
        base = base or t[1]
        emit(f"  k_refund_add + k_refund_apply, {name:13s} median {t[0]:7.3f} ms   min {t[1]:7.3f} ms   "
             f"{M / t[1] / 1e3:7.1f} M refunds/s   {t[1] / base:5.2f}x all distinct   "
             f"{np.unique(k).size} targets")
    for name, _ in shapes:
        dk = keys[name]
        t = timed(lambda: eng.reset_batch_device(M, dk.data_ptr(), ts.data_ptr(), cfg.data_ptr(), status.data_ptr(),
                                                 stream), repeats)
        emit(f"  k_reset_batch,                  {name:13s} median {t[0]:7.3f} ms   min {t[1]:7.3f} ms")
    torch.cuda.synchronize()
    assert eng.sync() == 0
    eng.close()


emit(f"--repeats {args.repeats}: device ms between two events on the caller's stream")
scenario("token bucket", rl_amd.TOKEN_BUCKET, args.repeats)
scenario("fixed window", rl_amd.FIXED_WINDOW, args.repeats)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
