#!/usr/bin/env python3
"""Timings of AllowAll (rl_allow_all_batch_device: the decide, k_allow_all_settle
and the refund kernels) on an MI355X, at M = 3 * (2^20 // 3) members in one call.

The members come in groups of three -- a token bucket, a fixed window and a
sliding window of one user (key ids 3u, 3u + 1, 3u + 2) -- over 2^20 // 3 users.
A group fails when its bucket member asks for more than the bucket holds (it is
denied and takes nothing); its two window members were allowed and are given
back.  The share of failing groups is 0 %, 10 % and 100 %.  Beside it, in the
same session and on the same arrays: a plain decide of the same M and a plain
refund of the same M (n = 1, every request contributes).  HIP events on the
caller's stream around one call, median of --repeats.

The settle kernel's own time is not visible between two events around the
call: run this script under `rocprofv3 --kernel-trace --stats` and read
k_allow_all_settle's row; this script does not write those rows
(profiles/allow_all_kernels.txt holds them, copied by hand; DESIGN.md §10k
has both tables).

  python scripts/allow_all_timing.py [--out profiles/allow_all_timing.txt]
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
USERS = (1 << 20) // 3
M = 3 * USERS
LIMIT = 1 << 50
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


dev = torch.device("cuda", 0)
eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1 << 22, max_batch=1 << 20,
                    flags=rl_amd.OPT_PIPELINE)
assert eng.allow_all_max() == 1 << 20
for alg in (rl_amd.TOKEN_BUCKET, rl_amd.FIXED_WINDOW, rl_amd.SLIDING_WINDOW):
    eng.register(alg, LIMIT, 3600 * NS)
key = np.arange(M, dtype=np.uint64)
cfg = (key % np.uint64(3)).astype(np.uint32)
first = (cfg == 0).astype(np.uint8)
rng = np.random.default_rng(5)
to_dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                    x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)
d_key, d_cfg, d_first = to_dev(key), to_dev(cfg), to_dev(first)
d_ts = torch.full((M,), T0 + 1000, dtype=torch.int64, device=dev)
outs = ([torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev) for _ in range(3)] +
        [torch.empty(M, dtype=torch.float64, device=dev)] + [torch.empty(M, dtype=torch.uint8, device=dev) for _ in range(2)])
stream = torch.cuda.current_stream(dev).cuda_stream
p = lambda t: t.data_ptr()

emit(f"--repeats {args.repeats}: device ms between two events on the caller's stream; M = {M} members, "
     f"{USERS} groups of 3 (TB + FW + SW of one user), tables of 2^21 / 2^22 slots")
# every key exists and holds taken units before anything is timed
eng.decide(key, np.full(M, T0, np.int64), np.full(M, 1 << 30, np.int64), cfg, want_tokens=False)
for share in (0.0, 0.1, 1.0):
    n = np.ones(M, np.int64)
    fail = rng.random(USERS) < share
    n[0::3][fail] = LIMIT + 1                     # the bucket member of a failing group
    d_n = to_dev(n)
    torch.cuda.synchronize()
    t = timed(lambda: eng.allow_all_device(M, p(d_key), p(d_ts), p(d_n), p(d_cfg), None, p(d_first),
                                           *[p(x) for x in outs], stream), args.repeats)
    torch.cuda.synchronize()
    assert eng.sync() == 0
    verdict, rollback = outs[5].cpu().numpy(), outs[6].cpu().numpy()
    assert int((verdict[0::3] != rl_amd.ALLOWED).sum()) == int(fail.sum())
    assert int((rollback == rl_amd.REFUND_DONE).sum()) == 2 * int(fail.sum())
    emit(f"  AllowAll, {100 * share:5.1f} % of the groups fail   median {t[0]:7.3f} ms   min {t[1]:7.3f} ms   "
         f"{M / t[1] / 1e3:7.1f} M members/s   {2 * int(fail.sum())} members given back")
d_one = torch.ones(M, dtype=torch.int64, device=dev)
t = timed(lambda: eng.decide_device(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), None, *[p(x) for x in outs[:5]], stream),
          args.repeats)
emit(f"  plain decide of the same M                median {t[0]:7.3f} ms   min {t[1]:7.3f} ms")
t = timed(lambda: eng.refund_device(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), None, p(outs[6]), stream), args.repeats)
torch.cuda.synchronize()
assert eng.sync() == 0 and bool((outs[6] == rl_amd.REFUND_DONE).all())
emit(f"  plain refund of the same M (all distinct)   median {t[0]:7.3f} ms   min {t[1]:7.3f} ms")
eng.close()
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
