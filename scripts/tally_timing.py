#!/usr/bin/env python3
"""Timing of the usage tally's kernel (k_tally, csrc/rl_tally.h) on an MI355X.

k_tally on the results of one 1M-request batch of configs[1] (token bucket,
Zipf 1.1 keys: the hot key holds ~12 % of the batch) and of one uniform
fixed-window batch, each decided on a warm engine first.  HIP events on the
tally's stream around one rl_tally_batch_device call, the minimum of
--repeats; the tally is cleared before every timed call, so each one claims
its records anew.  The time is set against the 21 B per request the kernel
must read at 8 TB/s -- a fraction, not a target.

  python scripts/tally_timing.py [--out profiles/tally_timing.txt]
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
import traces  # noqa: E402

M = 1_000_000
HBM_GBS = 8000.0
lines = []


def emit(s):
    print(s, flush=True)
    lines.append(s)


def scenario(name, gen, tb, win):
    dev = torch.device("cuda", 0)
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=tb, win_capacity=win, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE)
    for a, L, W in gen.configs:
        eng.register(a, L, W)
    eng.tally_enable()
    for _ in range(4):
        eng.decide(*gen.next_batch(), want_tokens=False)
    key, ts, n, cfg = gen.next_batch()
    res = eng.decide(key, ts, n, cfg, want_tokens=False)
    dk, dn, dc, dd = (torch.from_numpy(x).to(dev) for x in (key.view(np.int64), n, cfg.view(np.int32), res.decision))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: eng.tally_device(M, dk.data_ptr(), dc.data_ptr(), dn.data_ptr(), dd.data_ptr(), stream)
    t = []
    for i in range(args.repeats + 1):
        eng.tally_read(clear=True)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        if i:
            t.append(a.elapsed_time(b) * 1e3)
    r = eng.tally_read(top=3)
    denied = key[res.decision == rl_amd.DENIED]
    ids, cnt = np.unique(denied, return_counts=True)
    assert int(r.cfg["count"].sum()) + r.info.unknown_cfg + r.info.bad_codes == M
    assert int(r.cfg["count"][:, 0].sum()) == denied.size
    floor_us = 21.0 * M / (HBM_GBS * 1e9) * 1e6
    emit(f"{name}: {M} requests, {denied.size} denied on {ids.size} distinct keys "
         f"(most denied key: {int(cnt.max()) if cnt.size else 0} requests)")
    emit(f"  k_tally   min {min(t):8.1f} us   median {statistics.median(t):8.1f} us   of {args.repeats}")
    emit(f"  21 B/request at 8 TB/s = {floor_us:.1f} us: {floor_us / min(t):.3f} of the time is that read")
    emit(f"  key table: {r.info.key_slots} records, {r.info.keys_tracked} keys tracked, "
         f"untracked_requests {r.info.untracked_requests}")
    if r.keys.size:
        emit(f"  top key: id {int(r.keys[0]['key_id'])}, denied {int(r.keys[0]['denied'])}")
    eng.close()


emit(f"k_tally, --repeats {args.repeats}: device us between two events on the tally's stream, one call")
scenario("tb_zipf (configs[1])", traces.TokenBucketZipf(batch=M), 1 << 21, 1024)
scenario("fw_uniform", traces.FixedWindowUniform(batch=M), 1024, 1 << 21)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
