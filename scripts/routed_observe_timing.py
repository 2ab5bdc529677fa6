#!/usr/bin/env python3
"""Cost of observe= per routed decide step: configs[1]-shaped steps (token bucket
20 / 12 s, 1M keys Zipf 1.1, 1M requests), world 1 in place, through
shard.RoutedPipeline as bench.py builds it.

  --root DIR   the tree to import traces, rl_amd and shard from (default: this
               one; a built checkout of another commit for an A/B)
  --mode       today (no observe keyword: works on the parent too), none
               (observe=None), tally, both
Prints one line: ms per step of every timed window (host clock around the
window's steps, the flush and a device synchronise), after --warmup steps.  With
--label ending in "kernels" (mode both) it first times the counting calls alone
on one finished step, beside the array forms on the same requests: HIP events on
one stream, 9 calls after one.  Compare cases in fresh processes, alternating.
No threshold is attached to these figures."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--mode", required=True, choices=["today", "none", "tally", "both"])
ap.add_argument("--label", default="")
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--warmup", type=int, default=4)
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path[:0] = [root, os.path.join(root, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rl_amd  # noqa: E402
import shard  # noqa: E402
import traces  # noqa: E402

assert os.path.abspath(rl_amd.__file__).startswith(root), rl_amd.__file__
M = 1_000_000
dev = torch.device("cuda", 0)
gen = traces.TokenBucketZipf(batch=M, seed=3)
nb = args.warmup + args.steps * args.windows
host = [gen.next_batch() for _ in range(nb)]
ins = [(torch.from_numpy(k.view(np.int64)).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(n).to(dev),
        torch.from_numpy(c.view(np.int32)).to(dev)) for k, t, n, c in host]
router = rl_amd.Router(0, 1, M, M)
eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1024,
                    max_batch=router.capacity, device=0, flags=0)
for a, L, W in gen.configs:
    eng.register(a, L, W)
kw = {}
if args.mode == "none":
    kw = dict(observe=None)
elif args.mode in ("tally", "both"):
    eng.tally_enable(0)
    obs = [eng.tally_routed]
    if args.mode == "both":
        eng.hot_enable(1000)
        obs.append(eng.hot_routed)
    kw = dict(observe=obs)
pipe = shard.RoutedPipeline(router, eng.decide_routed, 1, M, dev, pg_req=None, pg_res=None, depth=4, exchange=False,
                            lookahead=1, decide_ev=eng.decide_routed_ev, **kw)
outs = [(torch.empty(M, dtype=torch.uint8, device=dev),) + tuple(torch.empty(M, dtype=torch.int64, device=dev)
                                                                 for _ in range(3)) for _ in range(pipe.depth)]
b0 = 0


def run(count):
    global b0
    for b in range(b0, b0 + count):
        pipe.step(b, *ins[b], *outs[b % pipe.depth])
    pipe.flush()
    b0 += count


run(args.warmup)
torch.cuda.synchronize()
assert eng.sync() == 0 and router.sync(None) == 0
if args.mode == "both" and args.label.endswith("kernels"):
    # device time of the counting kernels alone on the last finished step, beside the array forms
    import statistics
    s = pipe.slots[(b0 - 1) % pipe.depth]
    p = lambda t: t.data_ptr()
    cur = torch.cuda.current_stream(dev).cuda_stream
    a = (pipe.m_max, p(s["count"]), p(s["send"]), p(s["order"]), p(s["sms"]), p(s["res"]))
    k, _, n, c = ins[b0 - 1]
    d = outs[(b0 - 1) % pipe.depth][0]

    def timed(fn):
        ts = []
        for i in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i:
                ts.append(e0.elapsed_time(e1))
        return f"median {statistics.median(ts):6.3f} ms min {min(ts):6.3f} ms"

    ident = int(s["order"][:1].cpu()[0]) == -1
    print(f"kernels on one finished 1M step (identity form: {ident}), events on one stream, 9 calls after one:")
    print("  tally_routed      " + timed(lambda: eng.tally_routed(*a, p(s["scnt"]), 1, cur)))
    print("  tally_device      " + timed(lambda: eng.tally_device(M, p(k), p(c), p(n), p(d), cur)))
    print("  hot_routed        " + timed(lambda: eng.hot_routed(*a, stream=cur)))
    print("  hot_batch_device  " + timed(lambda: eng.hot_batch_device(M, p(k), p(c), p(n), p(d), cur)), flush=True)
    eng.tally_read(clear=True)
    eng.hot_read(clear=True)
ms = []
for w in range(args.windows):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
assert eng.sync() == 0 and router.sync(None) == 0
extra = ""
if args.mode in ("tally", "both"):
    t = eng.tally_read(top=1)
    extra = (f"  tally: routed steps {t.routed.steps} requests {t.routed.requests}, denied "
             f"{int(t.cfg['count'][:, 0].sum())}, keys tracked {t.keys_tracked}, top key denied "
             f"{int(t.keys[0]['denied']) if t.keys.size else 0}")
    if args.mode == "both":
        h = eng.hot_read(top=1)
        extra += f"; hot: total {h.info.total}, candidates {h.keys_tracked}, top estimate {int(h.keys[0]['estimate'])}"
print(f"{args.label or args.mode:14s} ms/step per window of {args.steps} steps: " +
      " ".join(f"{x:7.3f}" for x in ms) + extra, flush=True)
eng.close()
router.close()
