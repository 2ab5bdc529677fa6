#!/usr/bin/env python3
"""Device time of the refund step of the routed path (include/rl_route.h:
k_refund_add_routed + k_refund_apply) on an MI355X, at world 1 with the buckets
and results read in place, beside rl_refund_batch_device (k_refund_add +
k_refund_apply) on the same requests in the same session.

One step of 1M refunds (n = 1, ts in order: the merge leaves the
RL_ORDER_IDENTITY form) over 2^20 live fixed-window counters that hold 10^9
each, so no repeat deletes one:

  distinct   1M different keys
  zipf       keys Zipf 1.1 over the 2^20
  one key    every request the same key

step:    HIP events on the caller's stream around pack -> merge -> the engine's
         call -> unpack, all on that stream (the engine's kernels run on its
         replay stream; the caller's stream waits for them).
engine:  the same events around the engine's call alone, the step's pack and
         merge complete before the first event: two kernels plus two event
         hand-offs between streams.
array:   the same events around rl_refund_batch_device on the same requests as
         arrays.
Median and minimum of --repeats calls after one untimed call.  No threshold is
attached to these figures.

  python scripts/routed_refund_timing.py [--out profiles/routed_refund_timing.txt]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-rate-limiter_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402  (before the engine library: tests/conftest.py says why)

import rl_amd  # noqa: E402

M = 1_000_000
NKEYS = 1 << 20
HAVE = 10 ** 9
T0 = 1_760_000_000_000_000_000
NS = 1_000_000_000


def timed(fn, repeats, before=None):
    """ms between two events on the current stream around fn(); before() runs
    and completes ahead of the first event"""
    times = []
    for k in range(repeats + 1):
        if before is not None:
            before()
            torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda", 0)
    router = rl_amd.Router(0, 1, M, M)
    cap = router.capacity
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1024, win_capacity=1 << 21, max_batch=cap)
    eng.register(3, 10 ** 12, 3600 * NS)
    assert eng.refund_max() >= M
    keys = np.arange(1, NKEYS + 1, dtype=np.uint64)
    eng.decide(keys, np.full(NKEYS, T0), np.full(NKEYS, HAVE), np.zeros(NKEYS, np.uint32), want_tokens=False)
    now_ms = T0 // 1_000_000
    info_t = eng.table_info(now_ms)
    assert info_t.win_live == NKEYS, info_t.win_live

    rng = np.random.default_rng(11)
    shapes = (("distinct", keys[rng.permutation(NKEYS)[:M]]),
              ("zipf    ", keys[(rng.zipf(1.1, M) - 1) % NKEYS]),
              ("one key ", np.full(M, 12345, np.uint64)))
    ts = T0 + 1000 + np.arange(M, dtype=np.int64)
    ts_d = torch.from_numpy(ts).to(dev)
    n_d = torch.ones(M, dtype=torch.int64, device=dev)
    cfg_d = torch.zeros(M, dtype=torch.int32, device=dev)
    send = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    info = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    order = torch.empty(cap, dtype=torch.int32, device=dev)
    sms = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    res = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    status = torch.empty(M, dtype=torch.uint8, device=dev)
    outs = [torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev)
                                                              for _ in range(3)]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()

    emit(f"scripts/routed_refund_timing.py --repeats {args.repeats}: device ms between two events on the caller's "
         f"stream, world 1, read in place")
    emit(f"{M} refunds of n = 1 per step (bound m_max {cap}, rl_refund_max {eng.refund_max()}), "
         f"{info_t.win_live} live fixed-window counters in {info_t.win_capacity} slots, ts in order")
    for name, k in shapes:
        key_d = torch.from_numpy(k.view(np.int64)).to(dev)
        torch.cuda.synchronize()

        def front():
            router.pack(M, p(key_d), p(ts_d), p(n_d), p(cfg_d), p(send), p(info), p(slot), s)
            router.merge(p(send), p(info), p(order), p(sms), p(cnt), s)

        def engine():
            eng.refund_routed(cap, p(cnt), p(send), p(order), p(sms), p(res), s, s)

        def step():
            front()
            engine()
            router.unpack(M, p(slot), p(res), *[p(x) for x in outs], s)

        def array():
            eng.refund_device(M, p(key_d), p(ts_d), p(n_d), p(cfg_d), None, p(status), s)

        t_step = timed(step, args.repeats)
        done = int((outs[0] == rl_amd.REFUND_DONE).sum())
        ident = int(order[:1].cpu()[0]) == -1
        t_eng = timed(engine, args.repeats, before=front)
        t_arr = timed(array, args.repeats)
        torch.cuda.synchronize()
        assert eng.sync() == 0 and router.sync(None) == 0
        assert done == M and int((status == rl_amd.REFUND_DONE).sum()) == M and ident
        emit(f"  {name} ({np.unique(k).size:7d} targets)   "
             f"step   median {t_step[0]:7.3f} ms  min {t_step[1]:7.3f} ms   "
             f"engine call   median {t_eng[0]:7.3f} ms  min {t_eng[1]:7.3f} ms   "
             f"array form   median {t_arr[0]:7.3f} ms  min {t_arr[1]:7.3f} ms   "
             f"routed / array (medians) {t_eng[0] / t_arr[0]:5.2f}")
    eng.close()
    router.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
