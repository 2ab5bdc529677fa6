#!/usr/bin/env python3
"""Device time of the charge step of the routed path (include/rl_route.h:
k_charge_ask_routed, the routed decide on the engine's scratch,
k_charge_finish_routed) on an MI355X, at world 1 with the buckets and results
read in place, beside rl_charge_batch_device (k_charge_ask, the decide,
k_charge_finish) on the same requests in the same session.

One step of 1M charges (n = 1, ts in order: the merge leaves the
RL_ORDER_IDENTITY form) on 1M distinct keys, a third of them token buckets, a
third fixed windows and a third sliding windows, every limit 10^12 so that
every repeat is charged in full.

step:    HIP events on the caller's stream around pack -> merge -> the engine's
         call -> unpack, all on that stream (the engine's kernels run on its own
         streams; the caller's stream waits for the finish).
engine:  the same events around the engine's call alone, the step's pack and
         merge complete before the first event.
array:   the same events around rl_charge_batch_device on the same requests as
         arrays.
Median and minimum of --repeats calls after one untimed call.  No threshold is
attached to these figures.

  python scripts/routed_charge_timing.py [--out profiles/routed_charge_timing.txt]
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
T0 = 1_760_000_000_000_000_000
NS = 1_000_000_000
LIMIT = 10 ** 12


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
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 20, win_capacity=1 << 21, max_batch=cap)
    for alg in (1, 3, 2):                     # cfg 0: token bucket, 1: fixed window, 2: sliding window
        eng.register(alg, LIMIT, 3600 * NS)
    assert eng.charge_max() >= M
    rng = np.random.default_rng(13)
    keys = (np.arange(1, M + 1, dtype=np.uint64))[rng.permutation(M)]
    cfg = (keys % np.uint64(3)).astype(np.uint32)
    ts = T0 + 1000 + np.arange(M, dtype=np.int64)
    # the keys exist before the first timed call
    eng.decide(keys, np.full(M, T0), np.ones(M, np.int64), cfg, want_tokens=False)

    key_d = torch.from_numpy(keys.view(np.int64)).to(dev)
    ts_d = torch.from_numpy(ts).to(dev)
    n_d = torch.ones(M, dtype=torch.int64, device=dev)
    cfg_d = torch.from_numpy(cfg.view(np.int32)).to(dev)
    send = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    info = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    order = torch.empty(cap, dtype=torch.int32, device=dev)
    sms = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    res = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    outs = [torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev)
                                                              for _ in range(3)]
    arr = [torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev)
                                                             for _ in range(3)]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()

    def front():
        router.pack(M, p(key_d), p(ts_d), p(n_d), p(cfg_d), p(send), p(info), p(slot), s)
        router.merge(p(send), p(info), p(order), p(sms), p(cnt), s)

    def engine():
        eng.charge_routed(cap, p(cnt), p(send), p(order), p(sms), p(res), s, s)

    def step():
        front()
        engine()
        router.unpack(M, p(slot), p(res), *[p(x) for x in outs], s)

    def array():
        # decision, charged, remaining, reset_at; no tokens, as the routed result
        eng.charge_device(M, p(key_d), p(ts_d), p(n_d), p(cfg_d), None, p(arr[0]), p(arr[1]), p(arr[2]), p(arr[3]),
                          None, s)

    emit(f"scripts/routed_charge_timing.py --repeats {args.repeats}: device ms between two events on the caller's "
         f"stream, world 1, read in place")
    emit(f"{M} charges of n = 1 per step on {M} distinct keys (bound m_max {cap}, rl_charge_max {eng.charge_max()}): "
         f"{int((cfg == 0).sum())} token buckets, {int((cfg == 1).sum())} fixed windows, "
         f"{int((cfg == 2).sum())} sliding windows, ts in order")
    t_step = timed(step, args.repeats)
    full = int(((outs[0] == 1) & (outs[2] == 1)).sum())              # RL_ALLOWED, charged 1
    ident = int(order[:1].cpu()[0]) == -1
    t_eng = timed(engine, args.repeats, before=front)
    t_arr = timed(array, args.repeats)
    torch.cuda.synchronize()
    assert eng.sync() == 0 and router.sync(None) == 0
    assert full == M and int(((arr[0] == 1) & (arr[1] == 1)).sum()) == M and ident
    emit(f"  step          median {t_step[0]:7.3f} ms  min {t_step[1]:7.3f} ms")
    emit(f"  engine call   median {t_eng[0]:7.3f} ms  min {t_eng[1]:7.3f} ms")
    emit(f"  array form    median {t_arr[0]:7.3f} ms  min {t_arr[1]:7.3f} ms")
    emit(f"  routed engine call / array form (medians) {t_eng[0] / t_arr[0]:5.2f}, "
         f"difference {1000 * (t_eng[0] - t_arr[0]):7.1f} us")
    eng.close()
    router.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
