#!/usr/bin/env python3
"""Device time of the three kinds of routed step (include/rl_route.h) on an
MI355X: decide, peek (k_peek_routed) and reset (k_reset_routed), at world 1
with the buckets and results read in place.

  tb_zipf   one step of 1M requests over the configs[1] table: token bucket,
            2^21 slots, 1M keys Zipf 1.1 (warmed by four decide batches of the
            same trace); the batch's ts are in order, so the merge leaves the
            RL_ORDER_IDENTITY form

step:   HIP events on the result stream around pack -> merge -> the engine's
        call -> unpack, all on that stream (the engine's kernels run on its own
        streams; the stream waits for them).
engine: the same events around the engine's call alone, the step's pack and
        merge complete before the first event: the kernel(s) plus two event
        hand-offs between streams.
Minimum and median of --repeats calls after one untimed call.  The reset step is
timed last (it deletes the keys; a repeat finds them deleted and stores the
same word again).  Bytes per request of a peek or reset step's engine call: 32
in (the record) + 32 out (the result record) + one 32 B table line.

  python scripts/routed_ops_timing.py [--out profiles/routed_ops_timing.txt]
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
import traces  # noqa: E402

M = 1_000_000
HBM_BYTES_PER_S = 8e12       # the peak the README's roofline uses


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
    g = traces.TokenBucketZipf(batch=M)
    router = rl_amd.Router(0, 1, M, M)
    cap = router.capacity
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1024, max_batch=cap)
    for a, L, W in g.configs:
        eng.register(a, L, W)
    for _ in range(4):
        eng.decide(*g.next_batch(), want_tokens=False)
    key, ts, n, cfg = g.next_batch()
    in_order = not bool(np.any(ts[1:] < ts[:-1]))
    ins = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                            np.ascontiguousarray(x)).to(dev) for x in (key, ts, n, cfg.view(np.int32))]
    send = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    info = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    order = torch.empty(cap, dtype=torch.int32, device=dev)
    sms = torch.empty(cap, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    res = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    outs = [torch.empty(M, dtype=torch.uint8, device=dev)] + [torch.empty(M, dtype=torch.int64, device=dev)
                                                              for _ in range(3)]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()

    def front():
        router.pack(M, *[p(t) for t in ins], p(send), p(info), p(slot), s)
        router.merge(p(send), p(info), p(order), p(sms), p(cnt), s)

    def back():
        router.unpack(M, p(slot), p(res), *[p(x) for x in outs], s)

    def engine(call):
        return lambda: call(cap, p(cnt), p(send), p(order), p(sms), p(res), s, s)

    def step(call):
        e = engine(call)
        return lambda: (front(), e(), back())

    info_t = eng.table_info(int(ts[-1]) // 1_000_000)
    emit(f"scripts/routed_ops_timing.py --repeats {args.repeats}: device ms between two events on the result stream, "
         f"world 1, read in place")
    emit(f"tb_zipf: {M} requests per step (bound m_max {cap}), tables {info_t.tb_capacity} + {info_t.win_capacity} "
         f"slots, {info_t.tb_used + info_t.win_used} keys present, ts in order: {in_order}")
    per_req = 32 + 32 + 32
    for name, call in (("decide", eng.decide_routed), ("peek  ", eng.peek_routed), ("reset ", eng.reset_routed)):
        t_step = timed(step(call), args.repeats)
        t_eng = timed(engine(call), args.repeats, before=front)
        torch.cuda.synchronize()
        assert eng.sync() == 0 and router.sync(None) == 0
        line = (f"  {name} step   median {t_step[0]:8.3f} ms   min {t_step[1]:8.3f} ms     "
                f"engine call   median {t_eng[0]:8.3f} ms   min {t_eng[1]:8.3f} ms")
        if name.strip() != "decide":
            line += (f"   {M / t_eng[1] / 1e3:7.1f} M/s   {per_req} B/request -> "
                     f"{per_req * M / (t_eng[1] * 1e-3) / 1e12:5.2f} TB/s = "
                     f"{100 * per_req * M / (t_eng[1] * 1e-3) / HBM_BYTES_PER_S:4.1f} % of 8 TB/s")
        emit(line)
    dec = outs[0].cpu().numpy()
    emit(f"  after the reset steps: {int((dec == rl_amd.RESET_DONE).sum())} of {M} statuses RL_RESET_DONE")
    eng.close()
    router.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
