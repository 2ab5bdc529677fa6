#!/usr/bin/env python3
"""Device time of read-only queries (rl_peek_batch_device, k_peek) on an
MI355X, next to the same batch through decide and to the grouping's k_probe,
which also reads one random table line per request.

  tb_zipf   1M peeks over the configs[1] table: token bucket, 2^21 slots, 1M
            keys Zipf 1.1 (warmed by four decide batches of the same trace)
  fw_2e26   1M peeks over a 2^26-slot window table (4 GiB) with 8M keys present,
            uniform keys

peek: HIP events on the caller's stream around one rl_peek_batch_device call
(the stream waits for k_peek, so the interval is the kernel plus two event
hand-offs between streams); median and minimum of --repeats calls after one
untimed call.  decide: the same events around rl_decide_batch_device of the
same batch (every stage, three streams).  k_probe: the engine's own stage timer
(rl_engine_stage_times, stage 0) of those decide calls.  Bytes per request:
28 in (key 8, ts 8, n 8, cfg 4) + 33 out (decision 1, four 8-byte results) +
one table line (32 B token bucket, 64 B window).

  python scripts/peek_timing.py [--out profiles/peek_timing.txt]
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

NS = 1_000_000_000
M = 1_000_000
HBM_BYTES_PER_S = 8e12       # the peak the README's roofline uses


def to_dev(key, ts, n, cfg, dev):
    ins = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                            np.ascontiguousarray(x)).to(dev) for x in (key, ts, n, cfg.view(np.int32))]
    m = key.size
    outs = ([torch.empty(m, dtype=torch.uint8, device=dev)] +
            [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(m, dtype=torch.float64, device=dev)])
    return ins, outs


def timed(fn, repeats):
    """ms between two events on the current stream around fn()"""
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return statistics.median(t), min(t)


def scenario(name, eng, warm, batch, line_bytes, repeats, emit):
    dev = torch.device("cuda", 0)
    for b in warm:
        eng.decide(*b, want_tokens=False)
    ins, outs = to_dev(*batch, dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    args = (ins[0].numel(), ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), None,
            *[x.data_ptr() for x in outs], stream)
    t_peek = timed(lambda: eng.peek_device(*args), repeats)
    eng.set_timing(2)
    eng.stage_times()
    t_dec = timed(lambda: eng.decide_device(*args), repeats)
    torch.cuda.synchronize()
    assert eng.sync() == 0
    ms, nb = eng.stage_times()
    eng.set_timing(0)
    probe_ms = ms[0] / max(nb, 1)
    info = eng.table_info(int(batch[1][-1]) // 1_000_000)
    per_req = 28 + 33 + line_bytes
    emit(f"{name}: {M} requests, tables {info.tb_capacity} + {info.win_capacity} slots, "
         f"{info.tb_used + info.win_used} keys present")
    emit(f"  peek (k_peek)       median {t_peek[0]:8.3f} ms   min {t_peek[1]:8.3f} ms   "
         f"{M / t_peek[1] / 1e3:7.1f} M peeks/s   {per_req} B/request -> {per_req * M / (t_peek[1] * 1e-3) / 1e12:5.2f} TB/s "
         f"= {100 * per_req * M / (t_peek[1] * 1e-3) / HBM_BYTES_PER_S:4.1f} % of 8 TB/s")
    emit(f"  decide (all stages) median {t_dec[0]:8.3f} ms   min {t_dec[1]:8.3f} ms")
    emit(f"  k_probe (stage timer, mean of {nb} batches) {probe_ms:8.3f} ms    k_peek / k_probe {t_peek[1] / probe_ms:5.2f}x")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"scripts/peek_timing.py --repeats {args.repeats}: device ms between two events on the caller's stream")
    # configs[1]
    g = traces.TokenBucketZipf(batch=M)
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1024, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE)
    for a, L, W in g.configs:
        eng.register(a, L, W)
    warm = [g.next_batch() for _ in range(4)]
    scenario("tb_zipf", eng, warm, g.next_batch(), 32, args.repeats, emit)
    eng.close()
    # 2^26-slot window table, uniform keys
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1024, win_capacity=1 << 26, max_batch=M,
                        flags=rl_amd.OPT_PIPELINE, spill_capacity=1024)
    eng.register(rl_amd.FIXED_WINDOW, 100, 3600 * NS)
    rng = np.random.default_rng(7)
    nkeys = 8 * M
    t0 = traces.T0
    warm = [(np.arange(i * M, (i + 1) * M, dtype=np.uint64), np.full(M, t0 + i, np.int64), np.ones(M, np.int64),
             np.zeros(M, np.uint32)) for i in range(nkeys // M)]
    batch = (rng.integers(0, nkeys, M).astype(np.uint64), np.full(M, t0 + 1000, np.int64), np.ones(M, np.int64),
             np.zeros(M, np.uint32))
    scenario("fw_2e26", eng, warm, batch, 64, args.repeats, emit)
    eng.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
