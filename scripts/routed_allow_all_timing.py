#!/usr/bin/env python3
"""Device time of the routed AllowAll (shard.RoutedPipeline.allow_all,
include/rl_route.h) on an MI355X at world 1 with the buckets and
results read in place, at M = 3 * (2^20 // 3) members in one call.

The members are §10k's (scripts/allow_all_timing.py): groups of three -- a token
bucket, a fixed window and a sliding window of one user (key ids 3u, 3u + 1, 3u +
2).  A group fails when its bucket member asks for more than the bucket holds (it
is denied and takes nothing); its two window members were allowed and are given
back.  The share of failing groups is 0 %, 10 % and 100 %.  Per share, in one
session on the same arrays:

  compound   allow_all: decide step, settle, refund step packed with pack_sel
  by hand    the same without the selection: a decide step, the settle, and a
             refund step packed with Router.pack of all M members (n = g, so a
             member with nothing to give back travels as an INVALID request);
             the host round trip a caller without the settle on the device would
             add is not in this figure
  engine     Engine.allow_all_device on the same members (one engine call)
  count      the merged refund step's request count with pack and with pack_sel

and last rl_route_pack_sel with every request selected against rl_route_pack on
the same M requests.  HIP events on the caller's stream: the pipeline's request
stream waits for the first event and the caller's stream waits for the result
stream before the second.  Median and minimum of --repeats calls after one
untimed call.  No threshold is attached to these figures.

  python scripts/routed_allow_all_timing.py [--out profiles/routed_allow_all_timing.txt]
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
import shard  # noqa: E402

NS = 1_000_000_000
T0 = 1_760_000_000 * NS
USERS = (1 << 20) // 3
M = 3 * USERS
LIMIT = 1 << 50


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
    cur = torch.cuda.current_stream(dev)
    router = rl_amd.Router(0, 1, M, M)
    cap = router.capacity
    eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=1 << 21, win_capacity=1 << 22, max_batch=cap,
                        flags=rl_amd.OPT_PIPELINE)
    assert eng.allow_all_max() >= M
    for alg in (rl_amd.TOKEN_BUCKET, rl_amd.FIXED_WINDOW, rl_amd.SLIDING_WINDOW):
        eng.register(alg, LIMIT, 3600 * NS)
    pipe = shard.RoutedPipeline(router, eng.decide_routed, 1, M, "cuda:0", decide_ev=eng.decide_routed_ev,
                                refund=eng.refund_routed, refund_ev=eng.refund_routed_ev,
                                settle=eng.allow_all_settle)
    key = np.arange(M, dtype=np.uint64)
    cfg = (key % np.uint64(3)).astype(np.uint32)
    first = (cfg == 0).astype(np.uint8)
    rng = np.random.default_rng(5)
    to_dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else
                                        x.view(np.int32) if x.dtype == np.uint32 else x).to(dev)
    d_key, d_cfg, d_first = to_dev(key), to_dev(cfg), to_dev(first)
    d_ts = torch.full((M,), T0 + 1000, dtype=torch.int64, device=dev)
    u8 = lambda: torch.empty(M, dtype=torch.uint8, device=dev)
    i64 = lambda: torch.empty(M, dtype=torch.int64, device=dev)
    dec, verdict, rollback, sel = u8(), u8(), u8(), u8()
    rem, retry, reset, g = i64(), i64(), i64(), i64()
    tok = torch.empty(M, dtype=torch.float64, device=dev)
    p = lambda t: t.data_ptr()
    step_no = [0]

    def timed(fn):
        """ms between two events on the caller's stream around fn(): R starts
        after the first, the caller's stream has waited for U at the second"""
        t = []
        for i in range(args.repeats + 1):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cur)
            pipe.R.wait_event(a)
            fn()
            cur.wait_stream(pipe.U)
            b.record(cur)
            b.synchronize()
            if i:
                t.append(a.elapsed_time(b))
        return statistics.median(t), min(t)

    def refund_count():
        torch.cuda.synchronize()
        return int(pipe.slots[(step_no[0] - 1) % pipe.depth]["count"].cpu()[0])

    emit(f"scripts/routed_allow_all_timing.py --repeats {args.repeats}: device ms between two events on the caller's "
         f"stream, world 1, read in place")
    emit(f"M = {M} members, {USERS} groups of 3 (TB + FW + SW of one user), buckets of {cap}, tables of 2^21 / 2^22 "
         f"slots")
    # every key exists and holds taken units before anything is timed
    eng.decide(key, np.full(M, T0, np.int64), np.full(M, 1 << 30, np.int64), cfg, want_tokens=False)
    for share in (0.0, 0.1, 1.0):
        n = np.ones(M, np.int64)
        fail = rng.random(USERS) < share
        n[0::3][fail] = LIMIT + 1                     # the bucket member of a failing group
        d_n = to_dev(n)
        back = 2 * int(fail.sum())
        torch.cuda.synchronize()

        def compound():
            pipe.allow_all(step_no[0], d_key, d_ts, d_n, d_cfg, d_first, dec, rem, retry, reset, verdict, rollback)
            pipe.flush()
            step_no[0] += 2

        def by_hand():
            pipe.step(step_no[0], d_key, d_ts, d_n, d_cfg, dec, rem, retry, reset)
            pipe.flush()
            with torch.cuda.stream(pipe.U):
                eng.allow_all_settle(M, p(d_first), p(d_cfg), p(d_n), p(dec), p(verdict), p(g), p(sel),
                                     pipe.U.cuda_stream)
            pipe.R.wait_stream(pipe.U)
            pipe.step(step_no[0] + 1, d_key, d_ts, g, d_cfg, rollback, rem, retry, reset, op=shard.OP_REFUND)
            pipe.flush()
            step_no[0] += 2

        def engine():
            eng.allow_all_device(M, p(d_key), p(d_ts), p(d_n), p(d_cfg), None, p(d_first), p(dec), p(rem), p(retry),
                                 p(reset), p(tok), p(verdict), p(rollback), cur.cuda_stream)

        t_c = timed(compound)
        c_sel = refund_count()
        v, rb = verdict.cpu().numpy(), rollback.cpu().numpy()
        assert int((v[0::3] != rl_amd.ALLOWED).sum()) == int(fail.sum())
        assert int((rb == rl_amd.REFUND_DONE).sum()) == back and int((rb == rl_amd.INVALID).sum()) == M - back
        t_h = timed(by_hand)
        c_all = refund_count()
        assert int((rollback == rl_amd.REFUND_DONE).sum()) == back
        t_e = timed(engine)
        torch.cuda.synchronize()
        assert int((rollback == rl_amd.REFUND_DONE).sum()) == back
        assert eng.sync() == 0 and router.sync(None) == 0
        assert c_sel == back and c_all == M
        emit(f"  {100 * share:5.1f} % of the groups fail ({back:7d} give-backs)   "
             f"compound   median {t_c[0]:7.3f} ms  min {t_c[1]:7.3f} ms   "
             f"by hand (pack of all M)   median {t_h[0]:7.3f} ms  min {t_h[1]:7.3f} ms   "
             f"Engine.allow_all_device   median {t_e[0]:7.3f} ms  min {t_e[1]:7.3f} ms   "
             f"refund step count: pack {c_all}, pack_sel {c_sel}")

    # the selection's cost in the pack: every request selected against the plain pack
    send = torch.empty((cap, 4), dtype=torch.int64, device=dev)
    info = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    slot = torch.empty(M, dtype=torch.int32, device=dev)
    ones = torch.ones(M, dtype=torch.uint8, device=dev)
    d_one = torch.ones(M, dtype=torch.int64, device=dev)
    s = cur.cuda_stream
    torch.cuda.synchronize()
    res = {}
    for name, fn in (("pack", lambda: router.pack(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), p(send), p(info), p(slot), s)),
                     ("pack_sel, all ones", lambda: router.pack_sel(M, p(d_key), p(d_ts), p(d_one), p(d_cfg), p(ones),
                                                                    p(send), p(info), p(slot), s))):
        t = []
        for i in range(args.repeats + 1):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(cur)
            fn()
            b.record(cur)
            b.synchronize()
            if i:
                t.append(a.elapsed_time(b))
        res[name] = (statistics.median(t), min(t))
    emit(f"  the pack alone, {M} requests:   " + "   ".join(f"{k}   median {v[0]:6.3f} ms  min {v[1]:6.3f} ms"
                                                          for k, v in res.items()))
    assert router.sync(None) == 0
    del pipe
    eng.close()
    router.close()
    rl_amd.release_dedicated_streams()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
