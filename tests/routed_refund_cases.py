"""Cases and expectations for routed steps of four kinds -- decide, peek, reset
and refund (include/rl_route.h, shard.RoutedPipeline) -- TEST INFRASTRUCTURE
ONLY.

Built on routed_op_cases (the three earlier kinds) and refund_cases (the refund
contract on the Python oracle's keyspace).

  oracle_refund           rl_refund_routed_device over host pointers: the
      merged batch as ONE refund_cases.apply_refunds call
  routed_expectations     routed_op_cases.routed_expectations' merge restated
      with a refund kind: ONE shared store over every rank's steps, a refund
      step one apply_refunds call over the step's merged batch; optionally the
      coverage of the refund steps
  rank_batches            one app server's steps of the kinds D F P D F R F P D
  run_ranks               fresh processes, one per rank, that always answer and
      never outlive the test
"""
import importlib
import os
import queue
import socket
import time
import traceback

import numpy as np

import routed_op_cases as rc
import shard
from peek_cases import KEY_RESERVED
from refund_cases import DONE, INVALID, NOKEY, apply_refunds  # noqa: F401  (the statuses: for the tests)
from route_ops import _arr
from tracegen import T0

D, P, R, F = shard.OP_DECIDE, shard.OP_PEEK, shard.OP_RESET, shard.OP_REFUND
KINDS = [D, F, P, D, F, R, F, P, D]
DROPPED = rc.DROPPED
BAD_CFG = rc.BAD_CFG

new_sim, host_tensors, mismatches = rc.new_sim, rc.host_tensors, rc.mismatches


def refund_rows(sim, key, ts, n, cfg, sms):
    """the result records of one merged refund step, in merge order, applied to
    sim as one call -> (rows, apply_refunds' info)"""
    m = len(key)
    out = np.zeros((m, 4), np.int64)
    if m == 0:
        return out, {"targets": {}, "deleted": [], "expired": []}
    st, info = apply_refunds(sim, key, ts, n, cfg, sms)
    out[:, 0] = st
    return out, info


def step_rows(sim, op, key, ts, n, cfg, sms):
    if op == F:
        return refund_rows(sim, key, ts, n, cfg, sms)[0]
    return rc.step_rows(sim, op, key, ts, n, cfg, sms)


def oracle_refund(sim, world, cap):
    """rl_refund_routed_device over host pointers: request p is recv[order[p]]
    at store clock sms[p]; the merged batch is one refund call.  Status into
    field 0, zeros into the others."""
    def call(m_max, count, recv, order, sms, res, stream, out_stream=None):
        cnt = int(_arr(count, 1, np.int32)[0])
        if cnt == 0:
            return
        o = _arr(order, cnt, np.int32).astype(np.int64)
        rec = _arr(recv, 4 * world * cap, np.int64).reshape(world * cap, 4)[o]
        rows = refund_rows(sim, rec[:, 0].view(np.uint64), rec[:, 1], rec[:, 2],
                           (rec[:, 3] & 0xffffffff).astype(np.uint32), _arr(sms, cnt, np.int64))[0]
        _arr(res, 4 * world * cap, np.int64).reshape(world * cap, 4)[o] = rows
    return call


def new_cover():
    return {"status": set(), "multi_rank": 0, "del": 0, "decrby": 0, "clamped": 0, "dropped": 0}


def routed_expectations(all_batches, kinds, rank, configs, profile=0, cap=None, cover=None):
    """routed_op_cases.routed_expectations with the refund kind: all_batches[r][b]
    = (key, ts, n or None, cfg); per step, `rank`'s four result fields in its
    batch order.  A refund step is ONE apply_refunds call over the merged batch
    (a request past `cap` for its owner is dropped: RL_DROPPED, never applied,
    but it still advances the clock).  cover (new_cover()): what the refund
    steps met -- statuses, targets with contributors of two or more ranks,
    DELs, DECRBYs, clamped buckets."""
    ref = new_sim(configs, profile)
    world = len(all_batches)
    outs = []
    clock = -(1 << 63)
    for b, op in enumerate(kinds):
        parts = [all_batches[r][b] for r in range(world)]
        parts = [(p[0], p[1], np.zeros(p[0].size, np.int64) if p[2] is None else p[2], p[3]) for p in parts]
        U = [np.concatenate([p[f] for p in parts]) for f in range(4)]
        src = np.concatenate([np.full(p[0].size, r) for r, p in enumerate(parts)])
        pos = np.concatenate([np.arange(p[0].size) for p in parts])
        own = shard.owner_of(U[0].astype(np.uint64), world)
        arrive = np.empty_like(U[1])
        sent = np.ones(U[0].size, bool)
        for r in range(world):
            for w in range(world):
                idx = np.nonzero((src == r) & (own == w))[0]
                if cap is not None and idx.size > cap:
                    sent[idx[cap:]] = False
                    idx = idx[:cap]
                if idx.size:
                    arrive[idx] = np.maximum.accumulate(U[1][idx])
        live = np.nonzero(sent)[0]
        o = live[np.lexsort((pos[live], src[live], arrive[live]))]
        sms = np.maximum(arrive[o] // 1_000_000, clock)
        if U[1].size:
            clock = max(clock, int(U[1].max()) // 1_000_000)
        full = np.zeros((U[0].size, 4), np.int64)
        full[:, 0] = DROPPED
        if op == F:
            rows, info = refund_rows(ref, U[0][o], U[1][o], U[2][o], U[3][o], sms)
            full[o] = rows
            if cover is not None:
                cover["status"] |= set(rows[:, 0].tolist())
                cover["dropped"] += int((~sent).sum())
                gone = set(info["deleted"])
                cover["del"] += len(gone)
                for name, idx in info["targets"].items():
                    if len({int(src[o[i]]) for i in idx}) >= 2:
                        cover["multi_rank"] += 1
                    if name.startswith("tb:"):
                        limit = float(ref.cfgs[int(U[3][o[idx[0]]])][1])
                        cover["clamped"] += ref.db[name][0][0] == limit
                    elif name not in gone:
                        cover["decrby"] += 1
        else:
            full[o] = rc.step_rows(ref, op, U[0][o], U[1][o], U[2][o], U[3][o], sms)
        mine = src == rank
        outs.append([full[mine, f] for f in range(4)])
    return outs


def rank_batches(rank, configs, kinds=KINDS, m=1500, nkeys=400, reset_n_none=False, in_order=False):
    """one app server's steps, as routed_op_cases.rank_batches (its own arrival
    order, its clock skewed against the other ranks', some requests out of time
    order and some stamped windows behind, keys shared by all ranks; in_order:
    the peek and refund steps' ts sorted, which at world 1 takes the merge's
    RL_ORDER_IDENTITY form), with
      refund  half of them the (key, ts, cfg) of requests of this rank's last
              decide step (the windows those charged, wherever they live), the
              rest at the rank's current time; one refund 40 times in a row;
              keys never seen; n small or up to 2^40; a few n <= 0, unknown
              cfgs and the reserved key id"""
    rng = np.random.default_rng(5200 + rank)
    t = T0 + [0, -3_000_000_000, 1_200_000_000, -700_000_000][rank % 4]
    ncfg = len(configs)
    out, last = [], None
    for op in kinds:
        key = rng.integers(0, nkeys, m).astype(np.uint64)
        ts = t + np.cumsum(rng.choice([0, 1, 500, 90_000, 2_000_000], m)).astype(np.int64)
        ts[rng.random(m) < 0.05] -= 5_000_000
        ts += rng.choice([0, 0, 0, 0, 0, 0, 0, 0, -7_000_000_000, -130_000_000_000], m)
        t = int(ts.max()) + 1
        if op == D:
            n = rng.choice([1, 1, 2, 5], m).astype(np.int64)
        elif op == P:
            n = rng.choice([0, 1, 2, 5], m).astype(np.int64)
            n[rng.random(m) < 0.01] = -1
        elif op == F:
            n = rng.choice([1, 1, 1, 2, 3], m).astype(np.int64)
            big = rng.random(m) < 0.15
            n[big] = rng.integers(1, (1 << 40) + 1, int(big.sum()))
            n[0], n[1] = 1, 1 << 40
        else:
            n = rng.integers(-3, 1 << 40, m).astype(np.int64)
        if op in (R, F):
            if last is not None:
                pick = rng.integers(0, last[0].size, m // 2)
                key[:m // 2], ts[:m // 2] = last[0][pick], last[1][pick]
            key[m // 2:m // 2 + 40] = key[m // 2 - 1]                 # one target many times in a row
            ts[m // 2:m // 2 + 40] = ts[m // 2 - 1]
            key[-30:] = np.arange(30, dtype=np.uint64) + np.uint64(10 * nkeys)   # never seen
        if op == F:
            n[rng.random(m) < 0.01] = rng.choice([0, -1, -5])
        if in_order and op in (P, F):
            o = np.argsort(ts, kind="stable")
            key, ts, n = key[o], ts[o], n[o]
        cfg = (key % np.uint64(ncfg)).astype(np.uint32)
        if op != D:
            cfg[rng.random(m) < 0.01] = BAD_CFG
            key[rng.random(m) < 0.01] = np.uint64(KEY_RESERVED)
        if op == D:
            last = (key, ts)
        out.append((key, ts, None if (op == R and reset_n_none) else n, cfg))
    return out


def _rank_entry(rank, world, port, q, module, name, kwargs):
    """a rank's process: module.name(rank, world, **kwargs) -> (ok, info).
    Whatever happens -- an import that fails included -- the rank answers
    (rank, ok, info), with the traceback as info when it raised."""
    ok, info = False, None
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        ok, info = getattr(importlib.import_module(module), name)(rank, world, **kwargs)
    except BaseException:
        ok, info = False, traceback.format_exc()
    finally:
        q.put((rank, bool(ok), info))
        try:
            import torch.distributed as dist
            if dist.is_initialized():
                dist.destroy_process_group()
        except Exception:
            pass


def run_ranks(module, name, world, limit=240, **kwargs):
    """module.name(rank, world, **kwargs) in `world` freshly spawned processes
    -> {rank: (ok, info)}.  Returns as soon as every rank has answered; stops
    waiting when a rank has answered a failure or has ended without an answer
    (the others may then sit in a collective for good), or at `limit` seconds.
    No child is left running."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_rank_entry, args=(r, world, port, q, module, name, kwargs)) for r in range(world)]
    for p in procs:
        p.start()
    res, why = {}, None
    deadline = time.monotonic() + limit
    try:
        while len(res) < world and why is None:
            ended = [r for r, p in enumerate(procs) if r not in res and p.exitcode is not None]
            try:
                r, ok, info = q.get(timeout=2.0 if ended else 0.5)
                res[r] = (ok, info)
                if not ok:
                    why = f"rank {r} failed"
            except queue.Empty:
                if ended:   # looked once more after its end: it left no answer
                    why = f"ranks {ended} ended without an answer, exit codes {[procs[r].exitcode for r in ended]}"
                elif time.monotonic() > deadline:
                    why = f"ranks {[r for r in range(world) if r not in res]} still running after {limit} s"
    finally:
        for p in procs:
            if why is None:
                p.join(timeout=30)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
            if p.is_alive():
                p.kill()
                p.join()
    assert why is None, (why, res)
    return res
