"""Routed steps of the three kinds -- decide, peek, reset -- through
shard.RoutedPipeline on CPU (gloo): the routing kernels are their CPU
restatement (tests/route_ops.py) and the owner's engine is the Python oracle
(tests/routed_op_cases.py).  Every rank's results, every field of every
request, must equal ONE shared store that runs all ranks' steps in merge order:
a peek answers from the state the earlier steps left and changes nothing, a
reset deletes its keys for every later step.  tests/test_routed_ops_gpu.py runs
the HIP kernels and the engine."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

from tracegen import CONFIG_SETS

CONFIGS = CONFIG_SETS["mixed"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _outs(torch, batches):
    return [(torch.empty(b[0].size, dtype=torch.uint8),) + tuple(torch.empty(b[0].size, dtype=torch.int64)
                                                               for _ in range(3)) for b in batches]


def _pipeline(world, m, cap, sim, **kw):
    import route_ops
    import routed_op_cases as rc
    import shard
    ops = route_ops.NumpyRouteOps(world, cap)
    c = ops.capacity
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, world, c), world, m, "cpu", depth=4,
                                peek=rc.oracle_peek(sim, world, c), reset=rc.oracle_reset(sim, world, c), **kw)
    return ops, pipe


def _worker(rank, world, port, q, m=1500, cap=4096, exchange=None):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "distributed-rate-limiter_amd", "python"),
                    os.path.join(root, "tests")]
    import torch
    import torch.distributed as dist

    import routed_op_cases as rc
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ok, bad, ops = False, None, None
    try:
        sim = rc.new_sim(CONFIGS)
        pg_res = dist.new_group(backend="gloo")
        ops, pipe = _pipeline(world, m, cap, sim, pg_req=None, pg_res=pg_res, exchange=exchange)
        all_batches = [rc.rank_batches(r, CONFIGS, m=m) for r in range(world)]
        mine = all_batches[rank]
        ins = [rc.host_tensors(torch, bt) for bt in mine]
        outs = _outs(torch, mine)
        pipe.run(ins, outs, kinds=rc.KINDS)
        exp = rc.routed_expectations(all_batches, rc.KINDS, rank, CONFIGS, cap=ops.capacity)
        bad = rc.mismatches(outs, exp)
        ok = not bad
        nb = len(mine)
        # 3 collectives per step of any kind, and the one collective order
        ok = ok and pipe.exchange and pipe.collectives == 3 * nb and pipe.wait_s == 0.0
        want = [("req", 0)] + [x for b in range(1, nb) for x in (("req", b), ("res", b - 1))] + [("res", nb - 1)]
        ok = ok and list(pipe.order_log) == want
        # the cases are what they claim: every kind of row occurred and was compared
        dec = {b: outs[b][0].numpy() for b in range(nb)}
        peeks = np.concatenate([dec[b] for b in range(nb) if rc.KINDS[b] == rc.P])
        ok = ok and all((peeks == v).any() for v in (0, 1, 3))
        resets = dec[rc.KINDS.index(rc.R)]
        ok = ok and (resets == 3).any() and (resets == 1).any()
        ok = ok and ((resets == rc.DROPPED).any() == ops.overflow) and ((peeks == rc.DROPPED).any() == ops.overflow)
    finally:
        q.put((rank, ok, getattr(ops, "overflow", None), bad))
        dist.destroy_process_group()


def _run_ranks(world, **kw):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q), kwargs=kw) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in procs:
        r, ok, ov, bad = q.get(timeout=300)
        assert not bad, (r, bad)
        res[r] = (ok, ov)
    for p in procs:
        p.join(timeout=60)
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_routed_steps_of_three_kinds_match_one_shared_store(world):
    """kinds D P D R P D P, 1500 requests per rank and step over ~400 keys,
    skewed clocks, requests out of order: every field of every request on
    every rank, 3 collectives per step, the one collective order"""
    assert _run_ranks(world) == {r: (True, False) for r in range(world)}


def test_routed_peek_and_reset_steps_bucket_overflow():
    """buckets smaller than a rank's requests for one owner, in a peek step and
    in a reset step as in the decide steps: the requests past the capacity
    come back RL_DROPPED, a dropped reset was not applied -- the later decide
    and peek steps equal the shared store that skipped them"""
    assert _run_ranks(2, m=5000, cap=2048) == {0: (True, True), 1: (True, True)}


def test_routed_steps_world1_in_place():
    """world 1 without the exchange: no collective, the same kinds; the reset
    step leaves n out (the pipeline packs zeros of its own)"""
    import torch

    import routed_op_cases as rc
    sim = rc.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 1500, 4096, sim)
    assert not pipe.exchange
    mine = rc.rank_batches(1, CONFIGS, reset_n_none=True, peeks_in_order=True)
    assert mine[rc.KINDS.index(rc.R)][2] is None
    outs = _outs(torch, mine)
    pipe.run([rc.host_tensors(torch, bt) for bt in mine], outs, kinds=rc.KINDS)
    assert pipe.collectives == 0 and not ops.overflow
    assert not rc.mismatches(outs, rc.routed_expectations([mine], rc.KINDS, 0, CONFIGS))


def test_routed_peek_changes_nothing_and_reset_deletes():
    """the point of the two kinds, on one key: a peek step repeated gives the
    same answer and leaves the next decide unchanged; a reset step gives the
    key its full quota back"""
    import torch

    import routed_op_cases as rc
    from tracegen import T0
    sim = rc.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 8, 2048, sim)
    key = np.full(4, 10, np.uint64)                      # cfg 10: fixed window, 100 per 60 s
    cfg = np.full(4, 10, np.uint32)
    ts = T0 + np.arange(4, dtype=np.int64)
    kinds = [rc.D, rc.P, rc.P, rc.D, rc.R, rc.P]
    ns = [np.full(4, 20, np.int64), np.zeros(4, np.int64), np.zeros(4, np.int64), np.full(4, 1, np.int64), None,
          np.zeros(4, np.int64)]
    batches = [(key, ts + 10 * b, n, cfg) for b, n in enumerate(ns)]
    outs = _outs(torch, batches)
    pipe.run([rc.host_tensors(torch, bt) for bt in batches], outs, kinds=kinds)
    rem = [o[1].numpy().tolist() for o in outs]
    assert rem[0] == [80, 60, 40, 20]
    assert rem[1] == rem[2] == [20, 20, 20, 20]          # how much is left, twice
    assert rem[3] == [19, 18, 17, 16]                    # the peeks took nothing
    assert outs[4][0].numpy().tolist() == [1, 1, 1, 1]   # RL_RESET_DONE
    assert rem[5] == [100, 100, 100, 100]
    assert not rc.mismatches(outs, rc.routed_expectations([batches], kinds, 0, CONFIGS))


def test_routed_step_of_a_kind_without_its_callable():
    """a peek or reset step on a pipeline built without that callable raises
    ValueError before anything is enqueued; a decide step still works after"""
    import torch

    import route_ops
    import routed_op_cases as rc
    import shard
    sim = rc.new_sim(CONFIGS)
    ops = route_ops.NumpyRouteOps(1, 4096)
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, 1, ops.capacity), 1, 1500, "cpu", depth=4)
    mine = rc.rank_batches(0, CONFIGS, kinds=[rc.D])
    ins = rc.host_tensors(torch, mine[0])
    outs = _outs(torch, mine)
    calls = []
    ops.pack = lambda *a, _pack=ops.pack: (calls.append("pack"), _pack(*a))[1]
    for op in (shard.OP_PEEK, shard.OP_RESET, 7):
        with pytest.raises(ValueError):
            pipe.step(0, *ins, *outs[0], op=op)
    with pytest.raises(ValueError):
        pipe.step(0, ins[0], ins[1], None, ins[3], *outs[0])          # only a reset step may leave n out
    assert calls == [] and not pipe._pend and len(pipe.order_log) == 0
    pipe.step(0, *ins, *outs[0])
    pipe.flush()
    assert calls == ["pack"]
    assert not rc.mismatches(outs, rc.routed_expectations([mine], [rc.D], 0, CONFIGS))
