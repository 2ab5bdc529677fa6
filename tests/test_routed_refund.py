"""Routed refund steps (shard.OP_REFUND) through shard.RoutedPipeline on CPU
(gloo): the routing kernels are their CPU restatement (tests/route_ops.py) and
the owner's engine is the Python oracle (tests/routed_refund_cases.py).  Every
rank's results of the steps D F P D F R F P D must equal ONE shared store that
runs all ranks' steps in merge order, a refund step as ONE refund call over the
merged batch: all ranks' refunds of one target are summed and applied once.
tests/test_routed_refund_gpu.py runs the HIP kernels and the engine."""
import inspect

import numpy as np
import pytest

from tracegen import CONFIG_SETS, NS, T0

CONFIGS = CONFIG_SETS["mixed"]


def _outs(torch, batches):
    return [(torch.empty(b[0].size, dtype=torch.uint8),) + tuple(torch.empty(b[0].size, dtype=torch.int64)
                                                               for _ in range(3)) for b in batches]


def _pipeline(world, m, cap, sim, **kw):
    import route_ops
    import routed_op_cases as rc
    import routed_refund_cases as rf
    import shard
    ops = route_ops.NumpyRouteOps(world, cap)
    c = ops.capacity
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, world, c), world, m, "cpu", depth=4,
                                peek=rc.oracle_peek(sim, world, c), reset=rc.oracle_reset(sim, world, c),
                                refund=rf.oracle_refund(sim, world, c), **kw)
    return ops, pipe


# --- the case is what it claims ------------------------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3])
def test_case_coverage(world):
    """the nine steps' refunds meet DONE, NOKEY and INVALID, a target with
    contributors from two ranks (world > 1), a DEL, a DECRBY and a clamped
    bucket; n runs from 1 to 2^40 with some n <= 0"""
    import routed_refund_cases as rf
    assert rf.KINDS == [rf.D, rf.F, rf.P, rf.D, rf.F, rf.R, rf.F, rf.P, rf.D]
    all_batches = [rf.rank_batches(r, CONFIGS) for r in range(world)]
    cover = rf.new_cover()
    rf.routed_expectations(all_batches, rf.KINDS, 0, CONFIGS, cover=cover)
    assert cover["status"] == {rf.DONE, rf.NOKEY, rf.INVALID}
    assert cover["del"] > 0 and cover["decrby"] > 0 and cover["clamped"] > 0 and cover["dropped"] == 0
    if world > 1:
        assert cover["multi_rank"] > 0
    n = np.concatenate([b[2] for b, k in zip(all_batches[0], rf.KINDS) if k == rf.F])
    assert n.max() == 1 << 40 and (n == 1).any() and (n <= 0).any()
    key = np.concatenate([b[0] for b, k in zip(all_batches[0], rf.KINDS) if k == rf.F])
    assert (key == np.uint64((1 << 64) - 1)).any()


# --- worlds 2 and 3 over gloo -----------------------------------------------------------

def _worker(rank, world, m=1500, cap=4096):
    """one rank (routed_refund_cases.run_ranks) -> (ok, (overflow, mismatches))"""
    import torch
    import torch.distributed as dist

    import routed_refund_cases as rf
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sim = rf.new_sim(CONFIGS)
    pg_res = dist.new_group(backend="gloo")
    ops, pipe = _pipeline(world, m, cap, sim, pg_req=None, pg_res=pg_res)
    all_batches = [rf.rank_batches(r, CONFIGS, m=m) for r in range(world)]
    mine = all_batches[rank]
    outs = _outs(torch, mine)
    pipe.run([rf.host_tensors(torch, bt) for bt in mine], outs, kinds=rf.KINDS)
    cover = rf.new_cover()
    exp = rf.routed_expectations(all_batches, rf.KINDS, rank, CONFIGS, cap=ops.capacity, cover=cover)
    bad = rf.mismatches(outs, exp)
    ok = not bad
    nb = len(mine)
    # 3 collectives per step of any kind, and the one collective order
    ok = ok and pipe.exchange and pipe.collectives == 3 * nb and pipe.wait_s == 0.0
    want = [("req", 0)] + [x for b in range(1, nb) for x in (("req", b), ("res", b - 1))] + [("res", nb - 1)]
    ok = ok and list(pipe.order_log) == want
    refunds = np.concatenate([outs[b][0].numpy() for b in range(nb) if rf.KINDS[b] == rf.F])
    ok = ok and all((refunds == v).any() for v in (rf.NOKEY, rf.DONE, rf.INVALID))
    ok = ok and ((refunds == rf.DROPPED).any() == ops.overflow) and ((cover["dropped"] > 0) == ops.overflow)
    ok = ok and cover["multi_rank"] > 0
    return ok, (ops.overflow, bad)


def _run_ranks(world, **kw):
    import routed_refund_cases as rf
    res = rf.run_ranks(__name__, "_worker", world, **kw)
    return {r: (ok, info[0]) for r, (ok, info) in res.items()}


@pytest.mark.parametrize("world", [2, 3])
def test_routed_refund_steps_match_one_shared_store(world):
    """kinds D F P D F R F P D, 1500 requests per rank and step over ~400 keys,
    skewed clocks: every field of every request on every rank; the P and D
    steps after a refund step pin the state the refunds left"""
    assert _run_ranks(world) == {r: (True, False) for r in range(world)}


def test_routed_refund_bucket_overflow():
    """buckets smaller than a rank's requests for one owner: the refunds past
    the capacity come back RL_DROPPED and were not applied -- the later peek and
    decide steps equal the shared store that skipped them -- and still advance
    the store clock"""
    assert _run_ranks(2, m=5000, cap=2048) == {0: (True, True), 1: (True, True)}


# --- the sum rule across ranks ----------------------------------------------------------

def _sum_rule_worker(rank, world):
    import torch
    import torch.distributed as dist

    import routed_refund_cases as rf
    import shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shown = {}
    pg_res = dist.new_group(backend="gloo")
    configs = [(1, 10 ** 6, 60 * NS)]
    key = np.array([10], np.uint64)
    owner = int(shard.owner_of(key, 2)[0])
    last, when = float(T0) / 1e9, T0 // 1_000_000 + 120_000
    one = lambda n, t: (key, np.array([t], np.int64), np.array([n], np.int64), np.zeros(1, np.uint32))
    idle = (np.array([77], np.uint64), np.array([T0], np.int64), np.ones(1, np.int64), np.zeros(1, np.uint32))
    mine_n = [4, 45][rank]
    for name, kinds, steps in (
            ("one", [rf.F, rf.P], [one(mine_n, T0), one(0, T0 + 1)]),
            ("two", [rf.F, rf.F, rf.P], [one(4, T0) if rank == 0 else idle, one(45, T0) if rank == 1 else idle,
                                         one(0, T0 + 1)])):
        sim = rf.new_sim(configs)
        if rank == owner:   # the bucket of tests/test_refund_gpu.py::test_bucket_sum_rule
            sim.db["tb:10"] = [(0.9763120008305, last), when]
        ops, pipe = _pipeline(2, 8, 2048, sim, pg_req=None, pg_res=pg_res)
        outs = _outs(torch, steps)
        pipe.run([rf.host_tensors(torch, bt) for bt in steps], outs, kinds=kinds)
        shown[name] = {"status": [o[0].numpy().tolist() for o in outs[:-1]],
                       "tokens": "%.14g" % sim.db["tb:10"][0][0] if rank == owner else None,
                       "remaining": outs[-1][1].numpy().tolist()}
    return True, shown


def test_routed_refund_cross_rank_sum_rule():
    """the §10i example: a bucket holding 0.9763120008305; rank 0 refunds 4 and
    rank 1 refunds 45.  In one step the owner applies 49 once: 49.97631200083;
    in two steps 4 then 45: 49.976312000831 (%.14g requantises the stored
    tokens, so the two differ)"""
    import routed_refund_cases as rf
    res = {r: info for r, (ok, info) in rf.run_ranks(__name__, "_sum_rule_worker", 2).items()}
    tokens = {name: [res[r][name]["tokens"] for r in range(2) if res[r][name]["tokens"] is not None]
              for name in ("one", "two")}
    assert tokens == {"one": ["49.97631200083"], "two": ["49.976312000831"]}
    for r in range(2):
        assert res[r]["one"]["status"] == [[1]]                       # RL_REFUND_DONE on both ranks
        assert res[r]["one"]["remaining"] == res[r]["two"]["remaining"] == [49]   # the peek: floor(tokens)
    # in two steps the other rank refunds a key nobody has: RL_REFUND_NOKEY
    assert res[0]["two"]["status"] == [[1], [0]] and res[1]["two"]["status"] == [[0], [1]]


# --- world 1 ------------------------------------------------------------------------

def test_routed_refund_world1_in_place():
    """world 1 without the exchange: no collective, the same nine kinds"""
    import torch

    import routed_refund_cases as rf
    sim = rf.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 1500, 4096, sim)
    assert not pipe.exchange
    mine = rf.rank_batches(1, CONFIGS, reset_n_none=True, in_order=True)
    outs = _outs(torch, mine)
    pipe.run([rf.host_tensors(torch, bt) for bt in mine], outs, kinds=rf.KINDS)
    assert pipe.collectives == 0 and not ops.overflow
    assert not rf.mismatches(outs, rf.routed_expectations([mine], rf.KINDS, 0, CONFIGS))
    refunds = np.concatenate([outs[b][0].numpy() for b in range(len(mine)) if rf.KINDS[b] == rf.F])
    assert set(refunds.tolist()) == {rf.NOKEY, rf.DONE, rf.INVALID}


def test_routed_refund_gives_quota_back():
    """the point of the kind, on one key: a refund step gives back what a
    decide step took, a peek shows it, and the next decide has it"""
    import torch

    import routed_refund_cases as rf
    sim = rf.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 8, 2048, sim)
    key = np.full(4, 10, np.uint64)                      # cfg 10: fixed window, 100 per 60 s
    cfg = np.full(4, 10, np.uint32)
    ts = T0 + np.arange(4, dtype=np.int64)
    kinds = [rf.D, rf.F, rf.P, rf.F, rf.P, rf.F]
    ns = [np.full(4, 20, np.int64), np.full(4, 5, np.int64), np.zeros(4, np.int64), np.full(4, 1 << 40, np.int64),
          np.zeros(4, np.int64), np.full(4, 1, np.int64)]
    batches = [(key, ts + 10 * b, n, cfg) for b, n in enumerate(ns)]
    outs = _outs(torch, batches)
    pipe.run([rf.host_tensors(torch, bt) for bt in batches], outs, kinds=kinds)
    assert outs[0][1].numpy().tolist() == [80, 60, 40, 20]
    assert outs[1][0].numpy().tolist() == [1, 1, 1, 1]   # RL_REFUND_DONE: DECRBY 20
    assert outs[2][1].numpy().tolist() == [40] * 4
    assert outs[3][0].numpy().tolist() == [1, 1, 1, 1]   # count <= N: DEL
    assert outs[4][1].numpy().tolist() == [100] * 4
    assert outs[5][0].numpy().tolist() == [0, 0, 0, 0]   # RL_REFUND_NOKEY: nothing to refund
    assert all(not outs[b][f].numpy().any() for b in (1, 3, 5) for f in (1, 2, 3))
    assert not rf.mismatches(outs, rf.routed_expectations([batches], kinds, 0, CONFIGS))


# --- errors -------------------------------------------------------------------------

def test_routed_refund_step_errors():
    """a refund step on a pipeline built without refund= raises ValueError
    before anything is enqueued; so does a refund step with n=None (only a
    reset step may leave n out) and an unknown op; a refund step works once the
    callable is there"""
    import torch

    import route_ops
    import routed_op_cases as rc
    import routed_refund_cases as rf
    import shard
    assert shard.OP_REFUND == 3 and shard._OP_NAMES[shard.OP_REFUND] == "refund"
    sim = rf.new_sim(CONFIGS)
    ops = route_ops.NumpyRouteOps(1, 4096)
    calls = []
    ops.pack = lambda *a, _pack=ops.pack: (calls.append("pack"), _pack(*a))[1]
    mine = rf.rank_batches(0, CONFIGS, kinds=[rf.D, rf.F])
    ins = [rf.host_tensors(torch, bt) for bt in mine]
    outs = _outs(torch, mine)
    bare = shard.RoutedPipeline(ops, rc.py_decide(sim, 1, ops.capacity), 1, 1500, "cpu", depth=4)
    with pytest.raises(ValueError, match="refund"):
        bare.step(0, *ins[1], *outs[1], op=shard.OP_REFUND)
    params = inspect.signature(shard.RoutedPipeline).parameters
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("refund", "refund_ev"))
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, 1, ops.capacity), 1, 1500, "cpu", depth=4,
                                refund=rf.oracle_refund(sim, 1, ops.capacity))
    with pytest.raises(ValueError, match="reset"):
        pipe.step(0, ins[1][0], ins[1][1], None, ins[1][3], *outs[1], op=shard.OP_REFUND)
    for op in (4, 7, -1, "refund"):
        with pytest.raises(ValueError):
            pipe.step(0, *ins[1], *outs[1], op=op)
    assert calls == [] and not pipe._pend and not bare._pend and len(pipe.order_log) == 0
    pipe.run(ins, outs, kinds=[rf.D, rf.F])
    assert calls == ["pack", "pack"]
    assert not rf.mismatches(outs, rf.routed_expectations([mine], [rf.D, rf.F], 0, CONFIGS))
