"""Routed charge steps (shard.OP_CHARGE) through shard.RoutedPipeline on CPU
(gloo): the routing kernels are their CPU restatement (tests/route_ops.py) and
the owner's engine is the Python oracle (tests/routed_charge_cases.py).  Every
rank's results of the steps D C P D C R C F D must equal ONE shared store that
runs all ranks' steps in merge order, a charge step as ONE Charge call over the
merged batch.  tests/test_routed_charge_gpu.py runs the HIP
kernels and the engine."""
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
    import routed_charge_cases as cc
    import routed_op_cases as rc
    import routed_refund_cases as rf
    import shard
    ops = route_ops.NumpyRouteOps(world, cap)
    c = ops.capacity
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, world, c), world, m, "cpu", depth=4,
                                peek=rc.oracle_peek(sim, world, c), reset=rc.oracle_reset(sim, world, c),
                                refund=rf.oracle_refund(sim, world, c), charge=cc.oracle_charge(sim, world, c), **kw)
    return ops, pipe


# --- the case is what it claims ------------------------------------------------------

@pytest.mark.parametrize("world", [1, 2, 3])
def test_case_coverage(world):
    """the nine steps' charges meet every class of apply_charge but "error", a
    window over its limit and (world > 1) a bucket charged by two ranks in one
    step with a dup_denied contributor; n runs from 1 to 2^40 with some n <= 0"""
    import routed_charge_cases as cc
    assert cc.KINDS == [cc.D, cc.C, cc.P, cc.D, cc.C, cc.R, cc.C, cc.F, cc.D]
    all_batches = [cc.rank_batches(r, CONFIGS) for r in range(world)]
    cover = cc.charge_coverage(all_batches, CONFIGS)
    assert cover["dropped"] == 0 and cover["requests"] == 3 * 1500 * world
    n = np.concatenate([b[2] for b, k in zip(all_batches[0], cc.KINDS) if k == cc.C])
    assert n.max() == 1 << 40 and (n == 1).any() and (n <= 0).any()
    assert n.max() > max(L for _, L, _ in CONFIGS)
    key = np.concatenate([b[0] for b, k in zip(all_batches[0], cc.KINDS) if k == cc.C])
    assert (key == np.uint64((1 << 64) - 1)).any()


def test_case_coverage_in_order():
    """the world-1 case of the in-place tests (sorted charge steps) too"""
    import routed_charge_cases as cc
    cc.charge_coverage([cc.rank_batches(1, CONFIGS, reset_n_none=True, in_order=True)], CONFIGS)


# --- worlds 2 and 3 over gloo -----------------------------------------------------------

def _worker(rank, world, m=1500, cap=4096):
    """one rank (routed_refund_cases.run_ranks) -> (ok, (overflow, mismatches))"""
    import torch
    import torch.distributed as dist

    import routed_charge_cases as cc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sim = cc.new_sim(CONFIGS)
    pg_res = dist.new_group(backend="gloo")
    ops, pipe = _pipeline(world, m, cap, sim, pg_req=None, pg_res=pg_res)
    all_batches = [cc.rank_batches(r, CONFIGS, m=m) for r in range(world)]
    mine = all_batches[rank]
    outs = _outs(torch, mine)
    pipe.run([cc.host_tensors(torch, bt) for bt in mine], outs, kinds=cc.KINDS)
    cover = cc.new_cover()
    exp = cc.routed_expectations(all_batches, cc.KINDS, rank, CONFIGS, cap=ops.capacity, cover=cover)
    bad = cc.mismatches(outs, exp)
    ok = not bad
    nb = len(mine)
    # 3 collectives per step of any kind, and the one collective order
    ok = ok and pipe.exchange and pipe.collectives == 3 * nb and pipe.wait_s == 0.0
    want = [("req", 0)] + [x for b in range(1, nb) for x in (("req", b), ("res", b - 1))] + [("res", nb - 1)]
    ok = ok and list(pipe.order_log) == want
    steps = [b for b in range(nb) if cc.KINDS[b] == cc.C]
    dec = np.concatenate([outs[b][0].numpy() for b in steps])
    charged = np.concatenate([outs[b][2].numpy() for b in steps])
    asked = np.concatenate([mine[b][2] for b in steps])
    ok = ok and all((dec == v).any() for v in (cc.ALLOWED, cc.DENIED, cc.INVALID))
    # charged is never more than was asked, and all of it where the row is ALLOWED
    ok = ok and bool((charged >= 0).all() and (charged <= np.maximum(asked, 0)).all())
    ok = ok and bool((charged[dec == cc.ALLOWED] == asked[dec == cc.ALLOWED]).all())
    ok = ok and ((dec == cc.DROPPED).any() == ops.overflow) and ((cover["dropped"] > 0) == ops.overflow)
    ok = ok and cover["cross_rank_dup"] > 0
    return ok, (ops.overflow, bad)


def _run_ranks(world, **kw):
    import routed_charge_cases as cc
    res = cc.run_ranks(__name__, "_worker", world, **kw)
    return {r: (ok, info[0]) for r, (ok, info) in res.items()}


@pytest.mark.parametrize("world", [2, 3])
def test_routed_charge_steps_match_one_shared_store(world):
    """kinds D C P D C R C F D, 1500 requests per rank and step over ~400 keys,
    skewed clocks: every field of every request on every rank; the P, R, F and
    D steps after a charge step pin the state the charges left"""
    assert _run_ranks(world) == {r: (True, False) for r in range(world)}


def test_routed_charge_bucket_overflow():
    """buckets smaller than a rank's requests for one owner: the charges past
    the capacity come back RL_DROPPED and were not recorded -- the later peek
    and decide steps equal the shared store that skipped them -- and still
    advance the store clock"""
    assert _run_ranks(2, m=5000, cap=2048) == {0: (True, True), 1: (True, True)}


# --- the conservative bound across ranks --------------------------------------------------

def _bound_worker(rank, world):
    import torch
    import torch.distributed as dist

    import routed_charge_cases as cc
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pg_res = dist.new_group(backend="gloo")
    configs = [(1, 10, 60 * NS)]                       # a bucket of 10, one token per 6 s
    key = np.array([10], np.uint64)
    one = lambda n: (key, np.array([T0], np.int64), np.array([n], np.int64), np.zeros(1, np.uint32))
    idle = (np.array([77], np.uint64), np.array([T0], np.int64), np.ones(1, np.int64), np.zeros(1, np.uint32))
    shown = {}
    # every step at the one time stamp T0; rank 0 first takes 3 of the 10, so the bucket holds 7
    for name, asks in (("both_over", (9, 8)), ("one_over", (4, 8))):
        sim = cc.new_sim(configs)
        ops, pipe = _pipeline(2, 8, 2048, sim, pg_req=None, pg_res=pg_res)
        steps = [one(3) if rank == 0 else idle, one(asks[rank]), one(0)]
        kinds = [cc.D, cc.C, cc.P]
        outs = _outs(torch, steps)
        pipe.run([cc.host_tensors(torch, bt) for bt in steps], outs, kinds=kinds)
        all_steps = [[one(3), one(asks[0]), one(0)], [idle, one(asks[1]), one(0)]]
        bad = cc.mismatches(outs, cc.routed_expectations(all_steps, kinds, rank, configs))
        shown[name] = {"charge": [int(o.numpy()[0]) for o in outs[1]], "left": int(outs[2][1].numpy()[0]),
                       "bad": bad}
    return True, shown


def test_routed_charge_cross_rank_bound():
    """two ranks charge one bucket that holds 7 at one time stamp.  Both are
    asked against 7: n' = 7 each (or 4 and 7).  Rank 0 comes first in merge
    order (the ts tie goes by source rank) and takes its n'; rank 1's
    duplicate then finds less than its n', takes nothing and is RL_DENIED with
    charged 0.  The bucket ends below the smaller refused ask and is never
    negative: §10m's bound across ranks"""
    import routed_charge_cases as cc
    res = {r: info for r, (ok, info) in cc.run_ranks(__name__, "_bound_worker", 2).items()}
    for r in range(2):
        assert res[r]["both_over"]["bad"] == [] and res[r]["one_over"]["bad"] == []
    # rows are [decision, remaining, charged, reset_at]
    a, b = res[0]["both_over"], res[1]["both_over"]
    assert a["charge"][:3] == [cc.DENIED, 0, 7]        # 9 asked, the 7 there taken: short
    assert b["charge"][:3] == [cc.DENIED, 0, 0]        # 8 asked, n' = 7, nothing left: dup_denied
    assert a["left"] == b["left"] == 0 and 0 <= a["left"] < min(9, 8)
    a, b = res[0]["one_over"], res[1]["one_over"]
    assert a["charge"][:3] == [cc.ALLOWED, 3, 4]       # 4 asked and taken
    assert b["charge"][:3] == [cc.DENIED, 3, 0]        # 8 asked, n' = 7, 3 left: refused whole
    assert a["left"] == b["left"] == 3 and 0 <= a["left"] < 8


# --- world 1 ------------------------------------------------------------------------

def test_routed_charge_world1_in_place():
    """world 1 without the exchange: no collective, the same nine kinds"""
    import torch

    import routed_charge_cases as cc
    sim = cc.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 1500, 4096, sim)
    assert not pipe.exchange
    mine = cc.rank_batches(1, CONFIGS, reset_n_none=True, in_order=True)
    outs = _outs(torch, mine)
    pipe.run([cc.host_tensors(torch, bt) for bt in mine], outs, kinds=cc.KINDS)
    assert pipe.collectives == 0 and not ops.overflow
    assert not cc.mismatches(outs, cc.routed_expectations([mine], cc.KINDS, 0, CONFIGS))
    dec = np.concatenate([outs[b][0].numpy() for b in range(len(mine)) if cc.KINDS[b] == cc.C])
    assert set(dec.tolist()) == {cc.ALLOWED, cc.DENIED, cc.INVALID}


def test_routed_charge_records_usage():
    """the point of the kind, on one bucket and one window: a charge step takes
    what is there when the usage is more than the bucket holds (a decide of the
    same amount would take nothing), records a window's usage past its limit,
    and the following peek and decide see it"""
    import torch

    import routed_charge_cases as cc
    sim = cc.new_sim(CONFIGS)
    ops, pipe = _pipeline(1, 8, 2048, sim)
    key = np.array([0, 10], np.uint64)                   # cfg 0: bucket of 20; cfg 10: fixed window, 100 per 60 s
    cfg = np.array([0, 10], np.uint32)
    ts = T0 + np.arange(2, dtype=np.int64)
    kinds = [cc.D, cc.C, cc.P, cc.C, cc.D]
    ns = [np.array([5, 30], np.int64), np.array([50, 90], np.int64), np.zeros(2, np.int64),
          np.array([1, 1], np.int64), np.array([1, 1], np.int64)]
    batches = [(key, ts + 10 * b, n, cfg) for b, n in enumerate(ns)]
    outs = _outs(torch, batches)
    pipe.run([cc.host_tensors(torch, bt) for bt in batches], outs, kinds=kinds)
    row = lambda b, i: [int(outs[b][f].numpy()[i]) for f in range(3)]
    assert row(0, 0) == [cc.ALLOWED, 15, 0] and row(0, 1)[:2] == [cc.ALLOWED, 70]
    assert row(1, 0) == [cc.DENIED, 0, 15]               # 50 of usage, 15 there: all 15 taken
    assert row(1, 1) == [cc.DENIED, 0, 90]               # INCRBY 90 on 30: 120 > 100, recorded all the same
    assert row(2, 0)[:2] == [cc.ALLOWED, 0]              # Peek(key, 0): nothing left
    assert row(2, 1)[:2] == [cc.DENIED, 0]               # the window stands at 120 of 100
    assert row(3, 0) == [cc.DENIED, 0, 0]                # an empty bucket: nothing to take
    assert row(3, 1) == [cc.DENIED, 0, 1]                # the window counts on
    assert row(4, 0)[0] == cc.DENIED and row(4, 1)[0] == cc.DENIED
    assert not cc.mismatches(outs, cc.routed_expectations([batches], kinds, 0, CONFIGS))


# --- errors -------------------------------------------------------------------------

def test_routed_charge_step_errors():
    """a charge step on a pipeline built without charge= raises ValueError
    before anything is enqueued; so does a charge step with n=None (only a
    reset step may leave n out) and an unknown op; a charge step works once the
    callable is there"""
    import torch

    import route_ops
    import routed_charge_cases as cc
    import routed_op_cases as rc
    import shard
    assert shard.OP_CHARGE == 4 and shard._OP_NAMES[shard.OP_CHARGE] == "charge"
    sim = cc.new_sim(CONFIGS)
    ops = route_ops.NumpyRouteOps(1, 4096)
    calls = []
    ops.pack = lambda *a, _pack=ops.pack: (calls.append("pack"), _pack(*a))[1]
    mine = cc.rank_batches(0, CONFIGS, kinds=[cc.D, cc.C])
    ins = [cc.host_tensors(torch, bt) for bt in mine]
    outs = _outs(torch, mine)
    bare = shard.RoutedPipeline(ops, rc.py_decide(sim, 1, ops.capacity), 1, 1500, "cpu", depth=4)
    with pytest.raises(ValueError, match="charge"):
        bare.step(0, *ins[1], *outs[1], op=shard.OP_CHARGE)
    params = inspect.signature(shard.RoutedPipeline).parameters
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("charge", "charge_ev"))
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, 1, ops.capacity), 1, 1500, "cpu", depth=4,
                                charge=cc.oracle_charge(sim, 1, ops.capacity))
    with pytest.raises(ValueError, match="reset"):
        pipe.step(0, ins[1][0], ins[1][1], None, ins[1][3], *outs[1], op=shard.OP_CHARGE)
    for op in (5, 7, -1, "charge"):
        with pytest.raises(ValueError):
            pipe.step(0, *ins[1], *outs[1], op=op)
    assert calls == [] and not pipe._pend and not bare._pend and len(pipe.order_log) == 0
    pipe.run(ins, outs, kinds=[cc.D, cc.C])
    assert calls == ["pack", "pack"]
    assert not cc.mismatches(outs, cc.routed_expectations([mine], [cc.D, cc.C], 0, CONFIGS))
