"""The routed usage tally and top keys on CPU: shard.merge_tallies /
merge_hots against the reference models of the whole request multiset, and
shard.RoutedPipeline(observe=) with its collective reads usage() / top_keys()
over the routing kernels' CPU restatement (tests/route_ops.py), the Python
oracle as every owner's engine and a numpy observer that recounts from the
buffers it is handed (tests/routed_tally_cases.py).  DESIGN.md §10o;
tests/test_routed_tally_gpu.py runs the HIP kernels."""
import numpy as np
import pytest

import hot_cases
import tally_cases
from tracegen import CONFIG_SETS, T0

CONFIGS = CONFIG_SETS["mixed"]
NCFG = 6
SLOTS = 1024
WIDTH = 1 << 16
HOT_MIN = 6


# --- the merge functions ------------------------------------------------------------------

def _multiset(seed, m=6000, ids=260):
    """requests over `ids` scattered key ids, few enough denials per key for
    many ties: decisions 0..3, a few unknown configs, bad codes and the reserved key"""
    rng = np.random.default_rng(seed)
    rank = rng.zipf(1.4, m) % ids
    key = hot_cases.key_of_rank(rank + 1000 * seed)
    cfg = (rank % NCFG).astype(np.uint32)
    n = rng.choice([1, 1, 2, 5, 0, -1], m).astype(np.int64)
    dec = rng.choice([0, 1, 1, 2, 3], m).astype(np.uint8)
    cfg[rng.random(m) < 0.01] = NCFG + 3
    dec[rng.random(m) < 0.01] = 9
    key[rng.random(m) < 0.005] = np.uint64(tally_cases.KEY_RESERVED)
    return key, cfg, n, dec


def _denied_keys(key, cfg, dec):
    sel = (cfg < NCFG) & (dec == 0) & (key != np.uint64(tally_cases.KEY_RESERVED))
    return np.unique(key[sel])


def _case(world):
    """the first seeded multiset for which the reference models track every
    key, whole and in every owner's share: key tables of SLOTS records
    (tally_cases.fits) and a sketch of WIDTH columns in which no two keys meet"""
    import shard
    for seed in range(40):
        key, cfg, n, dec = _multiset(seed)
        own = shard.owner_of(key, world)
        den = _denied_keys(key, cfg, dec)
        ok = tally_cases.fits(den, SLOTS) and all(tally_cases.fits(den[shard.owner_of(den, world) == w], SLOTS)
                                                  for w in range(world))
        if ok and hot_cases.distinct_columns(np.unique(key), WIDTH):
            return (key, cfg, n, dec), own
    raise AssertionError("no seed fits")


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_merge_tallies_equals_whole(world):
    """the multiset split by owner, each share tallied, the reads merged: every
    config row, every info word and every key record of the whole multiset's
    tally; and the ranks' local top-k lists merge to the global top-k, ties on
    denied by key id"""
    import routed_tally_cases as tc
    import shard
    (key, cfg, n, dec), own = _case(world)
    whole = tally_cases.expected_tally(key, cfg, n, dec, NCFG)
    shares = [tally_cases.expected_tally(key[own == w], cfg[own == w], n[own == w], dec[own == w], NCFG)
              for w in range(world)]
    assert len(whole.keys) > 100 and whole.unknown_cfg and whole.bad_codes and whole.reserved[0]
    denied = sorted(v[0] for v in whole.keys.values())
    assert len(set(denied)) < len(denied) // 2                       # ties
    routed = [dict(steps=2, requests=int((own == w).sum()), dropped_requests=w) for w in range(world)]
    want_routed = dict(steps=2 * world, requests=key.size, dropped_requests=sum(range(world)))
    for top in (1, 5, 50, 10 ** 6):
        got = shard.merge_tallies([tc.tally_part_of(s, top, r) for s, r in zip(shares, routed)], top)
        tc.check_usage(got, whole, want_routed, top, f"world {world} top {top}")
    assert len(got["keys"]) == len(whole.keys)
    assert shard.merge_tallies([tc.tally_part_of(s, 0) for s in shares], 0)["keys"].size == 0


def test_merge_tallies_is_total():
    """a key id two ranks report -- impossible under the owner partition -- is
    summed and keeps the lowest rank's cfg; rows of unequal length and sums
    past 2^64 are handled"""
    import routed_tally_cases as tc
    import shard
    M, H = (1 << 64) - 1, (1 << 63) - 1
    # key 5 on rank 0: 2^64 - 1 units
    a = tally_cases.expected_tally([5, 5, 5, 6], [1, 1, 1, 0], [H, H, 1, 1], [0, 0, 0, 0], 2)
    b = tally_cases.expected_tally([5, 7, 7, 7], [2, 2, 2, 1], [4, 1, 1, 4], [0, 0, 1, 0], 3)
    got = shard.merge_tallies([tc.tally_part_of(a, 10), tc.tally_part_of(b, 10)], 10)
    rows = {int(r["key_id"]): (int(r["denied"]), int(r["units_denied"]), int(r["cfg_id"])) for r in got["keys"]}
    assert rows == {5: (4, (M + 4) & M, 1), 6: (1, 1, 0), 7: (2, 5, 1)}
    assert [int(k) for k in got["keys"]["key_id"]] == [5, 7, 6]
    assert got["cfg"].size == 3 and got["cfg"]["count"][:, 0].tolist() == [1, 4, 2]
    assert int(got["cfg"]["units"][1, 0]) == (M + 4) & M == 3


@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("weight", [hot_cases.REQUESTS, hot_cases.UNITS])
def test_merge_hots_equals_whole(world, weight):
    """the same split through hot_cases.HotModel: the merged candidates and
    estimates are the whole multiset's, the local top-k lists merge to the
    global top-k with ties on the estimate by key id, and the counters add up"""
    import routed_tally_cases as tc
    import shard
    (key, cfg, n, dec), own = _case(world)
    whole = hot_cases.model_of([(key, cfg, n, dec)], WIDTH, HOT_MIN, NCFG, weight)
    shares = [hot_cases.model_of([(key[own == w], cfg[own == w], n[own == w], dec[own == w])], WIDTH, HOT_MIN, NCFG,
                                 weight) for w in range(world)]
    want = whole.read()
    assert len(want) > 50 and len({e for _, e in want}) < len(want) // 2      # candidates, and ties
    assert all(e == whole.true[k] for k, e in want)                   # no two keys share a counter
    for top in (1, 5, 50, 10 ** 6):
        got = shard.merge_hots([tc.hot_part_of(s, top) for s in shares], top)
        assert [(int(r["key_id"]), int(r["estimate"])) for r in got["keys"]] == want[:top], (world, top)
        tc.check_top_keys(got, shares, top, f"world {world} top {top}")
        i = got["info"]
        assert (i["total"], i["skipped"], i["keys_tracked"]) == (whole.total, whole.skipped, len(want))
        assert (i["width"], i["depth"], i["hot_min"], i["weight"]) == (WIDTH, 4, HOT_MIN, weight)


def test_merge_hots_parameters_must_agree():
    """estimates of different sketches do not compare: ValueError; dropped is
    non-zero if any part's is; a key two parts report is summed"""
    import routed_tally_cases as tc
    import shard
    key = hot_cases.key_of_rank(np.arange(40) % 4)
    call = (key, np.zeros(40, np.uint32), np.ones(40, np.int64), np.ones(40, np.uint8))
    part = lambda **kw: tc.hot_part_of(hot_cases.model_of([call], kw.get("width", 64), kw.get("hot_min", 2), 1,
                                                          kw.get("weight", 0)), 10)
    for kw in (dict(width=128), dict(hot_min=3), dict(weight=1)):
        with pytest.raises(ValueError):
            shard.merge_hots([part(), part(**kw)], 10)
    odd = part()
    odd["info"]["depth"] = 5
    with pytest.raises(ValueError):
        shard.merge_hots([part(), odd], 10)
    full = part()
    full["info"]["dropped"] = 1
    got = shard.merge_hots([part(), full, part()], 10)
    assert got["info"]["dropped"] == 1 and got["info"]["total"] == 120
    assert sorted(int(e) for e in got["keys"]["estimate"]) == [30] * 4
    assert shard.merge_hots([part(), part()], 10)["info"]["dropped"] == 0


# --- the pipeline ---------------------------------------------------------------------

M_STEP, CAP = 600, 4096


def _pipeline(world, cap, sim, m=M_STEP, **kw):
    import routed_allow_all_cases as ra
    import routed_charge_cases as cc
    import routed_op_cases as rc
    import routed_refund_cases as rf
    import shard
    ops = ra.RouteOpsSel(world, cap)
    c = ops.capacity
    kw.setdefault("depth", 4)
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, world, c), world, max(m, 1800), "cpu",
                                peek=rc.oracle_peek(sim, world, c), reset=rc.oracle_reset(sim, world, c),
                                refund=rf.oracle_refund(sim, world, c), charge=cc.oracle_charge(sim, world, c),
                                settle=ra.numpy_settle(sim), **kw)
    return ops, pipe


def _run(pipe, mine):
    import torch

    import routed_allow_all_cases as ra
    import routed_tally_cases as tc
    ins = [ra.host_tensors(torch, bt) for bt in mine]
    outs = ra.new_outs(torch, tc.KINDS, mine)
    ra.run_kinds(pipe, tc.KINDS, ins, outs)
    return outs


def _rank(rank, world, pg_res=None, top=25):
    """one rank's steps of tc.KINDS with the numpy observer -> what went wrong, if anything"""
    import routed_charge_cases as cc
    import routed_tally_cases as tc
    all_batches = [tc.rank_batches(r, world, CONFIGS, m=M_STEP) for r in range(world)]
    ops, pipe = _pipeline(world, CAP, cc.new_sim(CONFIGS), pg_req=None, pg_res=pg_res)
    obs = tc.NumpyObserver(world, ops.capacity, len(CONFIGS))
    pipe.observe.append(obs)
    outs = _run(pipe, all_batches[rank])
    steps = tc.expected_steps(all_batches, tc.KINDS, CONFIGS, cap=ops.capacity)
    bad = []
    for b, (s, o) in enumerate(zip(steps, outs)):
        if not np.array_equal(o[0].numpy().astype(np.int64), s["rows"][s["src"] == rank, 0]):
            bad.append(("decisions", b))
    # once per decide step and once for AllowAll's member step, never for the
    # others: the observer saw exactly this owner's share of those steps, in merge order
    want = tc.observed_calls(steps, rank)
    if len(obs.calls) != tc.KINDS.count(tc.D) + 1 or len(obs.calls) != len(want):
        bad.append(("calls", len(obs.calls)))
    for j, (g, w) in enumerate(zip(obs.calls, want)):
        if not all(np.array_equal(np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64))
                   for x, y in zip(g, w)):
            bad.append(("call", j))
    e, mods, routed = tc.union_model(steps, world, len(CONFIGS), obs.hot_args)
    if not (len(e.keys) > top and e.count[:, 0].sum() > 0 and e.count[:, 1].sum() > 0 and e.count[:, 3].sum() > 0):
        bad.append(("coverage", len(e.keys)))
    before = pipe.collectives
    tc.check_usage(pipe.usage(obs.tally_read, top=top), e, routed, top, f"rank {rank}")
    tc.check_top_keys(pipe.top_keys(obs.hot_read, top=top), mods, top, f"rank {rank}")
    if not any(mod.candidates for mod in mods):
        bad.append(("no hot key", 0))
    if pipe.collectives != before or ops.overflow or routed["dropped_requests"]:
        bad.append(("collectives or drops", pipe.collectives))
    # a clearing read: the next one is empty on every rank
    pipe.usage(obs.tally_read, top=top, clear=True)
    empty = pipe.usage(obs.tally_read, top=top)
    if empty["keys"].size or empty["cfg"]["count"].any() or any(empty["routed"].values()):
        bad.append(("clear", 0))
    return bad


def test_pipeline_world1_counts_decide_steps():
    """world 1 without a group: kinds D P D C R D F D and one allow_all; the
    reads make no collective"""
    assert _rank(0, 1) == []


def _worker(rank, world):
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bad = _rank(rank, world, pg_res=dist.new_group(backend="gloo"))
    return not bad, bad


@pytest.mark.parametrize("world", [2, 3])
def test_pipeline_counts_on_the_owner(world):
    """gloo worlds: every rank's usage() / top_keys() equal the model over the
    union of all ranks' executed decide requests, each owner having been shown
    exactly its share"""
    import routed_charge_cases as cc
    res = cc.run_ranks(__name__, "_worker", world)
    assert {r: v for r, v in res.items()} == {r: (True, []) for r in range(world)}


def _drop_worker(rank, world, m=5000, cap=2048, nb=3):
    """decide steps only, buckets smaller than a rank's requests for one owner"""
    import torch
    import torch.distributed as dist

    import oracle
    import route_ops
    import routed_charge_cases as cc
    import routed_op_cases as rc
    import routed_tally_cases as tc
    import shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pg_res = dist.new_group(backend="gloo")
    all_batches = [rc.rank_batches(r, CONFIGS, kinds=[tc.D] * nb, m=m, nkeys=40) for r in range(world)]
    ops = route_ops.NumpyRouteOps(world, cap)
    obs = tc.NumpyObserver(world, ops.capacity, len(CONFIGS))
    sim = oracle.OracleSim(0)
    for a, L, W in CONFIGS:
        sim.add_config(a, L, W)
    pipe = shard.RoutedPipeline(ops, route_ops.oracle_decide(sim, world, ops.capacity), world, m, "cpu", depth=4,
                                pg_req=None, pg_res=pg_res, observe=[obs])
    outs = [(torch.empty(m, dtype=torch.uint8),) + tuple(torch.empty(m, dtype=torch.int64) for _ in range(3))
            for _ in range(nb)]
    pipe.run([cc.host_tensors(torch, bt) for bt in all_batches[rank]], outs)
    # decisions of ONE shared limiter, every rank's
    exp = [route_ops.shared_limiter_expectations(all_batches, r, CONFIGS, cap=ops.capacity) for r in range(world)]
    ok = all(np.array_equal(outs[b][0].numpy().astype(np.int64), exp[rank][b][0]) for b in range(nb))
    dec = np.concatenate([exp[r][b][0] for r in range(world) for b in range(nb)])
    sel = dec != tc.DROPPED
    cat = [np.concatenate([all_batches[r][b][f] for r in range(world) for b in range(nb)])[sel] for f in (0, 3, 2)]
    e = tally_cases.expected_tally(cat[0], cat[1], cat[2], tc.code(dec[sel]), len(CONFIGS))
    dropped = int((~sel).sum())
    got = pipe.usage(obs.tally_read, top=10)
    tc.check_usage(got, e, dict(steps=nb * world, requests=int(sel.sum()), dropped_requests=dropped), 10)
    return ok and dropped > 0 and ops.overflow, dropped


def test_pipeline_dropped_requests():
    """a capacity small enough to drop requests: dropped_requests equals the
    number of RL_DROPPED decisions cluster-wide, and the tally is that of the
    executed requests (decisions: route_ops.shared_limiter_expectations)"""
    import routed_charge_cases as cc
    res = cc.run_ranks(__name__, "_drop_worker", 2)
    assert res[0][0] and res[1][0], res
    assert res[0][1] == res[1][1] > 0


def test_pipeline_without_observe_is_unchanged():
    """observe=None and observe=[]: the pipeline issues exactly the calls it
    issues today -- the ops' call log, order_log, collectives and every output
    equal those of a pipeline built without the keyword; with an observer the
    outputs are still the same, and the observer ran on the result side of its
    step: after the unpack, before the next step's pack of the same buffer set"""
    import routed_charge_cases as cc
    import routed_tally_cases as tc

    mine = tc.rank_batches(0, 1, CONFIGS, m=M_STEP)
    runs = {}
    for name, kw in (("today", {}), ("none", dict(observe=None)), ("empty", dict(observe=[])), ("observed", None)):
        log = []
        ops, pipe = _pipeline(1, CAP, cc.new_sim(CONFIGS), exchange=True, depth=2, **(kw or {}))
        for f in ("pack", "pack_sel", "merge", "unpack"):
            setattr(ops, f, lambda *a, _f=getattr(ops, f), _n=f: (log.append(_n), _f(*a))[1])
        pipe._a2a = lambda out, inp, group, _p=pipe: (log.append("a2a"), out.copy_(inp),
                                                      setattr(_p, "collectives", _p.collectives + 1))[0]
        if kw is None:
            obs = tc.NumpyObserver(1, ops.capacity, len(CONFIGS))
            pipe.observe.append(lambda *a: (log.append("observe"), obs(*a))[1])
        outs = _run(pipe, mine)
        runs[name] = (log, list(pipe.order_log), pipe.collectives, [[x.numpy().copy() for x in o] for o in outs])
    for name in ("none", "empty"):
        assert runs[name][:3] == runs["today"][:3], name
        assert all(np.array_equal(x, y) for a, b in zip(runs[name][3], runs["today"][3]) for x, y in zip(a, b))
    log = runs["observed"][0]
    assert [x for x in log if x != "observe"] == runs["today"][0]
    assert runs["observed"][1:3] == runs["today"][1:3]
    assert all(np.array_equal(x, y) for a, b in zip(runs["observed"][3], runs["today"][3]) for x, y in zip(a, b))
    assert log.count("observe") == tc.KINDS.count(tc.D) + 1
    assert all(log[i - 1] == "unpack" for i, x in enumerate(log) if x == "observe")


def test_observe_keyword():
    import inspect

    import shard
    params = inspect.signature(shard.RoutedPipeline).parameters
    assert params["observe"].kind is inspect.Parameter.KEYWORD_ONLY and params["observe"].default is None
    for name in ("usage", "top_keys"):
        assert callable(getattr(shard.RoutedPipeline, name))
    assert callable(shard.merge_tallies) and callable(shard.merge_hots)
    assert T0 > 0
