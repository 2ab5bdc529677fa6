"""The routed AllowAll (shard.RoutedPipeline.allow_all, include/rl_route.h,
DESIGN.md §10l) on CPU (gloo): the routing kernels are their CPU restatement
(tests/route_ops.py, tests/routed_allow_all_cases.py) and the owner's engine is
the Python oracle.  The expectation is the oracle composition on ONE shared
store: a decide step of all ranks' members, the settle rule, then ONE refund
step with n = g.  tests/test_routed_allow_all_gpu.py runs the HIP kernels and
the engine."""
import inspect
import itertools

import numpy as np
import pytest

from oracle import rl_oracle_py as po
from tracegen import CONFIG_SETS, NS, T0

DECISIONS = [0, 1, 2, 3, 4, 7]
ALGS = [po.TOKEN_BUCKET, po.SLIDING_WINDOW, po.FIXED_WINDOW]


def short_patterns():
    """(first, decisions) of every byte pattern of `first` up to length 10
    crossed with decisions from {0, 1, 2, 3, 4, 7}: the full cross up to length
    4 (6^L decision vectors per pattern); above that, where the full cross has
    up to 6^10 vectors per pattern, each pattern with the six constant vectors
    and six seeded random ones"""
    rng = np.random.default_rng(11)
    for L in range(1, 11):
        for first in itertools.product([0, 1], repeat=L):
            if L <= 4:
                decs = itertools.product(DECISIONS, repeat=L)
            else:
                decs = [(d,) * L for d in DECISIONS] + [tuple(rng.choice(DECISIONS, L).tolist()) for _ in range(6)]
            for dec in decs:
                yield np.array(first, np.uint8), np.array(dec, np.uint8)


def long_patterns(seed=12, m=700):
    """random groups of 1 to 16 with runs of 15, 16, 17 and 33 among them"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 17, 60).tolist()
    for at, s in ((5, 15), (18, 16), (30, 17), (44, 33), (59, 17)):
        sizes.insert(at, s)
    first = np.zeros(sum(sizes), np.uint8)
    first[np.cumsum([0] + sizes[:-1])] = rng.choice([1, 2, 255], len(sizes))
    first[0] = rng.integers(0, 2)
    return first, rng.choice(DECISIONS, first.size, p=[0.2, 0.6, 0.05, 0.05, 0.05, 0.05]).astype(np.uint8), sizes


# --- the settle model -------------------------------------------------------------------

def test_settle_scans_equal_maximal_runs_short():
    """the kernel's two bounded scans against the definition, on every short pattern"""
    import routed_allow_all_cases as ra
    count = 0
    for first, dec in short_patterns():
        L = first.size
        n = np.arange(1, L + 1, dtype=np.int64)
        cfg = (np.arange(L) % 4).astype(np.uint32)     # config 3 is unknown
        a = ra.settle_routed(ALGS, first, n, cfg, dec, scans=True)
        b = ra.settle_routed(ALGS, first, n, cfg, dec, scans=False)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (first, dec)
        count += 1
    assert count > 30_000


def test_settle_long_runs():
    """runs of 15 and 16 settle, runs of 17 and 33 are INVALID on every member,
    with both forms of the model"""
    import routed_allow_all_cases as ra
    first, dec, sizes = long_patterns()
    n = np.ones(first.size, np.int64)
    cfg = (np.arange(first.size) % 3).astype(np.uint32)
    a = ra.settle_routed(ALGS, first, n, cfg, dec, scans=True)
    b = ra.settle_routed(ALGS, first, n, cfg, dec, scans=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    at = 0
    for s in sizes:
        if s > 16:
            assert (a[0][at:at + s] == po.INVALID).all()
        else:
            assert (a[0][at:at + s] == ra.BY_SEVERITY[max(ra.severity(d) for d in dec[at:at + s])]).all()
        at += s
    assert {15, 16, 17, 33} <= set(sizes)


def test_settle_severity_order_and_give_back():
    """INVALID next to DROPPED gives INVALID, DROPPED next to ERROR gives
    DROPPED, a byte of 5 or more is INVALID; g per algorithm: a bucket took
    when it allowed, a window when it allowed or denied; a dropped, error or
    invalid member took nothing; sel = g > 0"""
    import routed_allow_all_cases as ra
    pair = lambda a, b: ra.settle_routed(ALGS, np.zeros(2, np.uint8), np.ones(2, np.int64), np.zeros(2, np.uint32),
                                         np.array([a, b], np.uint8))[0].tolist()
    assert pair(po.INVALID, ra.DROPPED) == pair(ra.DROPPED, po.INVALID) == [po.INVALID] * 2
    assert pair(ra.DROPPED, po.ERROR) == pair(po.ERROR, ra.DROPPED) == [ra.DROPPED] * 2
    assert pair(po.ERROR, po.DENIED) == [po.ERROR] * 2 and pair(po.DENIED, po.ALLOWED) == [po.DENIED] * 2
    assert pair(po.ALLOWED, po.ALLOWED) == [po.ALLOWED] * 2
    assert pair(5, ra.DROPPED) == pair(255, po.ALLOWED) == [po.INVALID] * 2
    # one group per algorithm: members ALLOWED, DENIED, ERROR, INVALID, DROPPED, n = 10 .. 14
    dec = np.array([po.ALLOWED, po.DENIED, po.ERROR, po.INVALID, ra.DROPPED], np.uint8)
    n = np.arange(10, 15, dtype=np.int64)
    first = np.array([1, 0, 0, 0, 0], np.uint8)
    for c, want in ((0, [10, 0, 0, 0, 0]), (1, [10, 11, 0, 0, 0]), (2, [10, 11, 0, 0, 0]), (3, [0] * 5)):
        v, g, sel = ra.settle_routed(ALGS, first, n, np.full(5, c, np.uint32), dec)
        assert v.tolist() == [po.INVALID] * 5 and g.tolist() == want and sel.tolist() == [int(x > 0) for x in want]
    # a dropped member: the group is DROPPED, its takers give back, it gives nothing
    v, g, sel = ra.settle_routed(ALGS, first[:3], n[:3], np.array([0, 1, 2], np.uint32),
                                 np.array([po.ALLOWED, ra.DROPPED, po.DENIED], np.uint8))
    assert v.tolist() == [ra.DROPPED] * 3 and g.tolist() == [10, 0, 12] and sel.tolist() == [1, 0, 1]
    # an allowed group gives nothing back
    v, g, sel = ra.settle_routed(ALGS, first[:2], n[:2], np.array([0, 1], np.uint32), np.array([1, 1], np.uint8))
    assert v.tolist() == [po.ALLOWED] * 2 and not g.any() and not sel.any()


# --- the pack_sel model -----------------------------------------------------------------

def _pack(ops, key, ts, n, cfg, sel=None):
    m, cap, G = key.size, ops.capacity, ops.world
    send = np.zeros((G * cap, 4), np.int64)
    info = np.zeros((G, 4), np.int64)
    slot = np.zeros(max(m, 1), np.int32)
    a = [x.ctypes.data for x in (key.view(np.int64), ts, n, cfg.view(np.int32))]
    if sel is None:
        ops.pack(m, *a, send.ctypes.data, info.ctypes.data, slot.ctypes.data, None)
    else:
        ops.pack_sel(m, *a, sel.ctypes.data, send.ctypes.data, info.ctypes.data, slot.ctypes.data, None)
    return send, info, slot[:m]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_pack_sel_model(world):
    """stability, bucket offsets, info rows 1 to 3 over the whole batch and row
    0 over the selection; all ones equals pack; none selected: every count 0
    and every slot skipped; a skipped request neither counts nor drops"""
    import routed_allow_all_cases as ra
    import shard
    rng = np.random.default_rng(31 + world)
    m = 3000
    key = rng.integers(0, 500, m).astype(np.uint64)
    ts = T0 + np.cumsum(rng.integers(0, 1000, m)).astype(np.int64)
    ts[1500] -= 10_000_000                      # one inversion
    n = rng.integers(1, 9, m).astype(np.int64)
    cfg = rng.integers(0, 5, m).astype(np.uint32)
    own = shard.owner_of(key, world)
    cap = 2048
    for name, sel in (("random", (rng.random(m) < 0.3).astype(np.uint8)), ("all", np.ones(m, np.uint8)),
                      ("none", np.zeros(m, np.uint8)), ("bytes", rng.choice([0, 2, 255], m).astype(np.uint8))):
        ops = ra.RouteOpsSel(world, cap)
        send, info, slot = _pack(ops, key, ts, n, cfg, sel)
        pick = sel != 0
        assert (slot[~pick] == ra.SKIPPED_SLOT).all()
        for o in range(world):
            idx = np.nonzero((own == o) & pick)[0]
            keep, lost = idx[:cap], idx[cap:]
            assert info[o].tolist() == [keep.size, int(ts.min()), int(ts.max()), 2 * lost.size + 1]
            assert slot[keep].tolist() == list(range(o * cap, o * cap + keep.size))      # stable, from the offset
            assert (slot[lost] == -1).all()
            got = send[o * cap:o * cap + keep.size]
            assert np.array_equal(got[:, 0].view(np.uint64), key[keep]) and np.array_equal(got[:, 1], ts[keep])
            assert np.array_equal(got[:, 2], n[keep]) and np.array_equal(got[:, 3] >> 32, keep)
            assert np.array_equal(got[:, 3] & 0xffffffff, cfg[keep])
        if name == "all":
            ref = _pack(ra.RouteOpsSel(world, cap), key, ts, n, cfg)
            assert all(np.array_equal(x, y) for x, y in zip((send, info, slot), ref))
        if name == "none":
            assert not info[:, 0].any() and (info[:, 3] == 1).all() and not ops.overflow
    if world == 1:
        # 3000 requests for one owner, cap 2048: all of them overflow, a
        # selection of 2000 does not, and the skipped ones are neither counted
        # nor dropped
        ops = ra.RouteOpsSel(1, cap)
        sel = np.zeros(m, np.uint8)
        sel[rng.permutation(m)[:2000]] = 1
        _, info, slot = _pack(ops, key, ts, n, cfg, sel)
        assert info[0, 0] == 2000 and info[0, 3] == 1 and not ops.overflow and ops.sel_dropped == 0
        sel[:] = 1
        _, info, slot = _pack(ops, key, ts, n, cfg, sel)
        assert info[0, 0] == cap and info[0, 3] == 2 * (m - cap) + 1 and ops.overflow
    # empty batch
    e = np.zeros(0, np.int64)
    _, info, _ = _pack(ra.RouteOpsSel(world, cap), e.view(np.uint64), e, e, np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert info.tolist() == [[0, (1 << 63) - 1, -(1 << 63), 0]] * world


def test_unpack_skipped_slot():
    """real, dropped and skipped slots in one unpack"""
    import routed_allow_all_cases as ra
    ops = ra.RouteOpsSel(1, 2048)
    back = np.zeros((2048, 4), np.int64)
    back[:3] = [[1, 7, 8, 9], [0, 1, 2, 3], [2, 0, 0, 5]]
    slot = np.array([2, -1, 0, -2, 1, -2], np.int32)
    dec = np.zeros(6, np.uint8)
    o = [np.zeros(6, np.int64) for _ in range(3)]
    ops.unpack(6, slot.ctypes.data, back.ctypes.data, dec.ctypes.data, *(x.ctypes.data for x in o), None)
    assert dec.tolist() == [2, 4, 1, 3, 0, 3]
    assert [x.tolist() for x in o] == [[0, 0, 7, 0, 1, 0], [0, 0, 8, 0, 2, 0], [5, 0, 9, 0, 3, 0]]


# --- the case is what it claims ---------------------------------------------------------

@pytest.mark.parametrize("kind", ["tb", "fw", "sw", "mixed"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_case_coverage(kind, world):
    """routed_allow_all_cases.case asserts its coverage; the cross-rank
    transient takes are proved by re-running the oracle without rank 0"""
    import routed_allow_all_cases as ra
    _, all_batches, cover = ra.case(kind, world)
    assert cover["decide_dropped"] == 0 and cover["refund_dropped"] == 0
    if world > 1:
        assert cover["transient"] >= 5 and cover["multi_rank_targets"] >= 1


def test_case_dropped_member():
    """buckets of 500 records for ~800 members per owner: members past the
    capacity are RL_DROPPED in the decide step, their groups come back
    RL_DROPPED with the takers rolled back, and the refund step -- a
    subsequence of the decide step's sent members -- drops nothing"""
    import routed_allow_all_cases as ra
    _, _, cover = ra.case("mixed", 2, cap=500, check=False)
    assert cover["decide_dropped"] > 100 and cover["refund_dropped"] == 0
    assert cover["dropped_groups"] >= 20 and cover["dropped_takers_back"] >= 20
    assert cover["allowed"] >= 20 and cover["long_runs"] == [17]


# --- the compound through the pipeline --------------------------------------------------

def _pipeline(world, m, cap, sim, align=None, **kw):
    import routed_allow_all_cases as ra
    import routed_op_cases as rc
    import routed_refund_cases as rf
    import shard
    ops = ra.RouteOpsSel(world, cap) if align is None else ra.RouteOpsSel(world, cap, align=align)
    c = ops.capacity
    kw.setdefault("settle", ra.numpy_settle(sim))
    kw.setdefault("refund", rf.oracle_refund(sim, world, c))
    pipe = shard.RoutedPipeline(ops, rc.py_decide(sim, world, c), world, m, "cpu", depth=kw.pop("depth", 4),
                                peek=rc.oracle_peek(sim, world, c), **kw)
    return ops, pipe


def _want_order(lookahead):
    # kinds D A D P are the steps 0, (1, 2), 3, 4
    if lookahead == 0:
        return [(s, b) for b in range(5) for s in ("req", "res")]
    return [("req", 0), ("res", 0), ("req", 1), ("res", 1), ("req", 2), ("req", 3), ("res", 2), ("req", 4),
            ("res", 3), ("res", 4)]


def _worker(rank, world, kinds=("tb", "fw", "sw", "mixed"), cap=4096, align=None, lookaheads=(1, 0)):
    """one rank (routed_refund_cases.run_ranks): every kind's steps D A D P at
    each lookahead -> (ok, [what failed])"""
    import torch
    import torch.distributed as dist

    import routed_allow_all_cases as ra
    import routed_refund_cases as rf
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pg_res = dist.new_group(backend="gloo")
    bad = []
    for kind in kinds:
        configs, all_batches, cover = ra.case(kind, world, cap=None if align is None else cap, check=align is None)
        mine = all_batches[rank]
        for la in lookaheads:
            sim = rf.new_sim(configs)
            ops, pipe = _pipeline(world, 2048, cap, sim, align=align, pg_req=None, pg_res=pg_res, lookahead=la)
            outs = ra.new_outs(torch, ra.KINDS, mine)
            last = ra.run_kinds(pipe, ra.KINDS, [ra.host_tensors(torch, bt) for bt in mine], outs)
            exp = ra.routed_expectations(all_batches, ra.KINDS, rank, configs, cap=ops.capacity)
            miss = ra.mismatches(outs, exp)
            if miss:
                bad.append((kind, la, "outputs", miss))
            if last != 5 or list(pipe.order_log) != _want_order(la) or pipe.collectives != 15 or pipe.wait_s != 0.0:
                bad.append((kind, la, "order", list(pipe.order_log), pipe.collectives))
            if ops.sel_dropped:
                bad.append((kind, la, "pack_sel dropped a give-back", ops.sel_dropped))
            if align is not None:
                rb, v = outs[1][5].numpy(), outs[1][4].numpy()
                if not ((v == ra.DROPPED).any() and ops.overflow and not (rb == ra.DROPPED).any()):
                    bad.append((kind, la, "no dropped group"))
    return not bad, bad


@pytest.mark.parametrize("world", [2, 3])
def test_routed_allow_all_matches_one_shared_store(world):
    """TB, FW, SW and mixed; ~1500 members per rank in groups of 1 to 16 over
    ~120 keys, the steps D A D P at lookahead 1 and 0: every output of every
    step on every rank -- the decide step's four fields, verdict and rollback,
    and the D and P steps after the compound, which pin the state it left --
    and the collective order Res(pending), Req(b), Res(b), Req(b + 1)"""
    import routed_refund_cases as rf
    res = rf.run_ranks(__name__, "_worker", world)
    assert res == {r: (True, []) for r in range(world)}


def test_routed_allow_all_dropped_members():
    """buckets of 500: members dropped at the sender in the decide step make
    their groups RL_DROPPED, the takers of those groups are rolled back, and
    pack_sel drops no give-back"""
    import routed_refund_cases as rf
    res = rf.run_ranks(__name__, "_worker", 2, kinds=("mixed",), cap=500, align=1, lookaheads=(1,))
    assert res == {r: (True, []) for r in range(2)}


def test_routed_allow_all_world1_in_place():
    """world 1 without the exchange: no collective; every kind"""
    import torch

    import routed_allow_all_cases as ra
    import routed_refund_cases as rf
    for kind in ra.CASE_KINDS:
        configs, all_batches, cover = ra.case(kind, 1)
        sim = rf.new_sim(configs)
        ops, pipe = _pipeline(1, 2048, 4096, sim)
        assert not pipe.exchange
        mine = all_batches[0]
        outs = ra.new_outs(torch, ra.KINDS, mine)
        ra.run_kinds(pipe, ra.KINDS, [ra.host_tensors(torch, bt) for bt in mine], outs)
        assert pipe.collectives == 0 and not ops.overflow and ops.sel_dropped == 0
        store = []
        assert not ra.mismatches(outs, ra.routed_expectations(all_batches, ra.KINDS, 0, configs, sim_out=store))
        assert store[0].db == sim.db
        rb = outs[1][5].numpy()
        assert set(rb.tolist()) == {ra.DONE, ra.NOKEY, ra.INVALID}
        assert np.array_equal(rb != ra.INVALID, cover["g"][0] > 0)


def test_routed_allow_all_gives_quota_back():
    """the point of the verb on two keys: [A, B] with B over its limit fails,
    A's take is given back, a peek shows it and the next decide has it"""
    import torch

    import routed_allow_all_cases as ra
    import routed_refund_cases as rf
    configs = [(3, 100, 60 * NS), (1, 20, 12 * NS)]
    sim = rf.new_sim(configs)
    ops, pipe = _pipeline(1, 8, 2048, sim)
    key = np.array([10, 11, 10, 11], np.uint64)
    cfg = np.array([0, 1, 0, 1], np.uint32)
    ts = T0 + np.arange(4, dtype=np.int64)
    first = np.array([1, 0, 1, 0], np.uint8)
    batches = [(key, ts, np.array([30, 25, 5, 5], np.int64), cfg, first),      # [30 of 100, 25 of 20], [5, 5]
               (key, ts + 10, np.zeros(4, np.int64), cfg)]
    kinds = [ra.A, ra.P]
    outs = ra.new_outs(torch, kinds, batches)
    ra.run_kinds(pipe, kinds, [ra.host_tensors(torch, bt) for bt in batches], outs)
    dec, rem, _, _, verdict, rollback = (x.numpy().tolist() for x in outs[0])
    assert dec == [1, 0, 1, 1] and verdict == [0, 0, 1, 1]
    assert rollback == [ra.DONE, ra.INVALID, ra.INVALID, ra.INVALID]     # the bucket was denied: it took nothing
    assert outs[1][1].numpy().tolist() == [95, 15, 95, 15]
    assert not ra.mismatches(outs, ra.routed_expectations([batches], kinds, 0, configs))


# --- errors -----------------------------------------------------------------------------

def test_routed_allow_all_errors():
    """allow_all raises ValueError before anything is enqueued: without
    settle=, without a decide call, without a refund call, and at depth 1;
    settle is keyword-only; it works once everything is there"""
    import torch

    import routed_allow_all_cases as ra
    import routed_refund_cases as rf
    import shard
    configs, all_batches, _ = ra.case("mixed", 1)
    sim = rf.new_sim(configs)
    members = all_batches[0][1]
    ins = ra.host_tensors(torch, members)
    outs = ra.new_outs(torch, [ra.A], [members])[0]
    assert inspect.signature(shard.RoutedPipeline).parameters["settle"].kind is inspect.Parameter.KEYWORD_ONLY
    calls = []

    def build(**kw):
        ops, pipe = _pipeline(1, 2048, 4096, sim, **kw)
        for name in ("pack", "pack_sel"):
            setattr(ops, name, lambda *a, _f=getattr(ops, name), _n=name: (calls.append(_n), _f(*a))[1])
        return pipe

    for match, kw in (("settle", dict(settle=None)), ("refund", dict(refund=None)), ("depth", dict(depth=1))):
        pipe = build(**kw)
        with pytest.raises(ValueError, match=match):
            pipe.allow_all(0, *ins, *outs)
        assert not pipe._pend and len(pipe.order_log) == 0
    pipe = build()
    pipe._calls[shard.OP_DECIDE] = (None, None)
    with pytest.raises(ValueError, match="decide"):
        pipe.allow_all(0, *ins, *outs)
    assert calls == [] and not pipe._pend
    pipe = build()
    pipe.allow_all(0, *ins, *outs)
    pipe.flush()
    assert calls == ["pack", "pack_sel"]
