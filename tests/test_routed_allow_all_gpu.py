"""The routed AllowAll on the GPU (include/rl_route.h):
k_route_hist<true> / k_route_scatter<true> behind rl_route_pack_sel and the
skipped slot of k_route_unpack (csrc/rl_route.hip), k_allow_all_settle_routed
behind rl_allow_all_settle_device (csrc/rl_allow_all.h), and
shard.RoutedPipeline.allow_all end to end on the HIP engine, against the numpy
and plain-Python models and the oracle composition of
tests/routed_allow_all_cases.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import rl_oracle_py as po
from test_routed_allow_all import ALGS, long_patterns, short_patterns
from test_routed_ops_gpu import _dev
from tracegen import CONFIG_SETS, NS, T0

pytestmark = pytest.mark.gpu
DROPPED = 4


def _p(t):
    return t.data_ptr()


# --- 1. pack_sel ------------------------------------------------------------------------

class PackRig:
    """a Router and the numpy model side by side; device buffers of one pack"""

    def __init__(self, rl, world, max_m, cap):
        import torch

        import routed_allow_all_cases as ra
        self.torch, self.ra, self.world = torch, ra, world
        self.r = rl.Router(0, world, max_m, cap)
        self.cap = self.r.capacity
        self.model = lambda: ra.RouteOpsSel(world, cap)
        assert self.model().capacity == self.cap
        self.s = torch.cuda.current_stream().cuda_stream
        self.send = torch.zeros((world * self.cap, 4), dtype=torch.int64, device="cuda")
        self.info = torch.zeros((world, 4), dtype=torch.int64, device="cuda")
        self.slot = torch.zeros(max_m, dtype=torch.int32, device="cuda")

    def device(self, key, ts, n, cfg, sel):
        torch, m = self.torch, key.size
        ins = [_dev(torch, x) for x in (key, ts, n, cfg)]
        self.send.fill_(-3)
        self.slot.fill_(-9)
        if sel is None:
            self.r.pack(m, *[_p(t) for t in ins], _p(self.send), _p(self.info), _p(self.slot), self.s)
        else:
            d_sel = torch.from_numpy(sel).cuda()
            self.r.pack_sel(m, *[_p(t) for t in ins], _p(d_sel), _p(self.send), _p(self.info), _p(self.slot), self.s)
        torch.cuda.synchronize()
        return self.send.cpu().numpy(), self.info.cpu().numpy(), self.slot.cpu().numpy()[:m]

    def host(self, key, ts, n, cfg, sel):
        m, ops = key.size, self.model()
        send = np.full((self.world * self.cap, 4), -3, np.int64)
        info = np.zeros((self.world, 4), np.int64)
        slot = np.zeros(max(m, 1), np.int32)
        a = [x.ctypes.data for x in (key.view(np.int64), ts, n, cfg.view(np.int32))]
        ops.pack_sel(m, *a, sel.ctypes.data, send.ctypes.data, info.ctypes.data, slot.ctypes.data, None)
        return send, info, slot[:m], ops


def _sel_patterns(m):
    tile = np.zeros(m, np.uint8)
    tile[::1024] = 1
    last = np.zeros(m, np.uint8)
    last[-1] = 7
    alt = (np.arange(m) & 1).astype(np.uint8) * 255
    return {"none": np.zeros(m, np.uint8), "all": np.ones(m, np.uint8), "alternating": alt,
            "one per tile": tile, "last": last}


@pytest.mark.parametrize("world", [1, 2, 3])
def test_pack_sel_matches_model(rl, world):
    """send, send_info and slot against the numpy model at m around the wave,
    the block and the 1024-request tile, for five selections, with ts sorted
    and with one inversion between two skipped requests (the unsorted bit is
    still set); all ones: bit for bit Router.pack's"""
    rig = PackRig(rl, world, 4097, 4097)
    rng = np.random.default_rng(70 + world)
    for m in (1, 63, 64, 65, 1023, 1024, 1025, 4097):
        key = rng.integers(0, 1 << 40, m).astype(np.uint64)
        n = rng.integers(1, 1 << 40, m).astype(np.int64)
        cfg = rng.integers(0, 15, m).astype(np.uint32)
        for name, sel in _sel_patterns(m).items():
            for inverted in (False, True):
                ts = T0 + 1000 * np.arange(m, dtype=np.int64)
                skipped = np.nonzero(sel == 0)[0]
                if inverted:
                    if skipped.size < 2:
                        continue
                    ts[skipped[-1]] = ts[skipped[0]] - 1
                got = rig.device(key, ts, n, cfg, sel)
                send, info, slot, ops = rig.host(key, ts, n, cfg, sel)
                what = (world, m, name, inverted)
                assert np.array_equal(got[1], info), what
                assert np.array_equal(got[2], slot), what
                assert np.array_equal(got[0], send), what       # untouched records included
                assert (info[:, 3] & 1).all() == bool(inverted and m > 1) and not ops.overflow
                assert info[:, 0].sum() == int((sel != 0).sum())
                if name == "all":
                    ref = rig.device(key, ts, n, cfg, None)
                    assert all(np.array_equal(x, y) for x, y in zip(got, ref)), what
    assert rig.r.sync(None) == rl.RL_OK
    rig.r.close()


def test_pack_sel_capacity(rl):
    """world 2, 6000 requests of which ~3000 are owner 0's, buckets of 2048:
    with every request selected owner 0's overflow and the status is raised;
    with 2040 of owner 0's selected nothing is dropped -- the skipped requests
    of that owner are neither counted nor dropped -- and with 2100 selected
    exactly 52 are, the last ones in batch order"""
    import shard
    rig = PackRig(rl, 2, 6000, 2048)
    assert rig.cap == 2048
    rng = np.random.default_rng(9)
    m = 6000
    key = rng.integers(0, 1 << 40, m).astype(np.uint64)
    ts = T0 + np.arange(m, dtype=np.int64)
    n, cfg = np.ones(m, np.int64), np.zeros(m, np.uint32)
    mine = np.nonzero(shard.owner_of(key, 2) == 0)[0]
    other = np.nonzero(shard.owner_of(key, 2) == 1)[0]
    assert mine.size > 2600 and other.size > 2600
    for count, dropped in ((2040, 0), (2100, 52), (mine.size, mine.size - 2048)):
        sel = np.zeros(m, np.uint8)
        pick = np.sort(rng.permutation(mine)[:count])
        sel[pick] = 1
        sel[other[:100]] = 1
        got = rig.device(key, ts, n, cfg, sel)
        send, info, slot, ops = rig.host(key, ts, n, cfg, sel)
        assert all(np.array_equal(x, y) for x, y in zip(got, (send, info, slot)))
        assert got[1][0].tolist() == [count - dropped, int(ts[0]), int(ts[-1]), 2 * dropped]
        assert got[1][1].tolist() == [100, int(ts[0]), int(ts[-1]), 0]
        assert (got[2][sel == 0] == -2).all() and int((got[2] == -1).sum()) == dropped
        assert (got[2][pick[count - dropped:]] == -1).all()
        assert rig.r.sync(None) == (rl.RL_EOVERFLOW if dropped else rl.RL_OK)
    rig.r.close()


def test_unpack_real_dropped_and_skipped_slots(rl):
    """one unpack over real, dropped and skipped slots: a skipped request gets
    {RL_INVALID, 0, 0, 0}, a dropped one {RL_DROPPED, 0, 0, 0}"""
    import torch
    r = rl.Router(0, 1, 4096, 2048)
    m = 3000
    rng = np.random.default_rng(4)
    back = rng.integers(1, 1 << 50, (2048, 4)).astype(np.int64)
    back[:, 0] = rng.integers(0, 4, 2048)
    slot = rng.integers(0, 2048, m).astype(np.int32)
    slot[rng.random(m) < 0.3] = -1
    slot[rng.random(m) < 0.3] = -2
    slot[[0, 63, 64, m - 1]] = [-2, -1, -2, -2]
    outs = [torch.full((m,), 9, dtype=torch.uint8, device="cuda")] + \
        [torch.full((m,), 9, dtype=torch.int64, device="cuda") for _ in range(3)]
    d_back, d_slot = torch.from_numpy(back).cuda(), torch.from_numpy(slot).cuda()
    r.unpack(m, _p(d_slot), _p(d_back), *[_p(x) for x in outs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = back[np.where(slot < 0, 0, slot)]
    want[slot == -1] = [DROPPED, 0, 0, 0]
    want[slot == -2] = [po.INVALID, 0, 0, 0]
    assert (slot == -1).sum() > 100 and (slot == -2).sum() > 100 and (slot >= 0).sum() > 100
    for f in range(4):
        assert np.array_equal(outs[f].cpu().numpy().astype(np.int64), want[:, f]), f
    r.close()


# --- 2. the settle kernel ---------------------------------------------------------------

class SettleRig:
    def __init__(self, rl, max_batch):
        import torch
        self.torch = torch
        self.eng = rl.Engine(profile=0, tb_capacity=1 << 10, win_capacity=1 << 10, max_batch=max_batch)
        for a in ALGS:                       # config c: algorithm ALGS[c]; config 3 is unknown
            self.eng.register(a, 10, NS)
        self.s = torch.cuda.current_stream().cuda_stream

    def run(self, first, cfg, n, dec):
        torch, m = self.torch, first.size
        ins = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (first, cfg.view(np.int32), n, dec)]
        outs = [torch.full((m,), 99, dtype=torch.uint8, device="cuda"),
                torch.full((m,), -99, dtype=torch.int64, device="cuda"),
                torch.full((m,), 99, dtype=torch.uint8, device="cuda")]
        self.eng.allow_all_settle(m, *[_p(t) for t in ins], *[_p(t) for t in outs], self.s)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in outs]

    def check(self, first, dec, what, seed=0):
        import routed_allow_all_cases as ra
        rng = np.random.default_rng(seed)
        m = first.size
        cfg = rng.integers(0, 4, m).astype(np.uint32)
        n = rng.integers(1, 1 << 40, m).astype(np.int64)
        got = self.run(first, cfg, n, dec)
        want = ra.settle_routed(ALGS, first, n, cfg, dec, scans=False)
        for name, g, w in zip(("verdict", "g", "sel"), got, want):
            bad = np.nonzero(g != w)[0]
            assert bad.size == 0, (what, name, bad[:8], g[bad[:8]], w[bad[:8]])
        return got


def test_settle_kernel_short_patterns_and_edges(rl):
    """every short pattern (tests/test_routed_allow_all.py) concatenated into
    one launch; groups across the lanes 63|64 and the 256-thread block edge; a
    group ending at M - 1; first[0] == 0; M = 1; runs of 15, 16, 17 and 33"""
    rig = SettleRig(rl, 1 << 19)
    firsts, decs = [], []
    for first, dec in short_patterns():
        first = first.copy()
        first[0] = 1                         # each pattern starts its own group in the concatenation
        firsts.append(first)
        decs.append(dec)
    first, dec = np.concatenate(firsts), np.concatenate(decs)
    first[0] = 0
    assert 100_000 < first.size <= 1 << 19
    got = rig.check(first, dec, "short patterns")
    assert set(got[0].tolist()) == {0, 1, 2, 3, 4}
    # groups of 5 shifted so that one straddles 63|64 and one 255|256; the last ends at M - 1
    rng = np.random.default_rng(2)
    for shift in range(5):
        m = 600 + shift
        first = np.zeros(m, np.uint8)
        first[shift::5] = 1
        dec = rng.choice([0, 1, 2, 3, 4, 7], m, p=[0.1, 0.7, 0.05, 0.05, 0.05, 0.05]).astype(np.uint8)
        rig.check(first, dec, ("shift", shift), seed=shift)
    for d in (0, 1, 2, 3, 4, 200):
        v, g, sel = rig.check(np.array([0], np.uint8), np.array([d], np.uint8), ("M = 1", d), seed=d)
        assert v.tolist() == [d if d < 5 else 3]
    first, dec, sizes = long_patterns()
    rig.check(first, dec, "long runs")
    rig.eng.close()


def test_settle_kernel_grid_stride(rl):
    """M = rl_allow_all_grid_cap() + 4096 + 37: every thread strides to a second
    member; runs of 17 and 33 on the stride's seam; a ragged tail"""
    cap = rl.ALLOW_ALL_GRID_CAP
    m = cap + 4096 + 37
    assert m == 1024 * 256 + 4096 + 37
    rig = SettleRig(rl, 1 << 19)
    rng = np.random.default_rng(6)
    sizes = []
    while sum(sizes) < m:
        sizes.append(int(rng.integers(1, 17)))
    heads = np.cumsum([0] + sizes[:-1])
    first = np.zeros(sum(sizes), np.uint8)[:m]
    first[heads[heads < m]] = 1
    first[cap - 20:cap + 40] = 0
    first[[cap - 20, cap - 3, cap + 30]] = 1                     # runs of 17 and of 33 across the seam
    dec = rng.choice([0, 1, 2, 3, 4, 9], m, p=[0.1, 0.75, 0.04, 0.04, 0.04, 0.03]).astype(np.uint8)
    got = rig.check(first, dec, "grid stride")
    assert (got[0][cap - 20:cap + 30] == po.INVALID).all()
    assert set(got[0].tolist()) == {0, 1, 2, 3, 4}
    rig.eng.close()


# --- 3. the compound ---------------------------------------------------------------------

def _all_keys_peek(all_batches, configs, t):
    """a peek (n = 0) of every key any rank used, after everything"""
    key = np.unique(np.concatenate([b[0] for bs in all_batches for b in bs]))
    ncfg = len(configs)
    return (key, np.full(key.size, t, np.int64), np.zeros(key.size, np.int64),
            (key % np.uint64(ncfg)).astype(np.uint32))


def _compound_rank(rank, world, backend="nccl", exchange=None, cases=(("mixed", 0),), flags=0, lookahead=None):
    """one rank (routed_refund_cases.run_ranks) of the native path on cuda:0:
    per (kind, profile) the steps D A D P and a peek of every key, back to back
    -> (ok, info)"""
    import torch
    import torch.distributed as dist

    import rl_amd
    import routed_allow_all_cases as ra
    import shard
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    pg_res = dist.new_group(backend=backend)
    info = {"bad": [], "runs": 0}
    kinds = ra.KINDS + [ra.P]
    for kind, profile in cases:
        configs, all_batches, cover = ra.case(kind, world)
        t_end = max(int(b[1].max()) for bs in all_batches for b in bs) + 1000
        all_batches = [bs + [_all_keys_peek(all_batches, configs, t_end)] for bs in all_batches]
        mine = all_batches[rank]
        m = max(b[0].size for b in mine)
        router = rl_amd.Router(0, world, m, m)
        eng = rl_amd.Engine(profile=profile, tb_capacity=1 << 14, win_capacity=1 << 14,
                            max_batch=world * router.capacity, flags=flags)
        for a, L, W in configs:
            eng.register(a, L, W)
        pipe = shard.RoutedPipeline(router, eng.decide_routed, world, m, "cuda:0", pg_req=None, pg_res=pg_res,
                                    exchange=exchange, staged=backend == "gloo", decide_ev=eng.decide_routed_ev,
                                    peek=eng.peek_routed, peek_ev=eng.peek_routed_ev, refund=eng.refund_routed,
                                    refund_ev=eng.refund_routed_ev, settle=eng.allow_all_settle, lookahead=lookahead)
        ins = [tuple(_dev(torch, x) for x in bt) for bt in mine]
        outs = ra.new_outs(torch, kinds, mine, device="cuda")
        torch.cuda.synchronize()
        st0 = eng.stats()
        ra.run_kinds(pipe, kinds, ins, outs)           # no host synchronisation between the steps
        torch.cuda.synchronize()
        status = (eng.sync(), router.sync(None))
        exp = ra.routed_expectations(all_batches, kinds, rank, configs, profile=profile, cap=router.capacity)
        bad = ra.mismatches(outs, exp)
        st = eng.stats()
        # rl_stats moves as for the decide steps (D, A's, D): the refund and peek steps are not counted
        if bad or status != (0, 0) or int(st.batches) - int(st0.batches) != 3:
            info["bad"].append((kind, profile, status, int(st.batches) - int(st0.batches), bad))
        # at either lookahead: D's result side is issued before the compound's Req(1), Res(1), Req(2)
        head = [("req", 0), ("res", 0), ("req", 1), ("res", 1), ("req", 2)]
        if pipe.exchange and (pipe.collectives != 3 * 6 or list(pipe.order_log)[:5] != head):
            info["bad"].append((kind, profile, "collectives", pipe.collectives, list(pipe.order_log)))
        rb = outs[1][5].cpu().numpy()
        if not {ra.DONE, ra.NOKEY, ra.INVALID} <= set(rb.tolist()):
            info["bad"].append((kind, profile, "rollback values", sorted(set(rb.tolist()))))
        info["runs"] += 1
        info["exchange"] = pipe.exchange
        del pipe
        eng.close()
        router.close()
        rl_amd.release_dedicated_streams()
    return not info["bad"], info


def _spawn(world, backend, **kw):
    import routed_refund_cases as rf
    res = rf.run_ranks(__name__, "_compound_rank", world, limit=240, backend=backend, **kw)
    for r in range(world):
        ok, info = res[r]
        assert ok, (r, info)
    return res


ALL_CASES = tuple((k, p) for k in ("tb", "fw", "sw", "mixed") for p in (0, 1))


def test_routed_allow_all_in_place():
    """world 1 without the exchange, TB, FW, SW and mixed on both profiles:
    every output of D A D P, verdict and rollback, and a peek of every key
    afterwards, against the oracle composition"""
    res = _spawn(1, "nccl", cases=ALL_CASES)
    assert res[0][1]["runs"] == 8 and res[0][1]["exchange"] is False


def test_routed_allow_all_in_flight_on_a_pipelined_engine():
    """RL_OPT_PIPELINE: D A D P issued back to back with no host
    synchronisation between them; the decide after the compound sees its
    give-backs"""
    import rl_amd
    _spawn(1, "nccl", cases=(("mixed", 0), ("sw", 1)), flags=rl_amd.OPT_PIPELINE)


@pytest.mark.parametrize("lookahead", [0, 1])
def test_routed_allow_all_one_rank_rccl(lookahead):
    """world 1 with the exchange forced on: every step's three collectives over
    RCCL, in the order Res(pending), Req(b), Res(b), Req(b + 1)"""
    res = _spawn(1, "nccl", exchange=True, cases=(("mixed", 0), ("mixed", 1)), lookahead=lookahead)
    assert res[0][1]["exchange"] is True


def test_routed_allow_all_two_ranks_one_gpu():
    """two ranks (two engines, two routers) on the one GPU, all-to-alls through
    host memory: groups whose members live on both ranks, give-backs of both
    ranks summed on the owner, groups denied on the other rank's transient take"""
    _spawn(2, "gloo", cases=(("mixed", 0), ("fw", 1)))


def test_routed_allow_all_equals_engine_allow_all(rl):
    """world 1 in place, every member in one millisecond (one store clock, so
    the give-backs run at the clock the members decided at): outputs and state
    equal Engine.allow_all's on the same members"""
    import torch

    import routed_allow_all_cases as ra
    import shard
    from reset_cases import engine_keys
    configs = CONFIG_SETS["mixed"]
    _, all_batches, _ = ra.case("mixed", 1)
    key, _, n, cfg, first = all_batches[0][1]
    m = key.size
    ts = T0 + np.arange(m, dtype=np.int64)                    # one millisecond
    now_ms = T0 // 1_000_000
    router = rl.Router(0, 1, m, m)
    a = rl.Engine(profile=0, tb_capacity=1 << 14, win_capacity=1 << 14, max_batch=router.capacity)
    b = rl.Engine(profile=0, tb_capacity=1 << 14, win_capacity=1 << 14, max_batch=router.capacity)
    for alg, L, W in configs:
        a.register(alg, L, W)
        b.register(alg, L, W)
    pipe = shard.RoutedPipeline(router, a.decide_routed, 1, m, "cuda:0", decide_ev=a.decide_routed_ev,
                                refund=a.refund_routed, refund_ev=a.refund_routed_ev, settle=a.allow_all_settle)
    ins = tuple(_dev(torch, x) for x in (key, ts, n, cfg, first))
    outs = ra.new_outs(torch, [ra.A], [all_batches[0][1]], device="cuda")[0]
    pipe.allow_all(0, *ins, *outs)
    pipe.flush()
    torch.cuda.synchronize()
    assert a.sync() == rl.RL_OK and router.sync(None) == rl.RL_OK
    ref = b.allow_all(key, ts, n, cfg, first, server_ms=np.full(m, now_ms))
    got = [x.cpu().numpy() for x in outs]
    for name, g, w in zip(("decision", "remaining", "retry_after_ns", "reset_at_ns", "verdict", "rollback"), got,
                          (ref.decision, ref.remaining, ref.retry_after_ns, ref.reset_at_ns, ref.verdict, ref.rollback)):
        assert np.array_equal(g, w), name
    assert {ra.DONE, ra.INVALID} <= set(got[5].tolist()) and {0, 1, 3} <= set(got[4].tolist())
    zeros = np.zeros(m, np.int64)
    pa = a.peek(key, ts, zeros, cfg, np.full(m, now_ms), want_tokens=True)
    pb = b.peek(key, ts, zeros, cfg, np.full(m, now_ms), want_tokens=True)
    for f in ("decision", "remaining", "retry_after_ns", "reset_at_ns"):
        assert np.array_equal(getattr(pa, f), getattr(pb, f)), f
    assert np.array_equal(pa.tokens.view(np.uint64), pb.tokens.view(np.uint64))
    assert engine_keys(rl, a, now_ms) == engine_keys(rl, b, now_ms)
    del pipe
    a.close()
    b.close()
    router.close()
    rl.release_dedicated_streams()


# --- 4. the owner's refund bound ---------------------------------------------------------

def test_routed_allow_all_refund_bound(rl):
    """more give-backs in the merged refund step than the engine's refund bound.
    rl_refund_max is min(max_batch, 2^20) and a refund step never carries more
    requests than its decide step, which max_batch bounds too, so the bound can
    be passed only above 2^20: 2^20 + 4096 members in failing pairs [a fixed
    window that allows, a fixed window asked for twice its limit], every member a
    taker.  The give-backs past the bound come back rollback == RL_DROPPED, the
    next rl_engine_sync returns RL_EOVERFLOW, their takes are still in place,
    and re-issuing them as an OP_REFUND step restores the state before the
    compound"""
    import torch

    import shard
    L = 10 ** 9
    configs = [(3, L, 3600 * NS)]
    m = (1 << 20) + 4096
    router = rl.Router(0, 1, m, m)
    assert router.capacity == m
    eng = rl.Engine(profile=0, tb_capacity=1 << 10, win_capacity=1 << 14, max_batch=m)
    eng.register(*configs[0])
    bound = eng.refund_max()
    assert bound == 1 << 20
    nk = 1000
    keys = np.arange(1, nk + 1, dtype=np.uint64)
    zk = np.uint64(5000)
    allk = np.append(keys, zk)
    zc = np.zeros(allk.size, np.uint32)
    eng.decide(allk, np.full(allk.size, T0), np.full(allk.size, 5), zc)          # every key holds 5
    key = np.empty(m, np.uint64)
    key[0::2] = keys[np.arange(m // 2) % nk]
    key[1::2] = zk
    n = np.ones(m, np.int64)
    n[1::2] = 2 * L
    first = np.zeros(m, np.uint8)
    first[0::2] = 1
    ts = T0 + 10 + np.arange(m, dtype=np.int64)                                   # in time order: merge order = batch order
    cfg = np.zeros(m, np.uint32)
    pipe = shard.RoutedPipeline(router, eng.decide_routed, 1, m, "cuda:0", decide_ev=eng.decide_routed_ev,
                                peek=eng.peek_routed, peek_ev=eng.peek_routed_ev, refund=eng.refund_routed,
                                refund_ev=eng.refund_routed_ev, settle=eng.allow_all_settle)
    ins = tuple(_dev(torch, x) for x in (key, ts, n, cfg, first))
    new = lambda dt: torch.empty(m, dtype=dt, device="cuda")
    dec, verdict, rollback = new(torch.uint8), new(torch.uint8), new(torch.uint8)
    rem, retry, reset = new(torch.int64), new(torch.int64), new(torch.int64)
    pipe.allow_all(0, *ins, dec, rem, retry, reset, verdict, rollback)
    pipe.flush()
    torch.cuda.synchronize()
    assert eng.sync() == rl.RL_EOVERFLOW and eng.sync() == rl.RL_OK
    assert router.sync(None) == rl.RL_OK                                          # the sender dropped nothing
    d, v, rb = dec.cpu().numpy(), verdict.cpu().numpy(), rollback.cpu().numpy()
    assert (d[0::2] == po.ALLOWED).all() and (d[1::2] == po.DENIED).all() and (v == po.DENIED).all()
    assert (rb[:bound] == 1).all() and (rb[bound:] == DROPPED).all()
    now_ms = (T0 + 10 + m) // 1_000_000 + 1
    peek = lambda: eng.peek(allk, np.full(allk.size, T0 + 9), np.zeros(allk.size, np.int64), zc,
                            np.full(allk.size, now_ms)).remaining
    left = np.bincount((np.arange(m // 2) % nk)[bound // 2:], minlength=nk)        # the takes still in place
    assert left.sum() == 2048
    assert (L - peek()[:nk] == 5 + left).all()
    # the caller re-issues the dropped give-backs as a refund step
    again = tuple(_dev(torch, x[bound:]) for x in (key, ts, n, cfg))
    k = m - bound
    outs = (new(torch.uint8)[:k], new(torch.int64)[:k], new(torch.int64)[:k], new(torch.int64)[:k])
    pipe.step(2, *again, *outs, op=shard.OP_REFUND)
    pipe.flush()
    torch.cuda.synchronize()
    assert eng.sync() == rl.RL_OK
    assert (outs[0].cpu().numpy() == 1).all()
    assert (L - peek() == 5).all()                                                # Z too: every key as before the compound
    del pipe
    eng.close()
    router.close()
    rl.release_dedicated_streams()


# --- 5. arguments ------------------------------------------------------------------------

def test_new_calls_arguments(rl):
    """rl_route_pack_sel and rl_allow_all_settle_device: a null handle, a null
    array with m > 0 and m above max_batch are RL_EINVAL; m == 0 is a no-op"""
    import torch
    m = 64
    r = rl.Router(0, 1, 2048, 2048)
    eng = rl.Engine(profile=0, tb_capacity=1 << 10, win_capacity=1 << 10, max_batch=2048)
    eng.register(1, 10, NS)
    t = lambda dt, k=2048: torch.zeros(k, dtype=dt, device="cuda")
    fn = rl.lib.rl_route_pack_sel
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    # key, ts, n, cfg, sel, send, send_info, slot
    tensors = [t(torch.int64) for _ in range(3)] + [t(torch.int32), t(torch.uint8), t(torch.int64, 4 * 2048),
                                                    t(torch.int64, 4), t(torch.int32)]
    good = [r.h, m] + [_p(x) for x in tensors] + [None]
    assert fn(*good) == rl.RL_OK
    for k in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        bad = list(good)
        bad[k] = None
        assert fn(*bad) == rl.RL_EINVAL, k
    assert fn(*(good[:1] + [2049] + good[2:])) == rl.RL_EINVAL
    assert fn(r.h, 0, None, None, None, None, None, None, good[8], None, None) == rl.RL_OK
    assert fn(r.h, 0, None, None, None, None, None, None, None, None, None) == rl.RL_EINVAL   # the info rows are written
    torch.cuda.synchronize()
    assert r.sync(None) == rl.RL_OK
    fs = rl.lib.rl_allow_all_settle_device
    assert fs.restype is C.c_int and len(fs.argtypes) == 10
    st = [t(torch.uint8), t(torch.int32), t(torch.int64), t(torch.uint8), t(torch.uint8), t(torch.int64),
          t(torch.uint8)]
    good = [eng.h, m] + [_p(x) for x in st] + [None]
    assert fs(*good) == rl.RL_OK
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        bad = list(good)
        bad[k] = None
        assert fs(*bad) == rl.RL_EINVAL, k
    assert fs(*(good[:1] + [2049] + good[2:])) == rl.RL_EINVAL
    assert fs(eng.h, 0, None, None, None, None, None, None, None, None) == rl.RL_OK
    torch.cuda.synchronize()
    with pytest.raises(rl.EngineError):
        eng.allow_all_settle(2049, *good[2:9])
    assert eng.sync() == rl.RL_OK
    eng.close()
    r.close()
