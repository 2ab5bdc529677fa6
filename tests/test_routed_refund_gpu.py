"""The refund step of the routed path on the GPU: k_refund_add_routed and
k_refund_apply (csrc/rl_refund.h) behind rl_refund_routed_device
(include/rl_route.h), and shard.RoutedPipeline's refund kind end to end.  The
routed kernel is pinned to the array form (Engine.refund, itself pinned to the
oracle in tests/test_refund_gpu.py) and to refund_cases.apply_refunds on the
Python oracle, through the statuses and through Peek (n = 0, tokens as bit
patterns) of everything the engines hold; the whole path to ONE shared store
(tests/routed_refund_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import rl_snapshot as snap
from peek_cases import assert_peek, peek_expected
from refund_cases import DONE, INVALID, NOKEY, apply_refunds, new_sim
from reset_cases import engine_keys
from test_refund_gpu import engine_state
from test_routed_ops_gpu import SENTINEL, Rig, _dev, _fingerprint
from tracegen import CONFIG_SETS, NS, T0, skewed_trace

pytestmark = pytest.mark.gpu
CONFIGS = CONFIG_SETS["mixed"]
KEY_RESERVED = (1 << 64) - 1
DROPPED = 4


def merge_order(ts):
    """world 1: the merge order of one source -- by arrival (the running max of
    its ts), ties by position"""
    return np.lexsort((np.arange(ts.size), np.maximum.accumulate(ts))) if ts.size else np.zeros(0, np.int64)


def populate(rig, sim, seed, m=3000, nkeys=150):
    """test_routed_ops_gpu.populate, on the Python oracle as well: a routed
    decide step on app servers with skewed clocks -- token buckets, window
    entries and spilled windows"""
    key, ts, n, cfg, _ = skewed_trace(seed, m, nkeys, CONFIGS)
    sms = rig.route(key, ts, n, cfg)
    rig.eng.decide_routed(*rig.args())
    rig.results()
    assert rig.eng.sync() == rig.rl.RL_OK
    info = rig.eng.table_info(0)
    assert info.tb_used > 0 and info.win_used > 0 and info.spill_used > 0
    if sim is not None:
        for i in merge_order(ts).tolist():
            sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]), int(sms[i]))
    return key, ts, n, cfg


def refund_batch(rng, c, pop, in_order):
    """c refunds aimed at the populate step's own requests (their keys at their
    own times: windows of every age, wherever they live), at the time after
    them, at keys never seen; n small or up to 2^40; a few n <= 0, unknown cfgs
    and the reserved key; duplicates by construction (c picks of 150 keys)"""
    pkey, pts, _, _ = pop
    pick = rng.integers(0, pkey.size, c)
    key = pkey[pick].copy()
    ts = np.where(rng.random(c) < 0.6, pts[pick], int(pts.max()) + rng.integers(0, 3_000_000_000, c)).astype(np.int64)
    key[rng.random(c) < 0.1] += np.uint64(100_000)
    n = rng.choice([1, 1, 1, 2, 3], c).astype(np.int64)
    big = rng.random(c) < 0.1
    n[big] = rng.integers(1, (1 << 40) + 1, int(big.sum()))
    n[rng.random(c) < 0.03] = rng.choice([0, -1, -5])
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    cfg[rng.random(c) < 0.03] = 99
    key[rng.random(c) < 0.03] = np.uint64(KEY_RESERVED)
    return shape_order(key, ts, n, cfg, in_order)


def shape_order(key, ts, n, cfg, in_order):
    """ts sorted (the merge's RL_ORDER_IDENTITY form at world 1) or, for the
    explicit order, with a descent somewhere"""
    if in_order:
        o = np.argsort(ts, kind="stable")
        return key[o], ts[o], n[o], cfg[o]
    if ts.size > 1 and not np.any(ts[1:] < ts[:-1]):
        ts = ts.copy()
        ts[0] = ts.max() + 1
    return key, ts, n, cfg


def refund_step(rig, batch, want_identity=None, m_max=None):
    """pack -> merge -> refund_routed -> unpack of one batch: (the four result
    fields in the caller's order, every request's store clock)"""
    key, ts, n, cfg = batch
    sms = rig.route(key, ts, n, cfg)
    rig.eng.refund_routed(*rig.args(m_max))
    got = rig.results()
    if want_identity is not None and key.size > 1:
        assert rig.identity_form() == want_identity
    return got, sms


def peek_all(eng, key, ts, cfg, now_ms):
    return eng.peek(key, ts, np.zeros(key.size, np.int64), cfg, np.full(key.size, now_ms), want_tokens=True)


def assert_same_peek(a, b, what):
    for f in ("decision", "remaining", "retry_after_ns", "reset_at_ns"):
        x, y = getattr(a, f), getattr(b, f)
        bad = np.nonzero(x != y)[0]
        assert bad.size == 0, f"{what}: {f} differs at {bad[:8]}: {x[bad[:8]]} / {y[bad[:8]]}"
    assert np.array_equal(a.tokens.view(np.uint64), b.tokens.view(np.uint64)), f"{what}: tokens differ"


# --- 1. the routed kernel against the array form and the oracle -------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_refund_routed_equals_refund(rl, profile, in_order):
    """two engines populated alike; one runs pack -> merge -> refund_routed, the
    other Engine.refund of the same (key, ts, n, cfg, store clock): equal
    statuses at counts around the wave, the block and one bucket tile, and
    Peek (n = 0) of every populated key and window equal on all fields between
    the two and against apply_refunds on the Python oracle"""
    rng = np.random.default_rng(190 + profile)
    a, b = Rig(rl, profile, 8192), Rig(rl, profile, 8192)
    sim = new_sim(profile, CONFIGS)
    pop = populate(a, sim, 141 + profile)
    populate(b, None, 141 + profile)
    assert a.eng.table_info(0).spill_used > 0 and b.eng.table_info(0).spill_used > 0
    seen = set()
    now_ms = int(pop[1].max()) // 1_000_000
    for c in (0, 1, 63, 64, 65, 255, 257, 2049):
        key, ts, n, cfg = batch = refund_batch(rng, c, pop, in_order)
        st0 = a.eng.stats()
        got, sms = refund_step(a, batch, in_order)
        assert bytes(a.eng.stats()) == bytes(st0)                      # rl_stats does not move
        assert not got[1].any() and not got[2].any() and not got[3].any()
        ref = b.eng.refund(key, ts, n, cfg, sms) if c else np.zeros(0, np.uint8)
        assert np.array_equal(got[0], ref), f"count {c}: routed and array form differ"
        o = merge_order(ts)
        want = np.zeros(c, np.uint8)
        if c:
            want[o] = apply_refunds(sim, key[o], ts[o], n[o], cfg[o], sms[o])[0]
            now_ms = max(now_ms, int(sms.max()))
        assert np.array_equal(got[0], want), f"count {c}: status differs from the oracle"
        seen |= set(got[0].tolist())
    assert seen >= {NOKEY, DONE, INVALID}
    assert a.eng.sync() == rl.RL_OK and b.eng.sync() == rl.RL_OK
    pkey, pts, _, pcfg = pop
    pa, pb = peek_all(a.eng, pkey, pts, pcfg, now_ms), peek_all(b.eng, pkey, pts, pcfg, now_ms)
    assert_same_peek(pa, pb, "peek after the refunds")
    zeros = np.zeros(pkey.size, np.int64)
    assert_peek(pa, peek_expected(sim, pkey, pts, zeros, pcfg, np.full(pkey.size, now_ms)), CONFIGS, pcfg, "oracle")
    assert engine_keys(rl, a.eng, now_ms) == engine_keys(rl, b.eng, now_ms)
    a.close()
    b.close()


# --- 2. merge shapes ------------------------------------------------------------------

def _counter_rig(rl, max_m, keys, have, max_batch=None):
    """fixed-window counters holding `have` each, on the engine and the oracle"""
    configs = [(3, 10 ** 9, 3600 * NS)]
    rig = Rig(rl, 0, max_m, max_batch=max_batch, configs=configs, tb=1 << 6, win=1 << 12)
    sim = new_sim(0, configs)
    z = np.zeros(keys.size, np.uint32)
    for off in range(0, keys.size, 512):
        k = keys[off:off + 512]
        rig.eng.decide(k, np.full(k.size, T0), np.full(k.size, have), z[:k.size])
    for k in keys.tolist():
        sim.decide(int(k), T0, have, 0, T0 // 1_000_000)
    return rig, sim, configs


def _check_counters(rig, sim, configs, keys, what):
    z = np.zeros(keys.size, np.uint32)
    ts = np.full(keys.size, T0 + 9)
    now_ms = (T0 + 10_000) // 1_000_000
    got = peek_all(rig.eng, keys, ts, z, now_ms)
    assert_peek(got, peek_expected(sim, keys, ts, np.zeros(keys.size, np.int64), z, np.full(keys.size, now_ms)),
                configs, z, what)
    return got


def test_refund_routed_merge_shapes(rl):
    """in the explicit-order form (every lane's request comes through order[]):
    a wave whose 64 lanes all name one target, a wave of 64 different targets,
    one target's contributors across a wave boundary and across a block
    boundary, and one target at merge positions 0 and m - 1"""
    keys = np.arange(1, 201, dtype=np.uint64)
    have = 10 ** 7
    rig, sim, configs = _counter_rig(rl, 2048, keys, have)
    m = 1000
    which = np.empty(m, np.int64)
    which[:64] = 1                           # wave 0: one target
    which[64:128] = np.arange(100, 164)      # wave 1: 64 targets
    which[128:] = 170 + np.arange(m - 128) % 20
    which[188:197] = 2                       # across the wave boundary at 192
    which[250:263] = 3                       # across the block boundary at 256
    which[503:530] = 3                       # ... and again across 512
    for step, (first, last) in enumerate(((1, 1), (4, 4), (5, 6))):
        w = which.copy()
        w[0], w[-1] = first, last            # (4, 4): one target at positions 0 and m - 1 only
        key = keys[w - 1]
        n = np.arange(1, m + 1, dtype=np.int64) + step
        ts = np.full(m, T0 + 5, np.int64)
        ts[0] = T0 + 5000                    # a descent: the explicit order, which at world 1 is the received one
        cfg = np.zeros(m, np.uint32)
        got, sms = refund_step(rig, (key, ts, n, cfg), want_identity=False)
        want = apply_refunds(sim, key, ts, n, cfg, sms)[0]
        assert np.array_equal(got[0], want) and (want == DONE).all()
    assert rig.eng.sync() == rl.RL_OK
    got = _check_counters(rig, sim, configs, keys, "merge shapes")
    assert (10 ** 9 - got.remaining[3]) == have - (2 + 1001)          # key 4: positions 0 and m - 1 of step 1
    rig.close()


# --- 3. the sum rule on the device --------------------------------------------------------

def test_refund_routed_sum_rule(rl):
    """the bucket of §10i: 0.9763120008305 + 4 + 45.  The two refunds in one
    routed step -- in one wave, and in different blocks -- store q14(t + 49);
    the same two in two steps store q14(q14(t + 4) + 45)"""
    configs = [(1, 10 ** 6, 60 * NS)]
    last, when = float(T0) / 1e9, T0 // 1_000_000 + 120_000
    shown = {}
    for name in ("one wave", "two blocks", "two steps"):
        rig = Rig(rl, 0, 2048, configs=configs, tb=1 << 12, win=1 << 12)
        rig.eng.restore(snap.build(tb=[(10, 0.9763120008305, last, when)], profile=0, now_ms=0), 0)
        m = 2 if name == "one wave" else 600
        key = np.arange(m, dtype=np.uint64) + np.uint64(5000)       # the others: keys nobody has
        n = np.ones(m, np.int64)
        key[0], n[0] = 10, 4
        key[-1], n[-1] = 10, 45                                    # position 599: the third block
        ts, cfg = np.full(m, T0, np.int64), np.zeros(m, np.uint32)
        if name == "two steps":
            for j in (0, m - 1):
                got, _ = refund_step(rig, (key[[j]], ts[[j]], n[[j]], cfg[[j]]))
                assert got[0].tolist() == [DONE]
        else:
            got, _ = refund_step(rig, (key, ts, n, cfg), want_identity=True)
            assert got[0][[0, -1]].tolist() == [DONE, DONE] and (got[0][1:-1] == NOKEY).all()
        assert rig.eng.sync() == rl.RL_OK
        shown[name] = "%.14g" % engine_state(rig.eng, 0)["tb:10"][0]
        rig.close()
    assert shown == {"one wave": "49.97631200083", "two blocks": "49.97631200083", "two steps": "49.976312000831"}


# --- 4. the grid stride -----------------------------------------------------------------

def test_refund_routed_grid_stride(rl):
    """grid cap + 4096 + 37 requests, more than REFUND_GRID x REFUND_BLOCK
    threads: every thread strides to a second request, one target across the
    stride's seam and the ragged tail; against the array form"""
    cap = rl.REFUND_GRID_CAP
    m = cap + 4096 + 37
    assert m == 1024 * 256 + 4096 + 37
    keys = np.array([1, 2, 3], np.uint64)
    have = 10 ** 7
    a, sim, configs = _counter_rig(rl, m, keys, have, max_batch=1 << 19)
    b, _, _ = _counter_rig(rl, 2048, keys, have, max_batch=1 << 19)
    assert a.eng.refund_max() == 1 << 19 and a.cap >= m
    which = np.random.default_rng(1).integers(0, 3, m)
    which[:20_000] = 0
    which[cap - 130:cap + 130] = 1
    which[-37:] = 2
    key = keys[which]
    key[5::1000] = np.uint64(77)                                     # a key nobody has
    ts = T0 + 5 + np.arange(m, dtype=np.int64)
    n, cfg = np.ones(m, np.int64), np.zeros(m, np.uint32)
    n[7::1000] = 0
    got, sms = refund_step(a, (key, ts, n, cfg), want_identity=True)
    ref = b.eng.refund(key, ts, n, cfg, sms)
    assert np.array_equal(got[0], ref)
    assert np.array_equal(got[0], apply_refunds(sim, key, ts, n, cfg, sms)[0])
    assert set(ref.tolist()) == {NOKEY, DONE, INVALID}
    assert a.eng.sync() == rl.RL_OK and b.eng.sync() == rl.RL_OK
    pa = _check_counters(a, sim, configs, keys, "grid stride")
    pb = peek_all(b.eng, keys, np.full(3, T0 + 9), np.zeros(3, np.uint32), (T0 + 10_000) // 1_000_000)
    assert_same_peek(pa, pb, "grid stride")
    cnt = np.bincount(which[ref == DONE], minlength=3)
    assert cnt.min() > 50_000
    assert (10 ** 9 - pa.remaining).tolist() == (have - cnt).tolist()
    a.close()
    b.close()


# --- 5. the bound ---------------------------------------------------------------------

@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_refund_routed_bound(rl, in_order):
    """an engine with refund_max() == 512 and a step of 1500 refunds under m_max
    = 2048: the first 512 in merge order are applied as one call, the other 988
    come back {RL_DROPPED, 0, 0, 0}, nothing is written past 1500, and
    rl_engine_sync reports RL_EOVERFLOW once.  With m_max = 300 below
    refund_max only 300 run and nothing is written past m_max."""
    keys = np.arange(1, 401, dtype=np.uint64)
    have = 10 ** 6
    rig, sim, configs = _counter_rig(rl, 2048, keys, have, max_batch=512)
    assert rig.eng.refund_max() == 512 and rig.cap == 2048
    rng = np.random.default_rng(3)
    m = 1500
    key = keys[rng.integers(0, 400, m)]
    key[rng.random(m) < 0.05] += np.uint64(9000)                     # keys nobody has
    n = rng.integers(1, 50, m).astype(np.int64)
    n[rng.random(m) < 0.03] = 0
    cfg = np.zeros(m, np.uint32)
    ts = T0 + 5 + np.arange(m, dtype=np.int64)
    if not in_order:
        ts[0] = T0 + 5000                    # every request arrives then: the merge order is the received order
    for m_max, ran in ((2048, 512), (300, 300)):
        rig.res.fill_(SENTINEL)
        got, sms = refund_step(rig, (key, ts, n, cfg), want_identity=in_order, m_max=m_max)
        want = apply_refunds(sim, key[:ran], ts[:ran], n[:ran], cfg[:ran], sms[:ran])[0]
        assert np.array_equal(got[0][:ran], want)
        assert set(want.tolist()) == {NOKEY, DONE, INVALID}
        res = rig.res.cpu().numpy()
        assert not res[:ran, 1:].any()
        end = min(m, m_max)
        assert (res[ran:end] == [DROPPED, 0, 0, 0]).all() and (end - ran) == (988 if m_max == 2048 else 0)
        assert (res[end:] == SENTINEL).all()
        assert rig.eng.sync() == rl.RL_EOVERFLOW
        assert rig.eng.sync() == rl.RL_OK
        _check_counters(rig, sim, configs, keys, f"m_max {m_max}")
    rig.close()


# --- 6. nothing stored for NOKEY ----------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_refund_routed_nokey_stores_nothing(rl, profile):
    """a step of refunds for keys never seen and for targets expired at the
    step's store clock: every status is RL_REFUND_NOKEY, and rl_table_info, the
    live key sets, rl_engine_stats and the stored values are what they were --
    no insert, no lazy delete"""
    rig = Rig(rl, profile, 4096)
    pop = populate(rig, None, 151 + profile, m=3000, nkeys=100)
    now_ms = int(pop[1].max()) // 1_000_000
    before = (_fingerprint(rl, rig.eng, now_ms), engine_state(rig.eng, 0, profile))
    pkey, pts, _, pcfg = pop
    fresh = pkey[:500] + np.uint64(100_000)
    key = np.concatenate([pkey, fresh])
    ts = np.concatenate([pts, pts[:500]])
    cfg = np.concatenate([pcfg, pcfg[:500]])
    ts[0] = int(pts.max()) + 3600 * NS       # every request arrives an hour later: every TTL here has run out
    got, sms = refund_step(rig, (key, ts, np.full(key.size, 3, np.int64), cfg), want_identity=False)
    assert (sms >= now_ms + 3_599_000).all()
    assert (got[0] == NOKEY).all()
    assert rig.eng.sync() == rl.RL_OK
    assert (_fingerprint(rl, rig.eng, now_ms), engine_state(rig.eng, 0, profile)) == before
    rig.close()


# --- 7. order in flight ------------------------------------------------------------------

def test_refund_routed_order_in_flight(rl):
    """RL_OPT_PIPELINE: the steps D F P D F R F P D issued back to back on one
    stream with no host synchronisation between them -- every refund step sees
    the decides before it, every peek and decide after it the refunds"""
    import torch

    import routed_refund_cases as rf
    m = 2000
    mine = rf.rank_batches(0, CONFIGS, m=m)
    router = rl.Router(0, 1, m, m)
    cap = router.capacity
    eng = rl.Engine(profile=0, tb_capacity=1 << 14, win_capacity=1 << 14, max_batch=cap, flags=rl.OPT_PIPELINE)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    calls = {rf.D: eng.decide_routed, rf.P: eng.peek_routed, rf.R: eng.reset_routed, rf.F: eng.refund_routed}
    ins = [[_dev(torch, x) for x in bt] for bt in mine]
    outs = [[torch.empty(m, dtype=torch.uint8, device="cuda")] +
            [torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)] for _ in mine]
    bufs = [dict(send=torch.zeros((cap, 4), dtype=torch.int64, device="cuda"),
                 info=torch.zeros((1, 4), dtype=torch.int64, device="cuda"),
                 slot=torch.zeros(m, dtype=torch.int32, device="cuda"),
                 order=torch.zeros(cap, dtype=torch.int32, device="cuda"),
                 sms=torch.zeros(cap, dtype=torch.int64, device="cuda"),
                 cnt=torch.zeros(1, dtype=torch.int32, device="cuda"),
                 res=torch.zeros((cap, 4), dtype=torch.int64, device="cuda")) for _ in mine]
    torch.cuda.synchronize()
    for op, i, o, u in zip(rf.KINDS, ins, outs, bufs):
        router.pack(m, *[p(t) for t in i], p(u["send"]), p(u["info"]), p(u["slot"]), s)
        router.merge(p(u["send"]), p(u["info"]), p(u["order"]), p(u["sms"]), p(u["cnt"]), s)
        calls[op](cap, p(u["cnt"]), p(u["send"]), p(u["order"]), p(u["sms"]), p(u["res"]), s, s)
        router.unpack(m, p(u["slot"]), p(u["res"]), *[p(x) for x in o], s)
    torch.cuda.synchronize()
    assert eng.sync() == rl.RL_OK, eng.last_error()
    assert router.sync(None) == rl.RL_OK
    st = eng.stats()
    assert int(st.batches) == rf.KINDS.count(rf.D)
    cover = rf.new_cover()
    exp = rf.routed_expectations([mine], rf.KINDS, 0, CONFIGS, cap=cap, cover=cover)
    assert not rf.mismatches(outs, exp)
    assert cover["status"] == {NOKEY, DONE, INVALID} and cover["del"] and cover["decrby"] and cover["clamped"]
    eng.close()
    router.close()


# --- 8. the whole path ------------------------------------------------------------------

def _routed_refund_rank(rank, world, backend="nccl", exchange=None, m=3000):
    """one rank (routed_refund_cases.run_ranks) of the native routed path on
    cuda:0 running steps of the kinds D F P D F R F P D back to back: Router
    kernels, the HIP engine's four routed calls in their event form, the
    all-to-alls over `backend` -> (ok, info)"""
    import torch
    import torch.distributed as dist

    import rl_amd
    import routed_refund_cases as rf
    import shard
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    info = {}
    in_place = not exchange and world == 1
    all_batches = [rf.rank_batches(r, CONFIGS, m=m, reset_n_none=in_place, in_order=in_place)
                   for r in range(world)]
    mine = all_batches[rank]
    router = rl_amd.Router(0, world, m, m)
    eng = rl_amd.Engine(profile=0, tb_capacity=1 << 16, win_capacity=1 << 16, max_batch=world * router.capacity)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    pg_res = dist.new_group(backend=backend)
    pipe = shard.RoutedPipeline(router, eng.decide_routed, world, m, "cuda:0", pg_req=None, pg_res=pg_res,
                                exchange=exchange, staged=backend == "gloo", decide_ev=eng.decide_routed_ev,
                                peek=eng.peek_routed, peek_ev=eng.peek_routed_ev, reset=eng.reset_routed,
                                reset_ev=eng.reset_routed_ev, refund=eng.refund_routed,
                                refund_ev=eng.refund_routed_ev)
    ins = [tuple(None if x is None else _dev(torch, x) for x in bt) for bt in mine]
    outs = [(torch.empty(m, dtype=torch.uint8, device="cuda"),) +
            tuple(torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)) for _ in mine]
    torch.cuda.synchronize()
    pipe.run(ins, outs, kinds=rf.KINDS)
    torch.cuda.synchronize()
    info["engine_status"] = eng.sync()
    info["router_status"] = router.sync(None)
    info["collectives"] = pipe.collectives
    info["exchange"] = pipe.exchange
    info["batches"] = int(eng.stats().batches)
    info["spill_used"] = int(eng.table_info(0).spill_used)
    cover = rf.new_cover()
    exp = rf.routed_expectations(all_batches, rf.KINDS, rank, CONFIGS, cap=router.capacity, cover=cover)
    info["bad"] = rf.mismatches(outs, exp)
    info["cover"] = {k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in cover.items()}
    ok = not info["bad"]
    del pipe
    eng.close()
    router.close()
    return ok, info


def _spawn(world, backend, **kw):
    """fresh processes; every rank's work under one time limit, and none is
    waited for once another has failed"""
    import routed_refund_cases as rf
    return rf.run_ranks(__name__, "_routed_refund_rank", world, limit=240, backend=backend, **kw)


def _check(res, world, exchange):
    import routed_refund_cases as rf
    nb = len(rf.KINDS)
    for r in range(world):
        ok, info = res[r]
        assert ok, (r, info)
        assert info["exchange"] == exchange
        assert info["collectives"] == (3 * nb if exchange else 0), info   # 3 collectives per step of any kind
        assert info["engine_status"] == 0 and info["router_status"] == 0, info
        assert info["batches"] == rf.KINDS.count(rf.D), info          # only decide steps are counted
        assert info["spill_used"] > 0, info
        c = info["cover"]
        assert c["status"] == [NOKEY, DONE, INVALID] and c["del"] and c["decrby"] and c["clamped"], info
        assert (c["multi_rank"] > 0) == (world > 1), info


def test_routed_refund_one_rank_rccl():
    """world 1 with the exchange forced on: every step's three collectives over
    RCCL, the refund kernels between in-flight decides"""
    _check(_spawn(1, "nccl", exchange=True), 1, True)


def test_routed_refund_one_rank_in_place():
    """world 1 without the exchange: buckets and results read in place (the
    RL_ORDER_IDENTITY form in the peek and refund steps)"""
    _check(_spawn(1, "nccl"), 1, False)


def test_routed_refund_two_ranks_one_gpu():
    """two ranks (two engines, two routers) on the one GPU, all-to-alls through
    host memory (gloo): both ranks' refunds of one target summed on its owner"""
    _check(_spawn(2, "gloo"), 2, True)


# --- 9. arguments and symbols -----------------------------------------------------------

def test_refund_routed_arguments(rl):
    """argument checks as the peek and reset steps: a null count or a null
    array with m_max > 0 is RL_EINVAL, m_max above 32 bits is refused, m_max = 0
    is a no-op that records the event; no sticky status comes of any of it"""
    import torch
    rig = Rig(rl, 0, 2048, max_batch=1 << 20)
    assert rig.eng.refund_max() == 1 << 20
    scratch = 2 * (1 << 20) * 44             # the refund scratch the first refund of this engine allocates
    p = lambda t: t.data_ptr()
    fn = rl.lib.rl_refund_routed_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    assert fn(None, 0, None, None, None, None, None, None, None, None) == rl.RL_EINVAL   # no engine
    good = [rig.eng.h, 16, p(rig.cnt), p(rig.send), p(rig.order), p(rig.sms), p(rig.res), None, None, None]
    for k in (0, 2, 3, 4, 5, 6):
        bad = list(good)
        bad[k] = None
        assert fn(*bad) == rl.RL_EINVAL
    assert fn(*(good[:1] + [1 << 32] + good[2:])) == rl.RL_EINVAL
    ev = torch.cuda.Event()
    ev.record()
    torch.cuda.synchronize()
    # m_max = 0 allocates nothing: the 88 MiB of refund scratch are the first
    # real refund's to make
    free0 = torch.cuda.mem_get_info()[0]
    assert fn(rig.eng.h, 0, p(rig.cnt), None, None, None, None, rig.s, None, ev.cuda_event) == rl.RL_OK
    ev.synchronize()
    assert fn(rig.eng.h, 0, p(rig.cnt), None, None, None, None, None, None, None) == rl.RL_OK
    assert free0 - torch.cuda.mem_get_info()[0] < scratch // 4
    rig.res.fill_(SENTINEL)
    assert fn(*good) == rl.RL_OK                                     # a zero count: nothing to do
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] > scratch // 2       # and that call made the scratch
    assert (rig.res.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError):
        rig.eng.refund_routed_ev(*good[1:7], rig.s, None)
    for name in ("refund_routed", "refund_routed_ev"):
        assert callable(getattr(rl.Engine, name))
    assert rig.eng.sync() == rl.RL_OK
    rig.close()
