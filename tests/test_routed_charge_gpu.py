"""The charge step of the routed path on the GPU: k_charge_ask_routed and
k_charge_finish_routed (csrc/rl_charge.h) around the unchanged routed decide,
behind rl_charge_routed_device (include/rl_route.h), and shard.RoutedPipeline's
charge kind end to end.  The routed call is pinned to the array form
(Engine.charge, itself pinned to the oracle in tests/test_charge_gpu.py) and to
charge_cases.apply_charge on the Python oracle, through every result field,
through Peek (n = 0) of everything the engines hold, the stored values
themselves and a decide step that follows; the whole path to ONE shared store
(tests/routed_charge_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from charge_cases import apply_charge
from peek_cases import assert_peek, peek_expected
from refund_cases import new_sim
from reset_cases import engine_keys
from test_charge_gpu import SHAPE_CONFIGS, shape_call
from test_refund_gpu import engine_state, oracle_state
from test_routed_ops_gpu import SENTINEL, Rig, _dev
from test_routed_refund_gpu import assert_same_peek, merge_order, peek_all, populate, shape_order
from tracegen import CONFIG_SETS, NS, T0, skewed_trace

pytestmark = pytest.mark.gpu
CONFIGS = CONFIG_SETS["mixed"]
KEY_RESERVED = (1 << 64) - 1
ALLOWED, DENIED, INVALID, DROPPED = 1, 0, 3, 4
AMOUNTS = np.array([1, 1, 1, 2, 3, 7, 50, 1 << 40], np.int64)


def charge_batch(rng, c, pop, t0, in_order):
    """c charges on the populate step's keys after that step (a few windows
    behind it), amounts from 1 to 2^40; keys never seen; a few n <= 0, unknown
    cfgs and the reserved key; duplicates by construction (c picks of 150 keys)"""
    pkey = pop[0]
    key = pkey[rng.integers(0, pkey.size, c)].copy()
    ts = (t0 + np.cumsum(rng.choice([0, 1000, 250_000, 5_000_000], c))).astype(np.int64)
    ts[rng.random(c) < 0.1] -= 7_000_000_000
    key[rng.random(c) < 0.1] += np.uint64(100_000)
    n = rng.choice(AMOUNTS, c, p=[0.25, 0.15, 0.1, 0.15, 0.1, 0.12, 0.11, 0.02])
    n[rng.random(c) < 0.03] = rng.choice([0, -1, -5])
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    cfg[rng.random(c) < 0.03] = 99
    key[rng.random(c) < 0.03] = np.uint64(KEY_RESERVED)
    return shape_order(key, ts, n, cfg, in_order)


def charge_step(rig, batch, want_identity=None, m_max=None):
    """pack -> merge -> charge_routed -> unpack of one batch: (decision,
    remaining, charged, reset_at in the caller's order, every request's store
    clock); the received records are what they were"""
    key, ts, n, cfg = batch
    sms = rig.route(key, ts, n, cfg)
    rig.torch.cuda.synchronize()
    recv = rig.send.clone()
    rig.eng.charge_routed(*rig.args(m_max))
    got = rig.results()
    assert rig.torch.equal(rig.send, recv), "the call rewrote recv"
    if want_identity is not None and key.size > 1:
        assert rig.identity_form() == want_identity
    return got, sms


def rows_of(rows):
    """apply_charge's rows as the routed fields (decision, remaining, charged, reset_at)"""
    return [np.array([r[j] for r in rows], np.int64) for j in (0, 2, 1, 3)]


def assert_fields(got, want, what):
    for name, g, w in zip(("decision", "remaining", "charged", "reset_at"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} at {bad[:8]}: got {g[bad[:8]]} want {w[bad[:8]]}"


def array_fields(res):
    return [res.decision, res.remaining, res.charged, res.reset_at_ns]


# --- 1. the routed call against the array form and the oracle ---------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_charge_routed_equals_charge(rl, profile, in_order):
    """two engines populated alike; one runs pack -> merge -> charge_routed, the
    other Engine.charge of the same requests in merge order at the same store
    clocks: every field equal at counts around the wave, the block and above
    2048, and equal to apply_charge on the Python oracle.  Then the state: Peek
    (n = 0) of every populated key, the live keys, the stored values against
    the oracle's db, and a routed decide step that follows"""
    rng = np.random.default_rng(290 + profile)
    a, b = Rig(rl, profile, 8192), Rig(rl, profile, 8192)
    sim = new_sim(profile, CONFIGS)
    pop = populate(a, sim, 241 + profile)
    populate(b, None, 241 + profile)
    t0 = int(pop[1].max()) + 1000
    now_ms = t0 // 1_000_000
    seen = set()
    for c in (0, 1, 63, 64, 65, 2049):
        key, ts, n, cfg = batch = charge_batch(rng, c, pop, t0, in_order)
        st0 = a.eng.stats()
        got, sms = charge_step(a, batch, in_order)
        st1 = a.eng.stats()
        # rl_stats moves as a routed decide of bound B = min(m_max, charge_max)
        assert (st1.batches - st0.batches, st1.decisions - st0.decisions) == (1, a.cap)
        if c == 0:
            continue
        o = merge_order(ts)
        ref = b.eng.charge(key[o], ts[o], n[o], cfg[o], sms[o], want_tokens=False)
        assert_fields([g[o] for g in got], array_fields(ref), f"count {c}: routed and array form")
        rows, info = apply_charge(sim, key[o], ts[o], n[o], cfg[o], sms[o])
        assert_fields([g[o] for g in got], rows_of(rows), f"count {c}: the oracle")
        seen |= set(info["cls"].tolist())
        t0 = int(ts.max()) + 1000
        now_ms = max(now_ms, int(sms.max()))
    assert seen >= {"invalid", "full", "short", "empty", "dup_denied", "over"}, seen
    assert a.eng.sync() == rl.RL_OK and b.eng.sync() == rl.RL_OK
    # the state, not only the rows, is the array form's
    pkey, pts, _, pcfg = pop
    at = np.full(pkey.size, t0)
    pa, pb = peek_all(a.eng, pkey, at, pcfg, now_ms), peek_all(b.eng, pkey, at, pcfg, now_ms)
    assert_same_peek(pa, pb, "peek after the charges")
    zeros = np.zeros(pkey.size, np.int64)
    assert_peek(pa, peek_expected(sim, pkey, at, zeros, pcfg, np.full(pkey.size, now_ms)), CONFIGS, pcfg, "oracle")
    assert engine_keys(rl, a.eng, now_ms) == engine_keys(rl, b.eng, now_ms)
    sa, so = engine_state(a.eng, now_ms, profile), oracle_state(sim, now_ms)
    assert sa.keys() == so.keys(), sorted(sa.keys() ^ so.keys())[:6]
    for k, w in so.items():
        g = sa[k]
        if k.startswith("tb:"):
            assert np.array([g[:2]]).view(np.uint64).tolist() == np.array([w[:2]]).view(np.uint64).tolist() \
                and g[2] == w[2], (k, g, w)
        else:
            assert g == w, (k, g, w)
    # a decide step that follows
    key, ts, n, cfg, _ = skewed_trace(261 + profile, 3000, 150, CONFIGS)
    ts = ts + (t0 - int(ts.min()))
    sms = a.route(key, ts, n, cfg)
    a.eng.decide_routed(*a.args())
    got = a.results()
    want = np.zeros((key.size, 4), np.int64)
    for i in merge_order(ts).tolist():
        want[i] = sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]), int(sms[i]))[:4]
    for f, name in enumerate(("decision", "remaining", "retry_after", "reset_at")):
        bad = np.nonzero(got[f].astype(np.int64) != want[:, f])[0]
        assert bad.size == 0, f"the decide that follows: {name} at {bad[:8]}"
    assert a.eng.sync() == rl.RL_OK
    a.close()
    b.close()


# --- 2. the empty bucket's row ------------------------------------------------------------

@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_charge_routed_empty_bucket_row(rl, in_order):
    """a bucket of 5 emptied by a decide: a charge of it is RL_DENIED with
    charged 0 and remaining 0, and its reset_at is the ask's (the time the
    bucket is full again), not zero: no decide ran for it"""
    configs = [(1, 5, 3600 * NS), (3, 5, 3600 * NS)]
    rig = Rig(rl, 0, 2048, configs=configs, tb=1 << 8, win=1 << 8)
    sim = new_sim(0, configs)
    key = np.array([2, 4, 6, 3], np.uint64)                      # three buckets and a window
    cfg = np.array([0, 0, 0, 1], np.uint32)
    ts = np.full(4, T0, np.int64)
    rig.eng.decide(key, ts, np.full(4, 5, np.int64), cfg)
    for i in range(4):
        sim.decide(int(key[i]), T0, 5, int(cfg[i]), T0 // 1_000_000)
    ts2 = T0 + 1000 + np.arange(4, dtype=np.int64)
    if not in_order:
        ts2[0] = T0 + 9000
    n = np.array([3, 1, 1 << 40, 2], np.int64)
    got, sms = charge_step(rig, (key, ts2, n, cfg), want_identity=in_order)
    o = merge_order(ts2)
    rows, info = apply_charge(sim, key[o], ts2[o], n[o], cfg[o], sms[o])
    assert_fields([g[o] for g in got], rows_of(rows), "empty buckets")
    assert sorted(info["cls"].tolist()) == ["empty", "empty", "empty", "over"]
    assert got[0][:3].tolist() == [DENIED] * 3 and not got[1][:3].any() and not got[2][:3].any()
    assert (got[3][:3] > T0).all()                               # the ask's reset_at
    assert [int(g[3]) for g in got[:3]] == [DENIED, 0, 2]        # the window: 7 of 5, recorded
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 3. the grid stride -----------------------------------------------------------------

def test_charge_routed_grid_stride(rl):
    """grid cap + 4096 + 37 requests, more than CHARGE_GRID x CHARGE_BLOCK
    threads: every thread of both routed kernels strides to a second request,
    and the ragged tail; against the array form on a twin engine (pinned to the
    oracle at this size in tests/test_charge_gpu.py)"""
    cap = rl.CHARGE_GRID_CAP
    m = cap + 4096 + 37
    assert m == 1024 * 256 + 4096 + 37
    a = Rig(rl, 0, m, max_batch=1 << 19, configs=SHAPE_CONFIGS, tb=1 << 18, win=1 << 18)
    b = rl.Engine(profile=0, tb_capacity=1 << 18, win_capacity=1 << 18, max_batch=1 << 19)
    for alg, L, W in SHAPE_CONFIGS:
        b.register(alg, L, W)
    assert a.eng.charge_max() == 1 << 19 and a.cap >= m
    key, ts, n, cfg = shape_call(m, T0, 9)
    got, sms = charge_step(a, (key, ts, n, cfg), want_identity=True)
    ref = b.charge(key, ts, n, cfg, sms, want_tokens=False)
    assert_fields(got, array_fields(ref), "grid stride")
    for lo, hi in ((0, cap), (cap, m)):
        d, ch = got[0][lo:hi], got[2][lo:hi]
        assert {ALLOWED, DENIED, INVALID} <= set(d.tolist())
        assert ((d == DENIED) & (ch > 0)).any() and ((d == DENIED) & (ch == 0)).any()
    assert a.eng.sync() == rl.RL_OK and b.sync() == rl.RL_OK
    pk = np.unique(key[key != np.uint64(KEY_RESERVED)])[:4096]
    pc = (pk % np.uint64(4)).astype(np.uint32)
    now_ms = int(sms.max())
    at = np.full(pk.size, int(ts.max()))
    assert_same_peek(peek_all(a.eng, pk, at, pc, now_ms), peek_all(b, pk, at, pc, now_ms), "grid stride")
    a.close()
    b.close()


# --- 4. the bound ---------------------------------------------------------------------

@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_charge_routed_bound(rl, in_order):
    """an engine with charge_max() == 512 and a step of 700 charges under m_max
    = 2048: the first 512 in merge order run as one call and equal one array
    call of those 512, rows 512..699 come back {RL_DROPPED, 0, 0, 0}, nothing
    is written past 700, and rl_engine_sync reports RL_EOVERFLOW once"""
    rig = Rig(rl, 0, 2048, max_batch=512, configs=SHAPE_CONFIGS, tb=1 << 12, win=1 << 12)
    b = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=512)
    for alg, L, W in SHAPE_CONFIGS:
        b.register(alg, L, W)
    sim = new_sim(0, SHAPE_CONFIGS)
    assert rig.eng.charge_max() == 512 and b.charge_max() == 512 and rig.cap == 2048
    m, ran = 700, 512
    key, ts, n, cfg = shape_call(m, T0, 31)
    if not in_order:
        ts[0] = T0 + 5_000_000               # every request arrives then: the merge order is the received order
    rig.res.fill_(SENTINEL)
    st0 = rig.eng.stats()
    got, sms = charge_step(rig, (key, ts, n, cfg), want_identity=in_order)
    st1 = rig.eng.stats()
    assert (st1.batches - st0.batches, st1.decisions - st0.decisions) == (1, ran)
    ref = b.charge(key[:ran], ts[:ran], n[:ran], cfg[:ran], sms[:ran], want_tokens=False)
    assert_fields([g[:ran] for g in got], array_fields(ref), "the first 512")
    rows, info = apply_charge(sim, key[:ran], ts[:ran], n[:ran], cfg[:ran], sms[:ran])
    assert_fields([g[:ran] for g in got], rows_of(rows), "the first 512, oracle")
    assert {"full", "short", "dup_denied", "over", "invalid"} <= set(info["cls"].tolist())
    res = rig.res.cpu().numpy()
    assert (res[ran:m] == [DROPPED, 0, 0, 0]).all()
    assert (res[m:] == SENTINEL).all()
    assert (got[0][ran:] == DROPPED).all() and not got[2][ran:].any()
    assert rig.eng.sync() == rl.RL_EOVERFLOW
    assert rig.eng.sync() == rl.RL_OK
    assert b.sync() == rl.RL_OK
    # the dropped requests were not executed: the state is that of the 512
    pk = np.unique(key[key != np.uint64(KEY_RESERVED)])
    pc = (pk % np.uint64(4)).astype(np.uint32)
    now_ms, at = int(sms.max()), np.full(pk.size, int(ts.max()))
    assert_same_peek(peek_all(rig.eng, pk, at, pc, now_ms), peek_all(b, pk, at, pc, now_ms), "the bound")
    rig.close()
    b.close()


# --- 5. order in flight ------------------------------------------------------------------

def test_charge_routed_order_in_flight(rl):
    """RL_OPT_PIPELINE: the steps D C P D C R C F D issued back to back on one
    stream with no host synchronisation between them -- every charge step sees
    the steps before it, every later step the charges"""
    import torch

    import routed_charge_cases as cc
    m = 2000
    mine = cc.rank_batches(0, CONFIGS, m=m)
    router = rl.Router(0, 1, m, m)
    cap = router.capacity
    eng = rl.Engine(profile=0, tb_capacity=1 << 14, win_capacity=1 << 14, max_batch=cap, flags=rl.OPT_PIPELINE)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    calls = {cc.D: eng.decide_routed, cc.P: eng.peek_routed, cc.R: eng.reset_routed, cc.F: eng.refund_routed,
             cc.C: eng.charge_routed}
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
    for op, i, o, u in zip(cc.KINDS, ins, outs, bufs):
        router.pack(m, *[p(t) for t in i], p(u["send"]), p(u["info"]), p(u["slot"]), s)
        router.merge(p(u["send"]), p(u["info"]), p(u["order"]), p(u["sms"]), p(u["cnt"]), s)
        calls[op](cap, p(u["cnt"]), p(u["send"]), p(u["order"]), p(u["sms"]), p(u["res"]), s, s)
        router.unpack(m, p(u["slot"]), p(u["res"]), *[p(x) for x in o], s)
    torch.cuda.synchronize()
    assert eng.sync() == rl.RL_OK, eng.last_error()
    assert router.sync(None) == rl.RL_OK
    st = eng.stats()
    assert int(st.batches) == cc.KINDS.count(cc.D) + cc.KINDS.count(cc.C)   # a charge step counts as its decide
    cover = cc.new_cover()
    exp = cc.routed_expectations([mine], cc.KINDS, 0, CONFIGS, cap=cap, cover=cover)
    assert not cc.mismatches(outs, exp)
    assert cover["cls"] >= set(cc.CLASSES) and cover["window_over"]
    eng.close()
    router.close()


# --- 6. the whole path ------------------------------------------------------------------

def _routed_charge_rank(rank, world, backend="nccl", exchange=None, m=3000):
    """one rank (routed_refund_cases.run_ranks) of the native routed path on
    cuda:0 running steps of the kinds D C P D C R C F D back to back: Router
    kernels, the HIP engine's five routed calls in their event form, the
    all-to-alls over `backend` -> (ok, info)"""
    import torch
    import torch.distributed as dist

    import rl_amd
    import routed_charge_cases as cc
    import shard
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    info = {}
    in_place = not exchange and world == 1
    all_batches = [cc.rank_batches(r, CONFIGS, m=m, reset_n_none=in_place, in_order=in_place)
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
                                refund_ev=eng.refund_routed_ev, charge=eng.charge_routed,
                                charge_ev=eng.charge_routed_ev)
    ins = [tuple(None if x is None else _dev(torch, x) for x in bt) for bt in mine]
    outs = [(torch.empty(m, dtype=torch.uint8, device="cuda"),) +
            tuple(torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)) for _ in mine]
    torch.cuda.synchronize()
    pipe.run(ins, outs, kinds=cc.KINDS)
    torch.cuda.synchronize()
    info["engine_status"] = eng.sync()
    info["router_status"] = router.sync(None)
    info["collectives"] = pipe.collectives
    info["exchange"] = pipe.exchange
    info["batches"] = int(eng.stats().batches)
    cover = cc.new_cover()
    exp = cc.routed_expectations(all_batches, cc.KINDS, rank, CONFIGS, cap=router.capacity, cover=cover)
    info["bad"] = cc.mismatches(outs, exp)
    info["cover"] = {k: (sorted(v) if isinstance(v, set) else int(v)) for k, v in cover.items()}
    ok = not info["bad"]
    del pipe
    eng.close()
    router.close()
    return ok, info


def _spawn(world, backend, **kw):
    """fresh processes; every rank's work under one time limit, and none is
    waited for once another has failed"""
    import routed_charge_cases as cc
    return cc.run_ranks(__name__, "_routed_charge_rank", world, limit=240, backend=backend, **kw)


def _check(res, world, exchange):
    import routed_charge_cases as cc
    nb = len(cc.KINDS)
    for r in range(world):
        ok, info = res[r]
        assert ok, (r, info)
        assert info["exchange"] == exchange
        assert info["collectives"] == (3 * nb if exchange else 0), info   # 3 collectives per step of any kind
        assert info["engine_status"] == 0 and info["router_status"] == 0, info
        assert info["batches"] == cc.KINDS.count(cc.D) + cc.KINDS.count(cc.C), info
        c = info["cover"]
        assert set(c["cls"]) >= set(cc.CLASSES) and c["window_over"] and not c["dropped"], info
        assert (c["cross_rank_dup"] > 0) == (world > 1), info


def test_routed_charge_one_rank_rccl():
    """world 1 with the exchange forced on: every step's three collectives over
    RCCL, the charge kernels between in-flight decides"""
    _check(_spawn(1, "nccl", exchange=True), 1, True)


def test_routed_charge_one_rank_in_place():
    """world 1 without the exchange: buckets and results read in place (the
    RL_ORDER_IDENTITY form in the peek, refund and charge steps)"""
    _check(_spawn(1, "nccl"), 1, False)


def test_routed_charge_two_ranks_one_gpu():
    """two ranks (two engines, two routers) on the one GPU, all-to-alls through
    host memory (gloo): both ranks' charges of one bucket as one call on its
    owner"""
    _check(_spawn(2, "gloo"), 2, True)


# --- 7. arguments -----------------------------------------------------------------------

def test_charge_routed_arguments(rl):
    """argument checks as the other routed steps: a null count or a null array
    with m_max > 0 is RL_EINVAL, m_max above 32 bits is refused, m_max = 0 is a
    no-op that records the event and allocates nothing; the first real call
    makes the scratch; no sticky status comes of any of it"""
    import torch
    rig = Rig(rl, 0, 2048, max_batch=1 << 20)
    assert rig.eng.charge_max() == 1 << 20
    scratch = (1 << 20) * 93                 # the routed Charge scratch of this engine
    p = lambda t: t.data_ptr()
    fn = rl.lib.rl_charge_routed_device
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
    free0 = torch.cuda.mem_get_info()[0]
    st0 = rig.eng.stats()
    assert fn(rig.eng.h, 0, p(rig.cnt), None, None, None, None, rig.s, None, ev.cuda_event) == rl.RL_OK
    ev.synchronize()
    assert fn(rig.eng.h, 0, p(rig.cnt), None, None, None, None, None, None, None) == rl.RL_OK
    assert free0 - torch.cuda.mem_get_info()[0] < scratch // 4
    assert bytes(rig.eng.stats()) == bytes(st0)
    rig.res.fill_(SENTINEL)
    assert fn(*good) == rl.RL_OK                                     # a zero count: nothing to do
    torch.cuda.synchronize()
    assert free0 - torch.cuda.mem_get_info()[0] > scratch // 2       # and that call made the scratch
    assert (rig.res.cpu().numpy() == SENTINEL).all()
    with pytest.raises(ValueError):
        rig.eng.charge_routed_ev(*good[1:7], rig.s, None)
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


def test_charge_step_needs_its_callable(rl):
    """a charge step on a device pipeline built without charge= raises
    ValueError before anything is enqueued"""
    import torch

    import shard
    router = rl.Router(0, 1, 64, 64)
    eng = rl.Engine(profile=0, tb_capacity=1 << 8, win_capacity=1 << 8, max_batch=router.capacity)
    pipe = shard.RoutedPipeline(router, eng.decide_routed, 1, 64, "cuda:0", decide_ev=eng.decide_routed_ev,
                                refund=eng.refund_routed)
    z = lambda dt: torch.zeros(4, dtype=dt, device="cuda")
    with pytest.raises(ValueError, match="charge"):
        pipe.step(0, z(torch.int64), z(torch.int64), z(torch.int64), z(torch.int32), z(torch.uint8), z(torch.int64),
                  z(torch.int64), z(torch.int64), op=shard.OP_CHARGE)
    assert not pipe._pend and len(pipe.order_log) == 0
    torch.cuda.synchronize()
    assert eng.sync() == rl.RL_OK
    del pipe
    eng.close()
    router.close()
