"""The peek and reset steps of the routed path on the GPU: k_peek_routed /
k_reset_routed (csrc/rl_peek.h, csrc/rl_reset.h) behind rl_peek_routed_device /
rl_reset_routed_device (include/rl_route.h), and shard.RoutedPipeline's step
kinds end to end.  The routed kernels are pinned to the existing array-form
kernels (Engine.peek, Engine.reset_batch: themselves pinned to the oracle in
tests/test_peek_gpu.py and tests/test_reset_batch_gpu.py) on every field, and
the whole path to ONE shared store (tests/routed_op_cases.py)."""
import ctypes as C
import os
import socket

import numpy as np
import pytest

import reset_cases
from tracegen import CONFIG_SETS, T0, skewed_trace

pytestmark = pytest.mark.gpu
CONFIGS = CONFIG_SETS["mixed"]
KEY_RESERVED = (1 << 64) - 1
SENTINEL = -7


def _dev(torch, x):
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    elif x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class Rig:
    """one rank of world 1 in one process: a Router, its CPU restatement run in
    lock step (the store clock of every request) and an Engine; buffers of one
    step, read in place (no exchange)"""

    def __init__(self, rl, profile, max_m, max_batch=None, configs=CONFIGS, tb=1 << 14, win=1 << 14):
        import torch

        import route_ops
        self.rl, self.torch = rl, torch
        self.r = rl.Router(0, 1, max_m, max_m)
        self.cap = cap = self.r.capacity
        self.ops = route_ops.NumpyRouteOps(1, max_m)
        assert self.ops.capacity == cap
        self.eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch or cap)
        for a, L, W in configs:
            self.eng.register(a, L, W)
        self.s = torch.cuda.current_stream().cuda_stream
        self.send = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
        self.info = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
        self.slot = torch.zeros(max_m, dtype=torch.int32, device="cuda")
        self.order = torch.zeros(cap, dtype=torch.int32, device="cuda")
        self.sms = torch.zeros(cap, dtype=torch.int64, device="cuda")
        self.cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.res = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")

    def route(self, key, ts, n, cfg):
        """pack + merge of one step on the device and in the restatement ->
        the store clock of every request, in the caller's order"""
        torch, p = self.torch, lambda t: t.data_ptr()
        m = key.size
        self.m = m
        self.ins = [_dev(torch, x) for x in (key, ts, n, cfg)]     # kept alive until the step has run
        self.r.pack(m, *[p(t) for t in self.ins], p(self.send), p(self.info), p(self.slot), self.s)
        self.r.merge(p(self.send), p(self.info), p(self.order), p(self.sms), p(self.cnt), self.s)
        h = [torch.from_numpy(np.ascontiguousarray(x.view(np.int64) if x.dtype == np.uint64 else
                                                   (x.view(np.int32) if x.dtype == np.uint32 else x)))
             for x in (key, ts, n, cfg)]
        send = torch.zeros((self.cap, 4), dtype=torch.int64)
        info = torch.zeros((1, 4), dtype=torch.int64)
        slot = torch.zeros(max(m, 1), dtype=torch.int32)
        order = torch.zeros(self.cap, dtype=torch.int32)
        sms = torch.zeros(self.cap, dtype=torch.int64)
        cnt = torch.zeros(1, dtype=torch.int32)
        self.ops.pack(m, *[p(t) for t in h], p(send), p(info), p(slot), None)
        self.ops.merge(p(send), p(info), p(order), p(sms), p(cnt), None)
        assert int(cnt[0]) == m and not self.ops.overflow
        at = np.empty(self.cap, np.int64)                            # receive index -> merge position
        at[order.numpy()[:m].astype(np.int64)] = np.arange(m)
        return sms.numpy()[at[slot.numpy()[:m].astype(np.int64)]].copy()

    def args(self, m_max=None):
        p = lambda t: t.data_ptr()
        return (self.cap if m_max is None else m_max, p(self.cnt), p(self.send), p(self.order), p(self.sms),
                p(self.res), self.s, self.s)

    def identity_form(self):
        self.torch.cuda.synchronize()
        return int(self.order.cpu()[0]) == -1                        # RL_ORDER_IDENTITY as int32

    def results(self):
        """unpack of the step's result records -> (dec, rem, retry, reset) in the caller's order"""
        torch, p = self.torch, lambda t: t.data_ptr()
        outs = [torch.empty(max(self.m, 1), dtype=torch.uint8, device="cuda")] + \
            [torch.empty(max(self.m, 1), dtype=torch.int64, device="cuda") for _ in range(3)]
        self.r.unpack(self.m, p(self.slot), p(self.res), *[p(x) for x in outs], self.s)
        torch.cuda.synchronize()
        return [x.cpu().numpy()[:self.m] for x in outs]

    def close(self):
        self.eng.close()
        self.r.close()


def populate(rig, seed, m=6000, nkeys=150):
    """a routed decide step on app servers with skewed clocks: token buckets,
    window entries and spilled windows -> the latest ts of the step"""
    key, ts, n, cfg, _ = skewed_trace(seed, m, nkeys, CONFIGS)
    rig.route(key, ts, n, cfg)
    rig.eng.decide_routed(*rig.args())
    rig.results()
    assert rig.eng.sync() == rig.rl.RL_OK
    info = rig.eng.table_info(0)
    assert info.tb_used > 0 and info.win_used > 0 and info.spill_used > 0
    return key, ts, n, cfg


def peek_batch(rng, c, pop, in_order):
    """c peeks aimed at the populate step's own requests (their keys at their
    own times: windows of every age, wherever they live), at the time after
    them, at keys never seen; n in {0, 1, 2, 5}; a few n = -1, unknown cfgs and
    the reserved key"""
    pkey, pts, _, _ = pop
    pick = rng.integers(0, pkey.size, c)
    key = pkey[pick].copy()
    ts = np.where(rng.random(c) < 0.5, pts[pick], int(pts.max()) + rng.integers(0, 3_000_000_000, c)).astype(np.int64)
    key[rng.random(c) < 0.1] += np.uint64(100_000)
    n = rng.choice([0, 1, 2, 5], c).astype(np.int64)
    n[rng.random(c) < 0.03] = -1
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    cfg[rng.random(c) < 0.03] = 99
    key[rng.random(c) < 0.03] = np.uint64(KEY_RESERVED)
    if in_order:
        ts = np.sort(ts)
    elif c > 1 and not np.any(ts[1:] < ts[:-1]):
        ts[0], ts[-1] = ts[-1] + 1, ts[0]
    return key, ts, n, cfg


def assert_fields(got, want, what):
    for name, g, w in zip(("decision", "remaining", "retry_after", "reset_at"), got, want):
        g, w = np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:8]}: got {g[bad[:8]]} want {w[bad[:8]]}"


def check_peek_step(rig, batch, what, want_identity):
    key, ts, n, cfg = batch
    sms = rig.route(key, ts, n, cfg)
    rig.eng.peek_routed(*rig.args())
    got = rig.results()
    if key.size > 1:
        assert rig.identity_form() == want_identity, what
    ref = rig.eng.peek(key, ts, n, cfg, sms, want_tokens=False)
    assert_fields(got, (ref.decision, ref.remaining, ref.retry_after_ns, ref.reset_at_ns), what)
    return got


# --- 1. the routed peek kernel against the array-form kernel -------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_peek_routed_equals_peek(rl, profile, in_order):
    """pack -> merge -> peek_routed equals Engine.peek of the same (key, ts, n,
    cfg, store clock) on all four fields, at counts around the wave, the block
    and one bucket tile; ts in order takes the RL_ORDER_IDENTITY form, ts
    shuffled an explicit order"""
    rng = np.random.default_rng(90 + profile)
    rig = Rig(rl, profile, 8192)
    pop = populate(rig, 41 + profile)
    seen = set()
    for c in (0, 1, 63, 64, 65, 255, 257, 2049):
        got = check_peek_step(rig, peek_batch(rng, c, pop, in_order), f"count {c}", in_order)
        seen |= set(got[0].tolist())
    assert seen >= {0, 1, 3}                       # denied, allowed and invalid rows were all compared
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


def test_peek_routed_grid_stride(rl):
    """more requests than PEEK_GRID x PEEK_BLOCK threads: every thread strides
    to a second request; the bound is far above the engine's max_batch, which
    does not limit a peek step"""
    m = rl.PEEK_GRID_CAP + 300
    assert m == 262144 + 300
    rng = np.random.default_rng(7)
    rig = Rig(rl, 0, m, max_batch=8192)
    assert rig.cap > 8192
    key, ts, n, cfg, _ = skewed_trace(43, 6000, 150, CONFIGS)
    rig.eng.decide(key, ts, n, cfg, np.maximum.accumulate(ts) // 1_000_000)
    for in_order in (True, False):
        check_peek_step(rig, peek_batch(rng, m, (key, ts, n, cfg), in_order), f"stride, in order {in_order}", in_order)
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 2. the routed reset kernel against the array-form kernel ------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["mixed", "skew"])
def test_reset_routed_equals_reset_batch(rl, profile, kind):
    """two engines with one history; one gets reset_batch, the other pack ->
    merge -> reset_routed of the same resets (one of them 64 times in a row,
    unknown cfgs, the reserved key): equal statuses, equal live key sets, and
    the decide batch that follows equal field by field"""
    configs, first, (rkey, rts, rcfg), second, now_ms = reset_cases.reset_case(kind, 17 + profile)
    rkey = np.concatenate([rkey[:100], np.full(64, rkey[0]), rkey[100:], [np.uint64(KEY_RESERVED)] * 3])
    rts = np.concatenate([rts[:100], np.full(64, rts[0]), rts[100:], rts[:3]]).astype(np.int64)
    rcfg = np.concatenate([rcfg[:100], np.full(64, rcfg[0]), rcfg[100:], rcfg[:3]]).astype(np.uint32)
    rcfg[5::97] = 1000
    rig = Rig(rl, profile, 4096, configs=configs, tb=1 << 12, win=1 << 12)
    a = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=4096)
    for alg, L, W in configs:
        a.register(alg, L, W)
    for eng in (a, rig.eng):
        eng.decide(*first)
    assert reset_cases.engine_keys(rl, a, now_ms) == reset_cases.engine_keys(rl, rig.eng, now_ms)
    st_a = a.reset_batch(rkey, rts, rcfg)
    st0 = rig.eng.stats()
    rig.route(rkey, rts, np.zeros(rkey.size, np.int64), rcfg)
    rig.eng.reset_routed(*rig.args())
    got = rig.results()
    st1 = rig.eng.stats()
    assert (st0.batches, st0.decisions) == (st1.batches, st1.decisions)
    assert rig.eng.sync() == rl.RL_OK
    assert np.array_equal(got[0], st_a)
    assert set(st_a.tolist()) == {reset_cases.RESET_DONE, reset_cases.INVALID}
    assert np.array_equal(st_a, reset_cases.expected_status(rkey, rcfg, len(configs)))
    assert not got[1].any() and not got[2].any() and not got[3].any()
    for at in (0, now_ms, now_ms + 1500, now_ms + 120_000):
        ka, kb = reset_cases.engine_keys(rl, a, at), reset_cases.engine_keys(rl, rig.eng, at)
        assert ka == kb, f"live keys differ at {at}"
    da, db = a.decide(*second), rig.eng.decide(*second)
    assert_fields((db.decision, db.remaining, db.retry_after_ns, db.reset_at_ns),
                  (da.decision, da.remaining, da.retry_after_ns, da.reset_at_ns), "the batch after the resets")
    assert np.array_equal(da.tokens.view(np.uint64), db.tokens.view(np.uint64))
    a.close()
    rig.close()


# --- 3. bounds ---------------------------------------------------------------------

@pytest.mark.parametrize("op", ["peek", "reset"])
@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_routed_op_count_above_m_max(rl, op, in_order):
    """*count = m_max + 5: the first m_max requests get their result record,
    the rows past them keep the sentinel, rl_engine_sync reports RL_EOVERFLOW
    once; *count = 0: nothing is written, the status stays RL_OK"""
    rng = np.random.default_rng(11)
    rig = Rig(rl, 0, 2048)
    pop = populate(rig, 47, m=2000, nkeys=80)
    call = rig.eng.peek_routed if op == "peek" else rig.eng.reset_routed
    m, m_max = 300, 295
    key, ts, n, cfg = peek_batch(rng, m, pop, in_order)
    sms = rig.route(key, ts, n, cfg)
    # world 1: the merge order is the received order in both forms, so the
    # first m_max requests are the caller's first m_max
    ref = rig.eng.peek(key, ts, n, cfg, sms, want_tokens=False)
    rig.res.fill_(SENTINEL)
    call(*rig.args(m_max))
    got = rig.results()
    assert rig.identity_form() == in_order
    if op == "peek":
        assert_fields([g[:m_max] for g in got], [x[:m_max] for x in (ref.decision, ref.remaining, ref.retry_after_ns,
                                                                      ref.reset_at_ns)], "rows below m_max")
    else:
        assert np.array_equal(got[0][:m_max], reset_cases.expected_status(key, cfg, len(CONFIGS))[:m_max])
    res = rig.res.cpu().numpy()
    assert (res[m_max:] == SENTINEL).all()
    assert (res[:m_max, 0] != SENTINEL).all()
    assert rig.eng.sync() == rl.RL_EOVERFLOW
    assert rig.eng.sync() == rl.RL_OK
    empty = np.zeros(0, np.int64)
    rig.route(empty.astype(np.uint64), empty, empty, empty.astype(np.uint32))
    rig.res.fill_(SENTINEL)
    call(*rig.args())
    rig.torch.cuda.synchronize()
    assert (rig.res.cpu().numpy() == SENTINEL).all()
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


def test_routed_op_arguments(rl):
    """argument checks as rl_decide_routed_device_io: a null count or a null
    array with m_max > 0 is RL_EINVAL; m_max = 0 is a no-op; m_max above 32
    bits is refused; no sticky status comes of any of it"""
    rig = Rig(rl, 0, 2048)
    p = lambda t: t.data_ptr()
    for fn in (rl.lib.rl_peek_routed_device, rl.lib.rl_reset_routed_device):
        good = [rig.eng.h, 16, p(rig.cnt), p(rig.send), p(rig.order), p(rig.sms), p(rig.res), None, None, None]
        for k in (0, 2, 3, 4, 5, 6):
            bad = list(good)
            bad[k] = None
            assert fn(*bad) == rl.RL_EINVAL
        assert fn(*(good[:1] + [1 << 32] + good[2:])) == rl.RL_EINVAL
        assert fn(rig.eng.h, 0, p(rig.cnt), None, None, None, None, None, None, None) == rl.RL_OK
        assert fn(*good) == rl.RL_OK                                 # a zero count: nothing to do
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 4. nothing changes --------------------------------------------------------------

def _fingerprint(rl, eng, now_ms):
    out = []
    for at in (0, now_ms):
        info = eng.table_info(at)
        out.append(tuple(getattr(info, k) for k, _ in info._fields_[2:]))
        out.append(reset_cases.engine_keys(rl, eng, at))
    st = eng.stats()
    out.append(bytes(st))
    return out


@pytest.mark.parametrize("profile", [0, 1])
def test_peek_step_changes_nothing(rl, profile):
    """across a peek step the live key sets, rl_table_info and rl_engine_stats
    are what they were; across a reset step batches / decisions do not move"""
    rng = np.random.default_rng(5 + profile)
    rig = Rig(rl, profile, 4096)
    pop = populate(rig, 51 + profile, m=4000, nkeys=100)
    now_ms = int(pop[1].max()) // 1_000_000
    before = _fingerprint(rl, rig.eng, now_ms)
    for in_order in (True, False):
        check_peek_step(rig, peek_batch(rng, 3000, pop, in_order), "peek step", in_order)
        assert rig.eng.sync() == rl.RL_OK
        assert _fingerprint(rl, rig.eng, now_ms) == before
    key, ts, n, cfg = peek_batch(rng, 500, pop, True)
    rig.route(key, ts, n, cfg)
    rig.eng.reset_routed(*rig.args())
    got = rig.results()
    assert np.array_equal(got[0], reset_cases.expected_status(key, cfg, len(CONFIGS)))
    st = rig.eng.stats()
    assert bytes(st) == before[-1]
    assert rig.eng.sync() == rl.RL_OK
    assert _fingerprint(rl, rig.eng, now_ms)[1] != before[1]     # and the reset did delete keys
    rig.close()


# --- 5. the whole path ------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _routed_ops_rank(rank, world, port, backend, q, exchange=None, m=3000):
    """one rank of the native routed path on cuda:0 running steps of the kinds
    D P D R P D P back to back (no host synchronisation between steps): Router
    kernels, the HIP engine's three routed calls in their event form, the
    all-to-alls over `backend`"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "distributed-rate-limiter_amd", "python"), os.path.join(root, "tests")]
    import torch
    import torch.distributed as dist

    import rl_amd
    import routed_op_cases as rc
    import shard
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    ok, info = False, {}
    try:
        # in place, the reset step leaves n out (the pipeline packs zeros of
        # its own) and the peek steps' ts are in order (RL_ORDER_IDENTITY)
        in_place = not exchange and world == 1
        all_batches = [rc.rank_batches(r, CONFIGS, m=m, reset_n_none=in_place, peeks_in_order=in_place)
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
                                    reset_ev=eng.reset_routed_ev)
        ins = [tuple(None if x is None else _dev(torch, x) for x in bt) for bt in mine]
        outs = [(torch.empty(m, dtype=torch.uint8, device="cuda"),) +
                tuple(torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)) for _ in mine]
        torch.cuda.synchronize()
        pipe.run(ins, outs, kinds=rc.KINDS)
        torch.cuda.synchronize()
        info["engine_status"] = eng.sync()
        info["router_status"] = router.sync(None)
        info["collectives"] = pipe.collectives
        info["exchange"] = pipe.exchange
        st = eng.stats()
        info["batches"] = int(st.batches)
        info["spill_used"] = int(eng.table_info(0).spill_used)
        exp = rc.routed_expectations(all_batches, rc.KINDS, rank, CONFIGS, cap=router.capacity)
        info["bad"] = rc.mismatches(outs, exp)
        ok = not info["bad"]
        del pipe
        eng.close()
        router.close()
    finally:
        q.put((rank, ok, info))
        dist.destroy_process_group()


def _spawn(world, backend, **kw):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_routed_ops_rank, args=(r, world, port, backend, q), kwargs=kw) for r in range(world)]
    for p in procs:
        p.start()
    res = {r: (ok, info) for r, ok, info in (q.get(timeout=240) for _ in procs)}
    for p in procs:
        p.join(timeout=60)
    return res


def _check(res, world, exchange):
    import routed_op_cases as rc
    nb = len(rc.KINDS)
    for r in range(world):
        ok, info = res[r]
        assert ok, (r, info)
        assert info["exchange"] == exchange
        assert info["collectives"] == (3 * nb if exchange else 0), info
        assert info["engine_status"] == 0 and info["router_status"] == 0, info
        assert info["batches"] == rc.KINDS.count(rc.D), info       # only decide steps are counted
        assert info["spill_used"] > 0, info                          # peeks and resets met spilled windows


def test_routed_kinds_one_rank_rccl():
    """world 1 with the exchange forced on: every step's three collectives
    over RCCL, the engine's peek / reset kernels between in-flight decides"""
    _check(_spawn(1, "nccl", exchange=True), 1, True)


def test_routed_kinds_one_rank_in_place():
    """world 1 without the exchange: buckets and results read in place (the
    RL_ORDER_IDENTITY form where a step's ts are in order)"""
    _check(_spawn(1, "nccl"), 1, False)


def test_routed_kinds_two_ranks_one_gpu():
    """two ranks (two engines, two routers) on the one GPU, all-to-alls
    through host memory (gloo): merged orders of two sources"""
    _check(_spawn(2, "gloo"), 2, True)


# --- 6. symbols ---------------------------------------------------------------------

def test_routed_op_symbols(rl):
    """the C entry points, the binding's four methods, and the 32-byte wire
    records the kernels load and store as two 16-byte halves"""
    class Rec(C.Structure):
        _fields_ = [("key", C.c_uint64), ("ts", C.c_int64), ("n", C.c_int64), ("cfg", C.c_uint32), ("pos", C.c_uint32)]

    class Res(C.Structure):
        _fields_ = [("decision", C.c_int64), ("remaining", C.c_int64), ("retry_after_ns", C.c_int64),
                    ("reset_at_ns", C.c_int64)]

    assert C.sizeof(Rec) == 32 and C.sizeof(Res) == 32
    for name in ("rl_peek_routed_device", "rl_reset_routed_device"):
        fn = getattr(rl.lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == 10
        assert fn(None, 0, None, None, None, None, None, None, None, None) == rl.RL_EINVAL   # no engine
    for name in ("peek_routed", "peek_routed_ev", "reset_routed", "reset_routed_ev"):
        assert callable(getattr(rl.Engine, name))
    rec = np.zeros(1, np.dtype([("key", "<u8"), ("ts", "<i8"), ("n", "<i8"), ("cfg", "<u4"), ("pos", "<u4")]))
    assert rec.itemsize == 32
