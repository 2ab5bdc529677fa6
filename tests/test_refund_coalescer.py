"""Refunds through the coalescer (rl_coalescer_refund): one submission is one
launch and one engine call, in sequence order, never merged with the refund
submission next to it.  CPU: the host-backend seam over the Python oracle
(refund_cases.apply_refunds); GPU: the engine."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from oracle import rl_oracle_py as po
from refund_cases import DONE, INVALID, NOKEY, apply_refunds, bucket_counterexample, new_sim, warm
from tracegen import CONFIG_SETS, NS, T0, random_trace

CONFIGS = CONFIG_SETS["mixed"]
N = len(CONFIGS)
EINVAL = -22


def arr(p, n, ct):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))


class Store:
    """the host backend over one Python oracle; `gate` holds the batch function"""

    def __init__(self, configs=CONFIGS, profile=0):
        self.sim = new_sim(profile, configs)
        self.gate = threading.Event()
        self.gate.set()
        self.entered = threading.Event()
        self.log = []

    def batch(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        self.entered.set()
        self.gate.wait()
        rows = warm(self.sim, (arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                               arr(cfg, m, C.c_uint32), None))
        for i, (d, r, ra, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        self.log.append(("batch", m))
        return 0

    def refund(self, user, m, key, ts, n, cfg, status):
        st, _ = apply_refunds(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                              arr(cfg, m, C.c_uint32))
        arr(status, m, C.c_uint8)[:] = st
        self.log.append(("refund", m))
        return 0


def traces():
    tr = random_trace(9, 1200, 300, CONFIGS)
    cut = lambda a, b: tuple(x[a:b] for x in tr[:4])
    return cut(0, 800), cut(800, 801), cut(801, 1200)


def rows_of(got, m):
    return [tuple(int(got[j][i]) for j in range(4)) for i in range(m)]


def refunds_of(part, count, seed=1):
    """`count` refunds, n = 1 .. 3, each aimed at some key's last request of
    `part`: the store clock of a refund here is floor(ts / 1e6), and a key's
    store clock must not go back"""
    key, ts, n, cfg = part
    rng = np.random.default_rng(seed)
    last = np.array(sorted({int(k): i for i, k in enumerate(key.tolist())}.values()))
    idx = last[rng.integers(0, last.size, count)]
    return key[idx], ts[idx], rng.integers(1, 4, count).astype(np.int64), cfg[idx]


def test_sequence_order_against_neighbours(rl):
    """decide, refund, decide through the seam: the refund sees every request
    submitted before it and none submitted after it; its status is the
    oracle's; it counts in refunds / refund_launches only"""
    warm_tr, held, after = traces()
    store = Store()
    co = rl.Coalescer(store.batch, max_batch=4096, max_in_flight=2, refund=store.refund)
    t = co.submit(*warm_tr)
    assert co.wait(t, warm_tr[0].size)[0] == 0
    st0 = co.stats()
    rk, rt, rn, rc_ = refunds_of(warm_tr, 300)
    rc_ = rc_.copy()
    rc_[::50] = N                              # invalid ones travel with the rest
    # hold a decide in the backend, queue the refund and another decide behind it
    store.gate.clear()
    store.entered.clear()
    th = co.submit(*held)
    store.entered.wait()
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.refund(rk, rt, rn, rc_)))
    thr.start()
    while co.stats().pending < 300:
        time.sleep(0.0005)
    ta = co.submit(*after)
    assert co.stats().refund_launches == st0.refund_launches
    store.gate.set()
    thr.join()
    assert co.wait(th, 1)[0] == 0
    rc, got = co.wait(ta, after[0].size)
    assert rc == 0
    st1 = co.stats()
    co.close()
    ref = new_sim(0, CONFIGS)
    warm(ref, warm_tr + (None,))
    warm(ref, held + (None,))
    want_st, info = apply_refunds(ref, rk, rt, rn, rc_)
    want = warm(ref, after + (None,))
    assert out["r"][0] == 0 and np.array_equal(out["r"][1], want_st)
    assert (want_st == DONE).sum() > 50 and (want_st == INVALID).sum() == 6 and (want_st == NOKEY).sum() > 0
    assert rows_of(got, after[0].size) == [w[:4] for w in want]
    assert [x for x in store.log if x[0] == "refund"] == [("refund", 300)]
    assert store.log.index(("refund", 300)) == store.log.index(("batch", 1)) + 1     # between its neighbours
    assert (st1.refunds - st0.refunds, st1.refund_launches - st0.refund_launches) == (int((want_st == DONE).sum()), 1)
    assert (st1.submitted - st0.submitted, st1.decided - st0.decided) == (400, 400)
    assert (st1.resets, st1.reset_launches, st1.peeked) == (st0.resets, st0.reset_launches, st0.peeked)
    assert st1.batches - st0.batches == 2      # the two decides: a refund launch is no batch


def test_two_single_submissions_are_not_merged(rl):
    """the bucket example of DESIGN §10i: two refund submissions queued behind
    a held decide stay two engine calls in sequence order, and so leave
    q14(q14(t + a) + b); one submission of both leaves q14(t + a + b)"""
    t, a, b = bucket_counterexample()[0]
    configs = [(1, 10 ** 6, 60 * NS)]
    left = []
    for split in (True, False):
        store = Store(configs)
        store.sim.db["tb:1"] = [(t, float(T0) / 1e9), T0 // 1_000_000 + 120_000]
        co = rl.Coalescer(store.batch, max_batch=64, max_in_flight=1, refund=store.refund)
        store.gate.clear()
        store.entered.clear()
        th = co.submit([9], [T0], [1], [0])
        store.entered.wait()
        calls = [([1], [a]), ([1], [b])] if split else [([1, 1], [a, b])]
        res, ths = [None] * len(calls), []
        for j, (k, n) in enumerate(calls):
            def one(j=j, k=k, n=n):
                res[j] = co.refund(k, [T0] * len(k), n, [0] * len(k))
            x = threading.Thread(target=one)
            x.start()
            ths.append(x)
            while co.stats().pending < sum(len(c[0]) for c in calls[:j + 1]):   # queued in this order
                time.sleep(0.0005)
        store.gate.set()
        for x in ths:
            x.join()
        assert co.wait(th, 1)[0] == 0
        st = co.stats()
        co.close()
        assert all(r[0] == 0 and (r[1] == DONE).all() for r in res)
        assert [x for x in store.log if x[0] == "refund"] == [("refund", len(c[0])) for c in calls]
        assert (st.refunds, st.refund_launches) == (2, len(calls))
        left.append(store.sim.db["tb:1"][0][0])
    q = lambda x: po.lua_roundtrip(x, 0)
    assert left == [q(q(t + float(a)) + float(b)), q(t + float(a + b))] and left[0] != left[1]


def test_limits_and_old_struct_size(rl):
    """a submission above max_batch is RL_EINVAL and is not split; m = 0 is
    done at once; a backend without `refund` (null, or a struct from before
    the field) answers RL_EINVAL; the stats of a caller compiled before the
    refund counters stay inside its struct"""
    store = Store()
    co = rl.Coalescer(store.batch, max_batch=64, refund=store.refund)
    k = np.arange(65, dtype=np.uint64)
    rc, _ = co.refund(k, np.full(65, T0), np.ones(65, np.int64), np.zeros(65, np.uint32))
    assert rc == EINVAL and store.log == []
    rc, st = co.refund(k[:64], np.full(64, T0), np.ones(64, np.int64), np.zeros(64, np.uint32))
    assert rc == 0 and (st == NOKEY).all() and store.log == [("refund", 64)]
    assert co.refund([], [], [], [])[0] == 0 and store.log == [("refund", 64)]
    assert rl.lib.rl_coalescer_refund(co.h, 3, None, None, None, None, None) == EINVAL
    old = rl.rl_coalescer_stats()
    old.struct_size = rl.rl_coalescer_stats.refunds.offset
    old.refunds = old.refund_launches = 12345
    assert rl.lib.rl_coalescer_get_stats(co.h, C.byref(old)) == 0
    assert (old.refunds, old.refund_launches, old.struct_size) == (12345, 12345, rl.rl_coalescer_stats.refunds.offset)
    full = co.stats()
    assert (full.refunds, full.refund_launches, full.struct_size) == (0, 1, C.sizeof(rl.rl_coalescer_stats))
    co.close()
    # no refund function
    co = rl.Coalescer(store.batch, max_batch=64)
    assert co.refund([1], [T0], [1], [0])[0] == EINVAL
    co.close()
    # a backend struct from before the field
    keep = rl.BATCH_FN(store.batch)
    b = rl.rl_coalescer_backend(batch=keep, reset=C.cast(None, rl.RESET_FN), table_info=C.cast(None, rl.INFO_FN),
                                gc=C.cast(None, rl.GC_FN), user=None, peek=C.cast(None, rl.BATCH_FN),
                                reset_batch=C.cast(None, rl.RESET_BATCH_FN), refund=rl.REFUND_FN(store.refund))
    b.struct_size = rl.rl_coalescer_backend.refund.offset
    o = rl.rl_coalescer_opts(max_batch=64, max_in_flight=2)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == 0
    z = np.zeros(1, np.int64)
    p = z.ctypes.data_as(C.c_void_p)
    n_log = len(store.log)
    assert rl.lib.rl_coalescer_refund(h, 1, p, p, p, p, None) == EINVAL      # the field past its size is not read
    assert len(store.log) == n_log
    assert rl.lib.rl_coalescer_destroy(h) == 0
    b.struct_size = rl.rl_coalescer_backend.refund.offset + 4
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == EINVAL


@pytest.mark.gpu
def test_gpu_refund_between_decides(rl):
    """the engine behind the coalescer: decide, refund, decide, no drain; the
    oracle's statuses and decisions"""
    warm_tr, held, after = traces()
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12, flags=rl.OPT_PIPELINE)
    ref = new_sim(0, CONFIGS)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=1 << 12)
    t0 = co.submit(*warm_tr)
    rk, rt, rn, rc_ = refunds_of(warm_tr, 300)
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.refund(rk, rt, rn, rc_)))
    while co.stats().pending:                  # the warm-up is launched (not waited for)
        time.sleep(0.0005)
    thr.start()
    while co.stats().refund_launches == 0 and co.stats().pending == 0:   # the refund is queued, or launched
        time.sleep(0.0005)
    t1 = co.submit(*after)
    thr.join()
    rc0, got0 = co.wait(t0, warm_tr[0].size)
    rc1, got1 = co.wait(t1, after[0].size)
    assert (rc0, rc1, out["r"][0]) == (0, 0, 0)
    st = co.stats()
    # one submission above the engine's largest call is refused, unsplit
    big = np.zeros((1 << 12) + 1, np.int64)
    assert co.refund(big.astype(np.uint64), big, big + 1, big.astype(np.uint32))[0] == EINVAL
    co.close()
    assert eng.sync() == 0
    eng.close()
    want0 = warm(ref, warm_tr + (None,))
    want_st, _ = apply_refunds(ref, rk, rt, rn, rc_)
    want1 = warm(ref, after + (None,))
    assert np.array_equal(out["r"][1], want_st) and (want_st == DONE).sum() > 50
    assert rows_of(got0, warm_tr[0].size) == [w[:4] for w in want0]
    assert rows_of(got1, after[0].size) == [w[:4] for w in want1]
    assert (st.refunds, st.refund_launches) == (int((want_st == DONE).sum()), 1)
