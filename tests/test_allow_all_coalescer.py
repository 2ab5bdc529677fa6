"""AllowAll through the coalescer (rl_coalescer_allow_all) over the host-backend
seam, with the composition on the Python oracle plugged in
(allow_all_cases.apply_allow_all): one submission is one launch and one engine
call, in sequence order between its neighbours, never merged and never split;
its members count like requests."""
import ctypes as C
import threading
import time

import numpy as np

from allow_all_cases import apply_allow_all, group_spans
from oracle import rl_oracle_py as po
from refund_cases import apply_refunds, new_sim, py_peek, warm
from test_refund_coalescer import CONFIGS, EINVAL, N, Store, arr, refunds_of, rows_of, traces
from tracegen import NS, T0

EDEADLINE = -62


class AllStore(Store):
    """test_refund_coalescer.Store plus the AllowAll, reset and peek functions"""

    def allow_all(self, user, m, key, ts, n, cfg, first, dec, rem, retry, reset, verdict):
        self.entered.set()
        self.gate.wait()
        rows, v, g, rb, _ = apply_allow_all(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64),
                                            arr(n, m, C.c_int64), arr(cfg, m, C.c_uint32), arr(first, m, C.c_uint8))
        for i, (d, r, ra, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        arr(verdict, m, C.c_uint8)[:] = v
        self.log.append(("allow_all", m))
        return 0

    def reset_batch(self, user, m, key, ts, cfg, status):
        for k, t, c in zip(arr(key, m, C.c_uint64).tolist(), arr(ts, m, C.c_int64).tolist(),
                           arr(cfg, m, C.c_uint32).tolist()):
            self.sim.reset(c, k, t)
        arr(status, m, C.c_uint8)[:] = 1
        self.log.append(("reset", m))
        return 0

    def peek(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        k, t, c = arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(cfg, m, C.c_uint32)
        for i in range(m):
            d, r, ra, rs, _ = py_peek(self.sim, int(k[i]), int(t[i]), int(c[i]), int(t[i]) // 1_000_000)
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        self.log.append(("peek", m))
        return 0

    def coalescer(self, rl, **kw):
        return rl.Coalescer(self.batch, refund=self.refund, allow_all=self.allow_all, reset_batch=self.reset_batch,
                            peek=self.peek, **kw)


def members_of(part, groups, t, seed=2):
    """`groups` groups of 1 to 5 members on the keys of `part`, all at time t
    -> (key, ts, n, cfg, first)"""
    key, _, _, cfg = part
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 6, groups)
    idx = rng.integers(0, key.size, int(sizes.sum()))
    first = np.zeros(idx.size, np.uint8)
    first[np.cumsum(sizes)[:-1]] = 1
    return key[idx], np.full(idx.size, t, np.int64), rng.choice([1, 1, 2, 3, 7, 50], idx.size).astype(np.int64), \
        cfg[idx], first


def test_sequence_order_against_neighbours(rl):
    """decide | AllowAll, refund, AllowAll, reset, peek, decide queued behind a
    held decide: each runs in submission order on the state the ones before it
    left, and the oracle fed the same sequence gives every answer"""
    warm_tr, held, after = traces()
    store = AllStore()
    co = store.coalescer(rl, max_batch=4096, max_in_flight=2, tally_key_slots=256, hot_min=3)
    t = co.submit(*warm_tr)
    assert co.wait(t, warm_tr[0].size)[0] == 0
    st0 = co.stats()
    t_call = int(held[1][-1]) + 1000
    a1 = members_of(warm_tr, 60, t_call, 2)
    a2 = members_of(warm_tr, 40, t_call + 1000, 3)
    rk, rt, rn, rc_ = refunds_of(warm_tr, 100)
    zk, zc = warm_tr[0][:30], warm_tr[3][:30]
    zt = np.full(30, t_call + 2000)
    store.gate.clear()
    store.entered.clear()
    th = co.submit(*held)
    store.entered.wait()
    out, threads, queued = {}, [], 0
    steps = [("a1", lambda: co.allow_all(*a1), a1[0].size), ("refund", lambda: co.refund(rk, rt, rn, rc_), 100),
             ("a2", lambda: co.allow_all(*a2), a2[0].size), ("reset", lambda: co.reset_batch(zk, zt, zc), 30),
             ("peek", lambda: co.peek(zk, zt, np.zeros(30, np.int64), zc), 30)]
    for name, fn, m in steps:
        x = threading.Thread(target=lambda name=name, fn=fn: out.update({name: fn()}))
        x.start()
        threads.append(x)
        queued += m
        while co.stats().pending < queued:          # queued in this order
            time.sleep(0.0005)
    ta = co.submit(*after)
    assert co.stats().allow_all_launches == st0.allow_all_launches
    store.gate.set()
    for x in threads:
        x.join()
    assert co.wait(th, 1)[0] == 0
    rc, got = co.wait(ta, after[0].size)
    assert rc == 0
    st1 = co.stats()
    rct, tally = co.tally()
    rch, hot = co.hot(top=4)
    co.close()
    # the host tally and top keys count an AllowAll launch's members like a decide batch's requests
    assert (rct, rch) == (0, 0) and int(tally.cfg["count"].sum()) == st1.decided == hot.info.requests
    assert hot.info.batches == 5                     # three decides and the two AllowAll launches
    assert [x[0] for x in store.log[1:]] == ["batch", "allow_all", "refund", "allow_all", "reset", "peek", "batch"]
    ref = new_sim(0, CONFIGS)
    warm(ref, warm_tr + (None,))
    warm(ref, held + (None,))
    failed = 0
    for name, a in (("a1", a1), ("refund", None), ("a2", a2)):
        if a is None:
            want_st, _ = apply_refunds(ref, rk, rt, rn, rc_)
            assert out["refund"][0] == 0 and np.array_equal(out["refund"][1], want_st)
            continue
        rows, v, g, rb, _ = apply_allow_all(ref, *a)
        rc, res = out[name]
        assert rc == 0 and rows_of(res, a[0].size) == [w[:4] for w in rows], name
        assert np.array_equal(res[4], v), name
        failed += int((v != po.ALLOWED).sum())
        assert (v == po.ALLOWED).any() and (v == po.DENIED).any() and (g > 0).any(), name
    for k, tt, c in zip(zk.tolist(), zt.tolist(), zc.tolist()):
        ref.reset(c, k, tt)
    assert out["reset"][0] == 0 and (out["reset"][1] == 1).all()
    want_peek = [py_peek(ref, int(k), int(tt), int(c), int(tt) // 1_000_000)[:4] for k, tt, c in zip(zk, zt, zc)]
    assert out["peek"][0] == 0 and rows_of(out["peek"][1], 30) == want_peek
    assert rows_of(got, after[0].size) == [w[:4] for w in warm(ref, after + (None,))]
    # the members count like requests; the launches and groups have counters of their own
    members = a1[0].size + a2[0].size
    assert (st1.submitted - st0.submitted, st1.decided - st0.decided) == (400 + members, 400 + members)
    assert st1.allow_all_launches - st0.allow_all_launches == 2
    assert st1.allow_all_groups - st0.allow_all_groups == len(group_spans(a1[4])) + len(group_spans(a2[4])) == 100
    assert st1.batches - st0.batches == 3          # two decides and the reset launch
    assert st1.refund_launches - st0.refund_launches == 1 and st1.peeked - st0.peeked == 30


def test_two_adjacent_submissions_are_two_launches(rl):
    """two AllowAll submissions queued behind a held decide are two engine
    calls in order: the second group is denied on the first's transient take
    when both travel in one call, and allowed when each is a call of its own"""
    configs = [(1, 20, 12 * NS)]
    verdicts = []
    for split in (True, False):
        store = AllStore(configs)
        co = store.coalescer(rl, max_batch=64, max_in_flight=1)
        store.gate.clear()
        store.entered.clear()
        th = co.submit([9], [T0], [1], [0])
        store.entered.wait()
        one, two = ([1, 2], [15, 40], [1, 0]), ([1], [15], [1])
        calls = [one, two] if split else [tuple(a + b for a, b in zip(one, two))]
        res, ths = [None] * len(calls), []
        for j, (k, n, f) in enumerate(calls):
            x = threading.Thread(target=lambda j=j, k=k, n=n, f=f: res.__setitem__(
                j, co.allow_all(k, [T0] * len(k), n, [0] * len(k), f)))
            x.start()
            ths.append(x)
            while co.stats().pending < sum(len(c[0]) for c in calls[:j + 1]):
                time.sleep(0.0005)
        store.gate.set()
        for x in ths:
            x.join()
        assert co.wait(th, 1)[0] == 0
        st = co.stats()
        co.close()
        assert all(r[0] == 0 for r in res)
        assert [x for x in store.log if x[0] == "allow_all"] == [("allow_all", len(c[0])) for c in calls]
        assert (st.allow_all_launches, st.allow_all_groups) == (len(calls), 2)
        verdicts.append(np.concatenate([r[1][4] for r in res]).tolist())
        assert store.sim.db["tb:1"][0][0] == (5.0 if split else 20.0)
    assert verdicts == [[po.DENIED, po.DENIED, po.ALLOWED], [po.DENIED] * 3]


def test_limits_deadline_and_old_struct_size(rl):
    """above max_batch: RL_EINVAL, not split; m = 0 is done at once; null
    arrays; a deadline passed before the launch drops the submission unapplied;
    a backend without `allow_all` (null, or a struct from before the field) is
    RL_EINVAL; a caller compiled before the new counters keeps its struct"""
    store = AllStore()
    co = store.coalescer(rl, max_batch=64, max_in_flight=1)
    k = np.arange(65, dtype=np.uint64)
    one = lambda m: (k[:m], np.full(m, T0), np.ones(m, np.int64), np.zeros(m, np.uint32), np.ones(m, np.uint8))
    assert co.allow_all(*one(65))[0] == EINVAL and store.log == []
    rc, res = co.allow_all(*one(64))
    assert rc == 0 and (res[0] == po.ALLOWED).all() and (res[4] == po.ALLOWED).all()
    assert store.log == [("allow_all", 64)]
    assert co.allow_all([], [], [], [], [])[0] == 0 and len(store.log) == 1
    z = np.zeros(3, np.int64)
    p = z.ctypes.data_as(C.c_void_p)
    assert rl.lib.rl_coalescer_allow_all(co.h, 3, p, p, p, p, None, 0, p, p, p, p, p) == EINVAL
    assert rl.lib.rl_coalescer_allow_all(co.h, 3, None, None, None, None, None, 0, None, None, None, None, None) == EINVAL
    # a deadline that passes while a decide holds the backend
    st0 = co.stats()
    before = {name: list(v) for name, v in store.sim.db.items()}
    store.gate.clear()
    store.entered.clear()
    th = co.submit([900], [T0], [1], [0])
    store.entered.wait()
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.allow_all(*one(8), deadline_ns=rl.now_ns() + 2_000_000)))
    thr.start()
    thr.join()                                   # its wait ends at the deadline, the decide still held
    store.gate.set()
    assert co.wait(th, 1)[0] == 0
    assert out["r"][0] == EDEADLINE
    rc, _ = co.allow_all(*one(2))                # the queue moves on
    st1 = co.stats()
    assert rc == 0 and store.log[1:] == [("batch", 1), ("allow_all", 2)]
    assert st1.expired - st0.expired == 8 and st1.allow_all_launches - st0.allow_all_launches == 1
    assert (st1.submitted - st0.submitted, st1.decided - st0.decided) == (11, 3)
    assert all(store.sim.db[name] == v for name, v in before.items() if name not in ("tb:0", "tb:1"))
    old = rl.rl_coalescer_stats()
    old.struct_size = rl.rl_coalescer_stats.allow_all_groups.offset
    old.allow_all_groups = old.allow_all_launches = 12345
    assert rl.lib.rl_coalescer_get_stats(co.h, C.byref(old)) == 0
    assert (old.allow_all_groups, old.allow_all_launches) == (12345, 12345)
    assert (old.struct_size, old.refund_launches) == (rl.rl_coalescer_stats.allow_all_groups.offset, 0)
    full = co.stats()
    assert (full.allow_all_groups, full.allow_all_launches, full.struct_size) == (66, 2, C.sizeof(rl.rl_coalescer_stats))
    co.close()
    # no allow_all function
    co = rl.Coalescer(store.batch, max_batch=64, refund=store.refund)
    assert co.allow_all(*one(1))[0] == EINVAL
    co.close()
    # a backend struct from before the field
    keep = rl.BATCH_FN(store.batch)
    b = rl.rl_coalescer_backend(batch=keep, reset=C.cast(None, rl.RESET_FN), table_info=C.cast(None, rl.INFO_FN),
                                gc=C.cast(None, rl.GC_FN), user=None, peek=C.cast(None, rl.BATCH_FN),
                                reset_batch=C.cast(None, rl.RESET_BATCH_FN), refund=C.cast(None, rl.REFUND_FN),
                                allow_all=rl.ALLOW_ALL_FN(store.allow_all))
    b.struct_size = rl.rl_coalescer_backend.allow_all.offset
    o = rl.rl_coalescer_opts(max_batch=64, max_in_flight=2)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == 0
    n_log = len(store.log)
    assert rl.lib.rl_coalescer_allow_all(h, 3, p, p, p, p, p, 0, p, p, p, p, p) == EINVAL   # the field past its size is not read
    assert len(store.log) == n_log
    assert rl.lib.rl_coalescer_destroy(h) == 0
    b.struct_size = rl.rl_coalescer_backend.allow_all.offset + 4
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == EINVAL
