"""Charge through the coalescer (rl_coalescer_charge) over the host-backend
seam, with the composition on the Python oracle plugged in
(charge_cases.apply_charge): one submission is one launch and one engine call,
in sequence order between its neighbours, never merged and never split; its
requests count like a decide batch's."""
import ctypes as C
import threading
import time

import numpy as np

from charge_cases import apply_charge
from oracle import rl_oracle_py as po
from refund_cases import new_sim, warm
from test_refund_coalescer import CONFIGS, EINVAL, Store, arr, rows_of, traces
from tracegen import NS, T0

EAGAIN, EDEADLINE = -11, -62


class ChargeStore(Store):
    """test_refund_coalescer.Store plus the Charge function"""

    def charge(self, user, m, key, ts, n, cfg, dec, charged, rem, reset):
        self.entered.set()
        self.gate.wait()
        rows, _ = apply_charge(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                               arr(cfg, m, C.c_uint32))
        for i, (d, got, r, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(charged, m, C.c_int64)[i] = d, got
            arr(rem, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = r, rs
        self.log.append(("charge", m))
        return 0

    def coalescer(self, rl, **kw):
        return rl.Coalescer(self.batch, charge=self.charge, **kw)


def charges_of(part, count, t, seed=2):
    """`count` charges on the keys of `part`, all at time t -> (key, ts, n, cfg)"""
    key, _, _, cfg = part
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, key.size, count)
    return key[idx], np.full(count, t, np.int64), rng.choice([1, 1, 2, 3, 7, 50], count).astype(np.int64), cfg[idx]


def test_sequence_order_against_neighbours(rl):
    """decide | Charge, Charge, decide queued behind a held decide: each runs
    in submission order on the state the ones before it left, and the oracle
    fed the same sequence gives every answer"""
    warm_tr, held, after = traces()
    store = ChargeStore()
    co = store.coalescer(rl, max_batch=4096, max_in_flight=2, tally_key_slots=256, hot_min=3)
    t = co.submit(*warm_tr)
    assert co.wait(t, warm_tr[0].size)[0] == 0
    st0 = co.stats_charge()
    t_call = int(held[1][-1]) + 1000
    c1 = charges_of(warm_tr, 300, t_call, 2)
    c2 = charges_of(warm_tr, 200, t_call + 1000, 3)
    store.gate.clear()
    store.entered.clear()
    th = co.submit(*held)
    store.entered.wait()
    out, threads, queued = {}, [], 0
    for name, c in (("c1", c1), ("c2", c2)):
        x = threading.Thread(target=lambda name=name, c=c: out.update({name: co.charge(*c)}))
        x.start()
        threads.append(x)
        queued += c[0].size
        while co.stats().pending < queued:          # queued in this order
            time.sleep(0.0005)
    ta = co.submit(*after)
    assert co.stats_charge().charge_launches == st0.charge_launches
    store.gate.set()
    for x in threads:
        x.join()
    assert co.wait(th, 1)[0] == 0
    rc, got = co.wait(ta, after[0].size)
    assert rc == 0
    st1 = co.stats_charge()
    rct, tally = co.tally()
    rch, hot = co.hot(top=4)
    co.close()
    # the host tally and top keys count a Charge launch's requests like a decide batch's
    assert (rct, rch) == (0, 0) and int(tally.cfg["count"].sum()) == st1.decided == hot.info.requests
    assert hot.info.batches == 5                     # three decides and the two Charge launches
    assert [x[0] for x in store.log[1:]] == ["batch", "charge", "charge", "batch"]
    ref = new_sim(0, CONFIGS)
    warm(ref, warm_tr + (None,))
    warm(ref, held + (None,))
    seen = set()
    for name, c in (("c1", c1), ("c2", c2)):
        rows, info = apply_charge(ref, *c)
        rc, res = out[name]
        # (decision, charged, remaining, reset_at_ns)
        assert rc == 0 and rows_of(res, c[0].size) == [w[:4] for w in rows], name
        seen |= set(info["cls"].tolist())
    assert {"full", "short", "dup_denied", "over"} <= seen
    assert rows_of(got, after[0].size) == [w[:4] for w in warm(ref, after + (None,))]
    # the requests count like a decide's; the launches have a counter of their own
    assert (st1.submitted - st0.submitted, st1.decided - st0.decided) == (900, 900)
    assert st1.charge_launches - st0.charge_launches == 2
    assert st1.batches - st0.batches == 2          # the two decides
    assert st1.struct_size == C.sizeof(rl.rl_coalescer_stats_charge)


def test_two_adjacent_submissions_are_never_merged(rl):
    """two Charge submissions queued behind a held decide are two engine calls
    in order: the second one's ask reads what the first one left.  In one call
    the second request asks against the state before the call and is denied"""
    configs = [(1, 20, 12 * NS)]
    results = []
    for split in (True, False):
        store = ChargeStore(configs)
        co = store.coalescer(rl, max_batch=64, max_in_flight=1)
        store.gate.clear()
        store.entered.clear()
        th = co.submit([9], [T0], [1], [0])
        store.entered.wait()
        one, two = ([1], [15]), ([1], [15])
        calls = [one, two] if split else [tuple(a + b for a, b in zip(one, two))]
        res, ths = [None] * len(calls), []
        for j, (k, n) in enumerate(calls):
            x = threading.Thread(target=lambda j=j, k=k, n=n: res.__setitem__(
                j, co.charge(k, [T0] * len(k), n, [0] * len(k))))
            x.start()
            ths.append(x)
            while co.stats().pending < sum(len(c[0]) for c in calls[:j + 1]):
                time.sleep(0.0005)
        store.gate.set()
        for x in ths:
            x.join()
        assert co.wait(th, 1)[0] == 0
        st = co.stats_charge()
        co.close()
        assert all(r[0] == 0 for r in res)
        assert [x for x in store.log if x[0] == "charge"] == [("charge", len(c[0])) for c in calls]
        assert st.charge_launches == len(calls)
        results.append([(int(d), int(c)) for r in res for d, c in zip(r[1][0], r[1][1])])
    # two calls: 15 of 20, then the 5 that are left; one call: 15, then 15 asked of 5 is denied
    assert results == [[(po.ALLOWED, 15), (po.DENIED, 5)], [(po.ALLOWED, 15), (po.DENIED, 0)]]


def test_limits_queue_refusal_and_deadline(rl):
    """above max_batch: RL_EINVAL, not split; m = 0 is done at once; null
    arrays; a full queue refuses the submission; a deadline passed before the
    launch drops it unapplied; a backend without `charge` (null, or a struct
    from before the field) is RL_EINVAL"""
    store = ChargeStore()
    co = store.coalescer(rl, max_batch=64, max_in_flight=1, queue_cap=100)
    k = np.arange(65, dtype=np.uint64)
    one = lambda m: (k[:m], np.full(m, T0), np.ones(m, np.int64), np.zeros(m, np.uint32))
    assert co.charge(*one(65))[0] == EINVAL and store.log == []
    rc, res = co.charge(*one(64))
    assert rc == 0 and (res[0] == po.ALLOWED).all() and (res[1] == 1).all()
    assert store.log == [("charge", 64)]
    assert co.charge([], [], [], [])[0] == 0 and len(store.log) == 1
    z = np.zeros(3, np.int64)
    p = z.ctypes.data_as(C.c_void_p)
    assert rl.lib.rl_coalescer_charge(co.h, 3, p, p, None, p, 0, p, p, p, p) == EINVAL
    assert rl.lib.rl_coalescer_charge(co.h, 3, None, None, None, None, 0, None, None, None, None) == EINVAL
    assert rl.lib.rl_coalescer_charge(None, 0, None, None, None, None, 0, None, None, None, None) == EINVAL
    # a full queue, then a deadline that passes, while a decide holds the backend
    st0 = co.stats()
    store.gate.clear()
    store.entered.clear()
    th = co.submit([900], [T0], [1], [0])
    store.entered.wait()
    tq = co.submit(k[:60], np.full(60, T0), np.ones(60, np.int64), np.zeros(60, np.uint32))
    assert co.charge(*one(64))[0] == EAGAIN          # 60 pending + 64 > 100
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.charge(*one(8), deadline_ns=rl.now_ns() + 2_000_000)))
    thr.start()
    thr.join()                                   # its wait ends at the deadline, the decide still held
    store.gate.set()
    assert co.wait(th, 1)[0] == 0 and co.wait(tq, 60)[0] == 0
    assert out["r"][0] == EDEADLINE
    rc, _ = co.charge(*one(2))                   # the queue moves on
    st1 = co.stats_charge()
    assert rc == 0 and store.log[1:] == [("batch", 1), ("batch", 60), ("charge", 2)]
    assert st1.expired - st0.expired == 8 and st1.charge_launches == 2
    assert (st1.submitted - st0.submitted, st1.decided - st0.decided) == (71, 63)
    # a caller compiled before the counter: rl_coalescer_get_stats writes the struct of its time and no more
    big = (C.c_uint8 * C.sizeof(rl.rl_coalescer_stats_charge))()
    C.memset(big, 0xAB, C.sizeof(big))
    C.cast(big, C.POINTER(C.c_uint32))[0] = C.sizeof(big)
    assert rl.lib.rl_coalescer_get_stats(co.h, C.cast(big, C.POINTER(rl.rl_coalescer_stats))) == 0
    assert C.cast(big, C.POINTER(C.c_uint32))[0] == C.sizeof(rl.rl_coalescer_stats)
    assert bytes(big[C.sizeof(rl.rl_coalescer_stats):]) == b"\xab" * 8
    short = rl.rl_coalescer_stats_charge()
    short.struct_size = rl.rl_coalescer_stats_charge.charge_launches.offset
    short.charge_launches = 12345
    assert rl.lib.rl_coalescer_get_stats_charge(co.h, C.byref(short)) == 0
    assert (short.charge_launches, short.struct_size, short.decided) == (12345, C.sizeof(rl.rl_coalescer_stats),
                                                                         st1.decided)
    co.close()
    # no charge function
    co = rl.Coalescer(store.batch, max_batch=64)
    assert co.charge(*one(1))[0] == EINVAL
    co.close()
    # a backend struct from before the field: the function past its size is not read
    b = rl.rl_coalescer_backend_charge(batch=rl.BATCH_FN(store.batch), charge=rl.CHARGE_FN(store.charge))
    b.struct_size = C.sizeof(rl.rl_coalescer_backend)
    o = rl.rl_coalescer_opts(max_batch=64, max_in_flight=2)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == 0
    n_log = len(store.log)
    assert rl.lib.rl_coalescer_charge(h, 3, p, p, p, p, 0, p, p, p, p) == EINVAL
    assert len(store.log) == n_log
    assert rl.lib.rl_coalescer_destroy(h) == 0
    b.struct_size = C.sizeof(rl.rl_coalescer_backend) + 4
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == EINVAL
