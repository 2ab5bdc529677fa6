"""rl_coalescer_peek over a host backend (CPU): the Python oracle behind the
test seam, with peek_cases.peek_expected as the backend's `peek`."""
import ctypes as C
import threading

import numpy as np

from oracle import rl_oracle_py as po
from peek_cases import peek_expected
from tracegen import NS, T0

CONFIGS = [(1, 5, 60 * NS), (2, 4, 60 * NS), (3, 3, 60 * NS)]


def arr(p, n, dtype):
    """the backend's view of a C array argument"""
    ct = {np.uint64: C.c_uint64, np.int64: C.c_int64, np.uint32: C.c_uint32, np.uint8: C.c_uint8}[dtype]
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))


class OracleBackend:
    """rl_batch_fn / the peek function over one Python oracle; `log` records
    the calls in the order the coalescer made them"""

    def __init__(self):
        self.sim = po.Sim(po.REDIS7)
        for a, L, W in CONFIGS:
            self.sim.add_config(a, L, W)
        self.log = []

    def _run(self, fn, what, m, key, ts, n, cfg, dec, rem, retry, reset):
        k, t, nn, c = arr(key, m, np.uint64), arr(ts, m, np.int64), arr(n, m, np.int64), arr(cfg, m, np.uint32)
        self.log.append((what, m))
        out = fn(k, t, nn, c)
        arr(dec, m, np.uint8)[:], arr(rem, m, np.int64)[:] = out[0], out[1]
        arr(retry, m, np.int64)[:], arr(reset, m, np.int64)[:] = out[2], out[3]
        return 0

    def batch(self, user, m, *a):
        def decide(k, t, nn, c):
            rows = [self.sim.decide(int(k[i]), int(t[i]), int(nn[i]), int(c[i])) for i in range(m)]
            return [[r[j] for r in rows] for j in range(4)]
        return self._run(decide, "batch", m, *a)

    def peek(self, user, m, *a):
        return self._run(lambda k, t, nn, c: peek_expected(self.sim, k, t, nn, c), "peek", m, *a)


def one(key, n, cfg, t=T0):
    return (np.array([key], np.uint64), np.array([t], np.int64), np.array([n], np.int64), np.array([cfg], np.uint32))


def test_peek_sees_what_was_submitted_before_and_not_after(rl):
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=64, peek=be.peek)
    for cfg, limit in ((0, 5), (1, 4), (2, 3)):
        key = 100 + cfg
        ta = co.submit(*one(key, 2, cfg))                 # a: takes 2
        rc, p = co.peek(*one(key, 0, cfg, T0 + 1))        # sees a ...
        tb = co.submit(*one(key, 1, cfg, T0 + 2))         # ... and not b
        assert rc == 0 and p[0][0] == rl.ALLOWED and p[1][0] == limit - 2
        rc, a = co.wait(ta, 1)
        assert rc == 0 and a[1][0] == limit - 2
        rc, b = co.wait(tb, 1)
        assert rc == 0 and b[1][0] == limit - 3
        # a peek of more than is left is denied, and changes nothing
        rc, p = co.peek(*one(key, limit, cfg, T0 + 3))
        assert rc == 0 and p[0][0] == rl.DENIED
        rc, p = co.peek(*one(key, 0, cfg, T0 + 4))
        assert rc == 0 and p[1][0] == limit - 3
    # in the backend's order too: every peek between its neighbours
    assert [w for w, _ in be.log] == ["batch", "peek", "batch", "peek", "peek"] * 3
    st = co.stats()
    assert (st.submitted, st.decided, st.peeked) == (6, 6, 9)
    co.close()


def test_peek_without_a_peek_backend_is_einval(rl):
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=64)
    rc, _ = co.peek(*one(1, 0, 0))
    assert rc == rl.RL_EINVAL
    # the coalescer goes on working
    rc, out = co.decide(1, T0, 1, 0)
    assert rc == 0 and out[0] == rl.ALLOWED
    st = co.stats()
    assert (st.submitted, st.decided) == (1, 1)
    co.close()


def test_old_backend_struct_size_still_works(rl):
    """a caller compiled before `peek` existed passes the shorter struct"""
    be = OracleBackend()
    fn = rl.BATCH_FN(be.batch)
    b = rl.rl_coalescer_backend(batch=fn, reset=C.cast(None, rl.RESET_FN), table_info=C.cast(None, rl.INFO_FN),
                                gc=C.cast(None, rl.GC_FN), user=None, peek=rl.BATCH_FN(be.peek))
    b.struct_size = rl.rl_coalescer_backend.peek.offset
    o = rl.rl_coalescer_opts(max_batch=16)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == 0
    out = [np.empty(1, np.uint8)] + [np.empty(1, np.int64) for _ in range(3)]
    q = one(5, 0, 0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # the field past the caller's struct is not read: no peek backend
    assert rl.lib.rl_coalescer_peek(h, 1, *[ptr(x) for x in q], *[ptr(x) for x in out]) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_destroy(h) == 0
    b.struct_size = 12
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == rl.RL_EINVAL


def test_peeks_leave_submitted_and_decided_alone_under_threads(rl):
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=32, peek=be.peek)
    done = []

    def submitter(i):
        for j in range(30):
            rc, out = co.decide(i, T0 + j, 1, i % 3)
            done.append(rc)

    def peeker():
        for j in range(40):
            k = np.arange(7, dtype=np.uint64)
            rc, out = co.peek(k, np.full(7, T0 + 100), np.zeros(7, np.int64), (k % 3).astype(np.uint32))
            done.append(rc)
            assert (out[0] <= 1).all()

    ths = [threading.Thread(target=submitter, args=(i,)) for i in range(4)] + [threading.Thread(target=peeker)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert done.count(0) == 4 * 30 + 40
    st = co.stats()
    assert (st.submitted, st.decided, st.peeked, st.pending) == (120, 120, 280, 0)
    # a peek of more requests than max_batch is split across launches
    k = np.arange(100, dtype=np.uint64)
    rc, out = co.peek(k, np.full(100, T0 + 200), np.zeros(100, np.int64), (k % 3).astype(np.uint32))
    assert rc == 0 and co.stats().peeked == 380
    want = peek_expected(be.sim, k, np.full(100, T0 + 200), np.zeros(100, np.int64), (k % 3).astype(np.uint32))
    assert (out[0] == want[0]).all() and (out[1] == want[1]).all()
    co.close()
