"""RateLimiterRefund (Refund, RefundBatch) on both gRPC servers: over the
coalescer's host seam with the Python oracle as the store (CPU), and over the
HIP engine (GPU).  Both servers run on a test clock that advances 100 ms per
read, so the scenario crosses a 2 s window at a known request."""
import ctypes as C
import threading

import grpc
import numpy as np
import pytest

import rl_amd
import rl_grpc
import rl_server
from refund_cases import apply_refunds, new_sim, warm
from test_grpc import LIMITERS, start

NS = 1_000_000_000
S0 = 1_760_000_000 * NS          # a start of the 2 s windows; 20 s into a 60 s window
STEP = 100_000_000               # the k-th clock read is S0 + k * STEP
ERR_INVALID_N = "invalid n: must be greater than 0"


class StepClock:
    def __init__(self):
        self.k = 0
        self.lock = threading.Lock()

    def __call__(self):
        with self.lock:
            self.k += 1
            return S0 + self.k * STEP


def arr(p, n, ct):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))


class PyStore:
    """the coalescer's host backend: the Python oracle, keyed by engine key ids"""

    def __init__(self):
        self.sim = new_sim(0, [])

    def register(self, alg, limit, window):
        return self.sim.add_config(alg, limit, window)

    def batch(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        rows = warm(self.sim, (arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                               arr(cfg, m, C.c_uint32), None))
        for i, (d, r, ra, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        return 0

    def peek(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        from refund_cases import py_peek
        for i in range(m):
            t = int(arr(ts, m, C.c_int64)[i])
            d, r, ra, rs, _ = py_peek(self.sim, int(arr(key, m, C.c_uint64)[i]), t, int(arr(cfg, m, C.c_uint32)[i]),
                                      t // 1_000_000)
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        return 0

    def refund(self, user, m, key, ts, n, cfg, status):
        st, _ = apply_refunds(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                              arr(cfg, m, C.c_uint32))
        arr(status, m, C.c_uint8)[:] = st
        return 0

    def coalescer(self):
        return rl_amd.Coalescer(self.batch, max_batch=256, peek=self.peek, refund=self.refund)


def scenario(ch, co):
    a = rl_grpc.api("ratelimiter.proto")
    st, rf, status = rl_grpc.rate_limiter_stub(ch), rl_grpc.refund_stub(ch), rl_grpc.status_stub(ch)
    allow = lambda lim, key: st.Allow(a.AllowRequest(limiter=lim, key=key))
    # --- a sliding window of 3 per 2 s, across its rollover (every RPC below reads the clock once) ---
    for _ in range(14):
        allow("fw", "filler")                                    # reads 1 .. 14: 1.4 s of the window have passed
    assert [allow("sw", "u").remaining for _ in range(3)] == [2, 1, 0]          # 1.5, 1.6, 1.7 s
    denied = allow("sw", "u")                                    # 1.8 s: denied, and counted: the window holds 4
    assert not denied.allowed and denied.reset_at_unix_ns == S0 + 2 * NS
    assert rl_grpc.refund(rf, "sw", "u", 1) is True              # 1.9 s: the window current now -> 3
    # 2.0 s: the next window has begun; the denied response's reset time names the window it charged -> 2
    assert rl_grpc.refund(rf, "sw", "u", 1, denied.reset_at_unix_ns) is True
    # 2.1 s: the previous window's 2 weigh 2 * (1 - 0.1 / 2) = 1.9 (unrefunded: 4 -> 3.8, nothing left)
    assert rl_grpc.peek(status, "sw", "u").remaining == 2
    # 2.2 s: the current window holds nothing to give back to
    assert rl_grpc.refund(rf, "sw", "u", 1) is False
    # --- a fixed window and a bucket ---
    assert [allow("fw", "u1").remaining for _ in range(5)] == [4, 3, 2, 1, 0]
    over = allow("fw", "u1")
    assert not over.allowed                                      # counted: 6
    assert rl_grpc.refund(rf, "fw", "u1", 2, over.reset_at_unix_ns) is True     # -> 4
    assert allow("fw", "u1").allowed                             # -> 5
    assert st.AllowN(a.AllowNRequest(limiter="tb", key="k", n=5)).allowed
    assert not allow("tb", "k").allowed
    before = co.stats()
    res = rl_grpc.refund_batch(rf, [("fw", "u1", 1, over.reset_at_unix_ns), ("nope", "x", 1), ("fw", "u1", 2),
                                    ("fw", "u1", 0), ("tb", "k", 2, 999), ("fw", "ghost", 1)])
    # an unknown limiter and n <= 0 are that entry's error, not an RPC failure; a bucket ignores the window
    assert res == [(True, ""), (False, "unknown limiter 'nope'"), (True, ""), (False, ERR_INVALID_N), (True, ""),
                   (False, "")]
    after = co.stats()
    assert (after.refunds - before.refunds, after.refund_launches - before.refund_launches) == (3, 1)
    assert rl_grpc.peek(status, "fw", "u1").remaining == 3       # 5 - 1 - 2
    assert st.AllowN(a.AllowNRequest(limiter="tb", key="k", n=2)).allowed
    assert not allow("tb", "k").allowed
    # nothing to do, and nothing but errors: no submission
    assert rl_grpc.refund_batch(rf, []) == []
    assert rl_grpc.refund_batch(rf, [("a", "x", 1), ("fw", "y", -3)]) == [(False, "unknown limiter 'a'"),
                                                                         (False, ERR_INVALID_N)]
    assert co.stats().refund_launches == after.refund_launches
    # n = 0 and an unknown limiter on the unary call
    for n in (0, -1):
        with pytest.raises(grpc.RpcError) as e:
            rl_grpc.refund(rf, "fw", "u1", n)
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and e.value.details() == ERR_INVALID_N
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.refund(rf, "nope", "u1", 1)
    assert e.value.code() == grpc.StatusCode.NOT_FOUND and e.value.details() == "unknown limiter 'nope'"


def test_proto_has_the_refund_service_and_leaves_the_others_alone():
    a = rl_grpc.api()
    assert a.services["RateLimiterRefund"] == [("Refund", "RefundRequest", "RefundResponse"),
                                               ("RefundBatch", "RefundBatchRequest", "RefundBatchResponse")]
    assert [m for m, _, _ in a.services["RateLimiter"]] == ["Allow", "AllowN", "Reset", "AllowBatch"]
    assert [m for m, _, _ in a.services["RateLimiterStatus"]] == ["Peek"]
    assert [m for m, _, _ in a.services["RateLimiterAdmin"]] == ["ResetBatch"]
    assert [m for m, _, _ in a.services["RateLimiterMetrics"]] == ["Usage"]
    assert [m for m, _, _ in a.services["RateLimiterTopKeys"]] == ["TopKeys"]
    assert [(f.name, f.number) for f in a.RefundRequest.DESCRIPTOR.fields] == [
        ("limiter", 1), ("key", 2), ("n", 3), ("window_reset_at_unix_ns", 4)]
    assert [(f.name, f.number) for f in a.RefundResponse.DESCRIPTOR.fields] == [("applied", 1)]
    assert [(f.name, f.number) for f in a.RefundResult.DESCRIPTOR.fields] == [("applied", 1), ("error", 2)]


class Native:
    """the native server over a coalescer, on the stepping clock"""

    def __init__(self, store=None, backend=None):
        lims = [rl_server.Limiter.parse(s) for s in LIMITERS]
        register = backend.register if backend is not None else store.register
        for lim in lims:
            lim.cfg_id = register(lim.alg, lim.limit, lim.window_ns)
        self.backend = backend
        self.co = backend.start(1 << 12) if backend is not None else store.coalescer()
        self.srv = rl_amd.GrpcServer(
            self.co, [(l.name, l.cfg_id, l.alg, l.limit, l.window_ns, l.prefix, l.fail_open) for l in lims],
            io_threads=2, clock_start_ns=S0, clock_step_ns=STEP)
        self.ch = grpc.insecure_channel(f"127.0.0.1:{self.srv.port}")

    def close(self):
        self.ch.close()
        self.srv.close()
        if self.backend is not None:
            self.backend.close()
        else:
            self.co.close()


def python_server(register, make_co):
    svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in LIMITERS], None, register,
                                       clock=StepClock())
    svc.co = make_co()
    return (svc,) + start(svc)


def test_native_server_cpu():
    srv = Native(PyStore())
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close()


def test_python_server_cpu():
    store = PyStore()
    svc, ch, stop, th = python_server(store.register, store.coalescer)
    try:
        scenario(ch, svc.co)
    finally:
        ch.close()
        stop.set()
        th.join(10)
        svc.co.close()


@pytest.mark.gpu
def test_native_server_gpu():
    srv = Native(backend=rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12))
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close()


@pytest.mark.gpu
def test_python_server_gpu():
    be = rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)
    svc, ch, stop, th = python_server(be.register, lambda: be.start(1 << 12))
    try:
        scenario(ch, svc.co)
    finally:
        ch.close()
        stop.set()
        th.join(10)
        be.close()
