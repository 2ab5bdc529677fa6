"""RateLimiterMetrics.Usage on both gRPC servers: over the coalescer's host
seam with the CPU oracle as the store (CPU), and over the HIP engine (GPU)."""
import time

import grpc
import pytest

import rl_amd
import rl_grpc
import rl_server
from test_grpc import LIMITERS, Clock, OracleStore, start
from tracegen import T0

STEP = 1_250_000
NAMES = [s.split(":")[0] for s in LIMITERS]


class PyServer:
    """the Python server over a coalescer with the tally (or without)"""

    def __init__(self, backend=None, tally=True, names_cap=4096):
        self.be = backend
        store = None if backend else OracleStore()
        self.svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in LIMITERS], None,
                                                backend.register if backend else store.register, clock=Clock(),
                                                tally=tally, names_cap=names_cap)
        slots = 1024 if tally else 0
        self.co = backend.start(1 << 12, tally_key_slots=slots) if backend else \
            rl_amd.Coalescer(store.batch, max_batch=256, reset=store.reset, tally_key_slots=slots)
        self.svc.co = self.co
        self.ch, self.stop, self.th = start(self.svc)
        self.by_name = self.svc.by_name
        self.key_id = self.svc._key_id

    def close(self):
        self.ch.close()
        self.stop.set()
        self.th.join(10)
        if self.be:
            self.be.close()
        else:
            self.co.close()


class NativeServer:
    """the native server over a coalescer with the tally (or without)"""

    def __init__(self, backend=None, tally=True, names_cap=0, io_threads=2):
        self.be = backend
        self.store = store = None if backend else OracleStore()
        lims = [rl_server.Limiter.parse(s) for s in LIMITERS]
        for lim in lims:
            lim.cfg_id = (backend.register if backend else store.register)(lim.alg, lim.limit, lim.window_ns)
        slots = 1024 if tally else 0
        self.co = backend.start(1 << 12, tally_key_slots=slots) if backend else \
            rl_amd.Coalescer(store.batch, max_batch=256, reset=store.reset, tally_key_slots=slots)
        self.srv = rl_amd.GrpcServer(
            self.co, [(l.name, l.cfg_id, l.alg, l.limit, l.window_ns, l.prefix, l.fail_open) for l in lims],
            io_threads=io_threads, clock_start_ns=T0, clock_step_ns=STEP, tally=tally, names_cap=names_cap)
        self.ch = grpc.insecure_channel(f"127.0.0.1:{self.srv.port}")
        self.by_name = {l.name: l for l in lims}

    def key_id(self, lim, key):
        return int(rl_amd.hash_keys_host([key.encode()], 0, lim.prefix)[0])

    def close(self):
        self.ch.close()
        self.srv.close()
        if self.be:
            self.be.close()
        else:
            self.co.close()


def scenario(srv):
    a = rl_grpc.api("ratelimiter.proto")
    st, mx = rl_grpc.rate_limiter_stub(srv.ch), rl_grpc.metrics_stub(srv.ch)
    allow = lambda lim, key: st.Allow(a.AllowRequest(limiter=lim, key=key)).allowed
    assert [allow("fw", "u1") for _ in range(7)] == [True] * 5 + [False] * 2
    assert [allow("fw", "u2") for _ in range(6)] == [True] * 5 + [False]
    assert st.AllowN(a.AllowNRequest(limiter="tb", key="k", n=5)).allowed
    assert not allow("tb", "k")
    rs = st.AllowBatch(a.AllowBatchRequest(requests=[
        a.AllowNRequest(limiter="fw", key="u3", n=6), a.AllowNRequest(limiter="fw", key="u5", n=1),
        a.AllowNRequest(limiter="nope", key="x", n=1), a.AllowNRequest(limiter="fw", key="u4", n=0)])).results
    assert [r.allowed for r in rs] == [False, True, False, False] and rs[2].error and rs[3].error
    # a denied request that no response of this server went out for: its key has no name here
    fw = srv.by_name["fw"]
    ghost = srv.key_id(fw, "ghost")
    rc, out = srv.co.decide(ghost, T0 + 10 * STEP, 9, fw.cfg_id)
    assert rc == 0 and out[0] == rl_amd.DENIED
    u = rl_grpc.usage(mx, top=10)
    assert [x.limiter for x in u.limiters] == NAMES
    by = {x.limiter: x for x in u.limiters}
    row = lambda x: (x.allowed, x.denied, x.errors, x.invalid, x.units_allowed, x.units_denied)
    assert row(by["fw"]) == (11, 5, 0, 0, 11, 2 + 1 + 6 + 9)
    assert row(by["tb"]) == (1, 1, 0, 0, 5, 1)
    for name in ("sw", "tb2", "fwc"):
        assert row(by[name]) == (0, 0, 0, 0, 0, 0)
    assert (u.keys_tracked, u.untracked_requests) == (5, 0)
    tb = srv.by_name["tb"]
    want = {srv.key_id(fw, "u1"): ("fw", "u1", 2, 2), srv.key_id(fw, "u2"): ("fw", "u2", 1, 1),
            srv.key_id(fw, "u3"): ("fw", "u3", 1, 6), srv.key_id(tb, "k"): ("tb", "k", 1, 1),
            ghost: ("fw", "", 1, 9)}
    assert {k.key_hash: (k.limiter, k.key, k.denied, k.units_denied) for k in u.keys} == want
    assert u.keys[0].key == "u1"                               # most denied first ...
    assert [k.key_hash for k in u.keys[1:]] == sorted(k.key_hash for k in u.keys[1:])   # ... then by key id
    # a suspect key can be checked by its hash
    assert u.keys[0].key_hash == int(rl_amd.hash_keys_host([b"u1"], 0, fw.prefix)[0])
    # top bounds the list; reading twice changes nothing; a clear zeroes everything
    assert [k.key for k in rl_grpc.usage(mx, top=1).keys] == ["u1"]
    assert len(rl_grpc.usage(mx).keys) == 0
    assert rl_grpc.usage(mx, top=10, clear=True) == u
    z = rl_grpc.usage(mx, top=10)
    assert [x.limiter for x in z.limiters] == NAMES and all(row(x) == (0,) * 6 for x in z.limiters)
    assert len(z.keys) == 0 and (z.keys_tracked, z.untracked_requests) == (0, 0)
    assert not allow("fw", "u1")
    z = rl_grpc.usage(mx, top=10)
    assert row({x.limiter: x for x in z.limiters}["fw"]) == (0, 1, 0, 0, 0, 1)
    assert [(k.limiter, k.key, k.denied) for k in z.keys] == [("fw", "u1", 1)]


def names_scenario(srv):
    """a name map of two entries: the newest two denied keys keep their names"""
    a = rl_grpc.api("ratelimiter.proto")
    st, mx = rl_grpc.rate_limiter_stub(srv.ch), rl_grpc.metrics_stub(srv.ch)
    for key in ("a", "b", "a", "c"):            # `a` again makes it newer than `b`
        assert not st.AllowN(a.AllowNRequest(limiter="fw", key=key, n=6)).allowed
    u = rl_grpc.usage(mx, top=10)
    assert {k.key for k in u.keys} == {"a", "", "c"} and len(u.keys) == 3
    fw = srv.by_name["fw"]
    assert {k.key_hash: k.key for k in u.keys}[srv.key_id(fw, "b")] == ""


def off_scenario(srv):
    a = rl_grpc.api("ratelimiter.proto")
    assert rl_grpc.rate_limiter_stub(srv.ch).Allow(a.AllowRequest(limiter="fw", key="u")).allowed
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.usage(rl_grpc.metrics_stub(srv.ch), top=3)
    assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
    assert rl_grpc.rate_limiter_stub(srv.ch).Allow(a.AllowRequest(limiter="fw", key="u")).allowed


def run(make, fn):
    srv = make()
    try:
        fn(srv)
    finally:
        srv.close()


def test_proto_has_the_metrics_service_and_leaves_the_others_alone():
    a = rl_grpc.api()
    assert a.services["RateLimiterMetrics"] == [("Usage", "UsageRequest", "UsageResponse")]
    assert [m for m, _, _ in a.services["RateLimiter"]] == ["Allow", "AllowN", "Reset", "AllowBatch"]
    assert [m for m, _, _ in a.services["RateLimiterStatus"]] == ["Peek"]
    assert [m for m, _, _ in a.services["RateLimiterAdmin"]] == ["ResetBatch"]
    fields = lambda m: [(f.name, f.number) for f in m.DESCRIPTOR.fields]
    assert fields(a.UsageRequest) == [("top", 1), ("clear", 2)]
    assert fields(a.LimiterUsage) == [("limiter", 1), ("allowed", 2), ("denied", 3), ("errors", 4), ("invalid", 5),
                                      ("units_allowed", 6), ("units_denied", 7)]
    assert fields(a.ThrottledKey) == [("limiter", 1), ("key_hash", 2), ("key", 3), ("denied", 4), ("units_denied", 5)]
    assert fields(a.UsageResponse) == [("limiters", 1), ("keys", 2), ("untracked_requests", 3), ("keys_tracked", 4)]
    assert a.ThrottledKey.DESCRIPTOR.fields_by_name["key_hash"].type == 6      # fixed64


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_usage_cpu(server):
    run(server, scenario)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_names_are_bounded_cpu(server):
    run(lambda: server(names_cap=2), names_scenario)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_off_is_failed_precondition_cpu(server):
    run(lambda: server(tally=False), off_scenario)


def test_native_opts_of_the_old_size_serve_without_usage():
    """a caller compiled before `tally` passes the shorter rl_grpc_opts"""
    import ctypes as C
    store = OracleStore()
    co = rl_amd.Coalescer(store.batch, max_batch=64, tally_key_slots=64)
    o = rl_amd.rl_grpc_opts(io_threads=1, host=b"127.0.0.1", tally=1)
    o.struct_size = rl_amd.rl_grpc_opts.tally.offset
    h = C.c_void_p()
    L = rl_amd.grpc_lib()
    assert L.rl_grpc_server_start(co.h, None, 0, C.cast(C.pointer(o), C.c_void_p), C.byref(h)) == 0
    ch = grpc.insecure_channel(f"127.0.0.1:{L.rl_grpc_server_port(h)}")
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.usage(rl_grpc.metrics_stub(ch))
    assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION      # the field past the caller's struct is not read
    ch.close()
    assert L.rl_grpc_server_destroy(h) == 0
    o.struct_size = 12
    assert L.rl_grpc_server_start(co.h, None, 0, C.cast(C.pointer(o), C.c_void_p), C.byref(h)) == rl_amd.RL_EINVAL
    co.close()


def wait_for(cond, what, seconds=30.0):
    end = time.monotonic() + seconds
    while not cond():
        assert time.monotonic() < end, f"timed out waiting for {what}"


def raw_usage_call(port):
    """a Usage RPC written by hand on a plain socket (HTTP/2 preface, SETTINGS,
    HEADERS with literal header fields, one empty gRPC message): a client
    whose socket can be dropped with the stream still open, which grpcio's
    channel never does (it resets the stream first)"""
    import socket
    import struct
    frame = lambda typ, flags, sid, body: struct.pack(">I", len(body))[1:] + bytes([typ, flags]) + \
        struct.pack(">I", sid) + body
    lit = lambda k, v: b"\x00" + bytes([len(k)]) + k + bytes([len(v)]) + v     # literal, not indexed, no Huffman
    headers = b"".join(lit(k, v) for k, v in [
        (b":method", b"POST"), (b":scheme", b"http"), (b":path", b"/ratelimiter.v1.RateLimiterMetrics/Usage"),
        (b":authority", b"localhost"), (b"content-type", b"application/grpc"), (b"te", b"trailers")])
    sk = socket.create_connection(("127.0.0.1", port))
    sk.sendall(b"PRI * HTTP/2.0\r\n\r\nSM\r\n\r\n" + frame(4, 0, 0, b"") + frame(1, 4, 1, headers) +
               frame(0, 1, 1, b"\x00\x00\x00\x00\x00"))
    return sk


@pytest.mark.parametrize("how", ["reset", "drop"])
def test_native_usage_read_outlives_its_connection(how):
    """a scraper that goes away while its Usage read is queued: the store holds
    a batch (the coalescer's submitter sits in it, the read queued behind), the
    scraper goes -- `reset`: a grpcio channel closed, which resets the stream
    and then closes the socket; `drop`: a socket closed with the stream open --
    then the store lets go.  The read completes with no connection to answer;
    the server goes on serving and shuts down cleanly.  One event loop, so the
    health checks below pass through the loop after the close did."""
    srv = NativeServer(io_threads=1)
    try:
        a = rl_grpc.api("ratelimiter.proto")
        st, mx = rl_grpc.rate_limiter_stub(srv.ch), rl_grpc.metrics_stub(srv.ch)
        health = rl_grpc.health_stub(srv.ch)
        assert st.Allow(a.AllowRequest(limiter="fw", key="u")).allowed
        srv.store.entered.clear()
        srv.store.gate.clear()
        held = st.Allow.future(a.AllowRequest(limiter="fw", key="u"))
        assert srv.store.entered.wait(30)
        if how == "reset":
            ch2 = grpc.insecure_channel(f"127.0.0.1:{srv.srv.port}")
            fut = rl_grpc.metrics_stub(ch2).Usage.future(a.UsageRequest(top=4))
            wait_for(lambda: srv.co.stats().pending >= 1, "the Usage read to be queued")
            ch2.close()
            wait_for(lambda: srv.srv.stats().cancelled >= 1, "the server to see the stream reset")
            assert fut.cancelled() or fut.done()
        else:
            sk = raw_usage_call(srv.srv.port)
            wait_for(lambda: srv.co.stats().pending >= 1, "the Usage read to be queued")
            sk.close()
        H = rl_grpc.api("health.proto")
        for _ in range(3):
            assert health.Check(H.HealthCheckRequest(service="")).status == 1
        srv.store.gate.set()
        assert held.result(30).allowed
        u = rl_grpc.usage(mx, top=4)
        assert {x.limiter: x.allowed for x in u.limiters}["fw"] == 2
        assert st.Allow(a.AllowRequest(limiter="fw", key="u")).allowed
        assert srv.co.stats().pending == 0
    finally:
        srv.store.gate.set()
        srv.close()


def gpu_backend():
    return rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)


@pytest.mark.gpu
@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_usage_gpu(server):
    run(lambda: server(backend=gpu_backend()), scenario)


@pytest.mark.gpu
@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_off_is_failed_precondition_gpu(server):
    run(lambda: server(backend=gpu_backend(), tally=False), off_scenario)
