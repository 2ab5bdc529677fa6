"""RateLimiterTopKeys.TopKeys on both gRPC servers: over the coalescer's host
seam with the CPU oracle as the store (CPU), and over the HIP engine (GPU)."""
import grpc
import pytest

import hot_cases as H
import rl_amd
import rl_grpc
import rl_server
from test_grpc import LIMITERS, Clock, OracleStore, start
from test_tally_grpc import STEP, wait_for
from tracegen import T0

WIDTH, HOT_MIN, SLOTS = 1 << 12, 4, 256


def coalescer_opts(tally, hot):
    kw = dict(tally_key_slots=1024 if tally else 0)
    if hot:
        kw.update(hot_min=HOT_MIN, hot_width=WIDTH, hot_key_slots=SLOTS)
    return kw


class PyServer:
    """the Python server over a coalescer with the top keys (and the tally)"""

    def __init__(self, backend=None, hot=True, tally=True, names_cap=4096):
        self.be = backend
        store = None if backend else OracleStore()
        self.svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in LIMITERS], None,
                                                backend.register if backend else store.register, clock=Clock(),
                                                tally=tally, names_cap=names_cap, hot=hot)
        kw = coalescer_opts(tally, hot)
        self.co = backend.start(1 << 12, **kw) if backend else \
            rl_amd.Coalescer(store.batch, max_batch=256, reset=store.reset, **kw)
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
    """the native server: it serves TopKeys when its coalescer keeps the top keys"""

    def __init__(self, backend=None, hot=True, tally=True, names_cap=0, io_threads=2):
        self.be = backend
        self.store = store = None if backend else OracleStore()
        lims = [rl_server.Limiter.parse(s) for s in LIMITERS]
        for lim in lims:
            lim.cfg_id = (backend.register if backend else store.register)(lim.alg, lim.limit, lim.window_ns)
        kw = coalescer_opts(tally, hot)
        self.co = backend.start(1 << 12, **kw) if backend else \
            rl_amd.Coalescer(store.batch, max_batch=256, reset=store.reset, **kw)
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


class Sent:
    """the requests sent through a server, as the model sees them: the key id
    the server hashed, the limiter's config, n, the decision that came back"""

    def __init__(self, srv):
        self.srv, self.a = srv, rl_grpc.api("ratelimiter.proto")
        self.st = rl_grpc.rate_limiter_stub(srv.ch)
        self.mod = H.HotModel(WIDTH, HOT_MIN, len(LIMITERS))
        self.ids = {}

    def note(self, limiter, key, n, allowed):
        lim = self.srv.by_name[limiter]
        kid = self.srv.key_id(lim, key)
        self.ids[kid] = (limiter, key)
        self.mod.call([kid], [lim.cfg_id], [n], [1 if allowed else 0])

    def allow(self, limiter, key, n=1):
        r = self.st.AllowN(self.a.AllowNRequest(limiter=limiter, key=key, n=n)) if n != 1 else \
            self.st.Allow(self.a.AllowRequest(limiter=limiter, key=key))
        self.note(limiter, key, n, r.allowed)
        return r.allowed

    def batch(self, items):
        rs = self.st.AllowBatch(self.a.AllowBatchRequest(
            requests=[self.a.AllowNRequest(limiter=l, key=k, n=n) for l, k, n in items])).results
        for (l, k, n), r in zip(items, rs):
            if not r.error:                       # an unknown limiter or n <= 0 never reaches the engine
                self.note(l, k, n, r.allowed)
        return rs

    def want(self, names):
        """the model's read as (limiter, key_hash, key, estimate) rows, `names`: the key ids the server can name"""
        return [(self.ids[k][0], k, self.ids[k][1] if k in names else "", e) for k, e in self.mod.read()]


def rows(resp):
    return [(k.limiter, k.key_hash, k.key, k.estimate) for k in resp.keys]


def traffic(s):
    """`big`: allowed only, past hot_min; u1: past hot_min, denied twice; k: past hot_min inside one batch; the rest below"""
    assert [s.allow("tb2", "big") for _ in range(5)] == [True] * 5
    assert [s.allow("fw", "u1") for _ in range(7)] == [True] * 5 + [False] * 2
    assert [s.allow("fw", "small") for _ in range(2)] == [True] * 2
    rs = s.batch([("tb", "k", 1)] * 4 + [("nope", "x", 1), ("fw", "u4", 0), ("sw", "once", 1)])
    assert [r.allowed for r in rs] == [True] * 4 + [False, False, True] and rs[4].error and rs[5].error


def scenario(srv):
    s, tx = Sent(srv), rl_grpc.top_keys_stub(srv.ch)
    traffic(s)
    assert H.distinct_columns(sorted(s.ids), WIDTH)            # estimates are true weights, whatever the batches
    kid = lambda l, k: srv.key_id(srv.by_name[l], k)
    big, u1, k = kid("tb2", "big"), kid("fw", "u1"), kid("tb", "k")
    assert [x[0] for x in s.mod.read()] == [u1, big, k] and s.mod.total == 19
    # first scrape: the server has a name for the denied key only
    t = rl_grpc.top_keys(tx, top=10)
    assert rows(t) == s.want({u1})
    assert (t.total, t.keys_tracked, t.dropped, t.width, t.hot_min, t.weight) == (19, 3, 0, WIDTH, HOT_MIN, 0)
    assert t.keys[0].key_hash == int(rl_amd.hash_keys_host([b"u1"], 0, srv.by_name["fw"].prefix)[0])
    # its keys are watched now: one more request of each names it; `small` is not among them
    assert s.allow("tb2", "big") and s.allow("fw", "small")
    assert s.batch([("tb", "k", 1)])[0].allowed
    t = rl_grpc.top_keys(tx, top=10)
    assert rows(t) == s.want({u1, big, k}) and [x.key for x in t.keys] == ["u1", "big", "k"]
    assert [x.estimate for x in t.keys] == [7, 6, 5] and t.total == 22
    # top bounds the list (and the watch set: `k` stays named, it is in the map); reading changes nothing
    assert rows(rl_grpc.top_keys(tx, top=1)) == s.want({u1})[:1]
    assert len(rl_grpc.top_keys(tx).keys) == 0 and rl_grpc.top_keys(tx).keys_tracked == 3
    assert rl_grpc.top_keys(tx, top=10, clear=True) == t
    z = rl_grpc.top_keys(tx, top=10)
    assert len(z.keys) == 0 and (z.total, z.keys_tracked, z.dropped, z.width, z.hot_min) == (0, 0, 0, WIDTH, HOT_MIN)
    s.mod.clear()
    assert [s.allow("tb2", "big") for _ in range(4)] == [True] * 4
    assert rows(rl_grpc.top_keys(tx, top=10)) == s.want({big}) == [("tb2", big, "big", 4)]


def usage_scenario(make):
    """the same traffic with the top keys on and off: Usage answers the same"""
    got = []
    for hot in (True, False):
        srv = make(hot=hot)
        try:
            s = Sent(srv)
            traffic(s)
            if hot:
                rl_grpc.top_keys(rl_grpc.top_keys_stub(srv.ch), top=10)
            assert s.allow("tb2", "big") and not s.allow("fw", "u1")
            got.append(rl_grpc.usage(rl_grpc.metrics_stub(srv.ch), top=10))
        finally:
            srv.close()
    assert got[0] == got[1]
    by = {x.limiter: x for x in got[0].limiters}
    assert (by["fw"].allowed, by["fw"].denied, by["tb2"].allowed, by["tb"].allowed) == (7, 3, 6, 4)
    assert [(k.key, k.denied) for k in got[0].keys] == [("u1", 3)]


def without_tally_scenario(srv):
    """the tally off: a denied key is not remembered for its denial; it is named through the watch set like any other"""
    s, tx = Sent(srv), rl_grpc.top_keys_stub(srv.ch)
    assert [s.allow("fw", "u1") for _ in range(7)] == [True] * 5 + [False] * 2
    assert rows(rl_grpc.top_keys(tx, top=4)) == s.want(set())
    assert not s.allow("fw", "u1")
    assert rows(rl_grpc.top_keys(tx, top=4)) == s.want(set(s.ids)) and s.mod.read()[0][1] == 8
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.usage(rl_grpc.metrics_stub(srv.ch), top=3)
    assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION


def off_scenario(srv):
    a = rl_grpc.api("ratelimiter.proto")
    assert rl_grpc.rate_limiter_stub(srv.ch).Allow(a.AllowRequest(limiter="fw", key="u")).allowed
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.top_keys(rl_grpc.top_keys_stub(srv.ch), top=3)
    assert e.value.code() == grpc.StatusCode.FAILED_PRECONDITION
    assert rl_grpc.rate_limiter_stub(srv.ch).Allow(a.AllowRequest(limiter="fw", key="u")).allowed
    assert len(rl_grpc.usage(rl_grpc.metrics_stub(srv.ch), top=3).limiters) == len(LIMITERS)


def run(make, fn):
    srv = make()
    try:
        fn(srv)
    finally:
        srv.close()


def test_proto_has_the_top_keys_service():
    a = rl_grpc.api()
    assert a.services["RateLimiterTopKeys"] == [("TopKeys", "TopKeysRequest", "TopKeysResponse")]
    fields = lambda m: [(f.name, f.number) for f in m.DESCRIPTOR.fields]
    assert fields(a.TopKeysRequest) == [("top", 1), ("clear", 2)]
    assert fields(a.HotKey) == [("limiter", 1), ("key_hash", 2), ("key", 3), ("estimate", 4)]
    assert fields(a.TopKeysResponse) == [("keys", 1), ("total", 2), ("keys_tracked", 3), ("dropped", 4), ("width", 5),
                                         ("hot_min", 6), ("weight", 7)]
    assert a.HotKey.DESCRIPTOR.fields_by_name["key_hash"].type == 6      # fixed64


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_top_keys_cpu(server):
    run(server, scenario)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_usage_is_unchanged_cpu(server):
    usage_scenario(server)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_without_the_tally_cpu(server):
    run(lambda: server(tally=False), without_tally_scenario)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_off_is_failed_precondition_cpu(server):
    run(lambda: server(hot=False), off_scenario)


@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_watch_set_is_bounded_by_names_cap_cpu(server):
    """names_cap 1: the watch set is the first key of the latest response"""
    def fn(srv):
        s, tx = Sent(srv), rl_grpc.top_keys_stub(srv.ch)
        assert [s.allow("tb2", "a") for _ in range(6)] == [True] * 6
        assert [s.allow("tb2", "b") for _ in range(5)] == [True] * 5
        assert [x.key for x in rl_grpc.top_keys(tx, top=4).keys] == ["", ""]
        assert s.allow("tb2", "b") and s.allow("tb2", "a")
        assert [x.key for x in rl_grpc.top_keys(tx, top=4).keys] == ["a", ""]
    run(lambda: server(names_cap=1), fn)


def test_native_top_keys_read_outlives_its_connection():
    """a scraper that goes away while its TopKeys read is queued behind a batch
    the store holds (test_tally_grpc, `reset`): the read completes with no
    connection to answer, the server goes on serving and shuts down cleanly"""
    srv = NativeServer(io_threads=1)
    try:
        a = rl_grpc.api("ratelimiter.proto")
        st, tx = rl_grpc.rate_limiter_stub(srv.ch), rl_grpc.top_keys_stub(srv.ch)
        health, Hp = rl_grpc.health_stub(srv.ch), rl_grpc.api("health.proto")
        assert [st.Allow(a.AllowRequest(limiter="tb2", key="u")).allowed for _ in range(4)] == [True] * 4
        srv.store.entered.clear()
        srv.store.gate.clear()
        held = st.Allow.future(a.AllowRequest(limiter="tb2", key="u"))
        assert srv.store.entered.wait(30)
        ch2 = grpc.insecure_channel(f"127.0.0.1:{srv.srv.port}")
        fut = rl_grpc.top_keys_stub(ch2).TopKeys.future(a.TopKeysRequest(top=4, clear=True))
        wait_for(lambda: srv.co.stats().pending >= 1, "the TopKeys read to be queued")
        ch2.close()
        wait_for(lambda: srv.srv.stats().cancelled >= 1, "the server to see the stream reset")
        assert fut.cancelled() or fut.done()
        for _ in range(3):
            assert health.Check(Hp.HealthCheckRequest(service="")).status == 1
        srv.store.gate.set()
        assert held.result(30).allowed
        # the detached read ran, clear included, behind the held request: nothing left
        t = rl_grpc.top_keys(tx, top=4)
        assert (t.total, len(t.keys)) == (0, 0)
        assert st.Allow(a.AllowRequest(limiter="tb2", key="u")).allowed
        assert srv.co.stats().pending == 0
    finally:
        srv.store.gate.set()
        srv.close()


def gpu_backend():
    return rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)


@pytest.mark.gpu
@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_top_keys_gpu(server):
    run(lambda: server(backend=gpu_backend()), scenario)


@pytest.mark.gpu
@pytest.mark.parametrize("server", [PyServer, NativeServer])
def test_off_is_failed_precondition_gpu(server):
    run(lambda: server(backend=gpu_backend(), hot=False), off_scenario)
