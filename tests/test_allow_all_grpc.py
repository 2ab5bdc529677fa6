"""RateLimiterMulti (AllowAll, AllowAllBatch) on both gRPC servers: over the
coalescer's host seam with the composition on the Python oracle as the store
(CPU), and over the HIP engine (GPU).  Every answer is compared with the same
composition run beside the server (allow_all_cases.apply_allow_all), so the two
servers answer identically."""
import ctypes as C

import grpc
import pytest

import rl_amd
import rl_grpc
import rl_server
from allow_all_cases import apply_allow_all
from oracle import rl_oracle_py as po
from refund_cases import new_sim, py_peek
from test_grpc import LIMITERS
from test_refund_grpc import S0, STEP, Native, PyStore, arr, python_server

ERR_INVALID_N = "invalid n: must be greater than 0"
NAMES = [s.split(":")[0] for s in LIMITERS]


class AllStore(PyStore):
    """test_refund_grpc.PyStore plus the AllowAll function"""

    def allow_all(self, user, m, key, ts, n, cfg, first, dec, rem, retry, reset, verdict):
        rows, v, _, _, _ = apply_allow_all(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64),
                                           arr(n, m, C.c_int64), arr(cfg, m, C.c_uint32), arr(first, m, C.c_uint8))
        for i, (d, r, ra, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(rem, m, C.c_int64)[i] = d, r
            arr(retry, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = ra, rs
        arr(verdict, m, C.c_uint8)[:] = v
        return 0

    def coalescer(self):
        return rl_amd.Coalescer(self.batch, max_batch=256, peek=self.peek, refund=self.refund,
                                allow_all=self.allow_all)


class Ref:
    """the oracle beside the server: the same limiters, a key id of its own per
    formatted key, and the server's clock -- every RPC reads it once"""

    def __init__(self):
        self.lims = [rl_server.Limiter.parse(s) for s in LIMITERS]
        self.sim = new_sim(0, [(l.alg, l.limit, l.window_ns) for l in self.lims])
        self.ids, self.k = {}, 0

    def tick(self):
        self.k += 1
        return S0 + self.k * STEP

    def kid(self, lim, key):
        # the servers hash the formatted key: limiters of one prefix share a key's id
        return self.ids.setdefault((self.lims[NAMES.index(lim)].prefix, key), len(self.ids) + 1)

    def groups(self, groups):
        """one call of runnable groups -> per group (allowed, rows, denied_by, rolled_back)"""
        t = self.tick()
        flat = [(g, c) for g, checks in enumerate(groups) for c in checks]
        key = [self.kid(c[0], c[1]) for _, c in flat]
        cfg = [NAMES.index(c[0]) for _, c in flat]
        n = [c[2] for _, c in flat]
        first = [1 if i == 0 or flat[i - 1][0] != g else 0 for i, (g, _) in enumerate(flat)]
        rows, v, gb, _, _ = apply_allow_all(self.sim, key, [t] * len(key), n, cfg, first)
        out, at = [], 0
        for checks in groups:
            rs = rows[at:at + len(checks)]
            ok = [r[0] == po.ALLOWED for r in rs]
            out.append((all(ok), rs, ok.index(False) if not all(ok) else -1,
                        [bool(x > 0) for x in gb[at:at + len(checks)]]))
            at += len(checks)
        return out


def same(resp, want, lims, ref):
    allowed, rows, by, rolled = want
    assert (resp.allowed, resp.denied_by, list(resp.rolled_back)) == (allowed, by, rolled)
    assert len(resp.results) == len(rows)
    for x, (d, rem, retry, reset, _), name in zip(resp.results, rows, lims):
        assert d in (po.ALLOWED, po.DENIED)
        limit = ref.lims[NAMES.index(name)].limit
        assert (x.allowed, x.limit, x.remaining, x.retry_after_ns, x.reset_at_unix_ns, x.error) == \
            (d == po.ALLOWED, limit, rem, retry, reset, "")


def scenario(ch, co):
    a = rl_grpc.api("ratelimiter.proto")
    mu, st, status = rl_grpc.multi_stub(ch), rl_grpc.rate_limiter_stub(ch), rl_grpc.status_stub(ch)
    ref = Ref()
    # --- the unary call: a group that passes, then one the bucket denies ---
    g1 = [("fw", "u", 2), ("tb", "u", 3), ("tb2", "u2", 4)]
    want = ref.groups([g1])[0]
    assert want[0] is True
    same(rl_grpc.allow_all(mu, g1), want, [c[0] for c in g1], ref)
    g2 = [("fw", "u", 2), ("tb", "u", 3)]
    want = ref.groups([g2])[0]
    assert (want[0], want[2], want[3]) == (False, 1, [True, False])      # the window's 2 come back
    same(rl_grpc.allow_all(mu, g2), want, [c[0] for c in g2], ref)
    # --- the batch call: one launch; the requests that cannot run carry their error ---
    before = co.stats()
    run = [[("fw", "u", 1), ("tb", "u", 1)], [("fw", "u", 9), ("tb2", "u2", 1)], [("fw", "v", 1)]]
    reqs = [run[0], run[1], [("nope", "x", 1), ("fw", "u", 1)], [], [("fw", "u", 0)],
            [("fw", "k%d" % i, 1) for i in range(17)], run[2]]
    wants = ref.groups(run)
    assert [w[0] for w in wants] == [True, False, True] and wants[1][3] == [True, True]
    got = rl_grpc.allow_all_batch(mu, reqs)
    assert len(got) == 7
    for j, i in enumerate((0, 1, 6)):
        same(got[i], wants[j], [c[0] for c in run[j]], ref)
    for i, err, count in ((2, "unknown limiter 'nope'", 2), (3, "checks: need 1 to 16, got 0", 1),
                          (4, ERR_INVALID_N, 1), (5, "checks: need 1 to 16, got 17", 17)):
        assert (got[i].allowed, got[i].denied_by, list(got[i].rolled_back)) == (False, -1, [])
        assert [(x.error, x.allowed, x.limit) for x in got[i].results] == [(err, False, 0)] * count
    after = co.stats()
    assert (after.allow_all_launches - before.allow_all_launches, after.allow_all_groups - before.allow_all_groups) == (1, 3)
    assert after.submitted - before.submitted == 5
    # what is left is what the composition left
    for lim, key in (("fw", "u"), ("tb", "u"), ("tb2", "u2"), ("fw", "v")):
        t = ref.tick()
        want_rem = py_peek(ref.sim, ref.kid(lim, key), t, NAMES.index(lim), t // 1_000_000)[1]
        assert rl_grpc.peek(status, lim, key).remaining == want_rem, (lim, key)
    # nothing but errors: no submission
    got = rl_grpc.allow_all_batch(mu, [[("a", "x", 1)], []])
    ref.tick()
    assert [x.results[0].error for x in got] == ["unknown limiter 'a'", "checks: need 1 to 16, got 0"]
    assert rl_grpc.allow_all_batch(mu, []) == []
    ref.tick()
    assert co.stats().allow_all_launches == after.allow_all_launches
    # --- the error mapping of the unary call ---
    for checks, err in (([("nope", "x", 1)], "unknown limiter 'nope'"), ([("fw", "u", 1), ("tb", "u", 0)], ERR_INVALID_N),
                        ([("fw", "u", -2)], ERR_INVALID_N), ([], "checks: need 1 to 16, got 0"),
                        ([("fw", "k", 1)] * 17, "checks: need 1 to 16, got 17")):
        with pytest.raises(grpc.RpcError) as e:
            rl_grpc.allow_all(mu, checks)
        ref.tick()
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and e.value.details() == err
    # a member the store cannot execute (INCRBY overflow) on a fail-closed limiter: the RPC's error in the
    # unary call, that result's error in the batch call; the bucket's take comes back either way
    big = 1 << 62                                   # twice: past int64
    assert not st.AllowN(a.AllowNRequest(limiter="fw", key="big", n=big)).allowed
    ref.sim.decide(ref.kid("fw", "big"), ref.tick(), big, NAMES.index("fw"))
    over = [("tb2", "z", 2), ("fw", "big", big)]
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.allow_all(mu, over)
    text = "failed to check rate limit: script error (INCRBY overflow)"
    assert e.value.code() == grpc.StatusCode.UNAVAILABLE and e.value.details() == text
    got = rl_grpc.allow_all_batch(mu, [over])[0]
    assert (got.allowed, got.denied_by, list(got.rolled_back)) == (False, 1, [True, False])
    assert got.results[0].allowed and got.results[0].remaining == 8 and got.results[1].error == text
    assert rl_grpc.peek(status, "tb2", "z").remaining == 10


def test_proto_has_the_multi_service_and_leaves_the_others_alone():
    a = rl_grpc.api()
    assert a.services["RateLimiterMulti"] == [("AllowAll", "AllowAllRequest", "AllowAllResponse"),
                                              ("AllowAllBatch", "AllowAllBatchRequest", "AllowAllBatchResponse")]
    assert [m for m, _, _ in a.services["RateLimiter"]] == ["Allow", "AllowN", "Reset", "AllowBatch"]
    assert [m for m, _, _ in a.services["RateLimiterStatus"]] == ["Peek"]
    assert [m for m, _, _ in a.services["RateLimiterAdmin"]] == ["ResetBatch"]
    assert [m for m, _, _ in a.services["RateLimiterMetrics"]] == ["Usage"]
    assert [m for m, _, _ in a.services["RateLimiterTopKeys"]] == ["TopKeys"]
    assert [m for m, _, _ in a.services["RateLimiterRefund"]] == ["Refund", "RefundBatch"]
    assert [(f.name, f.number) for f in a.AllowNRequest.DESCRIPTOR.fields] == [("limiter", 1), ("key", 2), ("n", 3)]
    assert [(f.name, f.number) for f in a.AllowResponse.DESCRIPTOR.fields] == [
        ("allowed", 1), ("limit", 2), ("remaining", 3), ("retry_after_ns", 4), ("reset_at_unix_ns", 5), ("error", 6)]
    assert [(f.name, f.number) for f in a.AllowAllRequest.DESCRIPTOR.fields] == [("checks", 1)]
    assert [(f.name, f.number) for f in a.AllowAllResponse.DESCRIPTOR.fields] == [
        ("allowed", 1), ("results", 2), ("denied_by", 3), ("rolled_back", 4)]
    assert [(f.name, f.number) for f in a.AllowAllBatchRequest.DESCRIPTOR.fields] == [("requests", 1)]
    assert [(f.name, f.number) for f in a.AllowAllBatchResponse.DESCRIPTOR.fields] == [("responses", 1)]


def test_native_server_cpu():
    srv = Native(AllStore())
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close()


def test_python_server_cpu():
    store = AllStore()
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
