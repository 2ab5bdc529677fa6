"""RateLimiterAdmin.ResetBatch on both gRPC servers: over the coalescer's host
seam with the CPU oracle as the store (CPU), and over the HIP engine (GPU)."""
import grpc
import pytest

import rl_amd
import rl_grpc
import rl_server
from test_grpc import LIMITERS, Clock, OracleStore, start
from test_grpc_native import Native


def scenario(ch, co=None):
    a = rl_grpc.api("ratelimiter.proto")
    st, admin = rl_grpc.rate_limiter_stub(ch), rl_grpc.admin_stub(ch)
    allow = lambda lim, key: st.Allow(a.AllowRequest(limiter=lim, key=key))
    users = ["u1", "u2", "u3", "u4"]
    for u in users:
        assert [allow("fw", u).remaining for _ in range(5)] == [4, 3, 2, 1, 0]
        assert not allow("fw", u).allowed
    assert st.AllowN(a.AllowNRequest(limiter="tb", key="k", n=5)).allowed
    assert not allow("tb", "k").allowed
    before = co.stats() if co is not None else None
    errs = rl_grpc.reset_batch(admin, [("fw", "u1"), ("nope", "x"), ("fw", "u3"), ("tb", "k"), ("fw", "u1"),
                                       ("fw", "never-seen")])
    # an unknown limiter is that entry's error, not an RPC failure
    assert errs == ["", "unknown limiter 'nope'", "", "", "", ""]
    if co is not None:      # one coalescer submission
        after = co.stats()
        assert after.resets - before.resets == 5 and after.reset_launches - before.reset_launches == 1
    # a fresh quota for the keys named, and only for them
    assert allow("fw", "u1").remaining == 4 and allow("fw", "u3").remaining == 4
    assert not allow("fw", "u2").allowed and not allow("fw", "u4").allowed
    assert st.AllowN(a.AllowNRequest(limiter="tb", key="k", n=5)).allowed
    # nothing to do, and nothing but unknown limiters
    assert rl_grpc.reset_batch(admin, []) == []
    assert rl_grpc.reset_batch(admin, [("a", "x"), ("b", "y")]) == ["unknown limiter 'a'", "unknown limiter 'b'"]
    # the single Reset is still served
    st.Reset(a.ResetRequest(limiter="fw", key="u2"))
    assert allow("fw", "u2").remaining == 4
    with pytest.raises(grpc.RpcError) as e:
        st.Reset(a.ResetRequest(limiter="nope", key="u2"))
    assert e.value.code() == grpc.StatusCode.NOT_FOUND


def test_proto_has_the_admin_service_and_leaves_the_others_alone():
    a = rl_grpc.api()
    assert a.services["RateLimiterAdmin"] == [("ResetBatch", "ResetBatchRequest", "ResetBatchResponse")]
    assert [m for m, _, _ in a.services["RateLimiter"]] == ["Allow", "AllowN", "Reset", "AllowBatch"]
    assert [m for m, _, _ in a.services["RateLimiterStatus"]] == ["Peek"]
    assert [(f.name, f.number) for f in a.ResetBatchResponse.DESCRIPTOR.fields] == [("errors", 1)]
    assert [(f.name, f.number) for f in a.ResetBatchRequest.DESCRIPTOR.fields] == [("requests", 1)]
    assert list(a.ResetBatchResponse(errors=["", "x"]).errors) == ["", "x"]      # repeated


def test_native_server_cpu():
    srv = Native(LIMITERS, OracleStore())
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close()


def test_python_server_cpu():
    store = OracleStore()
    svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in LIMITERS], None, store.register,
                                       clock=Clock())
    svc.co = rl_amd.Coalescer(store.batch, max_batch=256, reset=store.reset)
    ch, stop, th = start(svc)
    try:
        scenario(ch, svc.co)
    finally:
        ch.close()
        stop.set()
        th.join(10)
        svc.co.close()


@pytest.mark.gpu
def test_native_server_gpu():
    be = rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)
    srv = Native(LIMITERS, backend=be, max_batch=1 << 12)
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close(be)


@pytest.mark.gpu
def test_python_server_gpu():
    be = rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)
    svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in LIMITERS], None, be.register,
                                       clock=Clock())
    svc.co = be.start(1 << 12)
    ch, stop, th = start(svc)
    try:
        scenario(ch, svc.co)
    finally:
        ch.close()
        stop.set()
        th.join(10)
        be.close()
