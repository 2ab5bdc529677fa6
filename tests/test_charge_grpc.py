"""RateLimiterCharge (Charge, ChargeBatch) on both gRPC servers: over the
coalescer's host seam with the composition on the Python oracle as the store
(CPU), and over the HIP engine (GPU).  Every answer is compared with the same
composition run beside the server (charge_cases.apply_charge), so the two
servers answer identically."""
import ctypes as C

import grpc
import pytest

import rl_amd
import rl_grpc
import rl_server
from charge_cases import apply_charge
from oracle import rl_oracle_py as po
from refund_cases import py_peek
from test_allow_all_grpc import NAMES, Ref
from test_refund_grpc import Native, PyStore, arr, python_server

ERR_INVALID_N = "invalid n: must be greater than 0"


class ChargeStore(PyStore):
    """test_refund_grpc.PyStore plus the Charge function"""

    def charge(self, user, m, key, ts, n, cfg, dec, charged, rem, reset):
        rows, _ = apply_charge(self.sim, arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(n, m, C.c_int64),
                               arr(cfg, m, C.c_uint32))
        for i, (d, got, r, rs, _) in enumerate(rows):
            arr(dec, m, C.c_uint8)[i], arr(charged, m, C.c_int64)[i] = d, got
            arr(rem, m, C.c_int64)[i], arr(reset, m, C.c_int64)[i] = r, rs
        return 0

    def coalescer(self):
        return rl_amd.Coalescer(self.batch, max_batch=256, peek=self.peek, charge=self.charge)


def charges(ref, items):
    """one call of runnable (limiter, key, n) items on the oracle beside the server -> rows"""
    t = ref.tick()
    rows, _ = apply_charge(ref.sim, [ref.kid(l, k) for l, k, _ in items], [t] * len(items), [n for _, _, n in items],
                           [NAMES.index(l) for l, _, _ in items])
    return rows


def same(resp, row, n):
    dec, got, rem, reset, _ = row
    assert dec in (po.ALLOWED, po.DENIED)
    assert (resp.charged, resp.short, resp.over_limit, resp.remaining, resp.reset_at_unix_ns, resp.error) == \
        (got, n - got, dec == po.DENIED, rem, reset, "")


def scenario(ch, co):
    cs, status = rl_grpc.charge_stub(ch), rl_grpc.status_stub(ch)
    ref = Ref()
    # --- the unary call: a bucket of 5 gives what it holds and stops at zero ---
    seen = []
    for lim, key, n in (("tb", "k", 3), ("tb", "k", 4), ("tb", "k", 1), ("fw", "u", 4), ("fw", "u", 3), ("sw", "u", 2),
                        ("sw", "u", 5), ("tb2", "z", 4)):
        row = charges(ref, [(lim, key, n)])[0]
        same(rl_grpc.charge(cs, lim, key, n), row, n)
        seen.append((row[0], row[1]))
    assert seen == [(po.ALLOWED, 3), (po.DENIED, 2), (po.DENIED, 0), (po.ALLOWED, 4), (po.DENIED, 3), (po.ALLOWED, 2),
                    (po.DENIED, 5), (po.ALLOWED, 4)]
    # --- the batch call: one launch; the requests that cannot run carry their error ---
    before = co.stats_charge()
    run = [("tb2", "a", 6), ("tb2", "a", 6), ("fw", "v", 2), ("fwc", "w", 9)]
    reqs = [run[0], ("nope", "x", 1), run[1], ("fw", "u", 0), run[2], ("tb", "k", -2), run[3]]
    rows = charges(ref, run)
    assert [(r[0], r[1]) for r in rows] == [(po.ALLOWED, 6), (po.DENIED, 0), (po.ALLOWED, 2), (po.DENIED, 9)]
    got = rl_grpc.charge_batch(cs, reqs)
    assert len(got) == 7
    for j, i in enumerate((0, 2, 4, 6)):
        same(got[i], rows[j], run[j][2])
    for i, err in ((1, "unknown limiter 'nope'"), (3, ERR_INVALID_N), (5, ERR_INVALID_N)):
        assert (got[i].error, got[i].charged, got[i].short, got[i].over_limit, got[i].remaining) == (err, 0, 0, False, 0)
    after = co.stats_charge()
    assert after.charge_launches - before.charge_launches == 1 and after.submitted - before.submitted == 4
    # what is left is what the composition left
    for lim, key in (("tb", "k"), ("fw", "u"), ("sw", "u"), ("tb2", "a"), ("fw", "v")):
        t = ref.tick()
        want_rem = py_peek(ref.sim, ref.kid(lim, key), t, NAMES.index(lim), t // 1_000_000)[1]
        assert rl_grpc.peek(status, lim, key).remaining == want_rem, (lim, key)
    # nothing but errors, and nothing at all: no submission
    got = rl_grpc.charge_batch(cs, [("a", "x", 1), ("fw", "y", -3)])
    ref.tick()
    assert [x.error for x in got] == ["unknown limiter 'a'", ERR_INVALID_N]
    assert rl_grpc.charge_batch(cs, []) == []
    ref.tick()
    assert co.stats_charge().charge_launches == after.charge_launches
    # --- the error mapping of the unary call: nothing is read, not even the clock ---
    for lim, n, err in (("nope", 1, "unknown limiter 'nope'"), ("fw", 0, ERR_INVALID_N), ("tb", -2, ERR_INVALID_N)):
        with pytest.raises(grpc.RpcError) as e:
            rl_grpc.charge(cs, lim, "u", n)
        assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT and e.value.details() == err
    # a request the store cannot execute (INCRBY overflow) on a fail-closed limiter: the RPC's error in the
    # unary call, that result's error in the batch call, and the rest of the batch runs
    big = 1 << 62                                   # twice: past int64
    row = charges(ref, [("fw", "big", big)])[0]
    assert (row[0], row[1]) == (po.DENIED, big)
    same(rl_grpc.charge(cs, "fw", "big", big), row, big)
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.charge(cs, "fw", "big", big)
    ref.tick()
    text = "failed to charge rate limit: script error (INCRBY overflow)"
    assert e.value.code() == grpc.StatusCode.UNAVAILABLE and e.value.details() == text
    rows = charges(ref, [("fw", "big", big), ("tb2", "q", 3)])
    assert rows[0][0] == po.ERROR
    got = rl_grpc.charge_batch(cs, [("fw", "big", big), ("tb2", "q", 3)])
    assert (got[0].error, got[0].charged) == (text, 0)
    same(got[1], rows[1], 3)


def test_proto_has_the_charge_service_and_leaves_the_others_alone():
    a = rl_grpc.api()
    assert a.services["RateLimiterCharge"] == [("Charge", "ChargeRequest", "ChargeResponse"),
                                               ("ChargeBatch", "ChargeBatchRequest", "ChargeBatchResponse")]
    assert list(a.services)[-1] == "RateLimiterCharge"
    assert [m for m, _, _ in a.services["RateLimiter"]] == ["Allow", "AllowN", "Reset", "AllowBatch"]
    assert [m for m, _, _ in a.services["RateLimiterStatus"]] == ["Peek"]
    assert [m for m, _, _ in a.services["RateLimiterAdmin"]] == ["ResetBatch"]
    assert [m for m, _, _ in a.services["RateLimiterMetrics"]] == ["Usage"]
    assert [m for m, _, _ in a.services["RateLimiterTopKeys"]] == ["TopKeys"]
    assert [m for m, _, _ in a.services["RateLimiterRefund"]] == ["Refund", "RefundBatch"]
    assert [m for m, _, _ in a.services["RateLimiterMulti"]] == ["AllowAll", "AllowAllBatch"]
    assert [(f.name, f.number) for f in a.ChargeRequest.DESCRIPTOR.fields] == [("limiter", 1), ("key", 2), ("n", 3)]
    assert [(f.name, f.number) for f in a.ChargeResponse.DESCRIPTOR.fields] == [
        ("charged", 1), ("short", 2), ("over_limit", 3), ("remaining", 4), ("reset_at_unix_ns", 5), ("error", 6)]
    assert [(f.name, f.number) for f in a.ChargeBatchRequest.DESCRIPTOR.fields] == [("requests", 1)]
    assert [(f.name, f.number) for f in a.ChargeBatchResponse.DESCRIPTOR.fields] == [("results", 1)]


def test_native_server_cpu():
    srv = Native(ChargeStore())
    try:
        scenario(srv.ch, srv.co)
    finally:
        srv.close()


def test_python_server_cpu():
    store = ChargeStore()
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
