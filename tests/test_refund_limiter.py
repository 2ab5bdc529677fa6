"""rll_refund_n / rll_refund_many: Refund through the host mirror of the
reference's Go API and its decorators (GPU)."""
import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_760_000_000 * NS
ALGS = ["token_bucket", "sliding_window", "fixed_window"]
ERR_INVALID_N = "invalid n: must be greater than 0"


def engine(rl):
    return rl.LimiterEngine(tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12)


def left(lim, key, t):
    r, err, code = lim.peek_n(key, 0, t)
    assert err is None
    return r.Remaining


@pytest.mark.parametrize("alg", ALGS)
def test_refund_gives_quota_back(rl, alg):
    """limit 10 over an hour (a bucket refills 1 token in 6 min: nothing in
    this test's few ms): take 7, give 2 back, take the rest"""
    e = engine(rl)
    lim = rl.new_limiter(e, alg, 10, 3600 * NS)
    r, _, _ = lim.allow_n("a", 7, T0)
    assert r.Allowed and r.Remaining == 3
    assert lim.refund_n("a", 2, T0 + 1000) == (True, None, rl.RLL_OK)
    assert left(lim, "a", T0 + 2000) == 5
    r, _, _ = lim.allow_n("a", 5, T0 + 3000)
    assert r.Allowed and r.Remaining == 0
    # a refund never exceeds the limit: all 10 back and more
    assert lim.refund_n("a", 50, T0 + 4000) == (True, None, rl.RLL_OK)
    assert left(lim, "a", T0 + 5000) == 10
    # a window counter at zero is deleted, so a second refund finds no key; a bucket is still there
    applied, err, code = lim.refund_n("a", 1, T0 + 6000)
    assert (applied, err, code) == (alg == "token_bucket", None, rl.RLL_OK)
    # a key never seen: nothing to refund, nothing interned, nothing stored
    now_ms = (T0 + 7000) // 1_000_000
    names = e.keys(now_ms)
    assert lim.refund_n("ghost", 3, T0 + 7000) == (False, None, rl.RLL_OK)
    assert e.keys(now_ms) == names
    r, _, _ = lim.allow_n("ghost", 10, T0 + 8000)
    assert r.Allowed and r.Remaining == 0
    e.close()


@pytest.mark.parametrize("alg", ["sliding_window", "fixed_window"])
def test_at_ns_picks_the_window(rl, alg):
    """a denied AllowN still raises the window's counter; the refund names the
    window by a time inside it, also after the window rolled over"""
    e = engine(rl)
    W = 60 * NS
    lim = rl.new_limiter(e, alg, 5, W)
    w0 = (T0 // W + 1) * W                      # a window start
    # 50 s into the window: its counter lives 60 s from its first INCRBY, so
    # it outlives the window by 50 s
    b = w0 + 50 * NS
    for i in range(5):
        assert lim.allow_n("k", 1, b + i)[0].Allowed
    r, _, _ = lim.allow_n("k", 3, b + 10)       # denied, counted: the window holds 8
    assert not r.Allowed
    reset_at = r.ResetAt
    assert reset_at == w0 + W
    # undo the denied request while its window is current: at_ns = 0 is now
    assert lim.refund_n("k", 3, b + 20) == (True, None, rl.RLL_OK)
    assert not lim.allow_n("k", 1, b + 30)[0].Allowed            # 5 of 5 used, and this one counted: 6
    # 10 s into the next window, refund 2 of the previous window by its reset time - 1
    t1 = w0 + W + 10 * NS
    assert lim.refund_n("k", 2, t1, reset_at - 1) == (True, None, rl.RLL_OK)
    # ... and the current window holds nothing yet: at_ns = 0 finds no key
    assert lim.refund_n("k", 1, t1) == (False, None, rl.RLL_OK)
    r, _, _ = lim.peek_n("k", 0, t1)
    if alg == "fixed_window":
        assert r.Remaining == 5                                  # the previous window is history
    else:
        assert r.Remaining == 5 - int(4 * (1 - 10 / 60))         # the previous window's 4, weighted 5/6: 3
    # a window that never was
    assert lim.refund_n("k", 1, t1, w0 - 5 * W) == (False, None, rl.RLL_OK)
    e.close()


def test_refund_many_is_one_call(rl):
    """refunds of one key are summed; invalid n fails the whole call before
    any I/O; at_ns per request"""
    e = engine(rl)
    lim = rl.new_limiter(e, "fixed_window", 100, 60 * NS)
    keys = ["k%d" % i for i in range(6)]
    for k in keys:
        assert lim.allow_n(k, 50, T0)[0].Allowed
    applied, err, code = lim.refund_many(["k0", "k1", "k0", "ghost", "k0", "k2"], [1, 2, 3, 4, 5, 50], now_ns=T0 + 1000)
    assert (applied.tolist(), err, code) == ([True, True, True, False, True, True], None, rl.RLL_OK)
    assert [left(lim, k, T0 + 2000) for k in keys[:4]] == [59, 52, 100, 50]
    applied, err, code = lim.refund_many(["k3", "k4"], [1, 0], now_ns=T0 + 3000)
    assert (applied, err, code) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert lim.refund_n("k3", -1, T0 + 3000) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert left(lim, "k3", T0 + 4000) == 50                     # nothing applied
    applied, err, code = lim.refund_many(["k3", "k3"], [1, 1], at_ns=[0, T0 - 3600 * NS], now_ns=T0 + 5000)
    assert (applied.tolist(), code) == ([True, False], rl.RLL_OK)
    assert lim.refund_many([], [])[2] == rl.RLL_OK
    e.close()


def test_closed_limiter_and_decorators(rl):
    """a closed limiter returns the error (never a fail-open Result, as Reset);
    the metrics decorator counts refunds and units under their own names, the
    logging decorator logs a refund at debug and a failure at error level"""
    e = engine(rl)
    lim = rl.new_limiter(e, "token_bucket", 10, 3600 * NS, fail_open=True)
    lim.add_metrics()
    lim.add_logging(capacity=64)
    assert lim.allow_n("a", 4, T0)[0].Allowed
    text0 = lim.metrics_text()
    assert "refund" not in text0
    lim.drain_logs()
    assert lim.refund_n("a", 3, T0 + 10) == (True, None, rl.RLL_OK)
    applied, _, _ = lim.refund_many(["a", "ghost"], [1, 7], now_ns=T0 + 20)
    assert applied.tolist() == [True, False]
    text = lim.metrics_text()
    assert 'rate_limiter_refunds_total{algorithm="token_bucket",applied="true"} 2\n' in text
    assert 'rate_limiter_refunds_total{algorithm="token_bucket",applied="false"} 1\n' in text
    assert 'rate_limiter_refunded_units_total{algorithm="token_bucket"} 4\n' in text
    assert text.startswith(text0)                   # decisions are counted as before
    logs, dropped = lim.drain_logs()
    assert [(lv, msg) for lv, msg, _ in logs] == [(0, "quota refunded")] * 3 and dropped == 0
    assert logs[0][2] == "key=a n=3 applied=true" and logs[2][2] == "key=ghost n=7 applied=false"
    lim.close()
    want = "failed to refund rate limit: engine: client is closed"
    assert lim.refund_n("a", 1, T0 + 30) == (None, want, rl.RLL_ERR_REFUND)
    assert lim.refund_many(["a", "b"], [1, 1], now_ns=T0 + 30)[1:] == (want, rl.RLL_ERR_REFUND)
    assert lim.refund_n("a", 0, T0 + 30) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)   # before any I/O
    logs, _ = lim.drain_logs()
    assert [(lv, msg) for lv, msg, _ in logs] == [(3, "rate limiter refund error")] * 3
    assert "error=" + want in logs[0][2]
    assert lim.metrics_text() == text               # failed refunds are not counted
    e.close()
