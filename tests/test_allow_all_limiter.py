"""rll_allow_all: AllowAll through the host mirror of the reference's Go API and
its decorators (GPU: the mirror owns an engine)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_760_000_000 * NS
ERR_INVALID_N = "invalid n: must be greater than 0"


def engine(rl):
    return rl.LimiterEngine(tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12)


def left(lim, key, t):
    r, err, code = lim.peek_n(key, 0, t)
    assert err is None
    return r.Remaining


def trio(rl, e, **kw):
    return (rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="tb", **kw),
            rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="fw", **kw),
            rl.new_limiter(e, "sliding_window", 10, 3600 * NS, prefix="sw", **kw))


def test_all_or_nothing(rl):
    """three limiters of limit 10: a group that passes keeps its takes; a
    group one member denies takes nothing, the denied window member's count
    included; every Result is the limiter's own, as rll_allow_n builds it"""
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    ok, res, by, err, code = rl.RateLimiter.allow_all([(tb, "u", 4), (fw, "u", 3), (sw, "u", 2)], T0)
    assert (ok, by, err, code) == (True, -1, None, rl.RLL_OK)
    assert [(r.Allowed, r.Limit, r.Remaining, r.RetryAfter) for r in res] == [(True, 10, 6, 0), (True, 10, 7, 0),
                                                                             (True, 10, 8, 0)]
    assert [left(l, "u", T0 + 1000) for l in (tb, fw, sw)] == [6, 7, 8]
    # the fixed window denies (7 + ... > 10): the bucket's 5 and both window counts come back
    ok, res, by, err, code = rl.RateLimiter.allow_all([(tb, "u", 5), (fw, "u", 8), (sw, "u", 1)], T0 + 2000)
    assert (ok, by, err, code) == (False, 1, None, rl.RLL_OK)
    assert [r.Allowed for r in res] == [True, False, True]
    assert res[0].Remaining == 1 and res[1].Remaining == 0 and res[1].RetryAfter > 0 and res[2].Remaining == 7
    single, _, _ = fw.peek_n("u", 8, T0 + 2000)
    assert (res[1].ResetAt, res[1].Limit) == (single.ResetAt, 10)
    assert [left(l, "u", T0 + 3000) for l in (tb, fw, sw)] == [6, 7, 8]
    # a group of one is AllowN, plus the give-back of a denied window member's INCRBY
    ok, res, by, _, _ = rl.RateLimiter.allow_all([(fw, "u", 9)], T0 + 4000)
    assert (ok, by, res[0].Allowed) == (False, 0, False) and left(fw, "u", T0 + 5000) == 7
    r, _, _ = fw.allow_n("u", 9, T0 + 6000)        # AllowN itself leaves the count raised
    assert not r.Allowed and left(fw, "u", T0 + 7000) == 0
    e.close()


def test_argument_errors_and_invalid_n(rl):
    """k = 0 and k = 17, a null limiter, limiters of two engines: RLL_ERR_ARG;
    n <= 0: ErrInvalidN before any I/O (nothing interned, nothing taken)"""
    e, e2 = engine(rl), engine(rl)
    tb, fw, sw = trio(rl, e)
    other = rl.new_limiter(e2, "token_bucket", 10, 3600 * NS)
    A = rl.RateLimiter.allow_all
    assert A([], T0)[3:] == ("", rl.RLL_ERR_ARG)
    assert A([(tb, "k%d" % i, 1) for i in range(17)], T0)[4] == rl.RLL_ERR_ARG
    assert A([(tb, "a", 1), (other, "a", 1)], T0)[4] == rl.RLL_ERR_ARG
    hs = (C.c_void_p * 2)(tb.h, None)
    keys = (C.c_char_p * 2)(b"a", b"a")
    lens = (C.c_size_t * 2)(1, 1)
    n = (C.c_int64 * 2)(1, 1)
    res = (rl.rll_result * 2)()
    cast = lambda x: C.cast(x, C.c_void_p)
    assert rl.lib.rll_allow_all(cast(hs), 2, cast(keys), cast(lens), cast(n), T0, 0, cast(res), None, None, None, 0) \
        == rl.RLL_ERR_ARG
    assert rl.lib.rll_allow_all(None, 2, cast(keys), cast(lens), cast(n), T0, 0, cast(res), None, None, None, 0) \
        == rl.RLL_ERR_ARG
    now_ms = T0 // 1_000_000
    assert e.keys(now_ms) == []                                  # none of the above interned or stored anything
    assert A([(tb, "a", 3), (fw, "a", 0)], T0)[3:] == (ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert A([(tb, "a", -1)], T0)[3:] == (ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert e.keys(now_ms) == [] and left(tb, "a", T0) == 10
    # sixteen members is the largest group
    ok, res, by, err, code = A([(tb, "k%d" % i, 1) for i in range(16)], T0)
    assert (ok, by, code, len(res)) == (True, -1, rl.RLL_OK, 16)
    e.close()
    e2.close()


def test_unknown_key_is_interned_as_allow_n_does(rl):
    """the keyspace after rll_allow_all equals the one after the same requests
    through rll_allow_n, names included"""
    ea, eb = engine(rl), engine(rl)
    la, lb = trio(rl, ea), trio(rl, eb)
    ok, _, _, _, _ = rl.RateLimiter.allow_all([(l, "fresh", 2) for l in la], T0)
    assert ok
    for l in lb:
        assert l.allow_n("fresh", 2, T0)[0].Allowed
    now_ms = T0 // 1_000_000
    assert ea.keys(now_ms) == eb.keys(now_ms) and len(ea.keys(now_ms)) >= 3
    ea.close()
    eb.close()


def test_fail_open_and_fail_closed_mix(rl):
    """a closed or cancelled fail-open member contributes its fail-open Result
    and the others are still checked; a fail-closed one fails the call before
    anything is sent"""
    e = engine(rl)
    op = rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="open", fail_open=True)
    cl = rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="closed", fail_open=False)
    fw = rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="fw")
    A = rl.RateLimiter.allow_all
    op.close()
    ok, res, by, err, code = A([(op, "a", 4), (fw, "a", 4)], T0)
    single, _, _ = op.allow_n("a", 4, T0)
    assert (ok, by, code) == (True, -1, rl.RLL_OK) and res[0] == single
    assert (res[0].Allowed, res[0].Limit, res[0].Remaining) == (True, 10, 0) and res[1].Remaining == 6
    # the open member stands aside, the window member denies: the group fails and takes nothing
    ok, res, by, _, _ = A([(op, "a", 4), (fw, "a", 7)], T0 + 1000)
    assert (ok, by, res[0].Allowed, res[1].Allowed) == (False, 1, True, False) and left(fw, "a", T0 + 2000) == 6
    # a cancelled context: the fail-open members answer, the fail-closed default fails the call
    ok, res, by, err, code = A([(op, "a", 1)], T0 + 3000, cancelled=True)
    assert (ok, code) == (True, rl.RLL_OK)
    assert A([(op, "a", 1), (fw, "a", 1)], T0 + 3000, cancelled=True)[3:] == (
        "failed to check rate limit: context canceled", rl.RLL_ERR_FAILED)
    cl.close()
    assert A([(fw, "a", 1), (cl, "a", 1)], T0 + 4000)[3:] == (
        "failed to check rate limit: engine: client is closed", rl.RLL_ERR_FAILED)
    assert cl.allow_n("a", 1, T0 + 4000)[1:] == ("failed to check rate limit: engine: client is closed", rl.RLL_ERR_FAILED)
    assert left(fw, "a", T0 + 5000) == 6                         # nothing was sent
    # a member the engine cannot execute: INCRBY overflow is that limiter's error, the group is rolled back
    big = rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="big")
    assert not big.allow_n("o", 1 << 62, T0 + 6000)[0].Allowed       # twice this is past int64
    out = A([(fw, "a", 1), (big, "o", 1 << 62)], T0 + 7000)
    assert out[3:] == ("failed to check rate limit: ERR increment or decrement would overflow", rl.RLL_ERR_FAILED)
    assert left(fw, "a", T0 + 8000) == 6
    e.close()


def test_decorators(rl):
    """the metrics decorator's two counters, exposed once the verb was used;
    the logging decorator: a denied group at debug, a failure at error level"""
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    for l in (tb, fw):
        l.add_metrics()
        l.add_logging(capacity=64)
    assert tb.allow_n("u", 1, T0)[0].Allowed
    text0 = tb.metrics_text()
    assert "allow_all" not in text0
    tb.drain_logs()
    A = rl.RateLimiter.allow_all
    assert A([(tb, "u", 2), (fw, "u", 2), (sw, "u", 2)], T0 + 10)[0] is True
    assert A([(tb, "u", 3), (fw, "u", 9), (sw, "u", 1)], T0 + 20)[0] is False      # the window denies
    assert A([(tb, "u", 20), (fw, "u", 1)], T0 + 30)[0] is False                   # the bucket denies, and took nothing
    text = tb.metrics_text()
    assert 'rate_limiter_allow_all_total{allowed="true"} 1\n' in text
    assert 'rate_limiter_allow_all_total{allowed="false"} 2\n' in text
    assert 'rate_limiter_allow_all_rolled_back_units_total{algorithm="token_bucket"} 3\n' in text
    assert text.startswith(text0)
    assert 'rate_limiter_allow_all_rolled_back_units_total{algorithm="fixed_window"} 10\n' in fw.metrics_text()
    logs, dropped = tb.drain_logs()
    assert [(lv, msg) for lv, msg, _ in logs] == [(0, "allow-all denied")] * 2 and dropped == 0
    assert logs[0][2] == "key=u n=3 member=0 denied_by=1 rolled_back_units=3"
    assert logs[1][2] == "key=u n=20 member=0 denied_by=0 rolled_back_units=0"
    fw.drain_logs()
    fw.close()
    want = "failed to check rate limit: engine: client is closed"
    assert A([(tb, "u", 1), (fw, "u", 1)], T0 + 40)[3:] == (want, rl.RLL_ERR_FAILED)
    for l in (tb, fw):
        logs, _ = l.drain_logs()
        assert [(lv, msg) for lv, msg, _ in logs] == [(3, "rate limiter allow-all error")]
        assert "error=" + want in logs[0][2]
    assert 'rate_limiter_allow_all_total{allowed="false"} 3\n' in tb.metrics_text()
    assert [left(l, "u", T0 + 50) for l in (tb, sw)] == [7, 8]
    e.close()
