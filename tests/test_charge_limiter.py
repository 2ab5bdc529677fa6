"""rll_charge_n / rll_charge_many: Charge through the host mirror of the
reference's Go API and its decorators (GPU: the mirror owns an engine)."""
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


def batches(rl, e):
    """decide batches the mirror's engine has run"""
    st = rl.rl_stats()
    assert rl.lib.rl_engine_stats(rl.lib.rll_engine_raw(e.h), C.byref(st)) == 0
    return st.batches


def trio(rl, e, **kw):
    return (rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="tb", **kw),
            rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="fw", **kw),
            rl.new_limiter(e, "sliding_window", 10, 3600 * NS, prefix="sw", **kw))


def test_charge_n(rl):
    """a bucket gives up what it holds and stops at zero; a window records the
    whole n, over its limit or not"""
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    c, err, code = tb.charge_n("u", 4, T0)
    assert (err, code) == (None, rl.RLL_OK)
    assert (c.charged, c.short, c.over_limit, c.remaining) == (4, 0, False, 6)
    allow, _, _ = tb.peek_n("u", 1, T0)
    assert c.reset_at_ns == allow.ResetAt
    c, _, _ = tb.charge_n("u", 9, T0 + 1000)              # 6 left: 6 charged, 3 short
    assert (c.charged, c.short, c.over_limit, c.remaining) == (6, 3, True, 0)
    c, _, _ = tb.charge_n("u", 2, T0 + 2000)              # empty: nothing charged, nothing stored
    assert (c.charged, c.short, c.over_limit, c.remaining) == (0, 2, True, 0)
    assert left(tb, "u", T0 + 3000) == 0
    assert not tb.allow_n("u", 1, T0 + 3000)[0].Allowed
    for lim in (fw, sw):
        c, _, _ = lim.charge_n("u", 7, T0)
        assert (c.charged, c.short, c.over_limit, c.remaining) == (7, 0, False, 3)
        c, _, _ = lim.charge_n("u", 8, T0 + 1000)         # 15 of 10: all recorded, over the limit
        assert (c.charged, c.short, c.over_limit, c.remaining) == (8, 0, True, 0)
        assert not lim.allow_n("u", 1, T0 + 2000)[0].Allowed
    e.close()


def test_charge_many_is_one_engine_call(rl):
    """many keys in one call; the second request for a bucket asks against the
    state before the call and can charge 0"""
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    b0 = batches(rl, e)
    got, err, code = tb.charge_many(["a", "b", "a", "c"], [6, 12, 6, 1], T0)
    assert (err, code) == (None, rl.RLL_OK) and batches(rl, e) - b0 == 1
    assert [(c.charged, c.short, c.over_limit) for c in got] == [(6, 0, False), (10, 2, True), (0, 6, True),
                                                                 (1, 0, False)]
    assert got[2].remaining == 4                          # as the decide read it: the caller charges again
    again, _, _ = tb.charge_n("a", 6, T0 + 1000)
    assert (again.charged, again.short) == (4, 2)
    got, _, _ = fw.charge_many(["a", "a", "b"], [6, 6, 1], T0)
    assert [(c.charged, c.over_limit, c.remaining) for c in got] == [(6, False, 4), (6, True, 0), (1, False, 9)]
    assert tb.charge_many([], [], T0) == ([], None, rl.RLL_OK)
    e.close()


def test_invalid_n_before_any_io(rl):
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    assert tb.charge_n("a", 0, T0) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert fw.charge_n("a", -3, T0) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert tb.charge_many(["a", "b"], [3, 0], T0) == (None, ERR_INVALID_N, rl.RLL_ERR_INVALID_N)
    assert e.keys(T0 // 1_000_000) == [] and left(tb, "a", T0) == 10
    assert rl.lib.rll_charge_n(None, b"a", 1, 1, T0, 0, None, None, 0) == rl.RLL_ERR_ARG
    assert rl.lib.rll_charge_many(None, 1, None, None, None, T0, 0, None, None, 0) == rl.RLL_ERR_ARG
    # the key is interned as rll_allow_n interns it
    e2 = engine(rl)
    t2 = trio(rl, e2)
    for la, lb in zip((tb, fw, sw), t2):
        assert la.charge_n("fresh", 2, T0)[0].charged == 2 and lb.allow_n("fresh", 2, T0)[0].Allowed
    assert e.keys(T0 // 1_000_000) == e2.keys(T0 // 1_000_000) and len(e.keys(T0 // 1_000_000)) >= 3
    e.close()
    e2.close()


def test_fail_open_and_fail_closed(rl):
    """a storage error: a fail-open limiter answers charged = 0 with no error,
    a fail-closed one returns the error"""
    e = engine(rl)
    op = rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="open", fail_open=True)
    cl = rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="closed", fail_open=False)
    for lim in (op, cl):
        assert lim.charge_n("a", 3, T0)[0].charged == 3
    c, err, code = op.charge_n("a", 3, T0 + 1000, cancelled=True)
    assert (err, code) == (None, rl.RLL_OK) and (c.charged, c.short, c.over_limit) == (0, 3, False)
    assert cl.charge_n("a", 3, T0 + 1000, cancelled=True) == (None, "failed to charge rate limit: context canceled",
                                                               rl.RLL_ERR_CHARGE)
    op.close()
    cl.close()
    got, err, code = op.charge_many(["a", "b"], [1, 2], T0 + 2000)
    assert (err, code) == (None, rl.RLL_OK) and [(c.charged, c.short) for c in got] == [(0, 1), (0, 2)]
    assert cl.charge_n("a", 1, T0 + 2000) == (None, "failed to charge rate limit: engine: client is closed",
                                              rl.RLL_ERR_CHARGE)
    live = rl.new_limiter(e, "token_bucket", 10, 3600 * NS, prefix="open")
    assert left(live, "a", T0 + 3000) == 7                # nothing was sent after the first charge
    # a request the engine cannot execute: INCRBY overflow
    for fail_open in (True, False):
        big = rl.new_limiter(e, "fixed_window", 10, 3600 * NS, prefix="big%d" % fail_open, fail_open=fail_open)
        c, _, _ = big.charge_n("o", 1 << 62, T0)
        assert (c.charged, c.over_limit) == (1 << 62, True)
        got = big.charge_n("o", 1 << 62, T0 + 1000)      # twice this is past int64
        if fail_open:
            assert got[1:] == (None, rl.RLL_OK) and (got[0].charged, got[0].short) == (0, 1 << 62)
        else:
            assert got == (None, "failed to charge rate limit: ERR increment or decrement would overflow",
                           rl.RLL_ERR_CHARGE)
    e.close()


def test_decorators(rl):
    """the metrics decorator's two counters, exposed once the verb was used;
    the logging decorator: a short charge at debug, a failure at error level"""
    e = engine(rl)
    tb, fw, sw = trio(rl, e)
    for lim in (tb, fw):
        lim.add_metrics()
        lim.add_logging(capacity=64)
    assert tb.allow_n("u", 1, T0)[0].Allowed
    text0 = tb.metrics_text()
    assert "charge" not in text0
    tb.drain_logs()
    assert tb.charge_n("u", 4, T0 + 10)[0].charged == 4
    got, _, _ = tb.charge_many(["u", "v"], [9, 2], T0 + 20)     # 5 left: 5 charged, 4 short
    assert [(c.charged, c.short) for c in got] == [(5, 4), (2, 0)]
    assert tb.charge_n("u", 0, T0 + 30)[2] == rl.RLL_ERR_INVALID_N
    text = tb.metrics_text()
    assert 'rate_limiter_charged_units_total{algorithm="token_bucket"} 11\n' in text
    assert 'rate_limiter_charge_short_units_total{algorithm="token_bucket"} 4\n' in text
    assert text.startswith(text0)
    assert fw.charge_n("u", 25, T0)[0].charged == 25
    ftext = fw.metrics_text()
    assert 'rate_limiter_charged_units_total{algorithm="fixed_window"} 25\n' in ftext
    assert 'rate_limiter_charge_short_units_total{algorithm="fixed_window"} 0\n' in ftext
    logs, dropped = tb.drain_logs()
    assert logs[0] == (0, "charge short", "key=u n=9 charged=5") and dropped == 0
    assert [(lv, msg) for lv, msg, _ in logs[1:]] == [(3, "rate limiter charge error")]       # n = 0
    assert fw.drain_logs()[0] == []
    tb.close()
    want = "failed to charge rate limit: engine: client is closed"
    assert tb.charge_n("u", 1, T0 + 40)[1:] == (want, rl.RLL_ERR_CHARGE)
    logs, _ = tb.drain_logs()
    assert [(lv, msg) for lv, msg, _ in logs] == [(3, "rate limiter charge error")] and "error=" + want in logs[0][2]
    assert 'rate_limiter_charged_units_total{algorithm="token_bucket"} 11\n' in tb.metrics_text()
    e.close()
