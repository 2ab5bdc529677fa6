"""rll_reset_many: ResetMany through the host mirror of the reference's Go API
and its decorators (GPU).  It is observably a loop of rll_reset."""
import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_760_000_000 * NS
ALGS = ["token_bucket", "sliding_window", "fixed_window"]


def engines(rl):
    return [rl.LimiterEngine(tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12) for _ in range(2)]


def traffic(lim, t, keys, n=2):
    return [lim.allow_n(k, n, t + i)[0] for i, k in enumerate(keys)]


@pytest.mark.parametrize("alg", ALGS)
def test_reset_many_equals_a_loop_of_reset(rl, alg):
    ea, eb = engines(rl)
    la, lb = (rl.new_limiter(e, alg, 3, 60 * NS) for e in (ea, eb))
    keys = ["user-%d" % i for i in range(40)]
    assert traffic(la, T0, keys) == traffic(lb, T0, keys)
    # every third key, a key never seen (both intern it), one key twice
    some = keys[::3] + ["ghost", keys[0]]
    for k in some:
        assert la.reset(k, T0 + 1000) is None
    assert lb.reset_many(some, T0 + 1000) is None
    now_ms = (T0 + 1000) // 1_000_000
    assert ea.keys(now_ms) == eb.keys(now_ms)
    assert len(ea.keys(now_ms)) == 40 - len(keys[::3])
    # the reset keys have a fresh quota, the others do not; new keys get the same ids
    more = keys + ["ghost", "new-1", "new-2"]
    ra, rb = traffic(la, T0 + 2000, more), traffic(lb, T0 + 2000, more)
    assert ra == rb
    assert [r.Allowed for r in rb[:6]] == [True, False, False, True, False, False]
    assert ea.keys(now_ms) == eb.keys(now_ms)
    assert lb.reset_many([], T0) is None
    for e in (ea, eb):
        e.close()


def test_closed_limiter_and_decorators(rl):
    ea, eb = engines(rl)
    la, lb = (rl.new_limiter(e, "fixed_window", 3, 60 * NS) for e in (ea, eb))
    for lim in (la, lb):
        lim.add_metrics()
        lim.add_logging(capacity=64)
    keys = ["k%d" % i for i in range(10)]
    assert traffic(la, T0, keys) == traffic(lb, T0, keys)
    # through both decorators: forwarded, nothing counted, nothing logged
    text, text_a = lb.metrics_text(), la.metrics_text()
    for k in keys[:5]:
        assert la.reset(k, T0 + 10) is None
    assert lb.reset_many(keys[:5], T0 + 10) is None
    assert lb.metrics_text() == text and la.metrics_text() == text_a
    assert la.drain_logs() == lb.drain_logs() == ([], 0)
    assert traffic(la, T0 + 20, keys) == traffic(lb, T0 + 20, keys)
    la.drain_logs(), lb.drain_logs()
    # closed: the text of rll_reset, one error record for the whole call, nothing interned
    la.close()
    lb.close()
    want = la.reset("k0", T0 + 30)
    assert want == "failed to reset rate limit: engine: client is closed"
    assert lb.reset_many(["k0", "never-seen", "k1"], T0 + 30) == want
    logs, dropped = lb.drain_logs()
    assert [(lv, msg) for lv, msg, _ in logs] == [(3, "rate limiter reset error")] and dropped == 0
    assert "error=" + want in logs[0][2]
    now_ms = (T0 + 30) // 1_000_000
    assert ea.keys(now_ms) == eb.keys(now_ms)
    for e in (ea, eb):
        e.close()
