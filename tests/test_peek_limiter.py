"""rll_peek_n: Peek through the host mirror of the reference's Go API and its
decorators (GPU)."""
import pytest

pytestmark = pytest.mark.gpu

NS = 1_000_000_000
T0 = 1_760_000_000 * NS


@pytest.fixture()
def eng(rl):
    e = rl.LimiterEngine(tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12)
    yield e
    e.close()


@pytest.mark.parametrize("alg", ["token_bucket", "sliding_window", "fixed_window"])
def test_peek_brackets_allow(rl, eng, alg):
    lim = rl.new_limiter(eng, alg, 3, 60 * NS)
    for _ in range(3):      # peeking does not consume
        r, err, code = lim.peek_n("alice", 0, T0)
        assert code == rl.RLL_OK and r.Allowed and (r.Limit, r.Remaining) == (3, 3)
    want, _, _ = lim.peek_n("alice", 1, T0 + 1)
    got, _, _ = lim.allow("alice", T0 + 1)
    assert got == want and got.Remaining == 2
    r, _, _ = lim.peek_n("alice", 0, T0 + 2)
    assert r.Allowed and r.Remaining == 2
    r, _, _ = lim.peek_n("alice", 3, T0 + 2)             # more than is left
    assert not r.Allowed and r.RetryAfter > 0
    assert lim.allow_n("alice", 2, T0 + 3)[0].Allowed    # the denied peek took nothing
    assert lim.peek_n("alice", 0, T0 + 4)[0].Remaining == 0


def test_invalid_n_closed_and_cancelled(rl, eng):
    closed_open = rl.new_limiter(eng, "token_bucket", 3, 60 * NS, prefix="fo", fail_open=True)
    closed_shut = rl.new_limiter(eng, "token_bucket", 3, 60 * NS, prefix="fc")
    r, err, code = closed_shut.peek_n("k", -1, T0)
    assert r is None and code == rl.RLL_ERR_INVALID_N and "invalid n" in err
    assert closed_shut.peek_n("k", 0, T0)[2] == rl.RLL_OK          # n == 0 is legal in a peek ...
    assert closed_shut.allow_n("k", 0, T0)[2] == rl.RLL_ERR_INVALID_N   # ... and only there
    # a cancelled context takes the error branch
    r, err, code = closed_shut.peek_n("k", 1, T0, cancelled=True)
    assert r is None and code == rl.RLL_ERR_FAILED and "context canceled" in err
    r, err, code = closed_open.peek_n("k", 1, T0, cancelled=True)
    assert code == rl.RLL_OK and r.Allowed and (r.Limit, r.Remaining, r.RetryAfter) == (3, 0, 0)
    # a closed limiter: fail-closed is an error, fail-open the fail-open Result of AllowN
    closed_open.close()
    closed_shut.close()
    r, err, code = closed_shut.peek_n("k", 1, T0)
    assert r is None and code == rl.RLL_ERR_FAILED and err == closed_shut.allow_n("k", 1, T0)[1]
    r, err, code = closed_open.peek_n("k", 1, T0)
    assert code == rl.RLL_OK and r == closed_open.allow_n("k", 1, T0)[0]


def test_unseen_key_is_not_interned_and_decorators_stay_silent(rl, eng):
    lim = rl.new_limiter(eng, "fixed_window", 3, 60 * NS)
    lim.add_metrics()
    lim.add_logging(capacity=64)
    assert lim.allow("seen", T0)[0].Allowed
    lim.drain_logs()
    keys = eng.keys(T0 // 1_000_000)
    text = lim.metrics_text()
    assert len(keys) == 1
    # a key never seen answers as a key without state
    for i in range(50):
        r, err, code = lim.peek_n("ghost-%d" % i, 0, T0 + 1)
        assert code == rl.RLL_OK and r.Allowed and r.Remaining == 3
    r, _, _ = lim.peek_n("ghost-0", 4, T0 + 1)
    assert not r.Allowed                                   # a denial is not logged either
    assert lim.peek_n("seen", 0, T0 + 1)[0].Remaining == 2
    assert lim.peek_n("seen", -5, T0 + 1)[2] == rl.RLL_ERR_INVALID_N
    assert eng.keys(T0 // 1_000_000) == keys
    assert lim.metrics_text() == text
    assert lim.drain_logs() == ([], 0)
    # the ghosts were never interned: the first new key gets the id right after "seen"
    # (its window key is listed under its own name, and only one key was added)
    assert lim.allow("ghost-7", T0 + 2)[0].Remaining == 2
    assert len(eng.keys(T0 // 1_000_000)) == 2
