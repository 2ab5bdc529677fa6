"""The GPU coalescer's staged-copy path (RL_COALESCER_ZC_MAX=0: every launch
copies its inputs to the slot's device block and its results back, as batches
above the zero-copy threshold do) for the operations that are not decides:
reset batches, refunds and peeks, between decide batches that see their effect.
Statuses and decisions equal the oracle's bit for bit."""
import threading

import numpy as np
import pytest

import oracle
from peek_cases import assert_peek, peek_expected, sim_decide
from refund_cases import DONE, apply_refunds, new_sim, warm
from reset_cases import apply_resets, expected_status
from tracegen import NS, T0, random_trace

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 20, 12 * NS), (3, 100, 60 * NS)]   # one token bucket, one fixed window
N = len(CONFIGS)
MAX_BATCH = 1 << 12
NAMES = ("decision", "remaining", "retry", "reset_at")


@pytest.fixture
def staged(rl, monkeypatch):
    """(engine, coalescer) with the zero-copy threshold at 0: the variable is
    read when the GPU backend is constructed"""
    monkeypatch.setenv("RL_COALESCER_ZC_MAX", "0")
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=MAX_BATCH, flags=rl.OPT_PIPELINE)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=MAX_BATCH)
    yield eng, co
    co.close()
    eng.close()


def trace(seed=5, m=600, nkeys=40):
    """a decide trace in three parts: 300, 150 and 150 requests"""
    tr = random_trace(seed, m, nkeys, CONFIGS)[:4]
    return [tuple(x[a:b] for x in tr) for a, b in ((0, 300), (300, 450), (450, m))]


def c_sim():
    sim = oracle.OracleSim(0)
    for a, L, W in CONFIGS:
        sim.add_config(a, L, W)
    return sim


def decide_and_check(co, sim, part, what):
    """one decide submission; its four result arrays equal the C oracle's"""
    rc, out = co.wait(co.submit(*part), part[0].size)
    assert rc == 0, what
    for name, a, b in zip(NAMES, out, sim.decide(*part)[:4]):
        assert np.array_equal(a, b), f"{what}: {name}"


def resets_of(part, count, seed):
    """`count` resets of keys of `part` at its last time (duplicates among
    them), two of them invalid: an unknown config and the reserved key"""
    rng = np.random.default_rng(seed)
    sel = rng.integers(0, part[0].size, count)
    key, cfg = part[0][sel].copy(), part[3][sel].copy()
    cfg[1] = N
    key[count // 2] = np.uint64((1 << 64) - 1)
    return key, np.full(count, part[1][-1]), cfg


def test_reset_batch_and_single_reset_between_decides(staged):
    eng, co = staged
    sim = c_sim()
    first, second, third = trace()
    decide_and_check(co, sim, first, "before the resets")
    rk, rt, rcfg = resets_of(first, 60, 1)
    rc, status = co.reset_batch(rk, rt, rcfg)
    assert rc == 0 and np.array_equal(status, expected_status(rk, rcfg, N))
    apply_resets(sim, rk, rt, rcfg, N)
    decide_and_check(co, sim, second, "after the reset batch")
    q = int(np.argmax(second[0] % np.uint64(2) == 1))        # a window key's request
    assert co.reset(int(second[0][q]), int(second[1][-1]), int(second[3][q])) == 0
    sim.reset(int(second[3][q]), int(second[0][q]), int(second[1][-1]), 0)
    assert co.reset(1, int(second[1][-1]), N) != 0           # an unknown config: the single reset's error
    decide_and_check(co, sim, third, "after the single reset")
    st = co.stats()
    assert (st.resets, st.reset_launches) == (58 + 1, 3)
    assert st.submitted == st.decided == 600
    assert eng.sync() == 0


def test_merged_reset_submissions_share_one_launch(staged):
    """A reset submission of eight full launches and 100 more, and a second
    one queued while its launches go out: the 100 and the second submission
    are one launch, the second one's status copied back from slot offset 100.
    When the second came too late for that (it then has a launch of its own)
    the pair is submitted again; every attempt is checked."""
    eng, co = staged
    sim = c_sim()
    first, second, _ = trace()
    decide_and_check(co, sim, first, "before the resets")
    a = resets_of(first, 8 * MAX_BATCH + 100, 2)
    b = resets_of(first, 60, 3)
    merged = False
    for attempt in range(20):
        before = co.stats()
        assert before.pending == 0
        out = {}
        thr = threading.Thread(target=lambda: out.update(a=co.reset_batch(*a)))
        thr.start()
        while co.stats().pending == 0 and thr.is_alive():    # a is queued (or already done)
            pass
        rc_b, st_b = co.reset_batch(*b)
        thr.join()
        rc_a, st_a = out["a"]
        assert (rc_a, rc_b) == (0, 0)
        assert np.array_equal(st_a, expected_status(a[0], a[2], N)), f"attempt {attempt}: first submission"
        assert np.array_equal(st_b, expected_status(b[0], b[2], N)), f"attempt {attempt}: second submission"
        st = co.stats()
        assert st.resets - before.resets == int((st_a == 1).sum() + (st_b == 1).sum())
        launches = st.reset_launches - before.reset_launches
        assert launches in (9, 10)
        if launches == 9:
            merged = True
            break
    apply_resets(sim, a[0], a[1], a[2], N)
    apply_resets(sim, b[0], b[1], b[2], N)
    decide_and_check(co, sim, second, "after the resets")
    assert merged, "the second reset submission never joined the first one's last launch"
    assert eng.sync() == 0


def test_refund_between_decides(staged):
    """decide, refund, decide, none waited for before the next is queued"""
    eng, co = staged
    ref = new_sim(0, CONFIGS)
    first, second, _ = trace()
    # refunds of n = 1 .. 3, each aimed at some key's last request of `first`
    # (a key's store clock must not go back), and two invalid ones
    rng = np.random.default_rng(4)
    last = np.array(sorted({int(k): i for i, k in enumerate(first[0].tolist())}.values()))
    idx = last[rng.integers(0, last.size, 120)]
    rk, rt, rn, rcfg = first[0][idx], first[1][idx], rng.integers(1, 4, 120).astype(np.int64), first[3][idx].copy()
    rcfg[7] = N
    rn[11] = 0
    t0 = co.submit(*first)
    rc, status = co.refund(rk, rt, rn, rcfg)
    t1 = co.submit(*second)
    rc0, got0 = co.wait(t0, first[0].size)
    rc1, got1 = co.wait(t1, second[0].size)
    assert (rc0, rc, rc1) == (0, 0, 0)
    rows = lambda got, m: [tuple(int(got[j][i]) for j in range(4)) for i in range(m)]
    want0 = warm(ref, first + (None,))
    want_st, _ = apply_refunds(ref, rk, rt, rn, rcfg)
    want1 = warm(ref, second + (None,))
    assert np.array_equal(status, want_st) and (want_st == DONE).sum() > 50 and (want_st == 3).sum() == 2
    assert rows(got0, first[0].size) == [w[:4] for w in want0]
    assert rows(got1, second[0].size) == [w[:4] for w in want1]
    st = co.stats()
    assert (st.refunds, st.refund_launches) == (int((want_st == DONE).sum()), 1)
    assert eng.sync() == 0


def test_peek_sees_what_was_submitted_before_and_not_after(staged):
    """decide, peek, decide, peek: a peek equals the Python oracle's answer on
    the state after the decides before it; the decides equal the C oracle,
    which never sees a peek"""
    eng, co = staged
    sim, psim = c_sim(), new_sim(0, CONFIGS)
    first, second, _ = trace()
    rng = np.random.default_rng(6)

    def queries(at):
        k = rng.integers(0, 44, 150).astype(np.uint64)       # keys 40 .. 43 were never seen
        return k, np.full(150, at), rng.integers(0, 3, 150).astype(np.int64), (k % np.uint64(N)).astype(np.uint32)

    t0 = co.submit(*first)
    q0 = queries(first[1][-1])
    rc_p0, p0 = co.peek(*q0)
    t1 = co.submit(*second)
    rc0, got0 = co.wait(t0, first[0].size)
    rc1, got1 = co.wait(t1, second[0].size)
    q1 = queries(second[1][-1])
    rc_p1, p1 = co.peek(*q1)
    assert (rc0, rc_p0, rc1, rc_p1) == (0, 0, 0, 0)
    sim_decide(psim, *first)
    assert_peek(p0, peek_expected(psim, *q0), CONFIGS, q0[3], "the first peek")
    sim_decide(psim, *second)
    assert_peek(p1, peek_expected(psim, *q1), CONFIGS, q1[3], "the second peek")
    for got, part in ((got0, first), (got1, second)):
        for name, a, b in zip(NAMES, got, sim.decide(*part)[:4]):
            assert np.array_equal(a, b), name
    st = co.stats()
    assert (st.peeked, st.submitted, st.decided) == (300, 450, 450)
    assert eng.sync() == 0
