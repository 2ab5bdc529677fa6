"""Refund's contract on the CPU (refund_cases.py): the seeded cases meet their
coverage, the sum rule is what it claims to be, and the split 32-bit sums of
the kernel rebuild N exactly."""
import copy

import numpy as np
import pytest

from oracle import rl_oracle_py as po
from refund_cases import (DONE, INT64_MAX, INVALID, KINDS, NOKEY, apply_refunds, bucket_counterexample, new_sim,
                          refund_case, split_sum, total, warm)
from tracegen import NS, T0


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_seeded_cases_cover(kind, profile):
    """the builder asserts its coverage; statuses are of the three kinds only"""
    configs, first, (rkey, rts, rn, rcfg, rsms), second, now_ms, cover = refund_case(kind, profile)
    assert 900 <= rkey.size <= 1100
    assert set(np.unique(cover["status"]).tolist()) == {NOKEY, DONE, INVALID}
    assert (rsms is None) == (kind == "tb")


@pytest.mark.parametrize("kind", ["fw", "sw", "skew"])
def test_window_sum_equals_single_refunds(kind):
    """for windows the per-target sum is m single refunds in any order:
    clamped decrements commute.  Three random orders, the whole keyspace."""
    configs, first, (rkey, rts, rn, rcfg, rsms), _, _, cover = refund_case(kind, 0)
    base = new_sim(0, configs)
    warm(base, first)
    one = copy.deepcopy(base)
    status, info = apply_refunds(one, rkey, rts, rn, rcfg, rsms)
    assert len(info["deleted"]) >= 5 and sum(len(v) >= 2 for v in info["targets"].values()) >= 50
    for seed in (1, 2, 3):
        sim = copy.deepcopy(base)
        order = np.random.default_rng(seed).permutation(rkey.size)
        for i in order:
            s = slice(i, i + 1)
            st, _ = apply_refunds(sim, rkey[s], rts[s], rn[s], rcfg[s], None if rsms is None else rsms[s])
            # a single refund of a target an earlier one deleted finds no key:
            # the call's status comes from the state before the call
            assert st[0] == status[i] or (st[0] == NOKEY and status[i] == DONE)
        assert sim.db == one.db, seed


def test_bucket_sum_differs_from_two_calls():
    """the example of DESIGN §10i: t = 0.9763120008305, a = 4, b = 45 -- one
    call (the sum) and two calls leave different tokens; a seeded search finds
    more such t, about 1 in 200"""
    found = bucket_counterexample()
    assert found[0] == (0.9763120008305, 4, 45)
    assert 5 <= len(found) - 1 <= 100          # of 4000 tries
    t, a, b = found[0]
    configs = [(1, 10 ** 6, 60 * NS)]
    sims = []
    for calls in ([[a, b]], [[a], [b]]):
        sim = new_sim(po.REDIS7, configs)
        sim.db["tb:1"] = [(t, float(T0) / 1e9), None]
        for ns in calls:
            st, _ = apply_refunds(sim, [1] * len(ns), [T0] * len(ns), ns, [0] * len(ns))
            assert (st == DONE).all()
        sims.append(sim.db["tb:1"][0][0])
    assert sims[0] == float("%.14g" % (t + 49.0)) and sims[1] == float("%.14g" % (float("%.14g" % (t + 4.0)) + 45.0))
    assert sims[0] != sims[1]
    assert ("%.14g" % sims[0], "%.14g" % sims[1]) == ("49.97631200083", "49.976312000831")


def test_saturation_and_carry():
    """N from the sums of the low and the high halves, in Python ints"""
    M32 = (1 << 32) - 1
    cases = [[1], [M32], [M32, 1], [1 << 32], [M32] * 5, [(1 << 32) + 5, M32, 7], [1 << 62], [1 << 62, 1 << 62],
             [(1 << 62) - 1, 1 << 62], [(1 << 62), (1 << 62) - 1, 1], [INT64_MAX], [INT64_MAX] * 3, [INT64_MAX - 1, 1],
             [INT64_MAX - 1, 2], [M32] * (1 << 20), [INT64_MAX] * (1 << 20)]
    rng = np.random.default_rng(3)
    for _ in range(200):
        cases.append([int(x) for x in rng.integers(1, 1 << int(rng.integers(1, 63)), int(rng.integers(1, 9)))])
    for ns in cases:
        assert split_sum(ns) == total(ns), ns[:4]
    assert total([1 << 62, 1 << 62]) == INT64_MAX and total([(1 << 62) - 1, 1 << 62]) == INT64_MAX
    assert total([(1 << 62) - 1, (1 << 62) - 1]) == INT64_MAX - 1
    # neither sum overflows 64 bits at the largest call
    assert (1 << 20) * M32 < 1 << 64 and (1 << 20) * (INT64_MAX >> 32) < 1 << 64


def test_nokey_stores_nothing():
    sim = new_sim(0, [(1, 20, 12 * NS), (3, 5, 2 * NS)])
    sim.decide(1, T0, 3, 0)
    sim.decide(2, T0, 3, 1)
    before = copy.deepcopy(sim.db)
    late = T0 + 3600 * NS
    st, info = apply_refunds(sim, [1, 2, 7, 8], [late, late, T0, T0], [1, 1, 1, 1], [0, 1, 0, 1])
    assert st.tolist() == [NOKEY] * 4 and len(info["expired"]) == 1     # key 2's window at `late` never was
    st, info = apply_refunds(sim, [2], [T0], [1], [1], [late // 1_000_000])
    assert st.tolist() == [NOKEY] and len(info["expired"]) == 1
    assert sim.db == before
