"""hot_cases.HotModel, the numpy restatement of the top keys, checked on the CPU:
against a brute-force sketch, and for the properties a count-min sketch with a
candidate set must have on the traces the GPU tests use."""
import numpy as np
import pytest

import hot_cases as H
from table_cases import mix64

U64 = np.uint64


def test_mix64_and_columns():
    # splitmix64's finaliser: mix64(0) == 0, and a published value of the generator's first output
    assert int(mix64(0)[0]) == 0
    assert int(mix64(0x9e3779b97f4a7c15)[0]) == 0xe220a8397b1dcdaf
    keys = np.array([0, 1, 77, (1 << 64) - 2], U64)
    cols = H.columns(keys, 1 << 10)
    assert cols.shape == (4, 4) and cols.min() >= 0 and cols.max() < 1 << 10
    for r in range(4):
        salt = int(mix64(r + 1)[0])
        assert cols[r].tolist() == [int(mix64(int(k) ^ salt)[0]) & 1023 for k in keys.tolist()]
    assert len({tuple(c) for c in cols.tolist()}) == 4          # the rows hash differently


@pytest.mark.parametrize("weight", [H.REQUESTS, H.UNITS])
def test_sketch_against_brute_force(weight):
    calls = H.zipf_calls(seed=5, sizes=(700, 333), ids=200)
    calls[0][2][::7] = -2                                       # n <= 0: skipped in units mode only
    mod = H.model_of(calls, 64, 20, weight=weight)
    assert mod.sketch.tolist() == H.brute_sketch(calls, 64, H.NCFG, weight)
    ok = [H.counted_mask(*c, H.NCFG, weight) for c in calls]
    assert mod.skipped == sum(int((~o).sum()) for o in ok) > 0
    assert mod.requests == 1033 and mod.batches == 2
    if weight == H.UNITS:
        assert mod.total == sum(int(c[2][o].sum()) for c, o in zip(calls, ok))
    else:
        assert mod.total == sum(int(o.sum()) for o in ok)
    assert int(mod.sketch[0].sum()) == int(mod.sketch[3].sum()) == mod.total


@pytest.mark.parametrize("width", [16, 64, 1 << 16])
def test_zipf_trace_properties(width):
    """no estimate below the true weight; every key whose true weight reaches
    hot_min is a candidate; false positives at width 64, none at 2^16"""
    mod = H.model_of(H.zipf_calls(), width, H.ZIPF_HOT_MIN)
    ks = sorted(mod.true)
    est = mod.estimate(ks).tolist()
    assert all(e >= mod.true[k] for k, e in zip(ks, est))
    hot, cand = mod.true_hot(), set(mod.candidates)
    assert len(hot) >= 5 and hot <= cand
    assert all(e >= H.ZIPF_HOT_MIN for _, e in mod.read())      # adds only: an estimate never falls
    if width == 64:
        assert len(cand - hot) >= 1
    if width == 1 << 16:
        assert cand == hot
        assert all(e == mod.true[k] for k, e in mod.read())
    if width == 16:
        assert len(cand) > 20 * len(hot)


def test_candidate_from_the_call_it_gets_there():
    """a key enters in the call that leaves its estimate at hot_min, not before;
    a key without a request in a call is not looked at in it"""
    a, b = 1001, 1002
    assert H.distinct_columns([a, b], 1 << 16)
    mod = H.HotModel(1 << 16, 10, 1)
    mod.call([a] * 9 + [b] * 10, [0] * 19, [1] * 19, [1] * 19)
    assert set(mod.candidates) == {b}
    mod.call([b], [0], [1], [0])
    assert set(mod.candidates) == {b}
    mod.call([a], [0], [1], [2])
    assert mod.read() == [(b, 11), (a, 10)]
    mod.clear()
    assert mod.read() == [] and not mod.sketch.any() and mod.total == 0


def test_collision_makes_a_false_positive():
    """two keys that share all four counters at width 16 (found by search):
    the light one is a candidate with the heavy one's weight"""
    keys = np.arange(1, 200000, dtype=U64)
    cols = H.columns(keys, 16)
    same = np.nonzero((cols == cols[:, :1]).all(axis=0))[0]
    assert same.size >= 2
    heavy, light = int(keys[same[0]]), int(keys[same[1]])
    mod = H.HotModel(16, 50, 1)
    mod.call([heavy] * 60 + [light], [0] * 61, [1] * 61, [1] * 61)
    assert mod.read() == sorted([(heavy, 61), (light, 61)], key=lambda x: (-x[1], x[0]))
    assert mod.true_hot() == {heavy}
