"""table_cases.py on the CPU: the hash restatements, the ids chosen by home
slot, and the spill load of ladder_trace on both oracles.  These are what puts
the cases of test_table_pressure_gpu.py inside or outside a table's capacity by
construction, not by the code under test."""
import numpy as np
import pytest

import oracle
from oracle import rl_oracle_py as po
from table_cases import home, keys_with_home, ladder_trace, mix64, one_key_per_home, spill_demand, spill_home
from tracegen import NS, T0

LADDER_CONFIGS = [(3, 5, 60 * NS), (2, 5, 60 * NS)]
D = 6


def test_mix64_is_the_splitmix64_finaliser():
    # splitmix64's first output for seed 0: the finaliser of the golden-ratio increment
    assert int(mix64(0x9E3779B97F4A7C15)[0]) == 0xE220A8397B1DCDAF
    # vectorised, input untouched, and the scalar form of rl_table.h in Python integers
    x = np.array([0, 1, 2 ** 63, 2 ** 64 - 2, 0x9E3779B97F4A7C15], np.uint64)
    keep = x.copy()

    def ref(v):
        M = (1 << 64) - 1
        v ^= v >> 30
        v = v * 0xbf58476d1ce4e5b9 & M
        v ^= v >> 27
        v = v * 0x94d049bb133111eb & M
        return v ^ v >> 31

    assert [int(v) for v in mix64(x)] == [ref(int(v)) for v in keep]
    assert np.array_equal(x, keep)
    assert [int(v) for v in spill_home(x, 1023)] == [ref(int(v) ^ 0x5bd1e9955bd1e995) & 1023 for v in keep]
    assert [int(v) for v in home(x, (1 << 14) - 1)] == [ref(int(v)) & 16383 for v in keep]


@pytest.mark.parametrize("spill", [False, True])
@pytest.mark.parametrize("slot", [0, 517, 1023])
def test_keys_with_home(slot, spill):
    mask = 1023
    ids = keys_with_home(mask, slot, 600, spill=spill)
    assert ids.size == 600 and ids.dtype == np.uint64
    assert (np.diff(ids.astype(np.int64)) > 0).all()         # distinct, ascending
    assert int(ids[-1]) < 700_000
    fn = spill_home if spill else home
    assert (fn(ids, mask) == slot).all()
    # the first ones: no id below the last was left out
    below = np.arange(int(ids[-1]) + 1, dtype=np.uint64)
    assert int((fn(below, mask) == slot).sum()) == 600
    more = keys_with_home(mask, slot, 5, spill=spill, start=int(ids[-1]) + 1)
    assert int(more[0]) > int(ids[-1]) and (fn(more, mask) == slot).all()


@pytest.mark.parametrize("mask,start,length", [(1023, 1000, 100), (1023, 1023, 1), (1023, 0, 1024),
                                               ((1 << 14) - 1, (1 << 14) - 4000, 8193)])
def test_one_key_per_home(mask, start, length):
    ids = one_key_per_home(mask, start, length)
    assert ids.size == length and np.unique(ids).size == length
    want = (start + np.arange(length)) & mask
    assert np.array_equal(home(ids, mask).astype(np.int64), want)
    if start + length > mask + 1:
        assert want[-1] < want[0]                            # the range wraps past the last slot


def _run(sim, tr, py):
    if py:
        rows = [sim.decide(int(k), int(t), int(n), int(c), int(s)) for k, t, n, c, s in zip(*tr)]
        return np.array([r[0] for r in rows])
    return sim.decide(*tr)[0]


@pytest.mark.parametrize("K,rounds,py", [(200, 8, False), (250, 8, False), (256, 8, False), (300, 8, False),
                                         (256, 4, False), (200, 4, True)])
def test_ladder_spill_demand(K, rounds, py):
    """Every user key of the ladder owns D live window keys at the end: K * (D - 2)
    of them are beyond the two of an entry.  With 8 rounds a third of the trace
    has touched 1 - (2/3)^8 = 96 % of the (key, skew) pairs, so the demand is
    then past 80 % of that.  With limit 5 both decisions occur."""
    sim = po.Sim(0) if py else oracle.OracleSim(0)
    for a, L, W in LADDER_CONFIGS:
        sim.add_config(a, L, W)
    tr = ladder_trace(7, K, D, rounds, LADDER_CONFIGS)
    m = tr[0].size
    assert m == K * D * rounds
    assert (np.diff(tr[4]) >= 0).all()                       # the store clock is monotone
    assert np.unique(tr[0]).size == K and set(np.unique(tr[2])) == {1, 2, 3}
    third = tuple(x[:m // 3] for x in tr)
    rest = tuple(x[m // 3:] for x in tr)
    dec = [_run(sim, third, py)]
    if rounds == 8:
        assert spill_demand(sim, int(third[4][-1])) > 0.8 * K * (D - 2)
    dec.append(_run(sim, rest, py))
    assert spill_demand(sim, int(tr[4][-1])) == K * (D - 2)
    dec = np.concatenate(dec)
    assert (dec == po.ALLOWED).any() and (dec == po.DENIED).any() and (dec <= 1).all()


def test_ladder_explicit_ids_and_start():
    ids = keys_with_home(1023, 1023, 40, spill=True)
    t0 = T0 + 30 * NS
    tr = ladder_trace(2, 40, D, 2, LADDER_CONFIGS, span_s=4, t0=int(t0), ids=ids)
    assert set(tr[0].tolist()) == set(ids.tolist())
    assert np.array_equal(tr[3], (tr[0] % np.uint64(2)).astype(np.uint32))
    assert tr[4][0] >= t0 // 1_000_000 and tr[4][-1] < t0 // 1_000_000 + 4000
    # every (key, skew) pair occurs `rounds` times
    skew = (tr[4] * 1_000_000 + 999_999 - tr[1]) // (60 * NS)
    pairs, counts = np.unique(np.stack([tr[0].astype(np.int64), skew]), axis=1, return_counts=True)
    assert pairs.shape[1] == 40 * D and (counts == 2).all()
