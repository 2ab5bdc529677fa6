"""tally_cases.py on the CPU: the numpy reference against the brute-force one,
and the table helpers that put the GPU cases inside or outside the key table by
construction."""
import numpy as np
import pytest

from table_cases import home, keys_with_home, one_key_per_home
from tally_cases import (KEY_RESERVED, PROBES, brute_tally, expected_tally, fill, fits, host_table)

U64 = np.uint64


def same(a, b):
    assert np.array_equal(a.count, b.count) and np.array_equal(a.units, b.units)
    assert (a.unknown_cfg, a.bad_codes, a.reserved) == (b.unknown_cfg, b.bad_codes, b.reserved)
    assert a.keys == b.keys


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_expected_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    m, ncfg = 4000, 7
    key = rng.integers(0, 60, m).astype(U64)
    key[rng.random(m) < 0.02] = U64(KEY_RESERVED)
    cfg = rng.integers(0, ncfg + 2, m).astype(np.uint32)
    cfg[rng.random(m) < 0.01] = 0xffffffff
    n = rng.choice([1, 2, 7, 0, -5, 1 << 62, (1 << 63) - 1], m).astype(np.int64)
    dec = rng.choice([0, 0, 1, 1, 2, 3, 4, 255], m).astype(np.uint8)
    a, b = expected_tally(key, cfg, n, dec, ncfg), brute_tally(key, cfg, n, dec, ncfg)
    same(a, b)
    assert a.unknown_cfg > 0 and a.bad_codes > 0 and a.reserved[0] > 0
    assert (a.units >= U64(1 << 62)).any()            # sums that wrapped or nearly did
    assert int(a.count.sum()) + a.unknown_cfg + a.bad_codes == m
    assert a.denied == int(a.count[:, 0].sum())
    # any split into batches adds up: the tally is a sum
    h = m // 3
    p, q = expected_tally(key[:h], cfg[:h], n[:h], dec[:h], ncfg), expected_tally(key[h:], cfg[h:], n[h:], dec[h:], ncfg)
    with np.errstate(over="ignore"):
        assert np.array_equal(p.count + q.count, a.count) and np.array_equal(p.units + q.units, a.units)


def test_wrap():
    e = expected_tally(np.arange(5), np.zeros(5), np.full(5, 1 << 62), np.ones(5), 1)
    assert int(e.units[0, 1]) == (5 << 62) % (1 << 64) == 1 << 62
    same(e, brute_tally(np.arange(5), np.zeros(5), np.full(5, 1 << 62), np.ones(5), 1))


def test_fits_and_fill():
    # 8 keys of one home slot in 16 slots: one run of 8
    ks = keys_with_home(15, 5, 8)
    assert (home(ks, 15) == U64(5)).all()
    occ = fill(ks, 16)
    assert occ.sum() == 8 and occ[5:13].all()
    assert fits(ks, 16)
    assert host_table(ks, 16) == set(ks.tolist())
    # a run that wraps round the end of the table
    ks = keys_with_home(15, 14, 4)
    assert np.nonzero(fill(ks, 16))[0].tolist() == [0, 1, 14, 15] and fits(ks, 16)
    # more keys than slots never fit; a full table of at most PROBES slots does
    assert not fits(np.arange(17), 16)
    assert fits(one_key_per_home(15, 0, 16), 16)
    # 65 keys of one home slot in 1024 slots: the run is longer than the probe
    # bound, so the last key to come finds no slot
    ks = keys_with_home(1023, 100, PROBES + 1)
    assert fill(ks, 1024).sum() == PROBES + 1 and not fits(ks, 1024)
    assert fits(ks[:PROBES], 1024)
    assert host_table(ks, 1024) == set(ks[:PROBES].tolist())
    # the occupied set does not depend on the order
    rng = np.random.default_rng(4)
    ks = rng.integers(0, 1 << 40, 700).astype(U64)
    assert np.array_equal(fill(ks, 1024), fill(ks[rng.permutation(700)], 1024))
    # the reserved key id is never tracked
    assert host_table([KEY_RESERVED, 3], 16) == {3}
