"""The directed chain traces (chain_cases.py) on the CPU: every case's predicate
holds on the Python oracle's per-step record -- the trace contains what it was
built for -- and the C oracle, which the GPU tests compare against, agrees
with the Python oracle bit for bit on every batch, on both profiles."""
import numpy as np
import pytest

import chain_cases as cc


@pytest.fixture(scope="module")
def c_sims(oracle_mod):
    sims = []
    for profile in (0, 1):
        sim = oracle_mod.OracleSim(profile)
        for i, c in enumerate(cc.CONFIGS):
            assert sim.add_config(*c) == i
        sims.append(sim)
    return sims


def _same(py, c, what):
    for name, a, b in zip(("decision", "remaining", "retry", "reset_at"), py, c):
        assert np.array_equal(a, b), f"{what}: {name} differs"
    assert np.array_equal(py[4].view(np.uint64), c[4].view(np.uint64)), f"{what}: tokens differ"


@pytest.mark.parametrize("family", list("abcdef"))
def test_predicates_and_oracle_agreement(c_sims, family):
    for case in cc.all_cases()[family]:
        for profile in (0, 1):
            rec = cc.replay(case, profile)
            # the density cases are defined for the Redis-7 profile alone
            # (near steps of its 14-digit decades)
            if profile == 0 or family != "c":
                cc.check(case, rec)
            for i, b in enumerate(case.batches):
                _same(rec.out[i], c_sims[profile].decide(*b), f"{case.name} profile {profile} batch {i}")


def test_case_inventory():
    """Every offset, burst length and segment length the suite promises is there."""
    cases = cc.all_cases()
    edges = {(c.claim["kind"], c.claim["o"]) for c in cases["a"]}
    assert edges == {(k, o) for k in cc.EDGE_KINDS for o in cc.EDGE_OFFSETS} | {("absent", 0)}
    assert set(cc.EDGE_OFFSETS) == {0, 1, 5, 6, 383, 384, 385, 2303, 2304, 2305, 4607, cc.L - 1}
    bursts = {(c.claim["start"], c.claim["B"]) for c in cases["b"]}
    assert bursts == {(s, b) for s in (0, cc.CH_W - 32) for b in (63, 64, 65, 129)} | {(0, cc.L)}
    lengths = sorted(n for c in cases["f"] for n in c.claim["counts"].values())
    assert set(lengths) >= {4097, 4607, 4609, 4991, 4993, 6911, 6913, 8191, 8193, 4096, 4608, 4992, 6912, 8192,
                            31, 32, 33, 4095}
    keys = [k for fam in cases.values() for c in fam for k in np.unique(c.test_batch[0]).tolist()]
    assert len(keys) == len(set(keys))          # a key id of its own per case
    for fam in cases.values():
        for c in fam:
            m = c.test_batch[0].size
            assert cc.L <= m <= 41_000 or c.small_max0
