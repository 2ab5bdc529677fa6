"""The directed window traces (window_cases.py) on the CPU: every case's
predicate holds on the Python oracle's per-request record -- the trace contains
what it was built for -- and the C oracle, which the GPU tests compare against,
agrees with the Python oracle bit for bit on every batch, on both profiles.
The straddle sets of family s are re-derived by their searches, and variants of
the weighted-count arithmetic that differ from the reference by a rounding
(the mutants below) must each change a visible result on both sets."""
from fractions import Fraction

import numpy as np
import pytest

import window_cases as wc


@pytest.fixture(scope="module")
def c_sims(oracle_mod):
    sims = []
    for profile in (0, 1):
        sim = oracle_mod.OracleSim(profile)
        for i, c in enumerate(wc.CONFIGS):
            assert sim.add_config(*c) == i
        sims.append(sim)
    return sims


def _same(py, c, what):
    for name, a, b in zip(("decision", "remaining", "retry", "reset_at"), py, c):
        assert np.array_equal(a, b), f"{what}: {name} differs"


@pytest.mark.parametrize("family", list("gbsc"))
def test_predicates_and_oracle_agreement(c_sims, family):
    for case in wc.all_cases()[family]:
        for profile in (0, 1):
            rec = wc.replay(case, profile)
            wc.check(case, rec, profile)
            for i, b in enumerate(case.batches):
                _same(rec.out[i], c_sims[profile].decide(*b), f"{case.name} profile {profile} batch {i}")


def test_case_inventory():
    """Every offset, run length and segment length the suite promises is there."""
    cases = wc.all_cases()
    assert len(wc.CONFIGS) <= 32          # the replay kernels' variant for up to 32 configs, as the flagship runs
    two = {(c.claim["cfg"], c.claim["runs"][0] - 1) for c in cases["g"] if c.claim["kind"] == "two-runs"}
    assert two == {(cfg, r) for cfg in (wc.FW_HI, wc.SW_HI, wc.FW_LO, wc.SW_LO)
                   for r in (0, 1, 5, 6, 7, 383, 384, 385, 768, 769)}
    lengths = {(c.claim["cfg"], sum(c.claim["runs"])) for c in cases["g"] if c.claim["kind"] == "length"}
    assert lengths == {(cfg, n) for cfg in (wc.FW_HI, wc.SW_HI) for n in (31, 32, 33, 4096, 4097)}
    assert {c.claim["kind"] for c in cases["g"]} == {"two-runs", "new-windows", "length", "dad"}
    at = {}
    for c in cases["b"]:
        at.setdefault((c.claim["kind"], c.claim["check"]), set()).add(c.claim["o"])
    offs = {1, 6, 383, 384, 385}
    assert at[("overflow", "overflow")] == at[("ttl", "ttl-reset")] == at[("ttl", "expired")] == offs
    assert at[("expire", "expired")] == at[("prev-spill", "prev-spill")] == offs
    assert at[("overflow", "first-error")] == at[("ttl0", "ttl_c")] == {0} and ("half", "expired") in at
    ttl0 = {wc.CONFIGS[c.claim["cfg"]][2] for c in cases["b"] if c.claim["kind"] == "ttl0"}
    assert ttl0 == {300_000_000, 700_000_000}
    before = {(c.claim["before"], c.claim["reset"]) for c in cases["b"] if c.claim["kind"] == "ttl"}
    assert before == {(512, True), (513, False), (1, True), (2, False)}
    assert {c.claim["kind"] for c in cases["c"]} == {"carried", "spilled", "run"}
    keys = [k for fam in cases.values() for c in fam for k in np.unique(c.test_batch[0]).tolist()]
    assert len(keys) == len(set(keys))          # key ids of its own per case
    for fam in cases.values():
        for c in fam:
            assert all(len(b[1]) <= wc.SMALL_MAX + 1 for b in c.batches)
            assert c.small_max0 == (len(c.test_batch[1]) == wc.SMALL_MAX)
    # runs: one heavy segment in one chunk, and one that spans chunks
    ps = [p for _, _, p in wc.S_RUNS]
    assert all(33 <= p <= 769 and p != 385 for p in ps) and min(ps) <= 384 and max(ps) >= 386
    assert 200 <= len(wc.S_LIGHT) <= 500


def test_straddle_sets_are_the_searches_results():
    assert wc.S_LIGHT == wc.search_light()
    assert wc.S_RUNS == wc.search_runs()


# --- the weighted count: reference arithmetic and mutants --------------------------------

def fused(p, el, W, cc):
    """fma(p, 1 - progress, cc): the product is not rounded before the sum"""
    one_minus = 1.0 - float(el) / float(W)
    return float(Fraction(float(p)) * Fraction(one_minus) + cc)


def reciprocal(p, el, W, cc):
    """elapsed * (1 / W) for elapsed / W"""
    progress = float(el) * (1.0 / float(W))
    return float(p) * (1.0 - progress) + float(cc)


def distributed(p, el, W, cc):
    """p - p * progress for p * (1 - progress)"""
    progress = float(el) / float(W)
    return (float(p) - float(p) * progress) + float(cc)


def progress_f32(p, el, W, cc):
    progress = float(np.float32(float(el) / float(W)))
    return float(p) * (1.0 - progress) + float(cc)


def complement_f32(p, el, W, cc):
    one_minus = float(np.float32(1.0 - float(el) / float(W)))
    return float(p) * one_minus + float(cc)


MUTANTS = [fused, reciprocal, distributed, progress_f32, complement_f32]
SETS = {"light": wc.light_points, "run": wc.all_run_points}


@pytest.mark.parametrize("which", list(SETS))
def test_reference_lands_on_both_sides(which):
    pts = SETS[which]()
    sides = wc.side_counts([q[:4] for q in pts])
    print(which, len(pts), "points; reference below / on / above the integer:", sides[-1], sides[0], sides[1])
    assert min(sides.values()) >= 3, sides


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__)
def test_mutant_is_caught(which, mutant):
    """The mutant changes the decision or `remaining` on at least 3 requests."""
    caught = sum(1 for *q, L in SETS[which]() if wc.visible(mutant(*q), L) != wc.visible(wc.weighted(*q), L))
    print(f"{mutant.__name__} on the {which} set: caught at {caught} requests")
    assert caught >= 3


def test_c_oracle_weighted_is_the_reference_arithmetic(oracle_mod):
    lib = oracle_mod.c_oracle()
    for p, el, W, cc, _ in wc.light_points() + wc.all_run_points():
        ws = 1_760_000_000
        got = lib.rlo_sw_weighted(ws * wc.NS + el, ws, W, p, cc)
        assert got == wc.weighted(p, el, W, cc), (p, el, W, cc)

