"""HIP engine vs CPU oracle on the directed chain traces (chain_cases.py), bit
for bit, on both profiles (GPU).

One engine and one oracle per test, a key id of its own per case.  The tests
whose names contain `witness` also read the engine's per-batch debug words
after the batch under test and assert, coarsely, that the chain took the path
the case was built for (words as named in csrc/rl_tb_chain.h):
  [1] near / exact passes     [3] windows resolved in full   [6] chain segments
  [20] one-decade tiles replayed exactly   [21] serial exact steps
  [60] multi-decade windows resolved   [64] / [65] windows summarized
  multi-decade / one-decade.
A variant build without one of these paths deselects them with
-k "not witness"."""
import numpy as np
import pytest

import chain_cases as cc
import oracle
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


class Pair:
    """The engine and the C oracle with chain_cases.CONFIGS registered."""

    def __init__(self, rl, profile):
        self.eng = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 16)
        self.sim = oracle.OracleSim(profile)
        for i, (a, lim, win) in enumerate(cc.CONFIGS):
            assert self.eng.register(a, lim, win) == self.sim.add_config(a, lim, win) == i

    def run(self, case):
        """Every batch of the case against the oracle; the debug words of the
        batch under test."""
        for i, (key, ts, n, cfg, sms) in enumerate(case.batches):
            res = self.eng.decide(key, ts, n, cfg, sms)
            ref = self.sim.decide(key, ts, n, cfg, sms)
            assert_same(res, ref, cc.CONFIGS, cfg, what=f"{case.name} batch {i}")
        return self.eng.debug_words().astype(np.int64)

    def close(self):
        self.eng.close()


def _cases(family, pick=lambda c: True):
    return [c for c in cc.all_cases()[family] if pick(c) and not c.small_max0]


def _run_all(rl, profile, cases):
    p = Pair(rl, profile)
    try:
        return [(c, p.run(c)) for c in cases]
    finally:
        p.close()


# --- parity -------------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", list(cc.EDGE_KINDS) + ["absent"])
def test_edge_events(rl, profile, kind):
    _run_all(rl, profile, _cases("a", lambda c: c.claim["kind"] == kind))


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("family", list("bcdef"))
def test_directed_families(rl, profile, family):
    _run_all(rl, profile, _cases(family))


@pytest.mark.parametrize("profile", [0, 1])
def test_even_lengths_without_small_path(rl, profile, monkeypatch):
    """The even segment lengths with the single-workgroup path off: a batch
    of one key with exactly 4096 requests reaches the chain."""
    _even_lengths(rl, profile, monkeypatch)


def _even_lengths(rl, profile, monkeypatch):
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    cases = [c for c in cc.all_cases()["f"] if c.name.startswith("lengths-even")]
    assert any(c.small_max0 for c in cases)
    return _run_all(rl, profile, cases)


# --- witnesses ------------------------------------------------------------------------

def _need(w, case, i, lo, what):
    assert w[i] >= lo, f"{case.name}: debug word [{i}] = {w[i]} < {lo}: {what}"


@pytest.mark.parametrize("profile", [0, 1])
def test_edge_events_witness(rl, profile):
    for case, w in _run_all(rl, profile, _cases("a")):
        _need(w, case, 6, 1, "no chain segment ran")
        if case.claim["o"] >= cc.CH_W:
            _need(w, case, 3, 1, "no window resolved in full before the event")
        if case.claim["kind"] in ("allow", "clamp_allow", "clamp_deny", "expiry", "absent"):
            _need(w, case, 21, 1, "no serial exact step")


@pytest.mark.parametrize("profile", [0, 1])
def test_bursts_witness(rl, profile):
    for case, w in _run_all(rl, profile, _cases("b")):
        _need(w, case, 6, 1, "no chain segment ran")
        _need(w, case, 21, case.claim["B"], "fewer serial exact steps than allows")


def test_density_witness(rl):
    for case, w in _run_all(rl, 0, _cases("c")):
        _need(w, case, 6, 1, "no chain segment ran")
        _need(w, case, 3, 1, "no window resolved in full")
        _need(w, case, 65, 1, "no one-decade window summarized")
        _need(w, case, 1, 1, "no near pass")
        assert w[64] == 0, f"{case.name}: {w[64]} multi-decade windows in a one-decade trace"
        if case.name in ("near-65", "near-384", "band-65"):
            _need(w, case, 20, 1, "the overflowing tile was not replayed exactly")
        if case.name == "band-64":
            # a full near list of steps that resolve to their nominal results, and
            # no step that can leave the regime: every tile commits from its summary
            assert w[20] == 0, f"{case.name}: {w[20]} tiles replayed exactly, none has more than {cc.CH_NE} near steps"


def test_even_lengths_witness(rl, monkeypatch):
    for case, w in _even_lengths(rl, 0, monkeypatch):
        _need(w, case, 6, len(case.claim["counts"]), "a segment of 4096 or more did not take the chain")


@pytest.mark.parametrize("profile", [0, 1])
def test_skew_magnitude_lengths_witness(rl, profile):
    for fam in "def":
        for case, w in _run_all(rl, profile, _cases(fam)):
            _need(w, case, 6, 1, "no chain segment ran")
            if fam == "d" and profile == 0:
                _need(w, case, 64, 1, "no multi-decade window summarized")
                _need(w, case, 60, 1, "no multi-decade window resolved")
            if case.name == "magnitude-one-decade" and profile == 0:
                # one-decade windows resolved in full: tiles whose sums came from the
                # int64 scan were committed
                _need(w, case, 3, 1, "no window resolved in full")
                assert w[64] == 0, f"{case.name}: {w[64]} multi-decade windows in a one-decade trace"
