"""The smallest segments the chain takes (GPU): single-key traces, bit for bit
against the CPU oracle on both profiles.

  4096          huge_min: one full window plus a 1792-request partial one (five tiles)
  2304 * 2 + 1  a one-request last window
  2304 * 3 + 17 several full windows plus a short one
each with deny-only, allow-heavy and mixed gaps (as test_gpu_parity._chain_trace),
one trace whose tokens cross 0.1 and 1.0 inside a window (the exit guess's
decade, speculative restart, the multi-decade windows' plan hand-off), and one
segment split over two batches (the chain's LDS state in a fresh launch).  The
single-workgroup path is off, so a 4096-request batch reaches the chain; word
[6] of the debug words (chain segments started) says that it did."""
import numpy as np
import pytest

from test_gpu_parity import run_both, split
from tracegen import NS, T0

pytestmark = pytest.mark.gpu

CONFIGS = [(1, 20, 12 * NS), (1, 10, NS), (1, 3, 300_000_000)]
CH_W = 2304   # requests per chain window (6 tiles of 384)


def _trace(kind, seed, m):
    """One key, m requests: the gap and n distributions of _chain_trace."""
    rng = np.random.default_rng(seed)
    if kind == "deny":        # 8 us gaps against 20 tokens / 12 s
        key, gaps, n = 0, np.rint(rng.exponential(8_000, m)), np.ones(m, np.int64)
    elif kind == "allow":     # 10/s with 15 ms gaps: allows mixed with denials
        key, gaps, n = 1, np.rint(rng.exponential(15_000_000, m)), rng.choice([1, 1, 1, 2], m).astype(np.int64)
    elif kind == "mixed":     # bursts of zero gaps, rare long gaps, huge n
        key = 1
        gaps = rng.choice([0, 1, 1000, 90_000, 400_000_000], m, p=[0.2, 0.2, 0.3, 0.29, 0.01])
        n = rng.choice([1, 1, 1, 2, 7], m).astype(np.int64)
        n[rng.random(m) < 0.001] = 1 << 62
    else:                     # "cross": 10/s, ~100 us gaps: 0 -> 0.1 -> 1.0 -> allow, about once per window
        key, gaps, n = 1, np.rint(rng.exponential(100_000, m)), np.ones(m, np.int64)
    ts = T0 + np.cumsum(gaps).astype(np.int64)
    return np.full(m, key, np.uint64), ts, n, np.full(m, key % 3, np.uint32), None


def _run(rl, profile, trace, sizes, monkeypatch):
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    eng, _ = run_both(rl, profile, CONFIGS, split(trace, sizes), tb=1 << 12, win=1 << 12, max_batch=1 << 14)
    try:
        assert int(eng.debug_words()[6]) >= 1, "the last batch's segment did not take the chain"
    finally:
        eng.close()


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["deny", "allow", "mixed"])
@pytest.mark.parametrize("m", [4096, 2 * CH_W + 1, 3 * CH_W + 17])
def test_smallest_chain_segments(rl, profile, kind, m, monkeypatch):
    seed = 4000 + 100 * ["deny", "allow", "mixed"].index(kind) + 10 * profile + m % 7
    _run(rl, profile, _trace(kind, seed, m), [m], monkeypatch)


@pytest.mark.parametrize("profile", [0, 1])
def test_tokens_cross_decades_inside_windows(rl, profile, monkeypatch):
    m = 3 * CH_W + 500
    _run(rl, profile, _trace("cross", 4700 + profile, m), [m], monkeypatch)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["deny", "cross"])
def test_segment_split_over_two_batches(rl, profile, kind, monkeypatch):
    h = 2 * CH_W + 100
    _run(rl, profile, _trace(kind, 4800 + profile, 2 * h), [h, h], monkeypatch)
