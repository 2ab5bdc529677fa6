"""HIP engine vs CPU oracle on the directed window traces (window_cases.py):
all four outputs bit for bit, on both profiles (GPU).

One engine and one oracle per test, key ids of its own per case.  Every family
runs through the launch paths that reach the window replay:
  * k_small (batches up to 4096 requests; the 4097 case takes the full sequence);
  * the full launch sequence (RL_SMALL_MAX=0): replay_rest under k_tb_chain;
  * the full sequence with RL_HEAVY_MIN above every segment length, where every
    segment is replayed serially (replay_win_serial).  The wave shortcut and
    the serial replay must both equal the oracle, so a disagreement tells which
    of wave_win_segment and fw_step / sw_step is wrong;
  * once, k_replay_light: every case interleaved into one batch of more than
    2^19 requests over uniform light keys.
Engine.stats() and the debug words count cooperative token-bucket segments
only (last_heavy), so no counter witnesses the heavy window segments: that a
case reaches the path it was built for is stated by window_cases.plan and by
the RL_HEAVY_MIN A/B above.

Peek's copy of the weighted count is pinned on the light-shape straddles."""
import numpy as np
import pytest

import oracle
import window_cases as wc
from test_gpu_parity import assert_same
from test_peek_gpu import Rig

pytestmark = pytest.mark.gpu

FAMILIES = list("gbsc")
SERIAL_HEAVY_MIN = 1 << 16          # above every segment length of the cases (at most 4097)


class Pair:
    """The engine and the C oracle with window_cases.CONFIGS registered."""

    def __init__(self, rl, profile, win=1 << 14, max_batch=1 << 16):
        self.eng = rl.Engine(profile=profile, tb_capacity=1 << 10, win_capacity=win, max_batch=max_batch)
        self.sim = oracle.OracleSim(profile)
        for i, (a, lim, win_ns) in enumerate(wc.CONFIGS):
            assert self.eng.register(a, lim, win_ns) == self.sim.add_config(a, lim, win_ns) == i

    def decide(self, batch, what):
        key, ts, n, cfg, sms = batch
        assert_same(self.eng.decide(key, ts, n, cfg, sms), self.sim.decide(key, ts, n, cfg, sms), wc.CONFIGS, cfg,
                    what=what)

    def run(self, case):
        for i, b in enumerate(case.batches):
            self.decide(b, f"{case.name} batch {i}")

    def close(self):
        self.eng.close()


def _run_family(rl, profile, family):
    p = Pair(rl, profile)
    try:
        for case in wc.all_cases()[family]:
            p.run(case)
    finally:
        p.close()


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_small_path(rl, profile, family, monkeypatch):
    monkeypatch.setenv("RL_SMALL_MAX", str(wc.SMALL_MAX))
    _run_family(rl, profile, family)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_full_sequence(rl, profile, family, monkeypatch):
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    _run_family(rl, profile, family)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("family", FAMILIES)
def test_full_sequence_serial_only(rl, profile, family, monkeypatch):
    assert SERIAL_HEAVY_MIN > max(len(c.test_batch[1]) for fam in wc.all_cases().values() for c in fam)
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    monkeypatch.setenv("RL_HEAVY_MIN", str(SERIAL_HEAVY_MIN))
    _run_family(rl, profile, family)


# --- k_replay_light ---------------------------------------------------------------------

LIGHT_M = 1 << 19
LIGHT_KEY0, LIGHT_KEYS = 1 << 40, 200_000       # ~2.6 requests per key and batch: no segment reaches HEAVY_MIN


def _uniform(rng, m, t0):
    key = (LIGHT_KEY0 + rng.integers(0, LIGHT_KEYS, m)).astype(np.uint64)
    ts = t0 + np.cumsum(rng.integers(0, 40_000, m)).astype(np.int64)
    return key, ts, np.ones(m, np.int64), (key % np.uint64(len(wc.CONFIGS))).astype(np.uint32), ts // wc.MS


def _interleave(rng, parts):
    """One batch of the parts' requests at random positions; each part keeps
    its own order (a key's requests lie in one part)."""
    sizes = [len(p[1]) for p in parts]
    total = sum(sizes)
    pos = rng.permutation(total)
    out = (np.empty(total, np.uint64), np.empty(total, np.int64), np.empty(total, np.int64), np.empty(total, np.uint32),
           np.empty(total, np.int64))
    o = 0
    for (key, ts, n, cfg, sms), s in zip(parts, sizes):
        at = np.sort(pos[o:o + s])
        o += s
        for dst, src in zip(out, (key, ts, n, cfg, ts // wc.MS if sms is None else sms)):
            dst[at] = src
    return out


@pytest.mark.parametrize("profile", [0, 1])
def test_light_replay(rl, profile):
    """Every case's batch under test, interleaved into one batch that the
    engine replays with k_replay_light (the recipe of
    test_gpu_parity.test_light_replay_and_misprediction: a large batch without
    a huge segment comes first)."""
    cases = [c for fam in wc.all_cases().values() for c in fam]
    rng = np.random.default_rng(19)
    p = Pair(rl, profile, win=1 << 20, max_batch=1 << 20)
    try:
        for c in cases:
            for i, b in enumerate(c.batches[:-1]):
                p.decide(b, f"{c.name} batch {i}")
        first = _uniform(rng, LIGHT_M, wc.T0)
        p.decide(first, "uniform batch")
        batch = _interleave(rng, [c.test_batch for c in cases] + [_uniform(rng, LIGHT_M, int(first[1][-1]))])
        assert np.unique(batch[0][batch[0] < LIGHT_KEY0]).size == sum(np.unique(c.test_batch[0]).size for c in cases)
        before = p.eng.stats().light_batches
        p.decide(batch, "the batch that carries the cases")
        assert p.eng.stats().light_batches - before == 1
    finally:
        p.close()


# --- Peek on the straddles --------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_peek_on_straddles(rl, profile):
    """After each point's first request (n = p in the window before), peek
    (key, ws1 + el, n) for n = cc and n = 0: the exact weighted count is the
    limit, or one below it, or (n = 0) an integer below; against the
    reference of test_peek_gpu (peek_cases.peek_expected over the Python
    oracle)."""
    case, = [c for c in wc.all_cases()["s"] if c.claim["kind"] == "light"]
    r = Rig(rl, profile, wc.CONFIGS)
    try:
        r.decide(case.batches[0], what=f"{case.name} batch 0")
        key, ts, n, cfg, sms = case.test_batch
        r.peek((key, ts, n, cfg, sms), what="n = cc")
        r.peek((key, ts, np.zeros_like(n), cfg, sms), what="n = 0")
        r.decide(case.test_batch, what=f"{case.name} batch 1")
    finally:
        r.close()
