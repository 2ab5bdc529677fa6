"""The plain finish (GPU): batches above the bucketed finish's limit.

Up to UP_MAX = 2^21 requests a batch's results reach the caller's order
through arrival-index buckets (k_unpermute_bucket, k_unpermute_bucket_out /
k_unpermute_routed_out).  Larger batches finish through k_unpermute, or
k_unpermute_routed on the routed path: stores scattered by arrival index, and
the Result fields computed from the engine's sorted-order copies of ts / n /
cfg, not from the caller's inputs.  RL_UP_MAX lowers the limit so that batches
of a few thousand requests take these kernels, rl_stats.plain_finish_batches
shows that they did, and one test runs at the real limit with no knob.  All
bit for bit against the CPU oracle."""
import functools

import numpy as np
import pytest

import oracle
from test_gpu_parity import assert_same
from tracegen import CONFIG_SETS, T0, random_trace

pytestmark = pytest.mark.gpu

UP_MAX = 1 << 21       # csrc/rl_group.h
CONFIGS = CONFIG_SETS["mixed"]


def _trace(seed, m, ff):
    """random_trace over the mixed configs with a hot token-bucket key (cfg 0)
    on 4200 requests of every m, and ~1 % rejected requests: n = 0 (random_trace's
    big_n), an unknown config id, the reserved key id"""
    key, ts, n, cfg, sms = random_trace(seed, 2 * m, 700, CONFIGS, fastforward=ff, big_n=True)
    rng = np.random.default_rng(seed + 1)
    for o in (0, m):
        key[o + rng.permutation(m)[:4200]] = 15 * 1000          # 15000 % 15 == 0: a token bucket (20 / 12 s)
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    r = rng.random(2 * m)
    cfg[r < 0.003] = len(CONFIGS) + 2
    key[(r >= 0.003) & (r < 0.006)] = np.uint64((1 << 64) - 1)
    return key, ts, n, cfg, sms


def _reference(sim, key, ts, n, cfg, sms):
    """the oracle's results; the reserved key id, which the oracle would
    decide, is rejected by the engine (include/rl_engine.h): left out, 3"""
    keep = key != np.uint64((1 << 64) - 1)
    sub = sim.decide(key[keep], ts[keep], n[keep], cfg[keep], None if sms is None else sms[keep])
    out = [np.full(key.size, 3, np.uint8)] + [np.zeros(key.size, np.int64) for _ in range(3)] + \
        [np.full(key.size, np.nan)]
    for full, x in zip(out, sub):
        full[keep] = x
    return tuple(out)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("ff", [False, True])
@pytest.mark.parametrize("m", [8191, 8192, 8193, 20_000])
def test_plain_finish_around_the_limit(rl, m, ff, profile, monkeypatch):
    """RL_UP_MAX=8192: batches of 8191 and 8192 take the buckets, 8193 and
    20,000 k_unpermute.  Two batches of m with state carried, the first with
    tokens, the second without (out.tok null); ff: an explicit server clock
    (32-byte records, sorted.sms).  A hot token-bucket key of 4200 requests
    per batch: the chain's committed runs and k_tb_expand feed the finish."""
    monkeypatch.setenv("RL_UP_MAX", "8192")
    monkeypatch.setenv("RL_SMALL_MAX", "4096")
    key, ts, n, cfg, sms = _trace(5000 + m + 2 * profile + int(ff), m, ff)
    eng = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 15)
    sim = oracle.OracleSim(profile)
    for a, L, W in CONFIGS:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    for b, want_tokens in enumerate([True, False]):
        s = slice(b * m, (b + 1) * m)
        part = (key[s], ts[s], n[s], cfg[s], None if sms is None else sms[s])
        assert int((part[0] == 15_000).sum()) >= 4096
        rejected = (part[2] <= 0) | (part[3] >= len(CONFIGS)) | (part[0] == np.uint64((1 << 64) - 1))
        assert m // 200 < int(rejected.sum()) < m // 25
        before = eng.stats().plain_finish_batches
        res = eng.decide(*part, want_tokens=want_tokens, check=False)
        assert res.status == rl.RL_OK, eng.last_error()
        assert (res.tokens is None) == (not want_tokens)
        assert_same(res, _reference(sim, *part), CONFIGS, part[3], what=f"batch {b}")
        assert np.all(res.decision[rejected] == 3)
        assert eng.stats().plain_finish_batches - before == (1 if m > 8192 else 0)
    eng.close()


def test_up_max_is_clamped(rl, monkeypatch):
    """RL_UP_MAX above 2^21 is clamped to it (the buckets are sized for 2^21):
    a batch of 20,000 takes the buckets"""
    monkeypatch.setenv("RL_UP_MAX", str(1 << 24))
    key, ts, n, cfg, sms = _trace(5100, 20_000, False)
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 15)
    sim = oracle.OracleSim(0)
    for a, L, W in CONFIGS:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    part = (key[:20_000], ts[:20_000], n[:20_000], cfg[:20_000], None)
    res = eng.decide(*part, check=False)
    assert_same(res, _reference(sim, *part), CONFIGS, part[3])
    assert eng.stats().plain_finish_batches == 0
    eng.close()


# --- the routed path: k_unpermute_routed ---------------------------------------------

def _check_routed(res, nbatch, exchange):
    from test_route_gpu import _check
    _check(res, 1, nbatch, exchange)
    assert res[0][1]["plain_finish_batches"] > 0, res[0][1]


def test_routed_plain_finish_time_order(monkeypatch):
    """world size 1, batches in time order (the merge's identity order
    marker): every step's 30,000 results through k_unpermute_routed"""
    from test_route_gpu import _spawn, mixed_batches
    monkeypatch.setenv("RL_UP_MAX", "8192")        # before the spawn: the rank inherits it
    gen = functools.partial(mixed_batches, nbatch=3, m=30_000, nkeys=40_000)
    _check_routed(_spawn(1, "nccl", gen), 3, False)


def test_routed_plain_finish_unsorted_batches(monkeypatch):
    """world size 1 with batches out of time order (skewed clocks): an
    explicit order array, results stored at order[p]"""
    from test_route_gpu import _spawn, skewed_batches
    monkeypatch.setenv("RL_UP_MAX", "8192")
    gen = functools.partial(skewed_batches, nbatch=3, m=30_000, nkeys=10_000)
    _check_routed(_spawn(1, "nccl", gen), 3, False)


# --- at the real limit, no knob --------------------------------------------------------

def test_plain_finish_at_two_to_the_21(rl, monkeypatch):
    """max_batch 2^22: a batch of exactly 2^21 requests (the bucketed finish
    with all 1024 bucket counters in use), then one of 2^21 + 1 (k_unpermute).
    Mixed configs, uniform keys over ~1M ids; a seeded 1/32 of the keys is
    replayed by the oracle bit for bit (keys never interact), every request is
    decided."""
    monkeypatch.delenv("RL_UP_MAX", raising=False)
    rng = np.random.default_rng(5200)
    eng = rl.Engine(profile=0, tb_capacity=1 << 20, win_capacity=1 << 21, max_batch=1 << 22)
    sim = oracle.OracleSim(0)
    for a, L, W in CONFIGS:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    t = T0
    for b, m in enumerate([UP_MAX, UP_MAX + 1]):
        key = rng.integers(0, 1_000_000, m).astype(np.uint64)
        ts = t + np.cumsum(rng.integers(0, 2000, m)).astype(np.int64)
        t = int(ts[-1])
        n = rng.choice([1, 1, 2], m).astype(np.int64)
        cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
        before = eng.stats().plain_finish_batches
        res = eng.decide(key, ts, n, cfg, want_tokens=(b == 1))
        assert eng.stats().plain_finish_batches - before == b
        assert np.all(res.decision <= 1), f"batch {b}"
        pick = (key * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(59)) == np.uint64(0)   # 1/32 of keys
        ref = sim.decide(key[pick], ts[pick], n[pick], cfg[pick])
        sub = rl.Decisions(res.decision[pick], res.remaining[pick], res.retry_after_ns[pick],
                           res.reset_at_ns[pick], None if res.tokens is None else res.tokens[pick])
        assert_same(sub, ref, CONFIGS, cfg[pick], what=f"batch {b}")
    eng.close()
