"""The many-config traces (tracegen.many_config_trace) on the CPU: the trace
contains what the GPU tests use it for -- every config id used, a hot
token-bucket key of at least 4096 requests per batch on the last config, heavy
keys, allows, denials and expiries on every algorithm -- and the C oracle,
which the GPU tests compare against, agrees with the Python oracle bit for bit
on both profiles."""
import numpy as np
import pytest

from oracle import rl_oracle_py as po
from tracegen import many_config_keys, many_config_trace


def _split(trace, sizes):
    key, ts, n, cfg, _ = trace
    out, o = [], 0
    for s in sizes:
        out.append((key[o:o + s], ts[o:o + s], n[o:o + s], cfg[o:o + s]))
        o += s
    return out


@pytest.mark.parametrize("N", [33, 65])
def test_trace_contents(N):
    assert N > 32
    configs, tr, sizes = many_config_trace(4000 + N, N)
    assert len(configs) == N and len(set(configs)) == N
    assert len({(L, W) for _, L, W in configs}) == N           # distinct limits / windows
    assert [a for a, _, _ in configs[:6]] == [1, 2, 3, 1, 2, 3]
    assert configs[N - 1][0] == 1                               # the hot key's config: a token bucket
    assert len(sizes) >= 3
    hot = many_config_keys(N, N - 1, 0)
    # a key's requests come both within the shortest window and after the
    # longest TTL (2 x 12 s): state is reused, and it expires
    o = np.argsort(tr[0], kind="stable")
    gap = np.diff(tr[1][o])[tr[0][o][1:] == tr[0][o][:-1]]
    assert int((gap < 300_000_000).sum()) > 1000 and int((gap > 25_000_000_000).sum()) > 1000
    for key, ts, n, cfg in _split(tr, sizes):
        assert np.array_equal(cfg, (key % np.uint64(N)).astype(np.uint32))
        assert set(np.unique(cfg).tolist()) == set(range(N))    # every config id
        assert int((key == hot).sum()) >= 4096                  # a huge segment (the chain)
        cnt = np.unique(key, return_counts=True)[1]
        heavy = (cnt >= 32) & (cnt < 4096)
        assert int(heavy.sum()) >= 6                            # heavy segments (one wave each)
        for c in (N - 1, N - 2, N - 3):                         # ... on ids >= 32 (N - 1 only at N = 33)
            k = many_config_keys(N, c, 1)
            assert 32 <= int((key == k).sum()) < 4096 and int(k % np.uint64(N)) == c
        assert int((n == 0).sum()) > 0 and int((n == 1 << 62).sum()) > 0


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("N", [33, 65])
def test_c_vs_python_many_configs(oracle_mod, profile, N):
    assert N > 32
    configs, tr, sizes = many_config_trace(4000 + N, N)
    csim = oracle_mod.OracleSim(profile)
    psim = po.Sim(profile)
    for i, (a, L, W) in enumerate(configs):
        assert csim.add_config(a, L, W) == psim.add_config(a, L, W) == i
    hot = many_config_keys(N, N - 1, 0)
    seen = {a: set() for a in (1, 2, 3)}
    hot_dec = set()
    alg = np.array([a for a, _, _ in configs])
    for b, (key, ts, n, cfg) in enumerate(_split(tr, sizes)):
        c = csim.decide(key, ts, n, cfg)
        py = [psim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i])) for i in range(key.size)]
        for f, name in enumerate(("decision", "remaining", "retry", "reset_at")):
            got = np.array([r[f] for r in py], dtype=c[f].dtype)
            ok = c[0] != 3 if f else np.ones(key.size, bool)
            assert np.array_equal(got[ok], c[f][ok]), f"batch {b}: {name} differs"
        is_tb = (alg[cfg] == 1) & (c[0] <= 1)
        ptok = np.array([r[4] for r in py], dtype=np.float64)
        assert np.array_equal(ptok[is_tb].view(np.uint64), c[4][is_tb].view(np.uint64)), f"batch {b}: tokens differ"
        for a in (1, 2, 3):
            seen[a] |= set(np.unique(c[0][alg[cfg] == a]).tolist())
        hot_dec |= set(np.unique(c[0][key == hot]).tolist())
    for a in (1, 2, 3):
        assert {0, 1, 3} <= seen[a], (a, seen[a])                # denied, allowed, rejected on every algorithm
    assert {0, 1} <= hot_dec                                    # the hot key is allowed and denied
