"""Cases and helpers for batched Reset (rl_reset_batch).

A reset batch is m (key, ts, cfg) triples with the effect of m single resets in
any order.  The expected state always comes from an oracle whose `reset` is
called once per executed request (`apply_resets`); it is compared through the
decisions of the trace that follows and through the live key set.

`reset_case` builds: a warm-up trace, a reset batch aimed at window keys that
exist (the times of the warm-up's own requests, so a key's window of any age is
hit wherever the engine keeps it), at the window after and before them, at
times far from any window, at keys never seen, with duplicates; and the trace
that follows.
"""
import numpy as np

from oracle import rl_oracle_py as po
from tracegen import CONFIG_SETS, NS, random_trace, skewed_trace

KEY_RESERVED = (1 << 64) - 1
RESET_DONE, INVALID = 1, 3
KIND_HASH, KIND_WINDOW = 0, 1

KINDS = ["tb", "fw", "sw", "mixed", "skew"]


def case_configs(kind):
    return CONFIG_SETS["sw"] + CONFIG_SETS["fw"] if kind == "skew" else CONFIG_SETS[kind]


def reset_case(kind, seed, m=6000, nkeys=60, ff=False):
    """-> (configs, first, (rkey, rts, rcfg), second, now_ms): decide `first`,
    reset the batch, decide `second`; now_ms is a server clock at the batch"""
    configs = case_configs(kind)
    if kind == "skew":
        tr = skewed_trace(seed, 2 * m, nkeys, configs)
    else:
        tr = random_trace(seed, 2 * m, nkeys, configs, fastforward=ff, big_n=True)
    first = tuple(None if x is None else x[:m] for x in tr)
    second = tuple(None if x is None else x[m:] for x in tr)
    key, ts, n, cfg, sms = first
    now_ms = int(sms[-1]) if sms is not None else int(ts[-1]) // 1_000_000
    rng = np.random.default_rng(seed + 1000)
    W = np.array([c[2] for c in configs], np.int64)
    # every third key is reset; the others must keep their exact state
    pick = np.nonzero(key % np.uint64(3) == 0)[0]
    pick = pick[rng.permutation(pick.size)[:400]]
    rk, rc = key[pick], cfg[pick]
    # the requests' own times, the window after, the window before, far away
    shift = rng.choice([0, 0, 0, 1, -1, 1000], pick.size)
    rt = ts[pick] + shift * W[rc]
    # each of those keys at the end of the warm-up too (the current window)
    uk = np.unique(rk)
    # keys never seen
    absent = np.arange(20, dtype=np.uint64) * np.uint64(3) + np.uint64(30 * nkeys)
    rkey = np.concatenate([rk, uk, absent, rk[:50], rk[:50]])
    rts = np.concatenate([rt, np.full(uk.size, ts[-1]), np.full(absent.size, ts[-1]), rt[:50], rt[:50]])
    rcfg = (rkey % np.uint64(len(configs))).astype(np.uint32)
    order = rng.permutation(rkey.size)
    return configs, first, (rkey[order], rts[order].astype(np.int64), rcfg[order]), second, now_ms


def valid(key, cfg, ncfg):
    """which requests of a reset batch are executed"""
    return (np.asarray(cfg).astype(np.int64) < ncfg) & (np.asarray(key, np.uint64) != np.uint64(KEY_RESERVED))


def expected_status(key, cfg, ncfg):
    return np.where(valid(key, cfg, ncfg), RESET_DONE, INVALID).astype(np.uint8)


def apply_resets(sim, key, ts, cfg, ncfg, server_ms=0, order=None):
    """sim.reset once per executed request, in `order` (default: as given); sim
    is the C oracle (oracle.OracleSim) or the Python one (rl_oracle_py.Sim)"""
    ok = valid(key, cfg, ncfg)
    idx = range(len(key)) if order is None else order
    c_sim = hasattr(sim, "lib")
    for i in idx:
        if not ok[i]:
            continue
        if c_sim:
            sim.reset(int(cfg[i]), int(key[i]), int(ts[i]), server_ms)
        else:
            sim.reset(int(cfg[i]), int(key[i]), int(ts[i]))


def py_keys(sim, now_ms):
    """the Python oracle's live keys at server clock now_ms, as OracleSim.keys
    lists them: {(id, kind, ws)}"""
    out = set()
    for k, (val, when) in sim.db.items():
        if sim._expired(when, now_ms):
            continue
        p = k.split(":")
        out.add((int(p[1]), KIND_HASH, 0) if p[0] == "tb" else (int(p[1]), KIND_WINDOW, int(p[2])))
    return out


KEY_REC = np.dtype([("key_id", np.uint64), ("window_start", np.int64), ("kind", np.uint32), ("pad_", np.uint32)])


def engine_keys(rl, eng, now_ms):
    """rl_table_keys(now_ms) -> {(id, kind, ws)}"""
    import ctypes as C
    cnt = C.c_uint64()
    assert rl.lib.rl_table_keys(eng.h, now_ms, None, 0, C.byref(cnt)) == 0
    out = np.zeros(cnt.value + 1, KEY_REC)
    assert rl.lib.rl_table_keys(eng.h, now_ms, out.ctypes.data_as(C.c_void_p), out.size, C.byref(cnt)) == 0
    assert cnt.value == out.size - 1
    out = out[:cnt.value]
    s = set(zip(out["key_id"].tolist(), out["kind"].tolist(), out["window_start"].tolist()))
    assert len(s) == cnt.value
    return s


def py_decide_rows(sim, tr):
    """the Python oracle's rows (decision, remaining, retry, reset_at, tokens);
    rows without tokens carry the one math.nan object, so lists of rows compare"""
    key, ts, n, cfg, sms = tr
    return [sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]), None if sms is None else int(sms[i]))
            for i in range(len(key))]


def new_sims(oracle, profile, configs):
    csim, psim = oracle.OracleSim(profile), po.Sim(profile)
    for a, L, W in configs:
        assert csim.add_config(a, L, W) == psim.add_config(a, L, W)
    return csim, psim
