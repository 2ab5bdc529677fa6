"""Expected values of read-only queries (rl_peek_batch) from the Python oracle.

A peek is the Result AllowN(key, n) would return against the state as it is,
with nothing changed.  The oracle has no such call, so `peek_expected` runs the
ordinary step and puts back the (at most two) keyspace entries it can touch:
"tb:<id>" for a token bucket, "w:<id>:<ws>" and "w:<id>:<pws>" for the window
algorithms.  n >= 1 goes through Sim.decide; n == 0 -- the status query, which
decide rejects -- calls the algorithm's step directly with requested = 0.
"""
import copy
import math

import numpy as np

from oracle import rl_oracle_py as po

INVALID_ROW = (po.INVALID, 0, 0, 0, math.nan)
KEY_RESERVED = (1 << 64) - 1


def touched_keys(sim, key, ts, cfg):
    """the db entries a request of config `cfg` can read or write"""
    alg, L, W = sim.cfgs[cfg]
    if alg == po.TOKEN_BUCKET:
        return ["tb:%d" % key]
    ws = po.window_start(ts, W)
    ks = ["w:%d:%d" % (key, ws)]
    if alg == po.SLIDING_WINDOW:
        ks.append("w:%d:%d" % (key, ws - po.go_f2i(po.duration_seconds(W))))
    return ks


def peek_one(sim, key, ts, n, cfg, server_ms=None):
    """(decision, remaining, retry_ns, reset_at_ns, tokens) of one peek; sim.db
    is left as it was"""
    key, ts, n, cfg = int(key), int(ts), int(n), int(cfg)
    if cfg < 0 or cfg >= len(sim.cfgs) or n < 0 or key == KEY_RESERVED:
        return INVALID_ROW
    s_ms = int(server_ms) if server_ms is not None else ts // 1_000_000
    ks = touched_keys(sim, key, ts, cfg)
    saved = [(k, copy.deepcopy(sim.db[k]) if k in sim.db else None) for k in ks]
    if n >= 1:
        row = sim.decide(key, ts, n, cfg, s_ms)
    else:
        alg, L, W = sim.cfgs[cfg]
        fn = {po.TOKEN_BUCKET: sim._tb, po.SLIDING_WINDOW: sim._sw, po.FIXED_WINDOW: sim._fw}[alg]
        row = fn(L, W, key, ts, 0, s_ms)
    for k, ent in saved:
        if ent is None:
            sim.db.pop(k, None)
        else:
            sim.db[k] = ent
    return row


def peek_expected(sim, key, ts, n, cfg, server_ms=None):
    """peek_one over arrays -> (decision u8, remaining, retry, reset, tokens) arrays"""
    m = len(key)
    dec = np.empty(m, np.uint8)
    rem, retry, reset = np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64)
    tok = np.full(m, np.nan)
    for i in range(m):
        d, r, ra, rs, t = peek_one(sim, key[i], ts[i], n[i], cfg[i], None if server_ms is None else server_ms[i])
        dec[i], rem[i], retry[i], reset[i], tok[i] = d, r, ra, rs, t
    return dec, rem, retry, reset, tok


def sim_decide(sim, key, ts, n, cfg, server_ms=None):
    """run a decide trace through the Python oracle (its results are not used:
    the engine's decisions are checked against the C oracle)"""
    for i in range(len(key)):
        sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]), None if server_ms is None else int(server_ms[i]))


def assert_peek(res, exp, configs, cfg, what=""):
    """a Decisions (or a 4/5-tuple of arrays) against peek_expected's arrays;
    tokens (token-bucket rows that ran) as bit patterns"""
    if not isinstance(res, tuple):
        res = (res.decision, res.remaining, res.retry_after_ns, res.reset_at_ns, res.tokens)
    dec, rem, retry, reset, tok = exp
    bad = np.nonzero(res[0] != dec)[0]
    assert bad.size == 0, f"{what} decision mismatch at {bad[:10]}: got={res[0][bad[:10]]} want={dec[bad[:10]]}"
    for name, a, b in [("remaining", res[1], rem), ("retry", res[2], retry), ("reset_at", res[3], reset)]:
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{what} {name} mismatch at {bad[:10]}: got={a[bad[:10]]} want={b[bad[:10]]}"
    if len(res) > 4 and res[4] is not None:
        cfg = np.asarray(cfg).astype(np.int64)
        alg = np.array([c[0] for c in configs])
        is_tb = (cfg < len(configs)) & (alg[np.minimum(cfg, len(configs) - 1)] == 1) & (dec <= 1)
        gb = res[4].view(np.uint64)[is_tb]
        rb = tok.view(np.uint64)[is_tb]
        bad = np.nonzero(gb != rb)[0]
        assert bad.size == 0, f"{what} tokens mismatch: got={res[4][is_tb][bad[:5]]} want={tok[is_tb][bad[:5]]}"
