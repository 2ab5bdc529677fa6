"""Cases that load the three HBM state tables (csrc/rl_table.h, rl_window.h).

Numpy restatements of the tables' hash functions, so that a test can choose
key ids by the slot they hash to -- many ids of one home slot, one id per home
slot of a range -- and a spill load generator: `ladder_trace` keeps D window
keys of every user key alive at once, D - 2 of which the engine must hold in
its spill table.  No GPU here: test_table_cases.py checks these helpers on the
CPU oracles, so that the GPU cases built from them are inside or outside a
table's capacity by construction.
"""
import numpy as np

from tracegen import NS, T0

U64 = np.uint64
SPILL_SALT = 0x5bd1e9955bd1e995


def mix64(x):
    """rl_table.h mix64 (the splitmix64 finaliser), vectorised over uint64"""
    x = np.array(x, dtype=U64, ndmin=1)          # a copy
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(0xbf58476d1ce4e5b9)
        x ^= x >> U64(27)
        x *= U64(0x94d049bb133111eb)
        x ^= x >> U64(31)
    return x


def home(k, mask):
    """home slot of key id k in a token-bucket or window table of mask + 1 slots"""
    return mix64(k) & U64(mask)


def spill_home(k, mask):
    """first slot of user key k's probe sequence in the spill table"""
    return mix64(np.asarray(k, U64) ^ U64(SPILL_SALT)) & U64(mask)


def keys_with_home(mask, home_slot, count, spill=False, start=0):
    """the first `count` ids >= start whose home slot (spill home, with
    spill=True) is `home_slot`, ascending"""
    fn = spill_home if spill else home
    out, got, chunk = [], 0, 1 << 18
    while got < count:
        ids = np.arange(start, start + chunk, dtype=U64)
        hit = ids[fn(ids, mask) == U64(home_slot)]
        out.append(hit)
        got += hit.size
        start += chunk
    return np.concatenate(out)[:count]


def one_key_per_home(mask, start, length, spill=False):
    """one id (the smallest) for each home slot of [start, start + length) mod
    the capacity, in the order of the range"""
    assert 0 < length <= mask + 1
    fn = spill_home if spill else home
    want = (np.arange(start, start + length, dtype=U64)) & U64(mask)
    first = np.full(mask + 1, -1, np.int64)
    lo, chunk = 0, 1 << 18
    while (first[want.astype(np.int64)] < 0).any():
        ids = np.arange(lo, lo + chunk, dtype=U64)
        h = fn(ids, mask).astype(np.int64)
        u, at = np.unique(h, return_index=True)      # the first id of each home in this chunk
        new = first[u] < 0
        first[u[new]] = ids[at[new]].astype(np.int64)
        lo += chunk
    return first[want.astype(np.int64)].astype(U64)


def ladder_trace(seed, K, D, rounds, configs, span_s=30, id0=1 << 20, t0=T0, ids=None):
    """Spill load: K user keys (id0 .. id0 + K - 1, or `ids`), cfg = key %
    len(configs), each requested `rounds` times at each of D clock skews 0, -W,
    -2W, ..., -(D - 1)W of its config's window W, in a seeded random order.
    True times are sorted uniform draws over span_s seconds from t0; the store
    clock is the true time in ms (monotone); n is drawn from {1, 1, 2, 3}.
    While no window start is crossed and nothing expires -- 60 s windows, a
    span of 30 s and t0 = T0, which lies 20 s into its minute -- every user
    key owns D live window keys, D - 2 of them outside its 2-slot entry."""
    rng = np.random.default_rng(seed)
    ids = np.arange(id0, id0 + K, dtype=U64) if ids is None else np.asarray(ids, U64)
    assert ids.size == K
    m = K * D * rounds
    key = np.tile(np.repeat(ids, D), rounds)
    step = np.tile(np.tile(np.arange(D, dtype=np.int64), K), rounds)
    order = rng.permutation(m)
    key, step = key[order], step[order]
    cfg = (key % U64(len(configs))).astype(np.uint32)
    W = np.array([c[2] for c in configs], np.int64)[cfg]
    true_t = t0 + np.sort(rng.integers(0, span_s * NS, m)).astype(np.int64)
    ts = true_t - step * W
    n = rng.choice([1, 1, 2, 3], m).astype(np.int64)
    return key, ts, n, cfg, true_t // 1_000_000


def spill_demand(sim, now_ms):
    """window keys the engine must hold outside the 2-slot entries: from the
    oracle's live keys at now_ms (OracleSim.keys: [(id, kind, ws)], kind 1 a
    window key), the sum over user keys of max(0, live window keys - 2); the
    Python oracle (rl_oracle_py.Sim) is read through reset_cases.py_keys"""
    from reset_cases import py_keys
    live = sim.keys(now_ms) if hasattr(sim, "lib") else py_keys(sim, now_ms)
    ids = np.array([k for k, kind, _ in live if kind == 1], U64)
    if ids.size == 0:
        return 0
    _, counts = np.unique(ids, return_counts=True)
    return int(np.maximum(counts - 2, 0).sum())
