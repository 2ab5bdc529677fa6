"""Reference for the top keys (rl_hot_*, include/rl_engine.h; csrc/rl_hot.h): a
numpy restatement of the count-min sketch and the candidate set -- mix64, the
four columns, phases A and B of every call, estimates at read time -- and the
trace builders the tests share.  No GPU here: test_hot_cases.py checks the
model's own properties, the GPU tests and the coalescer's host version are
compared with it for equality."""
import numpy as np

from table_cases import mix64

U64 = np.uint64
M64 = (1 << 64) - 1
KEY_RESERVED = M64
DEPTH = 4            # RL_HOT_DEPTH
PROBES = 64          # rl_hot.h HOT_PROBES
LDS_KEYS = 256       # rl_hot.h HOT_LDS_KEYS: keys a block of k_hot_add merges in LDS
BLOCK = 256          # rl_hot.h HOT_BLOCK
REQUESTS, UNITS = 0, 1


def columns(keys, width):
    """the column of every key in every row -> int64[DEPTH, len(keys)]:
    mix64(k ^ mix64(r + 1)) & (width - 1)"""
    keys = np.asarray(keys, U64).reshape(-1)
    assert width & (width - 1) == 0
    return np.stack([(mix64(keys ^ mix64(r + 1)[0]) & U64(width - 1)).astype(np.int64) for r in range(DEPTH)])


def _arrays(key, cfg, n, dec):
    key = np.asarray(key, U64).reshape(-1)
    cfg = np.asarray(cfg, np.uint32).reshape(-1)
    n = np.asarray(n, np.int64).reshape(-1)
    dec = np.asarray(dec, np.uint8).reshape(-1)
    assert key.size == cfg.size == n.size == dec.size
    return key, cfg, n, dec


def counted_mask(key, cfg, n, dec, ncfg, weight=REQUESTS):
    """which requests count: a registered config, a decision the limiter
    executed (denied, allowed, error), not the reserved key, and n > 0 in units mode"""
    key, cfg, n, dec = _arrays(key, cfg, n, dec)
    ok = (cfg < ncfg) & (dec <= 2) & (key != U64(KEY_RESERVED))
    if weight == UNITS:
        ok &= n > 0
    return ok


class HotModel:
    """the sketch, the candidate set (no table: as if every qualifying key
    found a slot) and the counters after any sequence of calls"""

    def __init__(self, width, hot_min, ncfg, weight=REQUESTS):
        self.width, self.hot_min, self.ncfg, self.weight = width, hot_min, ncfg, weight
        self.clear()

    def clear(self):
        self.sketch = np.zeros((DEPTH, self.width), U64)
        self.candidates = {}      # key id -> the config ids of its counted requests in the calls that found it hot
        self.true = {}            # key id -> its true weight (modulo 2^64)
        self.total = self.skipped = self.batches = self.requests = 0

    def call(self, key, cfg, n, dec, ncfg=None):
        """one rl_hot_batch* call: (A) all the adds, then (B) the look at the call's keys"""
        key, cfg, n, dec = _arrays(key, cfg, n, dec)
        if key.size == 0:
            return
        ok = counted_mask(key, cfg, n, dec, self.ncfg if ncfg is None else ncfg, self.weight)
        k, c = key[ok], cfg[ok]
        w = n[ok].astype(U64) if self.weight == UNITS else np.ones(k.size, U64)
        self.batches += 1
        self.requests += key.size
        self.skipped += int((~ok).sum())
        self.total = (self.total + sum(w.tolist())) & M64
        cols = columns(k, self.width)
        with np.errstate(over="ignore"):
            for r in range(DEPTH):
                np.add.at(self.sketch[r], cols[r], w)               # uint64: wraps
        for kk, ww in zip(k.tolist(), w.tolist()):
            self.true[kk] = (self.true.get(kk, 0) + ww) & M64
        ids = np.unique(k)
        est = self.estimate(ids)
        for kk in ids[est >= U64(self.hot_min)].tolist():
            self.candidates.setdefault(kk, set()).update(c[k == U64(kk)].tolist())

    def estimate(self, keys):
        """the minimum of each key's four counters, now"""
        keys = np.asarray(keys, U64).reshape(-1)
        cols = columns(keys, self.width)
        return np.min(np.stack([self.sketch[r][cols[r]] for r in range(DEPTH)]), axis=0) if keys.size else \
            np.zeros(0, U64)

    def read(self):
        """[(key id, estimate now)] of every candidate, estimate descending then key id"""
        ks = sorted(self.candidates)
        est = self.estimate(ks).tolist()
        return sorted(zip(ks, est), key=lambda x: (-x[1], x[0]))

    def true_hot(self):
        """keys whose true weight has reached hot_min"""
        return {k for k, v in self.true.items() if v >= self.hot_min}


def brute_sketch(calls, width, ncfg, weight=REQUESTS):
    """the sketch one request at a time with Python integers -> list of DEPTH lists"""
    salt = [int(mix64(r + 1)[0]) for r in range(DEPTH)]
    sk = [[0] * width for _ in range(DEPTH)]
    for key, cfg, n, dec in calls:
        for k, c, x, d in zip(*[np.asarray(a).tolist() for a in _arrays(key, cfg, n, dec)]):
            if c >= ncfg or d > 2 or k == KEY_RESERVED or (weight == UNITS and x <= 0):
                continue
            for r in range(DEPTH):
                col = int(mix64(k ^ salt[r])[0]) & (width - 1)
                sk[r][col] = (sk[r][col] + (x if weight == UNITS else 1)) & M64
    return sk


# --- traces ---------------------------------------------------------------------------

ZIPF_SIZES = (5000, 5037, 5074)     # none a multiple of 64 or 256
ZIPF_IDS = 3000
ZIPF_SEED = 11
ZIPF_HOT_MIN = 200
NCFG = 5


def key_of_rank(rank):
    """key ids of the Zipf ranks: scattered 64-bit ids"""
    return mix64(np.asarray(rank, U64) + U64(0x1234567))


def zipf_calls(seed=ZIPF_SEED, sizes=ZIPF_SIZES, ids=ZIPF_IDS, a=1.3, ncfg=NCFG, skips=True):
    """calls of a seeded Zipf(a) trace over `ids` key ids: [(key, cfg, n,
    dec)], with decisions 0 .. 2 and, with skips, a few requests that do not
    count (unregistered config, decision 3, the reserved key)"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, ids + 1) ** a
    p /= p.sum()
    calls = []
    for m in sizes:
        rank = rng.choice(ids, m, p=p)
        key = key_of_rank(rank)
        cfg = (rank % ncfg).astype(np.uint32)
        n = rng.choice([1, 1, 2, 5], m).astype(np.int64)
        dec = rng.choice([0, 1, 1, 2], m).astype(np.uint8)
        if skips:
            cfg[rng.random(m) < 0.01] = ncfg + 3
            dec[rng.random(m) < 0.01] = 3
            key[rng.random(m) < 0.005] = U64(KEY_RESERVED)
        calls.append((key, cfg, n, dec))
    return calls


def model_of(calls, width, hot_min, ncfg=NCFG, weight=REQUESTS):
    mod = HotModel(width, hot_min, ncfg, weight)
    for c in calls:
        mod.call(*c)
    return mod


def distinct_columns(keys, width):
    """no two of the keys share a counter in any row: every estimate is a true weight"""
    cols = columns(keys, width)
    return all(np.unique(cols[r]).size == cols.shape[1] for r in range(DEPTH))


def check_read(h, mod, what=""):
    """a read `h` (rl_amd.Hot holding every tracked key) against the model,
    whose candidates all found a slot: the same set, the model's estimates at
    read time, the order, the counters"""
    want = mod.read()
    got = [(int(r["key_id"]), int(r["estimate"])) for r in h.keys]
    assert h.keys_tracked == h.info.keys_tracked == len(want), f"{what}: {h.keys_tracked} tracked, model {len(want)}"
    assert sorted(got) == sorted(want), f"{what}: set or estimates differ"
    assert got == want, f"{what}: order"
    for r in h.keys:
        assert int(r["cfg_id"]) in mod.candidates[int(r["key_id"])], what
    i = h.info
    assert (i.total, i.skipped, i.batches, i.requests) == (mod.total, mod.skipped, mod.batches, mod.requests), \
        f"{what}: counters {(i.total, i.skipped, i.batches, i.requests)} != " \
        f"{(mod.total, mod.skipped, mod.batches, mod.requests)}"
    assert i.dropped == 0, what
