"""Cases and the expected results for Charge (rl_charge_batch).

The verb is a composition, and so is its expectation on the Python oracle:
`apply_charge` asks every request against the state before the call
(`refund_cases.py_peek` gives a bucket's `r`, the clamp n' = min(n, r) follows),
runs `Sim.decide` on n' per request in array order, and applies the result rule
in plain Python.

`charge_case` builds a warm-up trace, one Charge call of about 1500 requests
over about 120 keys, and the trace that follows.  It asserts its own coverage
from the oracle.
"""
import numpy as np

from oracle import rl_oracle_py as po
from refund_cases import new_sim, py_peek, warm
from reset_cases import KEY_RESERVED
from tracegen import CONFIG_SETS, random_trace

KINDS = ["tb", "fw", "sw", "mixed"]
# the seed of each kind's case: checked on the CPU (test_charge_cases.py) to
# meet the coverage the builder asserts
SEEDS = {"tb": 300, "fw": 301, "sw": 302, "mixed": 303}
LATE_MS = 10 ** 7                       # ms past the call's body: every TTL here has run out


def names_of(sim, key, ts, cfg):
    """the db keys the script of a valid request reads: the bucket, or the
    current window's counter"""
    alg, L, W = sim.cfgs[cfg]
    if alg == po.TOKEN_BUCKET:
        return "tb:%d" % key
    return "w:%d:%d" % (key, po.window_start(ts, W))


def apply_charge(sim, key, ts, n, cfg, server_ms=None):
    """one Charge call on sim -> (rows, info).  rows[i] = (decision, charged,
    remaining, reset_at_ns, tokens); tokens is 0.0 except for a bucket.  info:
    `np` the asked amounts n', `cls` one class per request -- "invalid", "full"
    (all of n charged and allowed), "short" (a bucket, 0 < charged < n),
    "empty" (a bucket, n' = 0), "dup_denied" (a bucket, n' >= 1 and the decide
    denied it), "over" (a window, the whole n recorded and the count above the
    limit), "error" -- and the index lists `fresh` (an executed request whose
    db key did not exist) and `expired` (it existed, dead at the request's
    clock)."""
    m = len(key)
    clock = lambda i: int(server_ms[i]) if server_ms is not None else int(ts[i]) // 1_000_000
    # 1. ask: read-only, every request against the state before the call
    ask = []
    for i in range(m):
        k, t, nn, c = int(key[i]), int(ts[i]), int(n[i]), int(cfg[i])
        if not (0 <= c < len(sim.cfgs)) or nn <= 0 or k == KEY_RESERVED:
            ask.append(("invalid", 0, None))
        elif sim.cfgs[c][0] == po.TOKEN_BUCKET:
            row = py_peek(sim, k, t, c, clock(i))
            ask.append(("tb", max(0, min(nn, row[1])), row))
        else:
            ask.append(("win", nn, None))
    # 2. decide on n' in array order, 3. the result rule
    rows, cls, fresh, expired = [], [], [], []
    for i in range(m):
        kind, take, arow = ask[i]
        k, t, nn, c = int(key[i]), int(ts[i]), int(n[i]), int(cfg[i])
        if kind == "invalid":
            rows.append((po.INVALID, 0, 0, 0, 0.0))
            cls.append("invalid")
            continue
        if kind == "tb" and take == 0:
            rows.append((po.DENIED, 0, 0, arow[3], arow[4]))
            cls.append("empty")
            continue
        ent = sim.db.get(names_of(sim, k, t, c))
        if ent is None:
            fresh.append(i)
        elif sim._expired(ent[1], clock(i)):
            expired.append(i)
        d, rem, _, reset, tok = sim.decide(k, t, take, c, None if server_ms is None else int(server_ms[i]))
        if kind == "tb":
            got = take if d == po.ALLOWED else 0
            dec = d if d >= po.ERROR else (po.ALLOWED if got == nn else po.DENIED)
            rows.append((dec, got, rem, reset, tok))
            cls.append("error" if d >= po.ERROR else "dup_denied" if d == po.DENIED else
                       "full" if got == nn else "short")
        else:
            got = nn if d in (po.ALLOWED, po.DENIED) else 0
            rows.append((d, got, rem, reset, 0.0))
            cls.append("error" if d >= po.ERROR else "full" if d == po.ALLOWED else "over")
    return rows, {"np": np.array([a[1] for a in ask], np.int64), "cls": np.array(cls), "fresh": fresh,
                  "expired": expired}


def charge_case(kind, profile=0, seed=None):
    """-> (configs, first_trace, (key, ts, n, cfg, sms), second_trace, now_ms,
    cover): decide `first_trace`, run the call, decide `second_trace`.  sms is
    None for kind "tb" (the nullable store clock).  `cover` is the coverage
    asserted here, from apply_charge on a warmed oracle of `profile`."""
    seed = SEEDS[kind] if seed is None else seed
    configs = CONFIG_SETS[kind]
    ncfg, nkeys, m = len(configs), 120, 6000
    tr = random_trace(seed, 2 * m, nkeys, configs, fastforward=kind in ("fw", "sw"), big_n=True)
    first_trace = tuple(None if x is None else x[:m] for x in tr)
    wts, wsms = first_trace[1], first_trace[4]
    rng = np.random.default_rng(seed + 4000)
    is_tb = np.array([a == po.TOKEN_BUCKET for a, _, _ in configs])

    # the body: the warm-up's keys, amounts from 1 to more than any limit
    amounts = np.array([1, 1, 1, 2, 3, 7, 50, 1 << 62], np.int64)
    B = 1400
    key = rng.integers(0, nkeys, B).astype(np.uint64)
    if kind == "mixed":                 # a third of the keys are buckets: half of the requests go to them
        buckets = np.nonzero(is_tb[np.arange(nkeys) % ncfg])[0].astype(np.uint64)
        half = rng.random(B) < 0.5
        key[half] = buckets[rng.integers(0, buckets.size, int(half.sum()))]
    n = rng.choice(amounts, B, p=[0.25, 0.15, 0.1, 0.15, 0.1, 0.12, 0.11, 0.02])
    cfg = (key % np.uint64(ncfg)).astype(np.uint32)
    gaps = rng.choice([0, 1000, 250_000, 5_000_000, 50_000_000], B, p=[0.1, 0.4, 0.2, 0.2, 0.1])
    # keys never seen: the call inserts them
    at = np.sort(rng.choice(B, 40, replace=False))
    key[at] = np.arange(40, dtype=np.uint64) + np.uint64(30 * nkeys)
    cfg[at] = (key[at] % np.uint64(ncfg)).astype(np.uint32)
    # a request of each invalid kind
    at = rng.choice(B, 30, replace=False)
    n[at[0::5]] = 0
    n[at[1::5]] = -5
    cfg[at[2::5]] = ncfg
    cfg[at[3::5]] = ncfg + 63
    key[at[4::5]] = np.uint64(KEY_RESERVED)
    # INCRBY overflow: three times 2^62 on one window counter, at one time
    if not is_tb.all():
        wc = int(np.nonzero(~is_tb)[0][0])
        key[700:703] = np.uint64(wc + ncfg * 7)
        cfg[700:703] = wc
        n[700:703] = 1 << 62
        gaps[701:703] = 0
    ts = int(wts[-1]) + 1000 + np.cumsum(gaps).astype(np.int64)
    # the tail: the warm-up's keys long after every TTL has run out
    T = 60
    tkey = rng.integers(0, nkeys, T).astype(np.uint64)
    tts = int(ts[-1]) + LATE_MS * 1_000_000 + np.cumsum(rng.choice([1000, 250_000], T)).astype(np.int64)
    key = np.concatenate([key, tkey])
    n = np.concatenate([n, rng.choice(amounts[:7], T)])
    cfg = np.concatenate([cfg, (tkey % np.uint64(ncfg)).astype(np.uint32)])
    ts = np.concatenate([ts, tts])
    M = key.size
    # The store clock of the call.  "tb": the nullable clock, floor(ts / 1e6).
    # The others: an explicit clock that runs with ts from the warm-up's last
    # store clock on ("mixed": one ms ahead of the requests' own).
    if kind == "tb":
        sms = None
    else:
        base = int(wsms[-1]) if wsms is not None else int(wts[-1]) // 1_000_000
        sms = base + 1 + (ts - int(wts[-1])) // 1_000_000
    now_ms = int(sms[-1]) if sms is not None else int(ts[-1]) // 1_000_000
    # the trace that follows, after the call on both clocks
    skey, sts, sn, scfg, ssms = (None if x is None else x[m:] for x in tr)
    sts = sts + max(max(int(ts[-1]) + 1000, (now_ms + 1) * 1_000_000) - int(sts[0]), 0)
    if ssms is not None:
        ssms = ssms + max(now_ms - int(ssms[0]), 0)
    second_trace = (skey, sts, sn, scfg, ssms)

    # coverage, on a warmed oracle
    sim = new_sim(profile, configs)
    warm(sim, first_trace)
    rows, info = apply_charge(sim, key, ts, n, cfg, sms)
    cls = info["cls"]
    cover = {c: int((cls == c).sum()) for c in ("full", "short", "empty", "dup_denied", "over", "error", "invalid")}
    cover.update(fresh=len(info["fresh"]), expired=len(info["expired"]), rows=rows, cls=cls, np=info["np"])
    bad = (n <= 0, cfg == ncfg, cfg == ncfg + 63, key == np.uint64(KEY_RESERVED))
    assert 1400 <= M <= 1600, M
    assert len({int(k) for k in key.tolist()} - {KEY_RESERVED}) >= 110
    assert cover["full"] >= 20, cover["full"]
    if is_tb.any():
        assert cover["short"] >= 20, cover["short"]
        assert cover["empty"] >= 20, cover["empty"]
        assert cover["dup_denied"] >= 1, cover["dup_denied"]
    if not is_tb.all():
        assert cover["over"] >= 20, cover["over"]
        assert cover["error"] >= 1, cover["error"]
    assert cover["fresh"] >= 1 and cover["expired"] >= 1, (cover["fresh"], cover["expired"])
    assert all((b & (cls == "invalid")).any() for b in bad) and (n[cls == "invalid"] == 0).any() \
        and (n[cls == "invalid"] < 0).any()
    return configs, first_trace, (key, ts, n, cfg, sms), second_trace, now_ms, cover
