"""Cases and the expected state for Refund (rl_refund_batch).

There is no reference script for this verb: the contract is restated here on
the Python oracle's keyspace (`oracle.rl_oracle_py.Sim.db`).  `apply_refunds`
groups the valid requests of one call by target, sums the n of those whose
target is live at their own store clock, and runs one script per target:

    token bucket   tokens = math.min(capacity, tokens + N), through tostring
    window         if count <= N then DEL else DECRBY N

Nothing is deleted lazily and nothing is inserted.

`refund_case` builds, on `reset_cases.reset_case`'s warm-up (6000 requests over
60 keys; 90 for the token buckets, see refund_case): a refund call of about
1000 requests aimed at the warm-up's own (key, ts) at their own store clocks, at the window after and before, at keys
never seen, at keys expired at the refund's store clock, invalid requests and
duplicates; and the trace that follows.  It asserts its own coverage.
"""
import numpy as np

from oracle import rl_oracle_py as po
from reset_cases import KEY_RESERVED, reset_case

NOKEY, DONE, INVALID = 0, 1, 3
INT64_MAX = (1 << 63) - 1
KINDS = ["tb", "fw", "sw", "mixed", "skew"]
# the seed of each kind's case: checked on the CPU (test_refund_cases.py) to
# meet the coverage the builder asserts
SEEDS = {"tb": 100, "fw": 101, "sw": 102, "mixed": 103, "skew": 104}


def total(ns):
    """N of a target: the sum of its contributors' n, saturated"""
    return min(sum(ns), INT64_MAX)


def split_sum(ns):
    """the device's form of the sum: the low and the high 32 bits of every n
    added apart, then hi * 2^32 + lo with the carry, saturated"""
    lo = sum(n & 0xffffffff for n in ns)
    hi = sum(n >> 32 for n in ns)
    h = hi + (lo >> 32)
    return INT64_MAX if h >= 1 << 31 else h << 32 | (lo & 0xffffffff)


def target_of(sim, key, ts, cfg):
    """the db key a valid request refunds"""
    alg, L, W = sim.cfgs[cfg]
    if alg == po.TOKEN_BUCKET:
        return "tb:%d" % key
    return "w:%d:%d" % (key, po.window_start(ts, W))


def apply_refunds(sim, key, ts, n, cfg, server_ms=None):
    """one refund call on sim.db -> (status, info); info: `targets` {db key:
    [request indices that contributed]}, `deleted` [db keys], `expired`
    [indices whose target is in the db but dead at the request's clock]"""
    m = len(key)
    status = np.full(m, INVALID, np.uint8)
    targets, expired = {}, []
    for i in range(m):
        k, t, nn, c = int(key[i]), int(ts[i]), int(n[i]), int(cfg[i])
        if not (0 <= c < len(sim.cfgs)) or nn <= 0 or k == KEY_RESERVED:
            continue
        s_ms = int(server_ms[i]) if server_ms is not None else t // 1_000_000
        name = target_of(sim, k, t, c)
        ent = sim.db.get(name)
        if ent is None or sim._expired(ent[1], s_ms):
            status[i] = NOKEY
            if ent is not None:
                expired.append(i)
            continue
        status[i] = DONE
        targets.setdefault(name, []).append(i)
    deleted = []
    for name, idx in targets.items():
        N = total([int(n[i]) for i in idx])
        ent = sim.db[name]
        if name.startswith("tb:"):
            cap = float(sim.cfgs[int(cfg[idx[0]])][1])
            tokens, last = ent[0]
            s = tokens + float(N)
            ent[0] = (po.lua_roundtrip(s if s < cap else cap, sim.profile), last)
        elif ent[0] <= N:
            del sim.db[name]
            deleted.append(name)
        else:
            ent[0] -= N
    return status, {"targets": targets, "deleted": deleted, "expired": expired}


def py_peek(sim, key, ts, cfg, s_ms):
    """the n = 0 status query on the Python oracle: the script's arithmetic
    with requested = 0 and none of its writes (nor its lazy deletes)"""
    alg, L, W = sim.cfgs[cfg]
    if alg == po.TOKEN_BUCKET:
        names = ["tb:%d" % key]
    else:
        ws = po.window_start(ts, W)
        names = ["w:%d:%d" % (key, ws), "w:%d:%d" % (key, ws - po.go_f2i(po.duration_seconds(W)))]
    saved = {k: (None if sim.db.get(k) is None else list(sim.db[k])) for k in names}
    fn = {po.TOKEN_BUCKET: sim._tb, po.SLIDING_WINDOW: sim._sw, po.FIXED_WINDOW: sim._fw}[alg]
    out = fn(L, W, key, ts, 0, s_ms)
    for k, v in saved.items():
        if v is None:
            sim.db.pop(k, None)
        else:
            sim.db[k] = v
    return out


def new_sim(profile, configs):
    sim = po.Sim(profile)
    for a, L, W in configs:
        sim.add_config(a, L, W)
    return sim


def warm(sim, tr):
    key, ts, n, cfg, sms = tr
    return [sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]), None if sms is None else int(sms[i]))
            for i in range(len(key))]


def refund_case(kind, profile=0, seed=None):
    """-> (configs, first, (rkey, rts, rn, rcfg, rsms), second, now_ms, cover):
    decide `first`, refund the call, decide `second`.  rsms is None for kind
    "tb" (the nullable store clock: floor(ts / 1e6)).  `cover` is the coverage
    the builder asserts, from apply_refunds on a warmed oracle of `profile`."""
    seed = SEEDS[kind] if seed is None else seed
    # 120 keys, not reset_case's 60: a refund must not take a key's store clock
    # back (below), so the live targets are the newest windows of each key, and
    # a sixth to a third of the keys (windows below 1 s: a TTL of int64(0.7) s
    # = 0 deletes the key at once) never have any; 60 keys leave fewer than the
    # 50 merged targets asserted here
    nkeys = 120
    configs, first, _, second, now_ms = reset_case(kind, seed, nkeys=nkeys, ff=kind in ("fw", "sw"))
    key, ts, n, cfg, sms = first
    m, ncfg = key.size, len(configs)
    clock = sms if sms is not None else ts // 1_000_000
    rng = np.random.default_rng(seed + 2000)
    W = np.array([c[2] for c in configs], np.int64)
    ok = np.nonzero(n > 0)[0]
    late = 10 ** 7                      # ms past the warm-up's end: every TTL here has run out
    amounts = np.array([1, 1, 1, 2, 3, 7, 50, 10 ** 6, 1 << 62], np.int64)

    # A user key's refunds carry the store clock of its last warm-up request
    # (or a later one): a store clock that went back for a key would ask for
    # window keys the engine has already reclaimed as expired (rl_window.h).
    last_clock, newest = {}, {}
    for i in ok.tolist():
        k = int(key[i])
        last_clock[k] = int(clock[i])
        newest[k] = (newest.get(k, ()) + (i,))[-2:]
    key_clock = lambda idx: np.array([last_clock[k] for k in key[idx].tolist()], np.int64)
    recent = np.array(sorted(i for v in newest.values() for i in v))   # every key's last two requests

    def own(count, p_amount, pool=ok):
        idx = pool[rng.integers(0, pool.size, count)]
        return idx, rng.choice(amounts, count, p=p_amount)

    usual = [0.3, 0.15, 0.1, 0.15, 0.1, 0.08, 0.06, 0.04, 0.02]
    parts = []                          # (key, ts, n, cfg, clock, class)
    # the warm-up's own (key, ts): every key's last two requests, whose windows
    # are live at the key's clock, and any request (windows of any age); some twice
    a_idx, a_n = own(300, usual, np.array(sorted(v[-1] for v in newest.values())))
    for count, pool in ((150, recent), (150, ok)):
        o_idx, o_n = own(count, usual, pool)
        a_idx, a_n = np.concatenate([a_idx, o_idx]), np.concatenate([a_n, o_n])
    parts.append((key[a_idx], ts[a_idx], a_n, cfg[a_idx], key_clock(a_idx), "own"))
    parts.append((key[a_idx[:150]], ts[a_idx[:150]], rng.choice(amounts[:7], 150), cfg[a_idx[:150]],
                  key_clock(a_idx[:150]), "dup"))
    # the same at the warm-up's last clock: live or expired by then
    e_idx, e_n = own(60, usual, recent)
    parts.append((key[e_idx], ts[e_idx], e_n, cfg[e_idx], np.full(60, now_ms), "now"))
    # the window after and the window before
    b_idx, b_n = own(100, usual, recent)
    shift = rng.choice([1, -1], 100)
    parts.append((key[b_idx], ts[b_idx] + shift * W[cfg[b_idx]], b_n, cfg[b_idx], key_clock(b_idx), "shift"))
    # keys never seen
    absent = np.arange(40, dtype=np.uint64) + np.uint64(30 * nkeys)
    parts.append((absent, np.full(40, ts[-1]), np.full(40, 3, np.int64), (absent % np.uint64(ncfg)).astype(np.uint32),
                  np.full(40, now_ms), "absent"))
    # keys expired at the refund's store clock
    x_idx, x_n = own(80, usual)
    parts.append((key[x_idx], ts[x_idx], x_n, cfg[x_idx], np.full(80, now_ms + late), "expired"))
    # invalid requests
    i_idx, _ = own(30, usual)
    ik, in_, ic = key[i_idx].copy(), np.full(30, 2, np.int64), cfg[i_idx].copy()
    in_[0::5] = 0
    in_[1::5] = -5
    ic[2::5] = ncfg
    ic[3::5] = ncfg + 63
    ik[4::5] = np.uint64(KEY_RESERVED)
    parts.append((ik, ts[i_idx], in_, ic, key_clock(i_idx), "invalid"))

    cls = np.concatenate([np.full(p[0].size, p[5]) for p in parts])
    rkey = np.concatenate([p[0] for p in parts]).astype(np.uint64)
    rts = np.concatenate([p[1] for p in parts]).astype(np.int64)
    rn = np.concatenate([p[2] for p in parts]).astype(np.int64)
    rcfg = np.concatenate([p[3] for p in parts]).astype(np.uint32)
    rsms = np.concatenate([p[4] for p in parts]).astype(np.int64)
    if kind == "tb":
        # the nullable store clock: a bucket's target does not depend on ts, so
        # the request's time carries the clock
        rts = rsms * 1_000_000 + rts % 1_000_000
        rsms = None
    order = rng.permutation(rkey.size)
    rkey, rts, rn, rcfg, cls = rkey[order], rts[order], rn[order], rcfg[order], cls[order]
    if rsms is not None:
        rsms = rsms[order]

    # coverage, on a warmed oracle
    sim = new_sim(profile, configs)
    warm(sim, first)
    live_keys = {k: sum(1 for name, (v, when) in sim.db.items()
                        if name.startswith("w:%d:" % k)) for k in range(nkeys)}
    status, info = apply_refunds(sim, rkey, rts, rn, rcfg, rsms)
    cover = {
        "done": int((status == DONE).sum()),
        "nokey_absent": int(((status == NOKEY) & (cls == "absent")).sum()),
        "nokey_expired": len(info["expired"]),
        "invalid": int((status == INVALID).sum()),
        "merged": sum(1 for idx in info["targets"].values() if len(idx) >= 2),
        "deleted": len(info["deleted"]),
        # window targets of user keys that own more than two window keys: the
        # entry holds two, the others live in the spill
        "crowded": sum(1 for name in info["targets"] if name.startswith("w:") and
                       live_keys[int(name.split(":")[1])] > 2),
        "status": status,
    }
    assert rkey.size >= 900
    assert cover["done"] >= 300, cover
    assert cover["nokey_absent"] >= 20, cover
    assert cover["nokey_expired"] >= 20, cover
    assert cover["invalid"] >= 10, cover
    assert cover["merged"] >= 50, cover
    if kind != "tb":                    # only a window key is ever deleted
        assert cover["deleted"] >= 5, cover
    if kind == "skew":
        assert cover["crowded"] >= 1, cover
    return configs, first, (rkey, rts, rn, rcfg, rsms), second, now_ms, cover


def bucket_counterexample(limit=10 ** 6, tries=4000, seed=7):
    """a stored 14-digit token count t and amounts a, b with
    q14(q14(t + a) + b) != q14(t + a + b): the fixed example of §10i first,
    then a seeded search -> [(t, a, b)]"""
    q = lambda x: po.lua_roundtrip(x, po.REDIS7)
    out = []
    rng = np.random.default_rng(seed)
    cand = [(0.9763120008305, 4, 45)]
    cand += [(q(float(rng.random())), int(rng.integers(1, 50)), int(rng.integers(1, 50))) for _ in range(tries)]
    for t, a, b in cand:
        if q(q(t + float(a)) + float(b)) != q(t + float(a + b)):
            out.append((t, a, b))
    return out
