"""Cases and the expected state for AllowAll (rl_allow_all_batch).

The verb is a composition, and so is its expectation on the Python oracle:
`apply_allow_all` runs `Sim.decide` per member in array order, the settle rule
in plain Python, and `refund_cases.apply_refunds` with n = g.

`allow_all_case` builds a warm-up trace, one AllowAll call of about 1500
members in groups of 1 to 16 over about 120 keys, and the trace that follows.
It asserts its own coverage from the oracle.

`scan_group` is a plain-Python model of the settle kernel's two bounded scans;
`run_group` is the direct "maximal run" definition it must agree with.
"""
import copy

import numpy as np

from oracle import rl_oracle_py as po
from refund_cases import DONE, INVALID, NOKEY, apply_refunds, new_sim, warm
from reset_cases import KEY_RESERVED
from tracegen import CONFIG_SETS, NS, random_trace

MAX_GROUP = 16
KINDS = ["tb", "fw", "sw", "mixed"]
# the seed of each kind's case: checked on the CPU (test_allow_all_cases.py) to
# meet the coverage the builder asserts
SEEDS = {"tb": 200, "fw": 201, "sw": 202, "mixed": 203}
ALG_NAME = {po.TOKEN_BUCKET: "tb", po.SLIDING_WINDOW: "sw", po.FIXED_WINDOW: "fw"}
# severity of a decision code: ALLOWED < DENIED < ERROR < INVALID
SEVERITY = {po.ALLOWED: 0, po.DENIED: 1, po.ERROR: 2, po.INVALID: 3}
BY_SEVERITY = {v: k for k, v in SEVERITY.items()}


# --- groups -----------------------------------------------------------------------

def run_group(first, i):
    """the definition: the maximal run that holds member i -> (head, end), end
    exclusive.  Member j starts a group when j == 0 or first[j] != 0."""
    m = len(first)
    head = i
    while head > 0 and not first[head]:
        head -= 1
    end = i + 1
    while end < m and not first[end]:
        end += 1
    return head, end


def scan_group(first, i, cap=MAX_GROUP):
    """the kernel's two bounded scans -> (head, end), or None for a run longer
    than cap: back at most cap members for the head, then from the head forward
    at most cap members for the end"""
    m = len(first)
    head = None
    for d in range(cap):
        h = i - d
        if h == 0 or first[h]:
            head = h
            break
    if head is None:
        return None
    for d in range(1, cap + 1):
        e = head + d
        if e >= m or first[e]:
            return head, e
    return None


def group_spans(first):
    """[(head, end)] of every group, in order"""
    heads = [i for i in range(len(first)) if i == 0 or first[i]]
    return list(zip(heads, heads[1:] + [len(first)]))


# --- the composition on the oracle ------------------------------------------------

def settle(sim, first, n, cfg, decisions, cap=MAX_GROUP):
    """the settle rule -> (verdict, g)"""
    m = len(first)
    verdict = np.empty(m, np.uint8)
    g = np.zeros(m, np.int64)
    for head, end in group_spans(first):
        if end - head > cap:
            v = po.INVALID
        else:
            v = BY_SEVERITY[max(SEVERITY[int(decisions[j])] for j in range(head, end))]
        verdict[head:end] = v
        if v == po.ALLOWED:
            continue
        for j in range(head, end):
            c, d = int(cfg[j]), int(decisions[j])
            if not 0 <= c < len(sim.cfgs):
                continue
            took = d == po.ALLOWED if sim.cfgs[c][0] == po.TOKEN_BUCKET else d in (po.ALLOWED, po.DENIED)
            if took:
                g[j] = int(n[j])
    return verdict, g


def decide_rows(sim, key, ts, n, cfg, server_ms=None):
    """Sim.decide per member in order; the reserved key id is not executed"""
    rows = []
    for i in range(len(key)):
        if int(key[i]) == KEY_RESERVED:
            rows.append((po.INVALID, 0, 0, 0, float("nan")))
            continue
        rows.append(sim.decide(int(key[i]), int(ts[i]), int(n[i]), int(cfg[i]),
                               None if server_ms is None else int(server_ms[i])))
    return rows


def apply_allow_all(sim, key, ts, n, cfg, first, server_ms=None):
    """one AllowAll call on sim -> (rows, verdict, g, rollback, info): decide,
    settle, refund; info is apply_refunds'"""
    rows = decide_rows(sim, key, ts, n, cfg, server_ms)
    verdict, g = settle(sim, first, n, cfg, [r[0] for r in rows])
    rollback, info = apply_refunds(sim, key, ts, g, cfg, server_ms)
    return rows, verdict, g, rollback, info


# --- the seeded case --------------------------------------------------------------

def allow_all_case(kind, profile=0, seed=None):
    """-> (configs, first_trace, (key, ts, n, cfg, sms, first), second_trace,
    now_ms, cover): decide `first_trace`, run the call, decide `second_trace`.
    sms is None for kind "tb" (the nullable store clock).  `cover` is the
    coverage asserted here, from apply_allow_all on a warmed oracle."""
    seed = SEEDS[kind] if seed is None else seed
    configs = CONFIG_SETS[kind]
    ncfg, nkeys, m = len(configs), 120, 6000
    tr = random_trace(seed, 2 * m, nkeys, configs, fastforward=kind in ("fw", "sw"), big_n=True)
    first_trace = tuple(None if x is None else x[:m] for x in tr)
    wts, wsms = first_trace[1], first_trace[4]
    rng = np.random.default_rng(seed + 3000)
    algs = sorted({ALG_NAME[a] for a, _, _ in configs})

    # the groups: sizes 1 to 16, small ones more often (they are the ones that pass)
    sizes = rng.choice(np.arange(1, 17), 260, p=np.array([6, 6, 4, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2]) / 34.0)
    groups = []                                     # [(keys, n, cfg)]
    amounts = np.array([1, 1, 1, 2, 3, 7, 50], np.int64)
    for s in sizes.tolist():
        gk = rng.integers(0, nkeys, s).astype(np.uint64)
        groups.append([gk, rng.choice(amounts, s), (gk % np.uint64(ncfg)).astype(np.uint32)])
    # groups with a member that is not executed: n = 0, n < 0, an unknown config, the reserved key
    for j, at in enumerate((5, 60, 130, 200)):
        gk, gn, gc = groups[at]
        if j == 0:
            gn[0] = 0
        elif j == 1:
            gn[-1] = -4
        elif j == 2:
            gc[0] = ncfg + 2
        else:
            gk[-1] = np.uint64(KEY_RESERVED)
    # runs of 17 and of 33 members
    for at, s in ((90, 17), (210, 33)):
        gk = rng.integers(0, nkeys, s).astype(np.uint64)
        groups.insert(at, [gk, np.ones(s, np.int64), (gk % np.uint64(ncfg)).astype(np.uint32)])
    # a transient take, on keys of config 0 nobody else uses: A has all its
    # quota, B is asked for twice its limit.  [A, B] fails and A's take is given
    # back -- after [A] has seen it and was denied
    L0 = configs[0][1]
    A, B = np.uint64(ncfg * 300), np.uint64(ncfg * 301)
    take = np.int64(3 * L0 // 4)
    t_first, t_second = 40, 140
    groups.insert(t_first, [np.array([A, B]), np.array([take, 2 * L0], np.int64), np.zeros(2, np.uint32)])
    groups.insert(t_second, [np.array([A]), np.array([take], np.int64), np.zeros(1, np.uint32)])

    key = np.concatenate([g[0] for g in groups]).astype(np.uint64)
    n = np.concatenate([g[1] for g in groups]).astype(np.int64)
    cfg = np.concatenate([g[2] for g in groups]).astype(np.uint32)
    first = np.zeros(key.size, np.uint8)
    heads = np.cumsum([0] + [g[0].size for g in groups[:-1]])
    first[heads] = rng.choice([1, 1, 2, 255], heads.size)
    first[0] = 0                                    # member 0 starts a group whatever its byte
    M = key.size
    gaps = rng.choice([0, 1000, 250_000, 5_000_000, 50_000_000], M, p=[0.1, 0.4, 0.2, 0.2, 0.1])
    ts = int(wts[-1]) + 1000 + np.cumsum(gaps).astype(np.int64)
    # The store clock of the call.  Window kinds: one clock for the whole call
    # (the store's clock is not the callers'), so that no window key a member
    # counted on dies between its decide and its give-back, both at that clock.
    # "tb": the nullable clock, floor(ts / 1e6); a bucket's TTL is renewed by
    # every request.
    if kind == "tb":
        sms, now_ms = None, int(ts[-1]) // 1_000_000
    else:
        now_ms = (int(wsms[-1]) if wsms is not None else int(wts[-1]) // 1_000_000) + 1
        sms = np.full(M, now_ms, np.int64)
    # the trace that follows, after the call on both clocks
    skey, sts, sn, scfg, ssms = (None if x is None else x[m:] for x in tr)
    shift = max(int(ts[-1]) + 1000, now_ms * 1_000_000) - int(sts[0])
    sts = sts + max(shift, 0)
    if ssms is not None:
        ssms = ssms + max(now_ms - int(ssms[0]), 0)
    elif kind != "tb":
        assert int(sts[0]) // 1_000_000 >= now_ms
    second_trace = (skey, sts, sn, scfg, ssms)

    # coverage, on a warmed oracle
    sim = new_sim(profile, configs)
    warm(sim, first_trace)
    warmed = copy.deepcopy(sim)
    rows, verdict, g, rollback, info = apply_allow_all(sim, key, ts, n, cfg, first, sms)
    dec = np.array([r[0] for r in rows], np.uint8)
    alg_of = lambda j: ALG_NAME[configs[int(cfg[j])][0]] if int(cfg[j]) < ncfg else None
    spans = group_spans(first)
    assert len(spans) == len(groups) and all(e - h == grp[0].size for (h, e), grp in zip(spans, groups))
    cover = {"allowed": 0, "failed_by": {a: 0 for a in algs}, "tb_rolled_back": 0, "win_denied_rolled_back": 0,
             "nokey": int(((rollback == NOKEY) & (g > 0)).sum()), "invalid_member": 0, "long_runs": [],
             "merged": sum(1 for idx in info["targets"].values() if len(idx) >= 2)}
    for h, e in spans:
        v = int(verdict[h])
        assert (verdict[h:e] == v).all()
        if e - h > MAX_GROUP:
            assert v == po.INVALID
            cover["long_runs"].append(e - h)
            continue
        if v == po.ALLOWED:
            cover["allowed"] += 1
            assert (g[h:e] == 0).all() and (rollback[h:e] == INVALID).all()
        if (dec[h:e] == po.INVALID).any():
            cover["invalid_member"] += 1
            assert v == po.INVALID
        if v == po.DENIED:
            for a in {alg_of(j) for j in range(h, e) if dec[j] == po.DENIED}:
                cover["failed_by"][a] += 1
        if v != po.ALLOWED:
            if any(alg_of(j) == "tb" and dec[j] == po.ALLOWED and g[j] > 0 for j in range(h, e)):
                cover["tb_rolled_back"] += 1
            cover["win_denied_rolled_back"] += sum(1 for j in range(h, e) if alg_of(j) in ("fw", "sw") and
                                                   dec[j] == po.DENIED and g[j] > 0 and rollback[j] == DONE)
    # the transient take: [A] is denied in the call, and allowed in the same
    # call without the group [A, B] before it
    h1, e1 = spans[t_first]
    h2, e2 = spans[t_second]
    assert key[h1] == A and key[h2] == A and e2 - h2 == 1
    assert verdict[h1] == po.DENIED and dec[h1] == po.ALLOWED and g[h1] == take
    assert verdict[h2] == po.DENIED
    keep = np.ones(M, bool)
    keep[h1:e1] = False
    without = copy.deepcopy(warmed)
    _, v2, _, _, _ = apply_allow_all(without, key[keep], ts[keep], n[keep], cfg[keep], first[keep],
                                     None if sms is None else sms[keep])
    cover["transient"] = int(v2[h2 - (e1 - h1)]) == po.ALLOWED
    cover.update(verdict=verdict, g=g, rollback=rollback, decision=dec)

    assert 1400 <= M <= 1800, M
    assert len({int(k) for k in key.tolist()} - {KEY_RESERVED}) >= 110
    assert cover["allowed"] >= 40, cover["allowed"]
    for a in algs:
        assert cover["failed_by"][a] >= 40, cover["failed_by"]
    if "tb" in algs:
        assert cover["tb_rolled_back"] >= 20, cover["tb_rolled_back"]
    if kind != "tb":
        assert cover["win_denied_rolled_back"] >= 20, cover["win_denied_rolled_back"]
    assert cover["nokey"] >= 1
    assert cover["transient"]
    assert cover["merged"] >= 1
    assert cover["invalid_member"] >= 4
    assert sorted(cover["long_runs"]) == [17, 33]
    return configs, first_trace, (key, ts, n, cfg, sms, first), second_trace, now_ms, cover
