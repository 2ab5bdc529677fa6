"""The HBM state tables under pressure (GPU): high load, directed collisions,
full tables, the probe bound, and the spill table at and past its capacity.

Every engine here has the minimum capacities (1024 slots per table, spill
included) unless a case says otherwise.  The cases are built from
table_cases.py, whose CPU tests show that they are inside or outside a table's
capacity by construction.  All five outputs are compared with the C oracle
(test_gpu_parity.assert_same: integers equal, `tokens` bit for bit); requests
the engine must reject are left out of the oracle's trace, so the accepted
ones are compared with an oracle that saw exactly them, in order."""
import numpy as np
import pytest

import oracle
from oracle import rl_oracle_py as po
from peek_cases import assert_peek, peek_expected
from reset_cases import apply_resets, engine_keys
from table_cases import home, keys_with_home, ladder_trace, one_key_per_home, spill_demand, spill_home
from test_gpu_parity import assert_same, split
from test_peek_gpu import Rig, cat
from tracegen import CONFIG_SETS, NS, T0, random_trace

pytestmark = pytest.mark.gpu

CAP = 1024
U64 = np.uint64
LADDER = [(3, 5, 60 * NS), (2, 5, 60 * NS)]
D = 6


class PRig(Rig):
    """test_peek_gpu.Rig (engine, C oracle, Python oracle) with every capacity
    given; py=False leaves the Python oracle out (no peeks in the test)"""

    def __init__(self, rl, profile, configs, tb=CAP, win=CAP, spill=CAP, max_batch=1 << 13, py=True):
        self.rl, self.profile, self.configs, self.py = rl, profile, configs, py
        self.eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch,
                             spill_capacity=spill)
        self.csim = oracle.OracleSim(profile)
        self.psim = po.Sim(profile)
        for a, L, W in configs:
            assert self.eng.register(a, L, W) == self.csim.add_config(a, L, W) == self.psim.add_config(a, L, W)
        info = self.eng.table_info(0)
        assert (info.tb_capacity, info.win_capacity, info.spill_capacity) == (tb, win, spill)

    def decide(self, part, what=""):
        if self.py:
            return super().decide(part, what)
        key, ts, n, cfg, sms = part
        assert_same(self.eng.decide(key, ts, n, cfg, sms), self.csim.decide(key, ts, n, cfg, sms), self.configs, cfg,
                    what=what)

    def decide_some(self, part, rejected, what=""):
        """decide `part`, of which the engine must reject exactly the requests
        `rejected` (a mask) with RL_ENOMEM; the others equal the oracle fed
        only them, in order"""
        key, ts, n, cfg, sms = part
        res = self.eng.decide(key, ts, n, cfg, sms, check=False)
        assert res.status == self.rl.RL_ENOMEM, what
        bad = np.nonzero((res.decision == self.rl.INVALID) != rejected)[0]
        assert bad.size == 0, f"{what}: rejected set differs at {bad[:10]} (keys {key[bad[:10]]})"
        self.check_kept(res, part, ~rejected, what)
        return res

    def check_kept(self, res, part, keep, what=""):
        """the requests `keep` of a decided batch against the oracle fed them alone"""
        kept = tuple(None if x is None else x[keep] for x in part)
        sub = self.rl.Decisions(res.decision[keep], res.remaining[keep], res.retry_after_ns[keep],
                                res.reset_at_ns[keep], res.tokens[keep])
        assert_same(sub, self.csim.decide(*kept), self.configs, kept[3], what=what)
        if self.py:
            for i in np.nonzero(keep)[0]:
                self.psim.decide(int(part[0][i]), int(part[1][i]), int(part[2][i]), int(part[3][i]),
                                 None if part[4] is None else int(part[4][i]))

    def check_keys(self, now_ms, what=""):
        got, want = engine_keys(self.rl, self.eng, now_ms), set(self.csim.keys(now_ms))
        assert got == want, f"{what}: engine only {sorted(got - want)[:5]}, oracle only {sorted(want - got)[:5]}"

    def reset(self, key, ts, cfg, now_ms):
        key, ts, cfg = np.asarray(key, U64), np.asarray(ts, np.int64), np.asarray(cfg, np.uint32)
        status = self.eng.reset_batch(key, ts, cfg)
        assert (status == self.rl.RESET_DONE).all()
        apply_resets(self.csim, key, ts, cfg, len(self.configs), now_ms)
        if self.py:
            apply_resets(self.psim, key, ts, cfg, len(self.configs))
        self.check_keys(now_ms, "after the resets")


def requests_of(rng, ids, cfgs, lo, hi, t_start, gap_ns=400_000):
    """every id of `ids` (config cfgs[j]) with lo..hi requests, interleaved in
    a random order, at increasing times from t_start -> (batch, end time)"""
    counts = rng.integers(lo, hi + 1, ids.size)
    order = rng.permutation(int(counts.sum()))
    key = np.repeat(np.asarray(ids, U64), counts)[order]
    cfg = np.repeat(np.asarray(cfgs, np.uint32), counts)[order]
    ts = t_start + 1 + np.cumsum(rng.integers(0, gap_ns, key.size)).astype(np.int64)
    n = rng.choice([1, 1, 2], key.size).astype(np.int64)
    return (key, ts, n, cfg, None), int(ts[-1])


def whole_keys(key, rejected):
    """-> the rejected ids, after checking that every id's requests are
    rejected all or none"""
    ids, inv = np.unique(key, return_inverse=True)
    tot = np.bincount(inv)
    rej = np.bincount(inv, weights=rejected).astype(np.int64)
    assert ((rej == 0) | (rej == tot)).all(), f"keys rejected in part: {ids[(rej != 0) & (rej != tot)][:10]}"
    return ids[rej > 0]


# --- a. high load, full parity ------------------------------------------------------

def high_load_trace(seed, m=40_000):
    """random_trace over the mixed configs with its 2000 keys relabelled so
    that 1000 are token-bucket ids and 1000 window ids (cfg = id % 15 as in
    the trace: 15 j + c with c a config of the wanted kind)"""
    configs = CONFIG_SETS["mixed"]
    k, ts, n, _, sms = random_trace(seed, m, 2000, configs, big_n=True)
    k = k.astype(np.int64)
    j = k - 1000
    key = np.where(k < 1000, 15 * k + k % 5, 15 * j + 5 + j % 10).astype(U64)
    return configs, (key, ts, n, (key % U64(15)).astype(np.uint32), sms)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("small", [True, False])
def test_high_load_parity(rl, profile, small, monkeypatch):
    """Both main tables at 95 % to 100 % load: long probe runs on every path
    (k_small on and off), then the key set and a peek of every key."""
    monkeypatch.setenv("RL_SMALL_MAX", "4096" if small else "0")
    configs, tr = high_load_trace(300 + profile)
    key, ts, n, cfg, _ = tr
    alg = np.array([c[0] for c in configs])[cfg]
    ntb = np.unique(key[(n > 0) & (alg == 1)]).size
    nwin = np.unique(key[(n > 0) & (alg != 1)]).size
    assert 0.95 * CAP <= ntb < CAP and 0.95 * CAP <= nwin < CAP
    r = PRig(rl, profile, configs, max_batch=1 << 15)
    sizes = [1, 7, 1000, 4096, 4097]
    for i, part in enumerate(split(tr, sizes + [key.size - sum(sizes)])):
        r.decide(part, f"batch {i}")
    assert r.eng.sync() == 0
    now_ms = int(ts[-1]) // 1_000_000
    info = r.eng.table_info(now_ms)
    assert (info.tb_used, info.win_used) == (ntb, nwin)
    r.check_keys(now_ms)
    rng = np.random.default_rng(profile)
    ids = np.unique(key)
    absent = np.arange(200, dtype=U64) + U64(15 * 5000)
    q = np.concatenate([ids, absent])
    r.peek((q, np.full(q.size, ts[-1] + 1000), rng.choice([0, 1, 3], q.size), (q % U64(15)).astype(np.uint32), None),
           "every key and 200 absent ones")
    r.close()


# --- b. one home slot -----------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["tb", "win"])
@pytest.mark.parametrize("slot", [0, 517, 1023])
def test_one_home_slot(rl, slot, kind, profile):
    """300 keys of one home slot inserted by one launch (they race for the
    slot by CAS and form one probe run of 300; from slot 1023 the run wraps to
    slot 0), then found again, peeked next to absent ids of the same home,
    reset in part and decided again."""
    configs = [(1, 20, 12 * NS), (1, 5, 60 * NS)] if kind == "tb" else [(2, 5, 60 * NS), (3, 5, 60 * NS)]
    both = keys_with_home(CAP - 1, slot, 350)
    assert (home(both, CAP - 1) == slot).all()
    ids, never = both[:300], both[300:]
    cfgs = (np.arange(300) % 2).astype(np.uint32)
    rng = np.random.default_rng(slot + profile)
    r = PRig(rl, profile, configs, max_batch=1 << 14)

    def used():
        info = r.eng.table_info(0)
        return (info.tb_used, info.win_used)

    want = (300, 0) if kind == "tb" else (0, 300)
    t = T0
    for b in range(2):
        part, t = requests_of(rng, ids, cfgs, 1, 40, t)
        assert part[0].size > 4096                        # the full launch sequence: k_probe's CAS race
        r.decide(part, f"batch {b}")
        assert used() == want
    q = np.concatenate([ids, never])
    qc = np.concatenate([cfgs, np.arange(50, dtype=np.uint32) % 2])
    res, exp = r.peek((q, np.full(q.size, t + 1000), rng.choice([0, 1, 3], q.size), qc, None), "one home")
    assert (exp[0] == po.DENIED).any() and (exp[0] == po.ALLOWED).any()
    assert used() == want
    r.reset(ids[::2], np.full(150, t + 1000), cfgs[::2], (t + 1000) // 1_000_000)
    part, t = requests_of(rng, ids, cfgs, 1, 40, t + 1000)
    r.decide(part, "after the resets")
    assert used() == want and r.eng.sync() == 0
    r.close()


# --- c. full table, deterministic -------------------------------------------------------

FULL_CONFIGS = [(1, 5, 60 * NS), (3, 5, 60 * NS), (2, 5, 60 * NS)]    # TTLs of 120 s, 60 s, 60 s / 120 s


@pytest.mark.parametrize("hot", [5000, 13_000])
def test_full_tables_reject_whole_keys(rl, hot):
    """Both main tables hold exactly 1024 keys.  New ids are then rejected as
    whole keys -- 200 light ones and a token-bucket id with `hot` requests; at
    13 000 the rejected requests form one segment and one MSD bucket longer
    than the sort's LDS chunk of 12 288 -- while the keys that fit stay
    bit-exact.  After every key expired, GC empties the tables and the
    rejected ids fit."""
    rng = np.random.default_rng(hot)
    r = PRig(rl, 0, FULL_CONFIGS, max_batch=1 << 15, py=False)
    old = np.arange(1, 2 * CAP + 1, dtype=U64)
    old_cfg = np.concatenate([np.zeros(CAP, np.uint32), 1 + (np.arange(CAP) % 2).astype(np.uint32)])
    part, t = requests_of(rng, old, old_cfg, 2, 4, T0)
    assert part[0].size > 4096
    r.decide(part, "batch 1: exactly full")
    assert r.eng.sync() == 0
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (CAP, CAP)
    # batch 2: old keys, 200 new light ids (half of them window ids) and the hot new id
    new = np.arange(1, 202, dtype=U64) + U64(1 << 20)
    new_cfg = np.concatenate([(np.arange(200) % 3).astype(np.uint32), [0]])
    o, _ = requests_of(rng, old, old_cfg, 0, 3, t)
    l, _ = requests_of(rng, new[:200], new_cfg[:200], 1, 3, t)
    h, _ = requests_of(rng, new[200:], new_cfg[200:], hot, hot, t)
    mixed = cat(o, l, h)
    order = rng.permutation(mixed[0].size)
    ts = t + 1 + np.cumsum(rng.integers(0, 100_000, order.size)).astype(np.int64)
    part = (mixed[0][order], ts, mixed[2][order], mixed[3][order], None)
    rejected = part[0] > U64(1 << 20)
    assert rejected.sum() >= hot + 200 and (~rejected).sum() > 1000
    r.decide_some(part, rejected, "batch 2")
    assert r.eng.sync() == rl.RL_ENOMEM       # the sticky status: reported once more, and cleared by that
    assert r.eng.sync() == 0
    # batch 3: old keys only, a batch below the single-workgroup cut
    part, t = requests_of(rng, old[::2], old_cfg[::2], 1, 3, int(ts[-1]))
    assert part[0].size <= 4096
    r.decide(part, "batch 3")
    assert r.eng.sync() == 0
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (CAP, CAP)
    # past every TTL: GC drops everything, and the rejected ids now fit
    t += 1000 * NS
    _, info = r.eng.table_gc(t // 1_000_000)
    assert (info.tb_used, info.win_used, info.spill_used) == (0, 0, 0)
    part, t = requests_of(rng, new, new_cfg, 3, 12, t)
    r.decide(part, "the rejected ids after GC")
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (int((new_cfg == 0).sum()), int((new_cfg != 0).sum()))
    r.close()


# --- d. full table, racing ----------------------------------------------------------------

def test_full_tables_racing(rl, monkeypatch):
    """One launch offers 1124 ids to each empty 1024-slot table.  Which 100
    lose is a race; that exactly 100 whole keys per table lose, that the
    tables end full, that the winners are bit-exact and that the losers stay
    the same in the next batch is not."""
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    rng = np.random.default_rng(4)
    r = PRig(rl, 0, FULL_CONFIGS, max_batch=1 << 16, py=False)
    extra = 100
    ids = np.concatenate([np.arange(CAP + extra, dtype=U64) + U64(1), np.arange(CAP + extra, dtype=U64) + U64(1 << 20)])
    cfgs = np.concatenate([np.zeros(CAP + extra, np.uint32), 1 + (np.arange(CAP + extra) % 2).astype(np.uint32)])
    t, lost = T0, None
    for b in range(2):
        part, t = requests_of(rng, ids, cfgs, 1, 40, t, gap_ns=100_000)
        assert 4096 < part[0].size <= 60_000
        res = r.eng.decide(*part, check=False)
        assert res.status == rl.RL_ENOMEM
        rejected = res.decision == rl.INVALID
        gone = whole_keys(part[0], rejected)
        assert (gone < U64(1 << 20)).sum() == extra and (gone >= U64(1 << 20)).sum() == extra
        if lost is not None:
            assert np.array_equal(gone, lost), "the second batch rejected other keys"
        lost = gone
        r.check_kept(res, part, ~rejected, f"batch {b}")
        info = r.eng.table_info(0)
        assert (info.tb_used, info.win_used) == (CAP, CAP)
    r.close()


# --- e. the probe bound -------------------------------------------------------------------

# probe_insert (rl_table.h): lim = min(mask, MAX_PROBES) = 8192 for a table of
# 2^14 slots, and the loop runs p = 0 .. lim inclusive (p <= lim): 8193 slots
# are examined, the home slot and the 8192 after it.
PROBES = (1 << 13) + 1


@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("kind", ["tb", "win"])
def test_probe_bound(rl, kind, small, monkeypatch):
    """A table of 2^14 slots with a run of 8193 occupied slots that wraps past
    the last slot (one key on each home slot, so nothing depends on the order
    of insertion).  An id whose home is the run's first slot finds no slot
    within the probe bound and is rejected, though half the table is empty;
    an id whose home is the second slot is accepted on its last probe.  The
    rejection also shows that table_cases.mix64 is the device's: were it not,
    the keys would scatter and nothing would be rejected.  The two ids arrive in
    a batch of 105 requests: k_small's probe_insert, and with RL_SMALL_MAX=0
    k_probe's probe_insert_at."""
    monkeypatch.setenv("RL_SMALL_MAX", "4096" if small else "0")
    cap = 1 << 14
    mask = cap - 1
    a = cap - 4000
    configs = [(1, 5, 60 * NS), (3, 5, 60 * NS)]
    c = 0 if kind == "tb" else 1
    ids = one_key_per_home(mask, a, PROBES)
    assert np.array_equal(home(ids, mask).astype(np.int64), (a + np.arange(PROBES)) & mask)
    cand = keys_with_home(mask, a, 2)
    x_out = cand[~np.isin(cand, ids)][0]                  # home a: 8193 occupied slots ahead of it
    cand = keys_with_home(mask, a + 1, 2)
    x_in = cand[~np.isin(cand, ids)][0]                   # home a + 1: the 8193rd slot is free
    rng = np.random.default_rng(c)
    r = PRig(rl, 0, configs, tb=cap, win=cap, max_batch=1 << 14, py=False)
    cfgs = np.full(PROBES, c, np.uint32)

    def used():
        info = r.eng.table_info(0)
        return info.tb_used if kind == "tb" else info.win_used

    part, t = requests_of(rng, ids, cfgs, 1, 1, T0, gap_ns=1000)
    r.decide(part, "the run")
    assert r.eng.sync() == 0 and used() == PROBES
    # x_in's own oracle for the peek below (keys do not interact)
    own = po.Sim(0)
    for cf in configs:
        own.add_config(*cf)
    k2 = np.concatenate([[x_out, x_in, x_out, x_in, x_in], ids[:100]]).astype(U64)
    ts2 = t + 1000 * (1 + np.arange(k2.size, dtype=np.int64))
    part = (k2, ts2, np.ones(k2.size, np.int64), np.full(k2.size, c, np.uint32), None)
    r.decide_some(part, k2 == x_out, "past the run")
    for i in np.nonzero(k2 == x_in)[0]:
        own.decide(int(x_in), int(ts2[i]), 1, c)
    assert used() == PROBES + 1
    assert r.eng.sync() == rl.RL_ENOMEM and r.eng.sync() == 0
    # Peek: the rejected id is a fresh key (and raises no status); x_in is found at the end of its probes
    t = int(ts2[-1]) + 1000
    q = (np.array([x_out, x_out, x_in, x_in], U64), np.full(4, t), np.array([0, 6, 0, 3]), np.full(4, c, np.uint32), None)
    res = r.eng.peek(*q)
    assert r.eng.sync() == 0
    fresh = po.Sim(0)
    for cf in configs:
        fresh.add_config(*cf)
    assert_peek(res, tuple(np.concatenate([f[:2], o[2:]])
                           for f, o in zip(peek_expected(fresh, *q), peek_expected(own, *q))), configs, q[3], "peek")
    assert list(res.decision[:2]) == [rl.ALLOWED, rl.DENIED]
    assert res.remaining[2] == 2                          # x_in: three of its five taken
    # Reset of the rejected id: nothing to delete, nothing inserted
    before = engine_keys(rl, r.eng, t // 1_000_000)
    assert (r.eng.reset_batch([x_out], [t], [c]) == rl.RESET_DONE).all()
    assert engine_keys(rl, r.eng, t // 1_000_000) == before and used() == PROBES + 1
    # Reset of x_in, found on its last probe; the next request creates it anew in its slot
    r.reset([x_in], [t], [c], t // 1_000_000)
    r.decide((np.array([x_in], U64), np.array([t + 1000]), np.array([2]), np.array([c], np.uint32), None), "x_in again")
    assert used() == PROBES + 1
    # GC at the same capacity keeps every key, wherever the rehash's race puts the two of home a + 1
    _, info = r.eng.table_gc(t // 1_000_000, 0, 0)
    assert (info.tb_capacity, info.win_capacity) == (cap, cap) and used() == PROBES + 1
    allk = np.concatenate([ids, [x_in]]).astype(U64)
    part, t = requests_of(rng, allk, np.full(allk.size, c, np.uint32), 1, 2, t, gap_ns=1000)
    r.decide(part, "after GC")
    assert r.eng.sync() == 0 and used() == PROBES + 1
    r.close()


# --- f. spill at load -------------------------------------------------------------------

def ladder_pairs(ids, t_ns):
    """(key, ts, cfg) of every (user key, window) pair of the ladder at true time t_ns"""
    key = np.repeat(np.asarray(ids, U64), D)
    cfg = (key % U64(len(LADDER))).astype(np.uint32)
    W = np.array([c[2] for c in LADDER], np.int64)[cfg]
    return key, t_ns - np.tile(np.arange(D, dtype=np.int64), len(ids)) * W, cfg


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("K,rounds,whole", [(250, 4, False), (256, 4, False), (256, 4, True), (250, 8, True),
                                            (256, 8, True), ("one home", 4, False), ("one home", 8, True)])
def test_spill_at_load(rl, profile, K, rounds, whole):
    """ladder_trace: every user key keeps 6 window keys alive, 4 of them in the
    spill: K = 250 needs 1000 of its 1024 slots, K = 256 all of them, and "one
    home" is 256 user keys whose spill home is the last slot, one run that wraps
    through the whole table.  24 requests per key replay as light segments (one
    thread each), 48 as heavy ones (a wave, whose lanes claim together); split,
    the first two batches take k_small.  Then a peek of every window key, a
    batched Reset of a third of them, a second ladder, and GC twice -- with
    nspill recounted by k_spill_rehash -- each followed by another round."""
    if K == "one home":
        ids = keys_with_home(CAP - 1, CAP - 1, 256, spill=True)
        assert (spill_home(ids, CAP - 1) == CAP - 1).all()
    else:
        ids = np.arange(K, dtype=U64) + U64(1 << 20)
    K = ids.size
    r = PRig(rl, profile, LADDER, max_batch=1 << 14)
    tr = ladder_trace(50 + profile, K, D, rounds, LADDER, ids=ids)
    m = tr[0].size
    seen = []
    for i, part in enumerate([tr] if whole else split(tr, [1, 500, m - 501])):
        res = r.eng.decide(*part)
        ref = r.csim.decide(*part)
        assert_same(res, ref, LADDER, part[3], f"ladder batch {i}")
        for k, t, n, c, s in zip(*part):
            r.psim.decide(int(k), int(t), int(n), int(c), int(s))
        seen.append(ref[0])
    seen = np.concatenate(seen)
    assert (seen == po.ALLOWED).any() and (seen == po.DENIED).any()

    def check(now_ms, what, exact=False):
        assert r.eng.sync() == 0, what
        r.check_keys(now_ms, what)
        info = r.eng.table_info(now_ms)
        assert info.spill_capacity == CAP
        assert info.spill_live == spill_demand(r.csim, now_ms) == K * (D - 2), what
        assert info.spill_used <= CAP, what
        if exact:
            assert info.spill_used == info.spill_live, what
        return info

    now_ms = int(tr[4][-1])
    check(now_ms, "after the ladder")
    # every (key, window) pair, peeked
    t1 = T0 + 30 * NS
    now_ms = t1 // 1_000_000
    rng = np.random.default_rng(K + rounds)
    pk, pt, pc = ladder_pairs(ids, t1)
    r.peek((pk, pt, rng.choice([0, 1, 2, 6], pk.size), pc, np.full(pk.size, now_ms)), "every window key", now_ms)
    # a third of them reset at the skewed times
    pick = rng.permutation(pk.size)[:pk.size // 3]
    r.reset(pk[pick], pt[pick], pc[pick], now_ms)
    assert r.eng.table_info(now_ms).spill_live < K * (D - 2)
    # a second ladder over the same keys brings every window key back
    for j, (rounds2, gc) in enumerate([(2, None), (1, (0, 0)), (1, (0, 4 * CAP))]):
        if gc:
            _, info = r.eng.table_gc(now_ms, *gc)
            assert info.win_capacity == (gc[1] or CAP)
            check(now_ms, f"after GC {gc}", exact=True)
        tr = ladder_trace(60 + j, K, D, rounds2, LADDER, span_s=2, t0=t1 + 2 * j * NS, ids=ids)
        r.decide(tr, f"ladder {j + 2}")
        now_ms = int(tr[4][-1])
        check(now_ms, f"after ladder {j + 2}", exact=gc is not None)
    r.close()


# --- g. spill exhaustion ----------------------------------------------------------------

@pytest.mark.parametrize("profile,small", [(0, True), (1, False)])
def test_spill_exhaustion(rl, profile, small, monkeypatch):
    """A ladder of K = 300 needs 1200 spill slots of 1024.  RL_ENOMEM is
    reported by the batch in which the oracle's spill demand first passes
    1024, and by none before; token-bucket keys and window keys that never
    spill, in the same batches, stay bit-exact; the spill ends full.  What the
    ladder's own keys answer between exhaustion and expiry is deliberately not
    asserted: a window key that found no spill slot is lost, which the oracle
    cannot model.  Once everything has expired GC empties the tables, and a
    ladder that fits matches the same oracle again.  (The batches are below the
    single-workgroup cut: once with k_small, once with the full launch sequence.)"""
    monkeypatch.setenv("RL_SMALL_MAX", "4096" if small else "0")
    configs = LADDER + [(1, 5, 60 * NS)]
    rng = np.random.default_rng(9 + profile)
    lad = ladder_trace(70 + profile, 300, D, 4, LADDER)
    m = lad[0].size
    # 300 token-bucket keys and 200 window keys at skew 0 (one live window each), 8 requests each
    xk = np.repeat(np.concatenate([np.arange(300, dtype=U64) + U64(1), np.arange(200, dtype=U64) + U64(1 << 30)]), 8)
    xk = xk[rng.permutation(xk.size)]
    xc = np.where(xk < U64(1 << 30), 2, (xk % U64(2)).astype(np.int64)).astype(np.uint32)
    xt = T0 + np.sort(rng.integers(0, 30 * NS, xk.size)).astype(np.int64)
    key, ts, n, cfg, sms = (np.concatenate(p) for p in zip(
        lad, (xk, xt, rng.choice([1, 1, 2], xk.size).astype(np.int64), xc, xt // 1_000_000)))
    order = np.argsort(sms, kind="stable")                 # merged by the store clock, which stays monotone
    tr = (key[order], ts[order], n[order], cfg[order], sms[order])
    side = (tr[0] < U64(1 << 20)) | (tr[0] >= U64(1 << 30))
    assert side.sum() == xk.size
    r = PRig(rl, profile, configs, max_batch=1 << 13, py=False)
    first_full, M = None, tr[0].size
    sizes = [M // 8] * 7 + [M - 7 * (M // 8)]
    for i, part in enumerate(split(tr, sizes)):
        res = r.eng.decide(*part, check=False)
        ref = r.csim.decide(*part)
        demand = spill_demand(r.csim, int(part[4][-1]))
        if first_full is None:
            if demand <= CAP:
                assert res.status == 0, f"batch {i}: RL_ENOMEM at a spill demand of {demand}"
                assert_same(res, ref, configs, part[3], f"batch {i}")
            else:
                first_full = i
                assert res.status == rl.RL_ENOMEM, f"batch {i}: spill demand {demand} and no RL_ENOMEM"
                assert r.eng.sync() == rl.RL_ENOMEM and r.eng.sync() == 0
        assert res.status in (0, rl.RL_ENOMEM)
        keep = side[sum(sizes[:i]):sum(sizes[:i + 1])]
        sub = rl.Decisions(res.decision[keep], res.remaining[keep], res.retry_after_ns[keep], res.reset_at_ns[keep],
                           res.tokens[keep])
        assert_same(sub, tuple(x[keep] for x in ref), configs, part[3][keep], f"batch {i}: keys outside the ladder")
    assert first_full is not None and 0 < first_full < len(sizes) - 1
    r.eng.sync()
    info = r.eng.table_info(int(tr[4][-1]))
    assert info.spill_used == CAP and info.tb_used == 300 and info.win_used == 500
    # past every TTL everything is expired, in the engine and in the oracle
    t2 = T0 + 600 * NS
    assert r.csim.keys(t2 // 1_000_000) == []
    _, info = r.eng.table_gc(t2 // 1_000_000)
    assert (info.spill_used, info.win_used, info.tb_used) == (0, 0, 0)
    lad = ladder_trace(80 + profile, 200, D, 4, LADDER, t0=t2)
    r.decide(lad, "a ladder that fits")
    assert r.eng.sync() == 0
    now_ms = int(lad[4][-1])
    r.check_keys(now_ms)
    assert r.eng.table_info(now_ms).spill_live == spill_demand(r.csim, now_ms) == 200 * (D - 2)
    r.close()
