"""Read-only quota queries (rl_peek_batch) on the GPU.

Every peek result -- and `tokens` as bit patterns -- is compared with
peek_cases.peek_expected over the Python oracle, which is fed the same decide
trace.  The engine's ordinary decisions in the same tests are still checked
against the C oracle, which runs the whole decide trace uninterrupted and never
sees a peek: a peek that wrote anything would show there, and in the table
fingerprints taken around every peek batch."""
import threading

import numpy as np
import pytest

import oracle
import rl_snapshot as snap
from oracle import rl_oracle_py as po
from peek_cases import assert_peek, peek_expected, sim_decide
from tracegen import CONFIG_SETS, NS, T0, random_config_trace, random_trace, skewed_trace

pytestmark = pytest.mark.gpu

BIG = 1 << 62


def assert_same(res, ref, configs, cfg, what=""):
    """test_gpu_parity.py's comparison with the C oracle"""
    dec, rem, retry, reset, tok = ref
    bad = np.nonzero(res.decision != dec)[0]
    assert bad.size == 0, f"{what} decision mismatch at {bad[:10]}: gpu={res.decision[bad[:10]]} ref={dec[bad[:10]]}"
    ok = dec != 3
    for name, a, b in [("remaining", res.remaining, rem), ("retry", res.retry_after_ns, retry),
                       ("reset_at", res.reset_at_ns, reset)]:
        bad = np.nonzero((a != b) & ok)[0]
        assert bad.size == 0, f"{what} {name} mismatch at {bad[:10]}: gpu={a[bad[:10]]} ref={b[bad[:10]]}"
    if res.tokens is not None:
        is_tb = np.array([configs[c][0] == 1 if c < len(configs) else False for c in cfg]) & (dec <= 1)
        bad = np.nonzero(res.tokens.view(np.uint64)[is_tb] != tok.view(np.uint64)[is_tb])[0]
        assert bad.size == 0, f"{what} tokens mismatch at {bad[:5]}"


def split(trace, sizes):
    key, ts, n, cfg, sms = trace
    out, o = [], 0
    for s in sizes:
        out.append((key[o:o + s], ts[o:o + s], n[o:o + s], cfg[o:o + s], None if sms is None else sms[o:o + s]))
        o += s
    return out


class Rig:
    """an engine, the C oracle (decides only) and the Python oracle (decides,
    and the expectation of every peek)"""

    def __init__(self, rl, profile, configs, tb=1 << 12, win=1 << 12, max_batch=1 << 15, flags=0):
        self.rl, self.profile, self.configs = rl, profile, configs
        self.eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch, flags=flags)
        self.csim = oracle.OracleSim(profile)
        self.psim = po.Sim(profile)
        for a, L, W in configs:
            assert self.eng.register(a, L, W) == self.csim.add_config(a, L, W) == self.psim.add_config(a, L, W)

    def decide(self, part, what=""):
        key, ts, n, cfg, sms = part
        assert_same(self.eng.decide(key, ts, n, cfg, sms), self.csim.decide(key, ts, n, cfg, sms), self.configs, cfg,
                    what=what)
        sim_decide(self.psim, key, ts, n, cfg, sms)

    def fingerprint(self, now_ms):
        """table_info, the snapshot's order-independent checksums and its
        sorted sections: at server clock 0 (every entry that exists) and at
        now_ms (the live ones)"""
        out = []
        for at in (0, now_ms):
            info = self.eng.table_info(at)
            out.append(tuple(getattr(info, k) for k, _ in info._fields_[2:]))
            p = snap.parse(self.eng.snapshot(at))
            out.append((int(p["header"]["payload_sum"]), int(p["header"]["header_sum"])))
            out.append(p["tb"][np.argsort(p["tb"]["key"], kind="stable")].tobytes())
            out.append(p["win"][np.argsort(p["win"]["key"], kind="stable")].tobytes())
            sp = p["spill"]
            out.append(sp[np.lexsort((sp["when"], sp["cnt"], sp["ws"], sp["key"]))].tobytes())
        return out

    def peek(self, batch, what="", now_ms=None):
        """peek the batch: results equal the expectation, nothing moved"""
        key, ts, n, cfg, sms = batch
        exp = peek_expected(self.psim, key, ts, n, cfg, sms)
        if now_ms is None:
            now_ms = int(np.max(sms)) if sms is not None else int(np.max(ts)) // 1_000_000
        before = self.fingerprint(now_ms)
        st0 = self.eng.stats()
        res = self.eng.peek(key, ts, n, cfg, sms)
        st1 = self.eng.stats()
        assert (st0.batches, st0.decisions) == (st1.batches, st1.decisions)
        assert self.eng.sync() == 0
        assert self.fingerprint(now_ms) == before, f"{what}: a peek changed the tables"
        assert_peek(res, exp, self.configs, cfg, what=what)
        return res, exp

    def close(self):
        self.eng.close()


def cat(*batches):
    """concatenate (key, ts, n, cfg, sms) batches (sms: all given or none)"""
    cols = list(zip(*batches))
    sms = None if cols[4][0] is None else np.concatenate(cols[4]).astype(np.int64)
    return (np.concatenate(cols[0]).astype(np.uint64), np.concatenate(cols[1]).astype(np.int64),
            np.concatenate(cols[2]).astype(np.int64), np.concatenate(cols[3]).astype(np.uint32), sms)


def parity_batch(first, second, configs, nkeys):
    """the peek batch of the parity test: the second half's requests, the same
    keys at n = 0, keys never seen, and the second half's keys with n = 2^63 - 1
    (INCRBY overflows on every window counter that holds anything)"""
    key, ts, n, cfg, sms = second
    m = key.size
    unseen = (np.arange(200, dtype=np.uint64) + np.uint64(10 * nkeys))
    at = lambda x, k: None if x is None else np.full(k, x[0], np.int64)
    return cat(second,
               (key, ts, np.zeros(m, np.int64), cfg, sms),
               (unseen, np.full(200, ts[0], np.int64), np.arange(200, dtype=np.int64) % 4,
                (unseen % np.uint64(len(configs))).astype(np.uint32), at(sms, 200)),
               (key, ts, np.full(m, (1 << 63) - 1, np.int64), cfg, sms))


# --- parity -----------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["tb", "sw", "fw", "mixed"])
@pytest.mark.parametrize("ff", [False, True])
def test_parity(rl, profile, kind, ff):
    configs = CONFIG_SETS[kind]
    seed = 900 + {"tb": 1, "sw": 2, "fw": 3, "mixed": 4}[kind] * 10 + profile * 2 + int(ff)
    nkeys = 300
    first, second = split(random_trace(seed, 16_000, nkeys, configs, fastforward=ff, big_n=True), [8000, 8000])
    r = Rig(rl, profile, configs)
    r.decide(first, "first half")
    batch = parity_batch(first, second, configs, nkeys)
    res, exp = r.peek(batch, "peek")
    assert (exp[0] == po.DENIED).any() and (exp[0] == po.ALLOWED).any()
    if kind != "tb":   # a token bucket has no INCRBY: its script cannot fail
        assert (exp[0] == po.ERROR).any()
    # the second half decides as if no peek had happened
    r.decide(second, "second half")
    r.close()


# --- launch shape -----------------------------------------------------------------

def test_launch_shapes(rl):
    """m = 1, 255, 256, 257 and one past what the capped grid covers with one
    request per thread (the grid-stride loop's second trip).  Peeks do not
    interact, so the large batches tile a base batch and its expectation."""
    configs = CONFIG_SETS["mixed"]
    nkeys = 200
    first, second = split(random_trace(77, 8000, nkeys, configs, big_n=True), [4000, 4000])
    r = Rig(rl, 0, configs, max_batch=1 << 19)     # one launch takes cap + 1 requests
    r.decide(first)
    base = parity_batch(first, second, configs, nkeys)
    exp = peek_expected(r.psim, *base)
    cap = rl.PEEK_GRID_CAP
    assert cap == 1024 * 256
    fp = r.fingerprint(int(second[1][-1]) // 1_000_000)
    for m in (1, 255, 256, 257, cap + 1, (1 << 19) + 5):   # the last: more than max_batch, chunked
        idx = np.arange(m) % base[0].size
        key, ts, n, cfg = (x[idx] for x in base[:4])
        res = r.eng.peek(key, ts, n, cfg)
        assert_peek(res, tuple(x[idx] for x in exp), configs, cfg, what=f"m={m}")
    # nothing moved
    assert fp == r.fingerprint(int(second[1][-1]) // 1_000_000)
    r.decide(second, "second half")
    r.close()


# --- probe runs -------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_probe_runs(rl, profile):
    """Small tables (the engine's minimum capacity) filled to ~75 %: long probe
    runs.  Every present key and 200 absent ones."""
    configs = [(1, 20, 12 * NS), (2, 100, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, profile, configs, tb=1 << 6, win=1 << 6)
    info = r.eng.table_info(0)
    ntb, nwin = int(info.tb_capacity * 0.75), int(info.win_capacity * 0.75)
    rng = np.random.default_rng(5 + profile)
    ids = rng.permutation(1 << 20)[:ntb + nwin].astype(np.uint64)
    cfg = np.concatenate([np.zeros(ntb, np.uint32), 1 + (np.arange(nwin) % 2).astype(np.uint32)])
    ts = T0 + np.arange(ids.size, dtype=np.int64) * 1000
    n = rng.choice([1, 2, 25, 120], ids.size).astype(np.int64)
    r.decide((ids, ts, n, cfg, None))
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (ntb, nwin)
    absent = (np.arange(200, dtype=np.uint64) + np.uint64(1 << 21))
    t1 = int(ts[-1]) + 5_000_000
    batch = cat((ids, np.full(ids.size, t1), rng.choice([0, 1, 30], ids.size), cfg, None),
                (absent, np.full(200, t1), np.arange(200) % 3, (absent % np.uint64(3)).astype(np.uint32), None))
    r.peek(batch, "75 % full")
    assert (r.eng.table_info(0).tb_used, r.eng.table_info(0).win_used) == (ntb, nwin)
    r.close()


def test_full_table_absent_key_is_fresh(rl):
    """Fill both tables until decide reports RL_ENOMEM; a key that is not in
    them peeks as a fresh key, without error and without a sticky status."""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS)]
    eng = rl.Engine(profile=0, tb_capacity=1 << 6, win_capacity=1 << 6, max_batch=1 << 12)
    fresh = po.Sim(0)
    for a, L, W in configs:
        eng.register(a, L, W)
        fresh.add_config(a, L, W)
    cap = eng.table_info(0).tb_capacity
    status = 0
    for c in (0, 1):
        ids = np.arange(cap + 64, dtype=np.uint64) + np.uint64(c << 30)
        out = eng.decide(ids, np.full(ids.size, T0), np.ones(ids.size, np.int64), np.full(ids.size, c, np.uint32),
                         check=False)
        assert out.status == rl.RL_ENOMEM
        assert (out.decision == rl.INVALID).sum() == 64        # the keys that found no slot
        status = out.status
    assert status == rl.RL_ENOMEM
    info = eng.table_info(0)
    assert (info.tb_used, info.win_used) == (cap, cap)
    absent = np.array([(1 << 40) + 1, (1 << 40) + 2, (1 << 40) + 3, (1 << 40) + 4], np.uint64)
    batch = (absent, np.full(4, T0 + 1000), np.array([0, 3, 0, 101], np.int64), np.array([0, 0, 1, 1], np.uint32), None)
    assert eng.sync() == rl.RL_ENOMEM       # the decides' sticky status, cleared by reading it
    res = eng.peek(*batch)
    assert_peek(res, peek_expected(fresh, *batch), configs, batch[3], what="full table")
    assert list(res.decision) == [rl.ALLOWED, rl.ALLOWED, rl.ALLOWED, rl.DENIED]
    assert eng.sync() == 0
    eng.close()


# --- spill ------------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_spill(rl, profile):
    """Skewed clocks on window limiters: window keys in the entry, in the spill
    table and nowhere, and a spilled window deleted by Reset (an ABSENT spill
    entry)."""
    configs = CONFIG_SETS["sw"] + CONFIG_SETS["fw"]
    nkeys = 60
    first, second = split(skewed_trace(41 + profile, 12_000, nkeys, configs), [6000, 6000])
    r = Rig(rl, profile, configs)
    r.decide(first, "first half")
    now_ms = int(first[4][-1])
    p = snap.parse(r.eng.snapshot(0))           # every window key that exists
    assert r.eng.table_info(0).spill_used > 0
    owners, counts = np.unique(p["spill"]["key"], return_counts=True)
    assert counts.max() >= 2                    # some key owns at least two spill entries

    def wcfg(k):
        return int(k) % len(configs)

    def batch_at(pairs):
        """peeks (n = 0 and 1) of (key, ws) at that window, at the window after
        it (sliding: it is then the previous window) and far from any window"""
        rows = []
        for k, ws in pairs:
            c = wcfg(k)
            W = configs[c][2]
            for t in (ws * NS + 1000, ws * NS + W + 1000, ws * NS + 1000 * W):
                for n in (0, 1):
                    rows.append((int(k), int(t), n, c))
        rows = np.array(rows, dtype=object)
        return (rows[:, 0].astype(np.uint64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64),
                rows[:, 3].astype(np.uint32), np.full(len(rows), now_ms, np.int64))

    in_entry = [(k, ws) for k, s in zip(p["win"]["key"], p["win"]["s"]) for ws, when in zip(s["ws"], s["when"])
                if when != snap.ABSENT]
    in_spill = list(zip(p["spill"]["key"], p["spill"]["ws"]))
    assert in_entry and in_spill
    r.peek(batch_at(in_entry[:150]), "window keys in the entry", now_ms)
    res, exp = r.peek(batch_at(in_spill[:150]), "window keys in the spill", now_ms)
    # Reset of one spilled window that is still live: its spill entry stays, ABSENT
    live = [(k, ws, c) for (k, ws), w, c in zip(in_spill, p["spill"]["when"], p["spill"]["cnt"])
            if snap.alive(np.array([w]), now_ms, profile)[0] and c > 0]
    assert live
    k, ws, _ = live[0]
    t_reset = int(ws) * NS + 1000
    r.eng.reset(wcfg(k), int(k), t_reset)
    r.psim.reset(wcfg(k), int(k), t_reset)
    r.csim.reset(wcfg(k), int(k), t_reset, now_ms)
    mine = [(kk, w) for kk, w in in_spill if kk == k]
    res, exp = r.peek(batch_at(mine), "after the reset of a spilled window", now_ms)
    r.decide(second, "second half")
    r.close()


# --- expiry edges -----------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_expiry_edges(rl, profile):
    """One key per algorithm, peeked with an explicit server clock at when - 1,
    when, when + 1 (the profiles differ at `when`), then decided at when + 1: a
    peek that deleted lazily, or failed to see the expiry, shows there."""
    configs = [(1, 20, 12 * NS), (2, 100, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, profile, configs)
    ws = po.window_start(T0, 60 * NS)
    t0 = ws * NS + 5 * NS                     # inside a 60 s window, for all three
    s0 = t0 // 1_000_000
    keys = np.array([11, 12, 13], np.uint64)
    cfg = np.array([0, 1, 2], np.uint32)
    r.decide((keys, np.full(3, t0), np.array([15, 60, 60]), cfg, np.full(3, s0)))
    ttl_ms = [24_000, 60_000, 60_000]
    rows = []
    for i in range(3):
        when = s0 + ttl_ms[i]
        for s in (when - 1, when, when + 1):
            for n in (0, 1, 50):
                rows.append((keys[i], t0 + 1_000_000, n, cfg[i], s))
                if i == 1:   # the sliding window's previous key: one window later
                    rows.append((keys[i], t0 + 60 * NS, n, cfg[i], s))
    rows = np.array(rows, dtype=object)
    batch = (rows[:, 0].astype(np.uint64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64),
             rows[:, 3].astype(np.uint32), rows[:, 4].astype(np.int64))
    res, exp = r.peek(batch, "expiry edges", s0)
    # not vacuous: the answers differ across the edge
    for i in range(3):
        sel = (batch[0] == keys[i]) & (batch[2] == 0) & (batch[1] == t0 + 1_000_000)
        assert len(set(exp[1][sel])) == 2, (i, exp[1][sel])
    for i in range(3):
        when = s0 + ttl_ms[i]
        r.decide((keys[i:i + 1], np.array([t0 + 2_000_000]), np.array([1]), cfg[i:i + 1], np.array([when + 1])),
                 f"decide at when + 1, key {i}")
    r.close()


# --- token-bucket arithmetic ------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_token_bucket_arithmetic(rl, profile):
    """ts before last_refill (negative elapsed), n = 0, 1, limit, limit + 1,
    2^62, on the fixed configs and on random configs with a limit >= 1e9 (where
    "%.14g" rounds the stored tokens)."""
    for what in ("fixed", "random"):
        if what == "fixed":
            configs = CONFIG_SETS["tb"]
            tr = random_trace(61 + profile, 4000, 40, configs)
            nk = 40
        else:
            configs, tr = random_config_trace(4, 1, 4000, nk=6)
            assert max(L for _, L, _ in configs) >= 10 ** 9
            nk = 6
        r = Rig(rl, profile, configs)
        r.decide(tr, what)
        keys = np.arange(nk + 3, dtype=np.uint64)
        rows = []
        for k in keys:
            c = int(k) % len(configs)
            L, W = configs[c][1], configs[c][2]
            for t in (int(tr[1][-1]) + W // 7, int(tr[1][-1]), int(tr[1][0]) - 3 * NS, int(tr[1][-1]) - W // 3):
                for n in (0, 1, L, L + 1, BIG):
                    rows.append((int(k), t, n, c))
        rows = np.array(rows, dtype=object)
        batch = (rows[:, 0].astype(np.uint64), rows[:, 1].astype(np.int64), rows[:, 2].astype(np.int64),
                 rows[:, 3].astype(np.uint32), None)
        res, exp = r.peek(batch, what)
        # the status query of a bucket is allowed whenever time has not gone
        # back (a refill negative beyond the balance leaves tokens < 0, and the
        # script's `tokens >= requested` then fails even for 0)
        assert (exp[0][(batch[2] == 0) & (batch[1] >= int(tr[1][-1]))] == po.ALLOWED).all()
        assert (exp[0] == po.DENIED).any()
        r.close()


# --- invalid requests -------------------------------------------------------------

def test_invalid_requests(rl):
    configs = CONFIG_SETS["mixed"]
    r = Rig(rl, 0, configs)
    key = np.array([1, 2, rl.KEY_RESERVED, 3, 4], np.uint64)
    n = np.array([-1, 1, 1, -(1 << 63), 0], np.int64)
    cfg = np.array([0, len(configs), 0, 5, 5], np.uint32)
    res, exp = r.peek((key, np.full(5, T0), n, cfg, None), "invalid")
    assert list(res.decision) == [rl.INVALID] * 4 + [rl.ALLOWED]
    assert r.eng.sync() == 0          # not even the reserved key raises the sticky status
    assert r.eng.peek(key[:0], key[:0], key[:0], key[:0]).decision.size == 0
    r.close()


# --- duplicates -------------------------------------------------------------------

def test_duplicates(rl):
    configs = CONFIG_SETS["mixed"]
    tr = random_trace(15, 3000, 30, configs)
    r = Rig(rl, 0, configs)
    r.decide(tr)
    for k in (0, 5, 10):      # a token bucket, a sliding and a fixed window key
        batch = (np.full(1000, k, np.uint64), np.full(1000, int(tr[1][-1]) + 1000), np.full(1000, 2),
                 np.full(1000, k % len(configs), np.uint32), None)
        res, exp = r.peek(batch, f"key {k}")
        for a in (res.decision, res.remaining, res.retry_after_ns, res.reset_at_ns, res.tokens.view(np.uint64)):
            assert (a == a[0]).all()
    r.close()


# --- order in flight --------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("size", [6000, 700])
def test_order_in_flight(rl, profile, size):
    """RL_OPT_PIPELINE, device API, no sync between the calls: batch A, peek P,
    batch B (above and below the engine's single-workgroup cut of 4096).  B
    re-uses A's keys and brings new keys that P also asks about (B's grouping
    may be inserting them while P runs).  P sees the state after A alone."""
    import torch
    configs = CONFIG_SETS["mixed"]
    nkeys = 200
    tr = random_trace(51 + profile, 2 * size, nkeys, configs, big_n=True)
    A, B = split(tr, [size, size])
    B = (B[0].copy(), B[1], B[2], B[3].copy(), None)
    B[0][::3] += np.uint64(1000)               # new keys, a third of B
    B[3][:] = (B[0] % np.uint64(len(configs))).astype(np.uint32)
    P = cat(B, (B[0], B[1], np.zeros(size, np.int64), B[3], None),
            (A[0], np.full(size, B[1][0]), np.zeros(size, np.int64), A[3], None))
    r = Rig(rl, profile, configs, flags=rl.OPT_PIPELINE)
    dev = torch.device("cuda", 0)

    def to_dev(b):
        key, ts, n, cfg, _ = b
        ins = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                                np.ascontiguousarray(x)).to(dev) for x in (key, ts, n, cfg.view(np.int32))]
        m = key.size
        outs = ([torch.empty(m, dtype=torch.uint8, device=dev)] +
                [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
                [torch.empty(m, dtype=torch.float64, device=dev)])
        return ins, outs

    (ia, oa), (ip, op_), (ib, ob) = to_dev(A), to_dev(P), to_dev(B)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda fn, i, o: fn(i[0].numel(), i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(),
                               None, *[x.data_ptr() for x in o], stream)
    call(r.eng.decide_device, ia, oa)
    call(r.eng.peek_device, ip, op_)
    call(r.eng.decide_device, ib, ob)
    torch.cuda.synchronize()
    assert r.eng.sync() == 0, r.eng.last_error()
    host = lambda o: rl.Decisions(*[x.cpu().numpy() for x in o])
    assert_same(host(oa), r.csim.decide(*A[:4]), configs, A[3], "A")
    sim_decide(r.psim, *A[:4])
    assert_peek(host(op_), peek_expected(r.psim, *P), configs, P[3], "P")
    assert_same(host(ob), r.csim.decide(*B[:4]), configs, B[3], "B")
    st = r.eng.stats()
    assert (st.batches, st.decisions) == (2, 2 * size)
    r.close()


# --- coalescer --------------------------------------------------------------------

def test_coalescer_peeks_between_decides(rl):
    """Threads submit decides while one thread peeks.  Every decide matches the
    C oracle in ticket order (the peeks left no trace) and stats.peeked counts
    the peeks."""
    configs = CONFIG_SETS["mixed"]
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12, flags=rl.OPT_PIPELINE)
    csim = oracle.OracleSim(0)
    for a, L, W in configs:
        eng.register(a, L, W)
        csim.add_config(a, L, W)
    co = rl.Coalescer(eng, max_batch=1 << 12)
    nthreads, per, m = 4, 40, 25
    # each thread has keys of its own, so every key's times stay in order
    # however the threads' submissions interleave (15 configs: 1500 keeps
    # key % 15, the trace's config of a key)
    trs = []
    for i in range(nthreads):
        k, ts, n, cfg, _ = random_trace(71 + i, per * m, 30, configs)
        trs.append((k + np.uint64(1500 * i), ts, n, cfg))
    tr = trs[-1]
    subs, lock, errs = [], threading.Lock(), []

    def submitter(i):
        for j in range(per):
            part = tuple(x[j * m:(j + 1) * m] for x in trs[i])
            t = co.submit(*part)
            rc, out = co.wait(t, m)
            with lock:
                subs.append((t, part, rc, out))

    peeked = [0]

    def peeker():
        rng = np.random.default_rng(1)
        for j in range(60):
            k = (rng.integers(0, 40, 16) + 1500 * rng.integers(0, nthreads, 16)).astype(np.uint64)
            rc, out = co.peek(k, np.full(16, tr[1][-1]), rng.integers(0, 3, 16),
                              (k % np.uint64(len(configs))).astype(np.uint32))
            if rc != 0 or not (out[0] <= 1).all():
                errs.append((rc, out[0]))
            peeked[0] += 16

    ths = [threading.Thread(target=submitter, args=(i,)) for i in range(nthreads)] + [threading.Thread(target=peeker)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs
    # quiescent: a peek through the coalescer equals the engine's own answer
    k = (np.arange(150, dtype=np.uint64) % np.uint64(38)) + np.uint64(1500) * (np.arange(150, dtype=np.uint64) // np.uint64(38))
    q = (k, np.full(150, tr[1][-1]), np.zeros(150, np.int64), (k % np.uint64(len(configs))).astype(np.uint32))
    rc, out = co.peek(*q)
    assert rc == 0
    st = co.stats()
    assert st.peeked == peeked[0] + 150
    assert st.submitted == st.decided == nthreads * per * m
    direct = eng.peek(*q)
    assert_peek(out, (direct.decision, direct.remaining, direct.retry_after_ns, direct.reset_at_ns, None), configs, q[3])
    for t, part, rc, out in sorted(subs, key=lambda s: s[0]):
        assert rc == 0
        ref = csim.decide(*part)
        res = rl.Decisions(*out, None)
        assert_same(res, ref, configs, part[3], what=f"ticket {t}")
    co.close()
    eng.close()


# --- gRPC -------------------------------------------------------------------------

def _peek_allow_peek(st_allow, st_peek, a, expect_first):
    """Peek three times, then Allow, then Peek: the Allow result is the
    oracle's first and the peeks bracket it"""
    import rl_grpc
    for _ in range(3):
        p = rl_grpc.peek(st_peek, "fw", "peeker")            # n omitted: the status query
        assert (p.allowed, p.limit, p.remaining) == (True, 3, 3)
    p1 = rl_grpc.peek(st_peek, "fw", "peeker", 1)
    g = st_allow.Allow(a.AllowRequest(limiter="fw", key="peeker"))
    assert (g.allowed, g.remaining, g.retry_after_ns, g.reset_at_unix_ns) == expect_first(g)
    assert (p1.allowed, p1.remaining, p1.reset_at_unix_ns) == (g.allowed, g.remaining, g.reset_at_unix_ns)
    p = rl_grpc.peek(st_peek, "fw", "peeker")
    assert (p.allowed, p.remaining, p.reset_at_unix_ns) == (True, 2, g.reset_at_unix_ns)
    p = rl_grpc.peek(st_peek, "fw", "peeker", 3)             # more than is left: denied, nothing taken
    assert not p.allowed and p.retry_after_ns > 0
    assert rl_grpc.peek(st_peek, "fw", "peeker").remaining == 2
    import grpc
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.peek(st_peek, "fw", "peeker", -1)
    assert e.value.code() == grpc.StatusCode.INVALID_ARGUMENT
    with pytest.raises(grpc.RpcError) as e:
        rl_grpc.peek(st_peek, "nope", "peeker")
    assert e.value.code() == grpc.StatusCode.NOT_FOUND


GRPC_LIMITERS = ["fw:fixed_window:3:60s", "tb:token_bucket:5:10s"]


def _first_allow(t):
    """the oracle's answer to the first Allow of a key on the fw limiter at t"""
    sim = oracle.OracleSim(0)
    c = sim.add_config(3, 3, 60 * NS)
    d, rem, retry, reset, _ = sim.decide([1], [t], [1], [c])
    return bool(d[0]), int(rem[0]), int(retry[0]), int(reset[0])


def test_grpc_native_peek(rl):
    import grpc
    import rl_grpc
    import rl_server
    be = rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)
    lims = [rl_server.Limiter.parse(s) for s in GRPC_LIMITERS]
    for lim in lims:
        lim.cfg_id = be.register(lim.alg, lim.limit, lim.window_ns)
    co = be.start(1 << 12)
    step = 1_250_000
    srv = rl.GrpcServer(co, [(l.name, l.cfg_id, l.alg, l.limit, l.window_ns, l.prefix, l.fail_open) for l in lims],
                        io_threads=2, clock_start_ns=T0, clock_step_ns=step)
    ch = grpc.insecure_channel(f"127.0.0.1:{srv.port}")
    try:
        # the server's clock ticks once per RPC that reads it: 4 peeks, then the Allow
        _peek_allow_peek(rl_grpc.rate_limiter_stub(ch), rl_grpc.status_stub(ch), rl_grpc.api("ratelimiter.proto"),
                         lambda g: _first_allow(T0 + 5 * step))
        assert co.stats().peeked == 7 and co.stats().decided == 1
    finally:
        ch.close()
        srv.close()
        be.close()


def test_grpc_python_server_peek(rl):
    import rl_grpc
    import rl_server
    from test_grpc import Clock, start
    be = rl_server.GpuBackend(0, 1 << 12, 1 << 12, 1 << 12)
    svc = rl_server.RateLimiterService([rl_server.Limiter.parse(s) for s in GRPC_LIMITERS], None, be.register,
                                       clock=Clock())
    svc.co = be.start(1 << 12)
    ch, stop, th = start(svc)
    try:
        _peek_allow_peek(rl_grpc.rate_limiter_stub(ch), rl_grpc.status_stub(ch), svc.a,
                         lambda g: _first_allow(svc.clock.t))
    finally:
        ch.close()
        stop.set()
        th.join(10)
        be.close()
