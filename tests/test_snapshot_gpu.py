"""Engine state snapshots (include/rl_snapshot.h) on the GPU: an engine that is
exported, closed and restored into a fresh engine (of other capacities, of
another world size, through the coalescer) goes on deciding exactly as the CPU
oracle does, which runs uninterrupted over the whole trace.  Tokens are
compared as bit patterns."""
import threading

import numpy as np
import pytest

import oracle
import rl_snapshot as snap
import shard
from tracegen import CONFIG_SETS, NS, T0, random_trace, skewed_trace

pytestmark = pytest.mark.gpu


# --- the helpers of test_gpu_parity.py -------------------------------------------

def assert_same(res, ref, configs, cfg, what=""):
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
        gb = res.tokens.view(np.uint64)[is_tb]
        rb = tok.view(np.uint64)[is_tb]
        bad = np.nonzero(gb != rb)[0]
        assert bad.size == 0, f"{what} tokens mismatch: gpu={res.tokens[is_tb][bad[:5]]} ref={tok[is_tb][bad[:5]]}"


def split(trace, sizes):
    key, ts, n, cfg, sms = trace
    out, o = [], 0
    for s in sizes:
        out.append((key[o:o + s], ts[o:o + s], n[o:o + s], cfg[o:o + s], None if sms is None else sms[o:o + s]))
        o += s
    return out


def make_pair(rl, profile, configs, tb, win, max_batch=1 << 15, flags=0):
    eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch, flags=flags)
    sim = oracle.OracleSim(profile)
    for a, L, W in configs:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    return eng, sim


def make_engine(rl, profile, configs, tb, win, max_batch=1 << 15, flags=0):
    eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch, flags=flags)
    for a, L, W in configs:
        eng.register(a, L, W)
    return eng


def first_ms(part):
    key, ts, n, cfg, sms = part
    return int(sms[0]) if sms is not None else int(ts[0]) // 1_000_000


def step(eng, sim, part, configs, what):
    key, ts, n, cfg, sms = part
    assert_same(eng.decide(key, ts, n, cfg, sms), sim.decide(key, ts, n, cfg, sms), configs, cfg, what=what)


def info_tuple(info):
    return tuple(getattr(info, k) for k, _ in info._fields_[2:])


def checked_snapshot(rl, eng, sim, now_ms, profile, world=1, rank=0):
    """the snapshot at now_ms: inspect accepts it, its counts are the live
    counts of the tables, and (world 1) its keys are the oracle's KEYS"""
    before = eng.table_info(now_ms)
    blob = eng.snapshot(now_ms, world, rank)
    assert info_tuple(eng.table_info(now_ms)) == info_tuple(before)      # the engine is unchanged
    rc, info = rl.snapshot_inspect(blob)
    assert rc == rl.RL_OK
    assert (info.profile, info.world, info.rank, info.now_ms, info.bytes) == (profile, world, rank, now_ms, blob.size)
    p = snap.parse(blob)
    assert [len(p[k]) for k in ("tb", "win", "spill")] == [info.tb_keys, info.win_keys, info.spill_keys]
    assert not p["win"]["nspill"].any()
    if world == 1:
        assert info.tb_keys == before.tb_live and info.spill_keys == before.spill_live
        # a window entry whose two slots expired still travels while its user
        # key owns spill entries (what table GC keeps): only a table that ever
        # spilled can hold more records than live entries
        assert info.win_keys >= before.win_live
        if before.spill_used == 0:
            assert info.win_keys == before.win_live
        keys = list(snap.logical_keys(p, now_ms, profile))
        want = sim.keys(now_ms)
        assert len(keys) == len(set(keys)) == len(want)
        assert set(keys) == set(want)
    return blob, info, before


# --- restart parity ---------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["tb", "sw", "fw", "mixed"])
@pytest.mark.parametrize("ff", [False, True])
def test_restart_parity(rl, profile, kind, ff):
    configs = CONFIG_SETS[kind]
    seed = 700 + {"tb": 1, "sw": 2, "fw": 3, "mixed": 4}[kind] * 10 + profile * 2 + int(ff)
    first, second = split(random_trace(seed, 40_000, 500, configs, fastforward=ff, big_n=True), [20_000, 20_000])
    a, sim = make_pair(rl, profile, configs, 1 << 12, 1 << 12)
    step(a, sim, first, configs, "first half")
    now_ms = first_ms(second)
    blob, info, before = checked_snapshot(rl, a, sim, now_ms, profile)
    assert info.tb_keys + info.win_keys > 0
    a.close()
    key, ts, n, cfg, sms = second
    ref = sim.decide(key, ts, n, cfg, sms)
    for cap in (1 << 10, 1 << 14):          # smaller and larger than the exporter's tables
        b = make_engine(rl, profile, configs, cap, cap)
        rc, after = b.restore(blob, now_ms)
        assert rc == rl.RL_OK
        assert (after.tb_capacity, after.win_capacity) == (cap, cap)
        assert (after.tb_used, after.tb_live) == (info.tb_keys, info.tb_keys)
        assert after.win_live == before.win_live and after.win_used <= info.win_keys
        assert after.spill_live == after.spill_used == info.spill_keys
        assert_same(b.decide(key, ts, n, cfg, sms), ref, configs, cfg, what=f"second half, capacity {cap}")
        b.close()


# --- spill entries ----------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_spill_entries_travel(rl, profile):
    configs = CONFIG_SETS["mixed"]
    first, second = split(skewed_trace(31 + profile, 40_000, 500, configs), [20_000, 20_000])
    a, sim = make_pair(rl, profile, configs, 1 << 13, 1 << 13)
    step(a, sim, first, configs, "first half")
    now_ms = first_ms(second)
    spill_live = a.table_info(now_ms).spill_live
    blob, info, _ = checked_snapshot(rl, a, sim, now_ms, profile)
    assert info.spill_keys > 0                      # the test is not vacuous
    a.close()
    b = make_engine(rl, profile, configs, 1 << 13, 1 << 13)
    _, after = b.restore(blob, now_ms)
    assert after.spill_live == spill_live == after.spill_used
    step(b, sim, second, configs, "second half")
    b.close()


# --- compaction edges -------------------------------------------------------------

EDGE_CONFIGS = [(1, 5, 60 * NS), (3, 5, 60 * NS)]


def edge_batch(nkeys, t, extra=0):
    """one batch of distinct keys at one timestamp: nkeys (+ extra new)
    token-bucket keys and as many fixed-window keys"""
    tbk = np.arange(nkeys + extra, dtype=np.uint64) * 3 + 11
    fwk = np.arange(nkeys + extra, dtype=np.uint64) * 5 + (1 << 40)
    key = np.concatenate([tbk, fwk])
    cfg = np.concatenate([np.zeros(tbk.size, np.uint32), np.ones(fwk.size, np.uint32)])
    perm = np.random.default_rng(nkeys).permutation(key.size)
    return key[perm], np.full(key.size, t, np.int64), np.ones(key.size, np.int64) * 2, cfg[perm], None


@pytest.mark.parametrize("nkeys,cap", [(0, 1024), (1, 1024), (63, 1024), (64, 1024), (65, 1024), (900, 1024),
                                       (3000, 1 << 20)])
def test_compaction_edges(rl, nkeys, cap):
    """wave-aggregated compaction at 0, 1, 63, 64, 65 exporting lanes, a nearly
    full table (900 of 1024 slots: long probe runs on import), and a large,
    mostly empty table (several grid-stride iterations with nothing to export)"""
    a, sim = make_pair(rl, 0, EDGE_CONFIGS, cap, cap, max_batch=1 << 13)
    if nkeys:
        step(a, sim, edge_batch(nkeys, T0), EDGE_CONFIGS, "first batch")
    now_ms = (T0 + NS) // 1_000_000
    blob, info, _ = checked_snapshot(rl, a, sim, now_ms, 0)
    assert (info.tb_keys, info.win_keys, info.spill_keys) == (nkeys, nkeys, 0)
    a.close()
    b = make_engine(rl, 0, EDGE_CONFIGS, cap, cap, max_batch=1 << 13)
    _, after = b.restore(blob, now_ms)
    assert (after.tb_used, after.tb_live, after.win_used, after.win_live) == (nkeys,) * 4
    step(b, sim, edge_batch(nkeys, T0 + NS, extra=5 if nkeys < 900 else 0), EDGE_CONFIGS, "second batch")
    b.close()


# --- expiry -----------------------------------------------------------------------

def test_expired_keys_are_not_exported(rl):
    configs = [(1, 5, NS), (3, 5, NS)]   # TB ttl 2 s, FW ttl 1 s
    a, sim = make_pair(rl, 0, configs, 1024, 1024, max_batch=4096)
    m = 2000
    key = np.arange(m, dtype=np.uint64)
    step(a, sim, (key, np.full(m, T0, np.int64), np.ones(m, np.int64), (key % 2).astype(np.uint32), None), configs,
         "first batch")
    now_ms = (T0 + 10 * NS) // 1_000_000
    assert a.table_info(now_ms).tb_used == 1000
    blob, info, _ = checked_snapshot(rl, a, sim, now_ms, 0)
    assert (info.tb_keys, info.win_keys, info.spill_keys, info.bytes) == (0, 0, 0, 128)
    # the live snapshot of 10 s earlier, restored now, brings nothing either
    early = a.snapshot(T0 // 1_000_000)
    assert rl.snapshot_inspect(early)[1].tb_keys == 1000
    for blob_ in (blob, early):
        b = make_engine(rl, 0, configs, 1024, 1024, max_batch=4096)
        _, after = b.restore(blob_, now_ms)
        assert after.tb_used == after.win_used == 0
        b.close()
    # restoring into the exporter itself is a GC
    _, after = a.restore(blob, now_ms)
    assert after.tb_used == after.win_used == 0
    key2 = key + m
    step(a, sim, (key2, np.full(m, T0 + 10 * NS, np.int64), np.ones(m, np.int64), (key2 % 2).astype(np.uint32),
                  None), configs, "after the restore")
    a.close()


# --- re-shard ---------------------------------------------------------------------

def key_set(blob, now_ms, profile=0):
    return set(snap.logical_keys(snap.parse(blob), now_ms, profile))


def test_reshard_split_and_merge(rl):
    configs = CONFIG_SETS["mixed"]
    first, second = split(random_trace(811, 40_000, 500, configs, big_n=True), [20_000, 20_000])
    a, sim = make_pair(rl, 0, configs, 1 << 12, 1 << 12)
    step(a, sim, first, configs, "first half")
    now_ms = first_ms(second)
    full = checked_snapshot(rl, a, sim, now_ms, 0)[0]
    parts = [checked_snapshot(rl, a, sim, now_ms, 0, world=2, rank=r)[0] for r in (0, 1)]
    a.close()
    sets = [key_set(b, now_ms) for b in parts]
    assert sets[0] and sets[1] and not (sets[0] & sets[1])
    assert sets[0] | sets[1] == key_set(full, now_ms)
    for r in (0, 1):
        ids = np.array([k for k, _, _ in sets[r]], dtype=np.uint64)
        assert (shard.owner_of(ids, 2) == r).all()
        p = snap.parse(parts[r])
        for sec in ("tb", "win", "spill"):       # records, live or not, follow their user key
            assert (shard.owner_of(p[sec]["key"], 2) == r).all()
    key, ts, n, cfg, sms = second
    ref = sim.decide(key, ts, n, cfg, sms)
    # split 1 -> 2: each new rank gets its blob and the requests it owns, in order
    owner = shard.owner_of(key, 2)
    for r in (0, 1):
        b = make_engine(rl, 0, configs, 1 << 12, 1 << 12)
        b.restore(parts[r], now_ms)
        mine = owner == r
        assert_same(b.decide(key[mine], ts[mine], n[mine], cfg[mine]), [x[mine] for x in ref], configs, cfg[mine],
                    what=f"rank {r} of 2")
        b.close()
    # merge 2 -> 1: the second import merges into a non-empty engine
    c = make_engine(rl, 0, configs, 1 << 12, 1 << 12)
    _, one = c.restore(parts[0], now_ms)
    _, both = c.restore(parts[1], now_ms)
    assert one.tb_live > 0 and both.tb_live > one.tb_live
    assert both.tb_live == sum(len(snap.parse(b)["tb"]) for b in parts)
    assert_same(c.decide(key, ts, n, cfg, sms), ref, configs, cfg, what="merged")
    c.close()


# --- a failed import changes nothing ------------------------------------------------

def test_failed_import_is_atomic(rl):
    """every way an import can fail leaves the tables as they were (table_info
    at the same clock is unchanged) and the next batch equal to the oracle's"""
    configs = CONFIG_SETS["mixed"]
    first, *rest = split(random_trace(823, 40_000, 500, configs, big_n=True), [20_000] + [5_000] * 4)
    a, sim = make_pair(rl, 0, configs, 1 << 12, 1 << 12)
    step(a, sim, first, configs, "first half")
    now_ms = first_ms(rest[0])
    blob = a.snapshot(now_ms)
    assert rl.snapshot_inspect(blob)[1].tb_keys > 0
    a.close()
    b = make_engine(rl, 0, configs, 1 << 12, 1 << 12)
    b.restore(blob, now_ms)

    # a snapshot under the other profile, and 3000 live keys for 1024 slots
    # (token-bucket keys of config 1, TTL 120 s, created at the clock of the import)
    m = 3000
    t_big = first_ms(rest[3])
    fresh = (np.arange(m, dtype=np.uint64) + (1 << 50), np.full(m, int(rest[3][1][0]), np.int64),
             np.ones(m, np.int64), np.ones(m, np.uint32))
    other = make_engine(rl, 1, configs, 1024, 1024)
    other.decide(*[x[:10] for x in fresh])
    big = make_engine(rl, 0, configs, 1 << 12, 1 << 12)
    big.decide(*fresh)
    flipped = blob.copy()
    flipped[128 + 8] ^= 0x04          # the first token-bucket record's tokens
    assert rl.snapshot_inspect(flipped)[0] == rl.RL_EINVAL
    # (what, blob, clock of the import, capacities, status); the import is
    # followed by the batch rest[i].  The same blob again comes at the clock of
    # the first import, where all its keys are still live: minutes later they
    # would have expired and the import would bring nothing, which is no error.
    cases = [
        ("the same blob again", blob, now_ms, (0, 0), rl.RL_EEXIST),
        ("one payload byte flipped", flipped, first_ms(rest[1]), (0, 0), rl.RL_EINVAL),
        ("the other profile", other.snapshot(t_big), first_ms(rest[2]), (0, 0), rl.RL_EINVAL),
        ("3000 keys for 1024 slots", big.snapshot(t_big), t_big, (1024, 1024), rl.RL_ENOMEM),
    ]
    other.close()
    big.close()
    assert rl.snapshot_inspect(cases[3][1])[1].tb_keys == m
    for part, (what, bad, t, caps, want) in zip(rest, cases):
        before = info_tuple(b.table_info(t))
        rc, _ = b.restore(bad, t, *caps, check=False)
        assert rc == want, (what, rc, b.last_error())
        assert info_tuple(b.table_info(t)) == before, what
        step(b, sim, part, configs, f"after: {what}")
    b.close()


# --- export leaves the engine alone -------------------------------------------------

@pytest.mark.parametrize("pipeline", [False, True])
def test_export_between_device_batches(rl, pipeline):
    """export called while two device-API batches are still queued (with
    RL_OPT_PIPELINE: in flight on the engine's three streams): it waits for
    them, sees exactly their state, and the batches after it are unaffected"""
    import torch
    configs = CONFIG_SETS["mixed"]
    tr = random_trace(91, 80_000, 400, configs, big_n=True)
    parts = split(tr, [20_000, 15_000, 25_000, 20_000])
    eng, sim = make_pair(rl, 0, configs, 1 << 14, 1 << 14, flags=rl.OPT_PIPELINE if pipeline else 0)
    dev = torch.device("cuda", 0)
    ins, outs = [], []
    for key, ts, n, cfg, _ in parts:     # inputs complete before the first call
        ins.append([torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
                    for x in (key, ts, n, cfg.view(np.int32))])
        m = key.size
        outs.append([torch.empty(m, dtype=torch.uint8, device=dev)] +
                    [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
                    [torch.empty(m, dtype=torch.float64, device=dev)])
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    now_ms = first_ms(parts[2])
    blob = None
    for i, ((k, t, n, c), o) in enumerate(zip(ins, outs)):
        if i == 2:
            blob = eng.snapshot(now_ms)
        eng.decide_device(k.numel(), k.data_ptr(), t.data_ptr(), n.data_ptr(), c.data_ptr(), None,
                          *[x.data_ptr() for x in o], stream)
    torch.cuda.synchronize()
    assert eng.sync() == 0, eng.last_error()
    for i, ((key, ts, n, cfg, _), o) in enumerate(zip(parts, outs)):
        if i == 2:
            assert rl.snapshot_inspect(blob)[0] == rl.RL_OK
            assert key_set(blob, now_ms) == set(sim.keys(now_ms))
        ref = sim.decide(key, ts, n, cfg)
        res = rl.Decisions(*[x.cpu().numpy() for x in o])
        assert_same(res, ref, configs, cfg, what=f"batch {i}")
    eng.close()


# --- through the coalescer ----------------------------------------------------------

CO_CONFIGS = [(1, 20, 12 * NS), (3, 100, 60 * NS), (2, 100, 60 * NS), (1, 5, NS)]
CO_T0 = (1_760_000_000 // 60) * 60 * NS


CO_SPAN = 25 * NS      # both phases lie in one minute, as the clocks of tests/test_coalescer.py do: request
                       # times are random, so the store clock (ts / 1e6) goes back and forth within a phase


def hammer(co, t_lo, seed, nthreads=2, subs=25, m=200, nkeys=300):
    """two threads submit chunks and wait for them: (ticket, inputs, results)"""
    out, lock, errors = [], threading.Lock(), []

    def worker(tid):
        rng = np.random.default_rng(seed + tid)
        for _ in range(subs):
            key = rng.integers(0, nkeys, m).astype(np.uint64)
            ts = (t_lo + rng.integers(0, CO_SPAN, m)).astype(np.int64)
            n = rng.choice([1, 1, 1, 2, 3], m).astype(np.int64)
            cfg = (key % len(CO_CONFIGS)).astype(np.uint32)
            t = co.submit(key, ts, n, cfg)
            rc, res = co.wait(t, m)
            if rc != 0:
                errors.append(rc)
            with lock:
                out.append((t, key, ts, n, cfg, res))

    th = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errors, errors
    return sorted(out, key=lambda r: r[0])


def test_coalescer_snapshot_and_restore(rl):
    sim = oracle.OracleSim(0)
    for a, L, W in CO_CONFIGS:
        sim.add_config(a, L, W)

    def check(recs):     # in ticket order, through the one oracle
        for t, key, ts, n, cfg, res in recs:
            dec, rem, retry, reset, _ = sim.decide(key, ts, n, cfg)
            assert np.array_equal(res[0], dec) and np.array_equal(res[1], rem)
            assert np.array_equal(res[2], retry) and np.array_equal(res[3], reset)

    e1 = make_engine(rl, 0, CO_CONFIGS, 1 << 12, 1 << 12, max_batch=1 << 12, flags=rl.OPT_PIPELINE)
    c1 = rl.Coalescer(e1, max_batch=1 << 12, max_in_flight=3)
    recs = hammer(c1, CO_T0, seed=5)
    assert sum(r[1].size for r in recs) == 10_000
    now_ms = (CO_T0 + CO_SPAN) // 1_000_000
    blob = c1.snapshot(now_ms)
    assert c1.stats().gc_runs == 0
    c1.close()
    e1.close()
    check(recs)
    assert rl.snapshot_inspect(blob)[0] == rl.RL_OK
    assert key_set(blob, now_ms) == set(sim.keys(now_ms))

    e2 = make_engine(rl, 0, CO_CONFIGS, 1 << 11, 1 << 11, max_batch=1 << 12, flags=rl.OPT_PIPELINE)
    c2 = rl.Coalescer(e2, max_batch=1 << 12, max_in_flight=3)
    rc, info = c2.restore(blob, now_ms)
    assert rc == rl.RL_OK and info.tb_live == rl.snapshot_inspect(blob)[1].tb_keys
    assert c2.restore(blob, now_ms)[0] == rl.RL_EEXIST
    st = c2.stats()
    assert (st.gc_runs, st.gc_failures) == (2, 1)
    recs = hammer(c2, CO_T0 + CO_SPAN, seed=9)
    assert sum(r[1].size for r in recs) == 10_000
    c2.close()
    e2.close()
    check(recs)


def test_host_backend_coalescer_has_no_snapshot(rl):
    def backend(user, m, *ptrs):
        return 0
    co = rl.Coalescer(backend, max_batch=8)
    with pytest.raises(rl.EngineError) as ei:
        co.snapshot(0)
    assert ei.value.code == rl.RL_EINVAL
    assert co.restore(snap.build(), 0)[0] == rl.RL_EINVAL
    co.close()
