"""More than 32 and more than 64 registered configs (GPU), bit for bit against
the CPU oracle.

With at most MAX_LCFG = 32 configs the replay kernels cache them in LDS
(k_tb_chain<true>, k_replay_light<true>); with 33 or more they read CfgDev
from global memory in every phase (the <false> instantiations, with an LDS pad
of their own).  The 65th and the 129th config make rl_config_register move
d_cfg to a larger allocation.  Every N below straddles or crosses one of these
limits; the traces (tracegen.many_config_trace) use every config id, carry a
hot token-bucket key of >= 4096 requests per batch on the LAST config (the
chain), heavy keys on the last three configs (one wave each) and huge n."""
import numpy as np
import pytest

import oracle
from oracle import rl_oracle_py as po
from peek_cases import assert_peek, peek_expected, sim_decide
from test_gpu_parity import assert_same, make_engine, run_both, split
from tracegen import NS, T0, many_config_keys, many_config_light_trace, many_config_trace, many_configs

pytestmark = pytest.mark.gpu

MAX_LCFG = 32      # csrc/rl_replay.h
CFG_CAP = 64       # rl_engine_create: d_cfg's first capacity, doubled when full
SIZES = [32, 33, 64, 65, 130]


def small_engine(rl, profile, flags=0, max_batch=1 << 15):
    return rl.Engine(profile=profile, tb_capacity=1 << 14, win_capacity=1 << 14, max_batch=max_batch, flags=flags)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("N", SIZES)
def test_full_sequence(rl, N, profile, monkeypatch):
    """the full launch sequence (RL_SMALL_MAX=0), three batches of 24k with
    state carried: at N >= 33 the hot key's huge segment goes through the
    chain of k_tb_chain<false>, the heavy keys through its wave replay"""
    assert (N > MAX_LCFG) == (N >= 33) and (N > CFG_CAP) == (N >= 65)
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    configs, tr, sizes = many_config_trace(4000 + N, N)
    assert len(sizes) >= 3 and configs[N - 1][0] == 1
    hot = many_config_keys(N, N - 1, 0)
    eng = small_engine(rl, profile)
    sim = oracle.OracleSim(profile)
    for a, L, W in configs:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    for i, (key, ts, n, cfg, sms) in enumerate(split(tr, sizes)):
        res = eng.decide(key, ts, n, cfg, sms)
        assert_same(res, sim.decide(key, ts, n, cfg, sms), configs, cfg, what=f"batch {i}")
        # the witness: the batch had a token-bucket segment of >= 4096 on
        # config N - 1 (id >= 32 when N >= 33) and replayed chain segments
        mine = key == hot
        assert int((mine & (n > 0)).sum()) >= 4096 and np.all(cfg[mine] == N - 1)
        assert eng.stats().last_heavy >= 1
    eng.close()


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("N", SIZES)
def test_small_batches(rl, N, profile, monkeypatch):
    """the same trace in batches of at most 4096: k_small"""
    assert (N > MAX_LCFG) == (N >= 33) and (N > CFG_CAP) == (N >= 65)
    monkeypatch.setenv("RL_SMALL_MAX", "4096")
    configs, tr, sizes = many_config_trace(4000 + N, N)
    total = sum(sizes)
    parts = [4096] * (total // 4096) + ([total % 4096] if total % 4096 else [])
    run_both(rl, profile, configs, split(tr, parts), tb=1 << 14, win=1 << 14, max_batch=4096)


@pytest.mark.parametrize("profile", [0, 1])
def test_light_replay_kernel(rl, profile, monkeypatch):
    """two batches of 2^19 requests (the smallest the engine lets the light
    replay kernel run at) with no hot key and 33 configs: the second batch
    takes k_replay_light<false>.  The oracle bounds the run time, and its
    miniredis profile takes four times as long per token-bucket step: there
    it replays a seeded quarter of the keys (keys never interact; the quarter
    still uses every config id), on the Redis-7 profile all of them."""
    N = 33
    assert N > MAX_LCFG
    monkeypatch.setenv("RL_SMALL_MAX", "4096")
    configs, tr, sizes = many_config_light_trace(4100 + profile, N)
    assert sizes == [1 << 19, 1 << 19]
    eng = make_engine(rl, profile, tb=1 << 17, win=1 << 17, max_batch=1 << 19)
    sim = oracle.OracleSim(profile)
    for a, L, W in configs:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    light = 0
    for i, (key, ts, n, cfg, _) in enumerate(split(tr, sizes)):
        before = eng.stats().light_batches
        res = eng.decide(key, ts, n, cfg)
        light += int(eng.stats().light_batches - before)
        assert np.all(res.decision <= 2)
        pick = np.ones(key.size, bool)
        if profile == 1:
            pick = (key * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(62)) == np.uint64(0)
        assert set(np.unique(cfg[pick]).tolist()) == set(range(N))
        ref = sim.decide(key[pick], ts[pick], n[pick], cfg[pick])
        sub = rl.Decisions(res.decision[pick], res.remaining[pick], res.retry_after_ns[pick],
                           res.reset_at_ns[pick], res.tokens[pick])
        assert_same(sub, ref, configs, cfg[pick], what=f"batch {i}")
    assert light >= 1 and eng.stats().light_batches >= 1
    eng.close()


# --- registration between batches, state carried -----------------------------------

GROW_TB = (30, 32, 64)      # token buckets whatever the cycle says (30 is one by the cycle)


def _grow_batch(rng, cfg_ids, t, m=20_000, hot=4500, with_hot=True):
    """m requests on configs cfg_ids: 12 keys per config (cfg = key % 1000,
    stable while configs are added) and the hot token-bucket key of config 30"""
    ids = np.asarray(cfg_ids, np.uint64)
    key = ids[rng.integers(0, ids.size, m)] + np.uint64(1000) * rng.integers(1, 13, m).astype(np.uint64)
    if with_hot:
        key[rng.permutation(m)[:hot]] = 30
    ts = t + np.cumsum(rng.choice([0, 1, 1000, 250_000, 50_000_000, 700_000_000], m,
                                  p=[0.05, 0.05, 0.4, 0.2, 0.2, 0.1])).astype(np.int64)
    n = rng.choice([1, 1, 1, 2, 3, 7], m).astype(np.int64)
    n[rng.random(m) < 0.01] = 1 << 62
    return (key, ts, n, (key % np.uint64(1000)).astype(np.uint32), None), int(ts[-1])


def grow_plan(seed):
    """[(configs registered when the batch is decided, batch)]: 32 configs;
    the 33rd (the hot key's state continues under the other kernel
    instantiation); 64; the 65th (d_cfg moves) with requests on configs 0, 31,
    32, 63 and 64 only; 130 (d_cfg moves again at the 129th)"""
    rng = np.random.default_rng(seed)
    configs = many_configs(seed, 130, tb_ids=GROW_TB)
    plan, t = [], T0
    for ncfg, ids, with_hot in [(32, range(32), True), (33, range(33), True), (64, range(64), True),
                                (65, [0, 31, 32, 63, 64], False), (130, range(130), True)]:
        b, t = _grow_batch(rng, list(ids), t, with_hot=with_hot)
        plan.append((ncfg, b))
    return configs, plan


def _register_up_to(eng, sim, configs, ncfg, have):
    for i in range(have, ncfg):
        a, L, W = configs[i]
        assert eng.register(a, L, W) == sim.add_config(a, L, W) == i
    return ncfg


@pytest.mark.parametrize("profile", [0, 1])
def test_register_between_batches(rl, profile, monkeypatch):
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    configs, plan = grow_plan(4200)
    assert [p[0] for p in plan] == [32, 33, 64, 65, 130] and 33 > MAX_LCFG and 65 > CFG_CAP and 130 > 2 * CFG_CAP
    eng = small_engine(rl, profile)
    sim = oracle.OracleSim(profile)
    have = 0
    for i, (ncfg, (key, ts, n, cfg, sms)) in enumerate(plan):
        have = _register_up_to(eng, sim, configs, ncfg, have)
        assert int(cfg.max()) == ncfg - 1
        res = eng.decide(key, ts, n, cfg, sms)
        assert_same(res, sim.decide(key, ts, n, cfg, sms), configs, cfg, what=f"batch {i} ({ncfg} configs)")
        if ncfg != 65:
            assert int((key == 30).sum()) >= 4096 and eng.stats().last_heavy >= 1
    eng.close()


def test_register_between_pipelined_batches(rl, monkeypatch):
    """the same through the device API with RL_OPT_PIPELINE: each step's batch
    enqueued as two halves back to back, then the next configs registered with
    those batches still in flight (registration drains); every batch against
    the oracle once all are done"""
    import torch
    monkeypatch.setenv("RL_SMALL_MAX", "0")
    configs, plan = grow_plan(4201)
    eng = small_engine(rl, 0, flags=rl.OPT_PIPELINE)
    sim = oracle.OracleSim(0)
    dev = torch.device("cuda", 0)
    steps = []
    for ncfg, b in plan:
        h = b[0].size // 2
        for part in split(b, [h, b[0].size - h]):
            key, ts, n, cfg, _ = part
            ins = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
                   for x in (key, ts, n, cfg.view(np.int32))]
            m = key.size
            outs = [torch.empty(m, dtype=torch.uint8, device=dev)] + \
                [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] + \
                [torch.empty(m, dtype=torch.float64, device=dev)]
            steps.append((ncfg, part, ins, outs))
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    have, refs = 0, []
    for ncfg, (key, ts, n, cfg, _), (k, t, nn, c), o in steps:
        have = _register_up_to(eng, sim, configs, ncfg, have)
        eng.decide_device(k.numel(), k.data_ptr(), t.data_ptr(), nn.data_ptr(), c.data_ptr(), None,
                          *[x.data_ptr() for x in o], stream)
        refs.append(sim.decide(key, ts, n, cfg))
    torch.cuda.synchronize()
    assert eng.sync() == 0, eng.last_error()
    for i, ((ncfg, (key, ts, n, cfg, _), _, o), ref) in enumerate(zip(steps, refs)):
        res = rl.Decisions(*[x.cpu().numpy() for x in o])
        assert_same(res, ref, configs, cfg, what=f"batch {i} ({ncfg} configs)")
    eng.close()


# --- boundary ids ------------------------------------------------------------------

@pytest.mark.parametrize("N", [32, 33, 64, 65])
def test_boundary_config_ids(rl, N, monkeypatch):
    """in one batch: requests on config N - 1 are decided, requests with cfg ==
    N and cfg == N + 63 are rejected (decision 3), and every other result is
    what it is without them -- a batch for k_small, then one for the full
    launch sequence"""
    assert (N > MAX_LCFG) == (N >= 33) and (N > CFG_CAP) == (N >= 65)
    monkeypatch.setenv("RL_SMALL_MAX", "4096")
    configs, tr, _ = many_config_trace(4300 + N, N, nbatch=1, m=13_000, hot=4200)
    rng = np.random.default_rng(N)
    eng = small_engine(rl, 0)
    sim = oracle.OracleSim(0)
    for a, L, W in configs:
        assert eng.register(a, L, W) == sim.add_config(a, L, W)
    for i, (key, ts, n, cfg, _) in enumerate(split(tr, [3500, 9500])):
        cfg = cfg.copy()
        bad = rng.permutation(key.size)[:300]
        cfg[bad[:150]] = N
        cfg[bad[150:]] = N + 63
        unknown = cfg >= N
        keep = ~unknown
        res = eng.decide(key, ts, n, cfg, check=False)
        assert res.status == rl.RL_OK
        assert np.all(res.decision[unknown] == 3)
        last = keep & (cfg == N - 1) & (n > 0)
        assert int(last.sum()) > 1000 and np.all(res.decision[last] <= 1)
        ref = sim.decide(key[keep], ts[keep], n[keep], cfg[keep])
        sub = rl.Decisions(res.decision[keep], res.remaining[keep], res.retry_after_ns[keep],
                           res.reset_at_ns[keep], res.tokens[keep])
        assert_same(sub, ref, configs, cfg[keep], what=f"batch {i}")
    eng.close()


# --- Peek and Reset (k_peek and k_reset read d_cfg[cfg]) ------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_peek_and_reset_high_config_ids(rl, profile):
    N = 66
    assert N - 1 > CFG_CAP and N > MAX_LCFG
    configs = many_configs(4400, N, tb_ids=())
    ids = np.array([0, 31, 32, 33, 34, 63, 64, 65], np.uint64)      # TB, SW and FW at >= 32 and at > 64
    assert {configs[c][0] for c in (32, 33, 34)} == {1, 2, 3} and {configs[c][0] for c in (63, 64, 65)} == {1, 2, 3}
    rng = np.random.default_rng(4400 + profile)
    eng = small_engine(rl, profile)
    csim, psim = oracle.OracleSim(profile), po.Sim(profile)
    for a, L, W in configs:
        assert eng.register(a, L, W) == csim.add_config(a, L, W) == psim.add_config(a, L, W)

    def batch(m, t):
        key = ids[rng.integers(0, ids.size, m)] + np.uint64(1000) * rng.integers(1, 9, m).astype(np.uint64)
        ts = t + np.cumsum(rng.choice([0, 1000, 250_000, 50_000_000, 700_000_000], m)).astype(np.int64)
        return key, ts, rng.choice([1, 1, 2, 3], m).astype(np.int64), (key % np.uint64(1000)).astype(np.uint32)

    t = T0
    for rnd in range(3):
        key, ts, n, cfg = batch(5000, t)
        t = int(ts[-1])
        assert_same(eng.decide(key, ts, n, cfg), csim.decide(key, ts, n, cfg), configs, cfg, what=f"round {rnd}")
        sim_decide(psim, key, ts, n, cfg)
        # peeks: every key of every id, n = 0 (status), 1 and 5, now and 3 s on
        pk = np.repeat(ids, 9) + np.uint64(1000) * np.tile(np.arange(9, dtype=np.uint64), ids.size)   # key 0: unseen
        pk = np.tile(pk, 6)
        pn = np.repeat(np.array([0, 1, 5, 0, 1, 5], np.int64), pk.size // 6)
        pts = np.full(pk.size, t, np.int64) + np.repeat(np.array([0, 0, 0, 3, 3, 3], np.int64) * NS, pk.size // 6)
        pcfg = (pk % np.uint64(1000)).astype(np.uint32)
        exp = peek_expected(psim, pk, pts, pn, pcfg)
        assert_peek(eng.peek(pk, pts, pn, pcfg), exp, configs, pcfg, what=f"peek {rnd}")
        # Reset of two keys of every id, in all three simulators
        for c in ids.tolist():
            for j in (1, 2):
                k = c + 1000 * j
                eng.reset(c, k, t)
                csim.reset(c, k, t)
                psim.reset(c, k, t)
        exp = peek_expected(psim, pk, pts, pn, pcfg)
        assert_peek(eng.peek(pk, pts, pn, pcfg), exp, configs, pcfg, what=f"peek after reset {rnd}")
    eng.close()


# --- the routed path ---------------------------------------------------------------

ROUTED_N = 40


def many_config_batches(rank, nbatch=3, m=20_000, N=ROUTED_N):
    """one rank's steps over N configs, cfg = key % N, in time order"""
    assert rank == 0            # one seed: the configs are many_configs(4500, N)
    _, (key, ts, n, cfg, _), sizes = many_config_trace(4500, N, nbatch=nbatch, m=m)
    out, o = [], 0
    for s in sizes:
        out.append((key[o:o + s], ts[o:o + s], n[o:o + s], cfg[o:o + s]))
        o += s
    return out


def test_routed_path_one_rank_many_configs():
    """world size 1 with 40 configs (buckets and results read in place): the
    routed records' config ids and the engine's <false> replay behind
    rl_decide_routed_device"""
    from test_route_gpu import _check, _spawn
    assert ROUTED_N > MAX_LCFG
    configs = many_configs(4500, ROUTED_N)
    _check(_spawn(1, "nccl", many_config_batches, configs=configs), 1, 3, False)
