"""The usage tally on the GPU (rl_tally_*, csrc/rl_tally.h) against
tally_cases.expected_tally: of the C oracle's decisions where a test decides,
of arrays fed straight to the tally where it is about the kernel's shapes."""
import ctypes as C

import numpy as np
import pytest

import oracle
from table_cases import home, keys_with_home, one_key_per_home
from tally_cases import KEY_RESERVED, LDS_CFGS, check_read, expected_tally, fits
from tracegen import CONFIG_SETS, NS, T0, many_configs, random_trace

pytestmark = pytest.mark.gpu
U64 = np.uint64


def engine(rl, configs, profile=0, flags=0, max_batch=1 << 15, key_slots=0, tally=True):
    eng = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=max_batch, flags=flags)
    for a, L, W in configs:
        eng.register(a, L, W)
    if tally:
        eng.tally_enable(key_slots)
    return eng


def sim_of(profile, configs):
    sim = oracle.OracleSim(profile)
    for a, L, W in configs:
        sim.add_config(a, L, W)
    return sim


def oracle_decide(sim, key, ts, n, cfg):
    """the C oracle's outputs; the reserved key id, which the oracle does not
    know, is RL_INVALID and never reaches it"""
    ok = key != U64(KEY_RESERVED)
    out = [np.full(key.size, 3, np.uint8), np.zeros(key.size, np.int64), np.zeros(key.size, np.int64),
           np.zeros(key.size, np.int64), np.full(key.size, np.nan)]
    for o, r in zip(out, sim.decide(key[ok], ts[ok], n[ok], cfg[ok])):
        o[ok] = r
    return out


def to_dev(*arrs):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                             np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                             np.ascontiguousarray(x)).to(dev) for x in arrs]


def tally_dev(eng, key, cfg, n, dec):
    """one rl_tally_batch_device call: one launch whatever max_batch is"""
    import torch
    t = to_dev(np.asarray(key, U64), np.asarray(cfg, np.uint32), np.asarray(n, np.int64), np.asarray(dec, np.uint8))
    torch.cuda.synchronize()
    eng.tally_device(t[0].numel(), *[x.data_ptr() for x in t], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def mixed_trace(seed, m, configs):
    """random_trace with n <= 0 and 2^62, unknown config ids and the reserved key"""
    key, ts, n, cfg, _ = random_trace(seed, m, 300, configs, big_n=True)
    rng = np.random.default_rng(seed + 1000)
    cfg = cfg.copy()
    key = key.copy()
    cfg[rng.random(m) < 0.02] = len(configs)
    cfg[rng.random(m) < 0.01] = len(configs) + 77
    cfg[rng.random(m) < 0.005] = 0xffffffff
    key[rng.random(m) < 0.01] = U64(KEY_RESERVED)
    n[rng.random(m) < 0.01] = -3
    return key, ts, n, cfg


# --- 1. counters against decisions ----------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_counters_against_decisions(rl, profile):
    configs = CONFIG_SETS["mixed"]
    key, ts, n, cfg = mixed_trace(7 + profile, 5000, configs)
    eng, sim = engine(rl, configs, profile), sim_of(profile, configs)
    decs = []
    for lo, hi in [(0, 1700), (1700, 3400), (3400, 5000)]:
        s = slice(lo, hi)
        got = eng.decide(key[s], ts[s], n[s], cfg[s], check=False)
        ref = oracle_decide(sim, key[s], ts[s], n[s], cfg[s])
        assert np.array_equal(got.decision, ref[0])
        eng.tally(key[s], cfg[s], n[s], got.decision)
        decs.append(ref[0])
    dec = np.concatenate(decs)
    e = expected_tally(key, cfg, n, dec, len(configs))
    assert e.unknown_cfg > 50
    assert e.count[:, 0].sum() > 300 and e.count[:, 1].sum() > 300 and e.count[:, 3].sum() > 50
    assert fits(list(e.keys), 65536)
    t = eng.tally_read(top=1000)
    check_read(t, e, len(configs), f"profile {profile}")
    assert (t.info.batches, t.info.requests, t.info.key_slots) == (3, 5000, 65536)
    assert eng.sync() == 0
    eng.close()


# --- 2. shapes ------------------------------------------------------------------------

def test_shapes(rl):
    """one launch each: m around the wave, the block and what the capped grid
    covers with one request per thread; one denied key in all 64 lanes of a
    wave; 64 distinct denied keys in a wave; allowed and denied lanes in turn"""
    cap = rl.TALLY_GRID_CAP
    assert cap == 1024 * 256
    configs = CONFIG_SETS["mixed"][:6]
    eng = engine(rl, configs)
    rng = np.random.default_rng(3)
    cases = {}
    for m in (1, 63, 64, 65, 257, cap + 1):
        cases[f"m={m}"] = (rng.integers(0, 40, m).astype(U64), rng.integers(0, 7, m).astype(np.uint32),
                           rng.choice([1, 2, 5, 0, -1], m).astype(np.int64),
                           rng.choice([0, 0, 1, 1, 2, 3, 9], m).astype(np.uint8))
    one = np.full(64, 77, U64)
    cases["one denied key x 64"] = (one, np.full(64, 2, np.uint32), np.arange(1, 65).astype(np.int64),
                                    np.zeros(64, np.uint8))
    cases["64 denied keys"] = (np.arange(1000, 1064).astype(U64), np.full(64, 1, np.uint32), np.full(64, 3, np.int64),
                               np.zeros(64, np.uint8))
    cases["interleaved"] = (np.tile(np.array([5, 5, 6, 5], U64), 48), np.tile(np.array([0, 0, 3, 0], np.uint32), 48),
                            np.tile(np.array([2, 2, 1, 4], np.int64), 48), np.tile(np.array([0, 1, 0, 1], np.uint8), 48))
    # a full wave of one config and one decision (the wave adds once), then the same with one lane off
    cases["uniform wave"] = (np.arange(64).astype(U64), np.full(64, 4, np.uint32), np.full(64, 1 << 40, np.int64),
                             np.ones(64, np.uint8))
    off = np.ones(128, np.uint8)
    off[100] = 2
    cases["uniform wave, one lane off"] = (np.arange(128).astype(U64), np.full(128, 4, np.uint32),
                                          np.full(128, 7, np.int64), off)
    for what, (key, cfg, n, dec) in cases.items():
        tally_dev(eng, key, cfg, n, dec)
        e = expected_tally(key, cfg, n, dec, len(configs))
        assert fits(list(e.keys), 65536)
        t = eng.tally_read(top=100, clear=True)
        check_read(t, e, len(configs), what)
        assert (t.info.batches, t.info.requests) == (1, key.size), what
    # nothing to count, and null arrays
    assert rl.lib.rl_tally_batch_device(eng.h, 0, None, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_tally_batch(eng.h, 0, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_tally_batch_device(eng.h, 3, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_batch(eng.h, 3, None, None, None, None) == rl.RL_EINVAL
    t = eng.tally_read()
    assert (t.info.batches, t.info.requests, t.keys_tracked) == (0, 0, 0) and not t.cfg["count"].any()
    eng.close()


# --- 3. hot key -----------------------------------------------------------------------

def test_hot_key(rl):
    """100,000 denied requests of one key among 30,000 others, in one host
    call of four chunks: the key's count and units are exact, it ranks first"""
    configs = CONFIG_SETS["mixed"][:4]
    rng = np.random.default_rng(5)
    m = 130_000
    key = rng.integers(0, 5000, m).astype(U64)
    cfg = (key % U64(4)).astype(np.uint32)
    dec = rng.choice([0, 1, 1, 1], m).astype(np.uint8)
    n = rng.choice([1, 2, 3], m).astype(np.int64)
    hot = rng.permutation(m)[:100_000]
    key[hot], cfg[hot], dec[hot] = U64(123456789), 1, 0
    eng = engine(rl, configs)
    eng.tally(key, cfg, n, dec)
    e = expected_tally(key, cfg, n, dec, 4)
    assert e.keys[123456789][0] == 100_000 and fits(list(e.keys), 65536)
    t = eng.tally_read(top=len(e.keys))
    check_read(t, e, 4)
    top = eng.tally_read(top=1).keys
    assert (int(top[0]["key_id"]), int(top[0]["denied"]), int(top[0]["units_denied"]), int(top[0]["cfg_id"])) == \
        (123456789, 100_000, int(n[hot].sum()), 1)
    assert (t.info.batches, t.info.requests) == (1, m)
    eng.close()


# --- 4. many configs ------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_many_configs(rl, profile):
    """70 configs, more than the kernel keeps in LDS: requests on the six
    highest ids only, which go to the global counters directly"""
    N = 70
    assert N - 6 >= LDS_CFGS
    configs = many_configs(3, N)
    key, ts, n, _, _ = random_trace(31 + profile, 4000, 90, configs, big_n=True)
    cfg = (N - 6 + key % U64(6)).astype(np.uint32)
    cfg[::97] = N            # unknown
    eng, sim = engine(rl, configs, profile), sim_of(profile, configs)
    got = eng.decide(key, ts, n, cfg, check=False)
    ref = oracle_decide(sim, key, ts, n, cfg)
    assert np.array_equal(got.decision, ref[0])
    tally_dev(eng, key, cfg, n, got.decision)
    e = expected_tally(key, cfg, n, ref[0], N)
    assert not e.count[:N - 6].any() and (e.count[N - 6:, :2] > 0).all()
    check_read(eng.tally_read(top=200), e, N, f"profile {profile}")
    # a config registered after the tally was enabled: a zero row, and counted from then on
    c = eng.register(3, 2, NS)
    assert c == N
    t = eng.tally_read()
    assert t.cfg.size == N + 1 and not t.cfg["count"][N].any() and np.array_equal(t.cfg["count"][:N], e.count)
    eng.tally([1, 1, 2], [N, N, N + 1], [4, 5, 6], [1, 0, 0])
    t = eng.tally_read()
    assert t.cfg["count"][N].tolist() == [1, 1, 0, 0] and t.cfg["units"][N].tolist() == [5, 4]
    assert t.info.unknown_cfg == e.unknown_cfg + 1 and np.array_equal(t.cfg["count"][:N], e.count)
    eng.close()


def test_rows_grow_with_configs(rl):
    """the tally enabled with three configs, 67 more registered afterwards:
    the counter rows move to a larger array with what they held"""
    configs = many_configs(3, 70)
    eng = engine(rl, configs[:3])
    first = ([1, 2, 3, 3], [0, 1, 2, 3], [4, 5, 6, 7], [1, 0, 1, 1])
    eng.tally(*first)
    for a, L, W in configs[3:]:
        eng.register(a, L, W)
    second = ([1, 8, 9, 9], [0, 63, 64, 69], [1, 2, 3, 4], [0, 0, 1, 0])
    eng.tally(*second)
    e = expected_tally(*[np.concatenate([np.asarray(x), np.asarray(y)]) for x, y in zip(first, second)], 70)
    e.count[3, 1] -= U64(1)       # config 3 was not registered yet when the first batch came
    e.units[3, 1] -= U64(7)
    e.unknown_cfg += 1
    check_read(eng.tally_read(top=10), e, 70)
    eng.close()


# --- 5. key table ---------------------------------------------------------------------

def test_key_table(rl):
    configs = CONFIG_SETS["mixed"][:3]
    eng = engine(rl, configs, key_slots=16)
    rng = np.random.default_rng(8)
    # eight denied keys of one home slot: a probe run of eight, all exact
    ks = keys_with_home(15, 9, 8, start=1 << 20)
    assert (home(ks, 15) == U64(9)).all() and fits(ks, 16)
    key = ks[rng.integers(0, 8, 3000)]
    key[:8] = ks
    cfg = (key % U64(3)).astype(np.uint32)
    n = rng.choice([1, 2, 9], 3000).astype(np.int64)
    dec = rng.choice([0, 0, 1], 3000).astype(np.uint8)
    dec[:8] = 0
    eng.tally(key, cfg, n, dec)
    e = expected_tally(key, cfg, n, dec, 3)
    assert len(e.keys) == 8
    t = eng.tally_read(top=16, clear=True)
    check_read(t, e, 3, "one home slot")
    assert t.info.key_slots == 16
    # 64 distinct denied keys into 16 slots: which keys get a slot depends on
    # the order the waves arrive in; a tracked key is exact, the rest is summed
    ks = np.arange(5000, 5064).astype(U64)
    key = ks[rng.integers(0, 64, 6000)]
    key[:64] = ks
    cfg = (key % U64(3)).astype(np.uint32)
    n = rng.choice([1, 2, 9], 6000).astype(np.int64)
    dec = np.zeros(6000, np.uint8)
    tally_dev(eng, key[:3000], cfg[:3000], n[:3000], dec[:3000])
    tally_dev(eng, key[3000:], cfg[3000:], n[3000:], dec[3000:])
    e = expected_tally(key, cfg, n, dec, 3)
    t = eng.tally_read(top=64)
    assert 1 <= t.keys_tracked <= 16 and t.keys.size == t.keys_tracked == t.info.keys_tracked
    # 16 probes cover the whole table: a key finds a free slot while there is one
    assert t.keys_tracked == 16
    for r in t.keys:
        assert (int(r["denied"]), int(r["units_denied"])) == tuple(e.keys[int(r["key_id"])][:2])
    assert int(t.keys["denied"].sum()) + t.info.untracked_requests == e.denied == 6000
    assert int(t.keys["units_denied"].sum()) + t.info.untracked_units == e.units_denied
    assert np.array_equal(t.cfg["count"], e.count) and np.array_equal(t.cfg["units"], e.units)
    # the reserved key id is never tracked
    eng.tally_read(clear=True)
    eng.tally([KEY_RESERVED, KEY_RESERVED, 4], [0, 0, 0], [3, 4, 5], [0, 0, 0])
    t = eng.tally_read(top=4)
    assert t.keys["key_id"].tolist() == [4] and (t.info.untracked_requests, t.info.untracked_units) == (2, 7)
    eng.close()


# --- 6. wrap --------------------------------------------------------------------------

def test_units_wrap(rl):
    """five allowed and five denied requests of n = 2^62, and n = 2^63 - 1
    twice: the sums modulo 2^64, in the config's row and the key's record"""
    eng = engine(rl, CONFIG_SETS["mixed"][:2])
    key = np.array([1, 2, 3, 4, 5, 9, 9, 9, 9, 9, 6, 6], U64)
    cfg = np.array([0] * 5 + [1] * 5 + [0, 0], np.uint32)
    n = np.array([1 << 62] * 10 + [(1 << 63) - 1] * 2, np.int64)
    dec = np.array([1] * 5 + [0] * 5 + [0, 0], np.uint8)
    eng.tally(key, cfg, n, dec)
    e = expected_tally(key, cfg, n, dec, 2)
    assert int(e.units[0, 1]) == 1 << 62 and int(e.units[1, 0]) == 1 << 62 and int(e.units[0, 0]) == (1 << 64) - 2
    t = eng.tally_read(top=8)
    check_read(t, e, 2)
    eng.close()


# --- 7. read and clear ----------------------------------------------------------------

def test_read_and_clear(rl):
    eng = engine(rl, CONFIG_SETS["mixed"][:3], key_slots=16)
    ks = one_key_per_home(15, 0, 16)              # fills the table: one key per slot
    extra = int(keys_with_home(15, 3, 2, start=int(ks.max()) + 1)[0])
    key = np.concatenate([ks, ks[:5]])
    cfg, n, dec = (key % U64(3)).astype(np.uint32), np.full(21, 2, np.int64), np.zeros(21, np.uint8)
    eng.tally(key, cfg, n, dec)
    eng.tally([extra, extra, 7], [1, 1, 2], [5, 6, 1], [0, 0, 1])     # no slot left for `extra`
    e = expected_tally(key, cfg, n, dec, 3)
    a, b = eng.tally_read(top=16), eng.tally_read(top=16)
    assert a.cfg.tobytes() == b.cfg.tobytes() and a.keys.tobytes() == b.keys.tobytes()
    assert bytes(a.info) == bytes(b.info)
    assert a.keys_tracked == 16 and {int(k) for k in a.keys["key_id"]} == set(ks.tolist())
    assert a.keys["key_id"][:5].tolist() == sorted(ks[:5].tolist())       # denied twice, by key id
    assert (a.info.untracked_requests, a.info.untracked_units, a.info.batches, a.info.requests) == (2, 11, 2, 24)
    assert a.cfg["count"][1, 0] == e.count[1, 0] + 2 and a.cfg["count"][2, 1] == 1
    c = eng.tally_read(top=16, clear=True)
    assert c.cfg.tobytes() == a.cfg.tobytes() and c.keys.tobytes() == a.keys.tobytes()
    z = eng.tally_read(top=16)
    assert not z.cfg["count"].any() and not z.cfg["units"].any() and z.keys.size == 0 and z.keys_tracked == 0
    i = z.info
    assert (i.keys_tracked, i.untracked_requests, i.untracked_units, i.unknown_cfg, i.bad_codes, i.batches,
            i.requests, i.key_slots) == (0, 0, 0, 0, 0, 0, 0, 16)
    # from zero again; the key that had no slot gets one now
    eng.tally([extra, extra, 7], [1, 1, 2], [5, 6, 1], [0, 0, 1])
    t = eng.tally_read(top=16)
    check_read(t, expected_tally([extra, extra, 7], [1, 1, 2], [5, 6, 1], [0, 0, 1], 3), 3)
    assert (t.info.batches, t.info.requests) == (1, 3)
    eng.close()


# --- 8. ordering ----------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("size", [6000, 700])
def test_order_in_flight(rl, profile, size):
    """RL_OPT_PIPELINE, device API, one stream, no host sync: decide, tally,
    decide, tally, read.  Each tally sees the decisions of the batch before it
    (above and below the engine's single-workgroup cut of 4096)."""
    import torch
    configs = CONFIG_SETS["mixed"]
    key, ts, n, cfg, _ = random_trace(41 + profile, 2 * size, 200, configs, big_n=True)
    eng, sim = engine(rl, configs, profile, flags=rl.OPT_PIPELINE), sim_of(profile, configs)
    dev = torch.device("cuda", 0)
    parts = [slice(0, size), slice(size, 2 * size)]
    ins = [to_dev(key[s], ts[s], n[s], cfg[s]) for s in parts]
    outs = [[torch.full((size,), 9, dtype=torch.uint8, device=dev)] +
            [torch.empty(size, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(size, dtype=torch.float64, device=dev)] for _ in parts]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for i, o in zip(ins, outs):
        eng.decide_device(size, i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), None,
                          *[x.data_ptr() for x in o], stream)
        eng.tally_device(size, i[0].data_ptr(), i[3].data_ptr(), i[2].data_ptr(), o[0].data_ptr(), stream)
    t = eng.tally_read(top=400)
    ref = np.concatenate([sim.decide(key[s], ts[s], n[s], cfg[s])[0] for s in parts])
    torch.cuda.synchronize()
    assert eng.sync() == 0
    assert np.array_equal(np.concatenate([o[0].cpu().numpy() for o in outs]), ref)
    check_read(t, expected_tally(key, cfg, n, ref, len(configs)), len(configs))
    assert (t.info.batches, t.info.requests) == (2, 2 * size)
    eng.close()


# --- 9. off means untouched -----------------------------------------------------------

def test_off_is_einval(rl):
    eng = engine(rl, CONFIG_SETS["mixed"][:2], tally=False)
    z8, z4, z1 = np.zeros(4, U64), np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert rl.lib.rl_tally_batch(eng.h, 4, p(z8), p(z4), p(z8), p(z1)) == rl.RL_EINVAL
    assert rl.lib.rl_tally_batch_device(eng.h, 4, p(z8), p(z4), p(z8), p(z1), None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_batch_device(eng.h, 0, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_read(eng.h, None, 0, None, None, 0, None, None, 0) == rl.RL_EINVAL
    with pytest.raises(rl.EngineError):
        eng.tally_read()
    # bad options; a second enable
    o = rl.rl_tally_opts(key_slots=16)
    o.struct_size = 4
    assert rl.lib.rl_tally_enable(eng.h, C.byref(o)) == rl.RL_EINVAL
    assert rl.lib.rl_tally_enable(eng.h, C.byref(rl.rl_tally_opts(key_slots=(1 << 24) + 1))) == rl.RL_EINVAL
    eng.tally_enable(100)                       # rounded up
    assert eng.tally_read().info.key_slots == 128
    assert rl.lib.rl_tally_enable(eng.h, C.byref(rl.rl_tally_opts())) == rl.RL_EINVAL
    eng.close()


@pytest.mark.parametrize("profile", [0, 1])
def test_decisions_and_stats_untouched(rl, profile):
    """the same trace on an engine with the tally on (and a tally behind every
    batch) and on one without: every decide output bit for bit, and rl_stats.
    On the tallying engine the whole rl_stats struct is the same bytes before
    and after the tally calls; across the two engines every field is compared
    but stamp_cycles, which are timers (10 ns ticks of the last replay)."""
    configs = CONFIG_SETS["mixed"]
    key, ts, n, cfg = mixed_trace(51 + profile, 9000, configs)
    a, b = engine(rl, configs, profile), engine(rl, configs, profile, tally=False)
    for lo in range(0, 9000, 3000):
        s = slice(lo, lo + 3000)
        ra = a.decide(key[s], ts[s], n[s], cfg[s], check=False)
        rb = b.decide(key[s], ts[s], n[s], cfg[s], check=False)
        before = bytes(a.stats())
        a.tally(key[s], cfg[s], n[s], ra.decision)
        tally_dev(a, key[s], cfg[s], n[s], ra.decision)
        a.tally_read(top=10, clear=lo == 3000)
        assert bytes(a.stats()) == before
        assert ra.status == rb.status
        for f in ("decision", "remaining", "retry_after_ns", "reset_at_ns"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
        # tokens: defined for decided token-bucket requests (configs 0 .. 4 of the mixed set)
        tb = (cfg[s] < 5) & (ra.decision <= 1)
        assert tb.sum() > 500 and ra.tokens[tb].tobytes() == rb.tokens[tb].tobytes()
    sa, sb = a.stats(), b.stats()
    for f, _ in rl.rl_stats._fields_:
        if f != "stamp_cycles":
            va, vb = getattr(sa, f), getattr(sb, f)
            assert (list(va) == list(vb)) if hasattr(va, "__len__") else va == vb, f
    assert a.sync() == b.sync() == 0
    a.close()
    b.close()
