"""The top keys on the GPU (rl_hot_*, csrc/rl_hot.h) against hot_cases.HotModel:
every comparison is equality with the model -- the tracked set (false positives
included), every estimate at read time, the order and the counters."""
import ctypes as C

import numpy as np
import pytest

import hot_cases as H
from table_cases import mix64
from tally_cases import fits
from tracegen import CONFIG_SETS, NS, many_config_trace

pytestmark = pytest.mark.gpu
U64 = np.uint64
CONFIGS = CONFIG_SETS["mixed"][:H.NCFG]


def engine(rl, configs=CONFIGS, flags=0, max_batch=1 << 15, hot=None, tally=False, profile=0):
    """hot: (hot_min, width, key_slots[, weight]) or None"""
    eng = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=max_batch, flags=flags)
    for a, L, W in configs:
        eng.register(a, L, W)
    if tally:
        eng.tally_enable(0)
    if hot:
        eng.hot_enable(*hot)
    return eng


def to_dev(*arrs):
    import torch
    dev = torch.device("cuda", 0)
    return [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                             np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                             np.ascontiguousarray(x)).to(dev) for x in arrs]


def hot_dev(eng, key, cfg, n, dec):
    """one rl_hot_batch_device call: one k_hot_add and one k_hot_pick launch whatever max_batch is"""
    import torch
    t = to_dev(np.asarray(key, U64), np.asarray(cfg, np.uint32), np.asarray(n, np.int64), np.asarray(dec, np.uint8))
    torch.cuda.synchronize()
    eng.hot_batch_device(t[0].numel(), *[x.data_ptr() for x in t], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def one_call(mod, eng, key, cfg, n, dec):
    key, cfg, n, dec = (np.asarray(key, U64), np.asarray(cfg, np.uint32), np.asarray(n, np.int64),
                        np.asarray(dec, np.uint8))
    hot_dev(eng, key, cfg, n, dec)
    mod.call(key, cfg, n, dec)


# --- 1. three calls, false positives included -------------------------------------------

def test_three_calls(rl):
    """5000, 5037 and 5074 requests (no multiple of 64 or 256), width 64: the
    tracked set is the model's candidate set with its false positives"""
    calls = H.zipf_calls()
    assert [c[0].size for c in calls] == [5000, 5037, 5074]
    eng = engine(rl, hot=(H.ZIPF_HOT_MIN, 64, 4096))
    mod = H.HotModel(64, H.ZIPF_HOT_MIN, H.NCFG)
    for c in calls:
        one_call(mod, eng, *c)
    assert len(set(mod.candidates) - mod.true_hot()) >= 1 and fits(list(mod.candidates), 4096)
    h = eng.hot_read(top=4096)
    H.check_read(h, mod, "zipf")
    i = h.info
    assert (i.width, i.depth, i.key_slots, i.hot_min, i.weight) == (64, 4, 4096, H.ZIPF_HOT_MIN, 0)
    assert (i.batches, i.requests) == (3, 5000 + 5037 + 5074) and i.skipped > 100
    # the top three only: the same order, cut
    top = eng.hot_read(top=3)
    assert [(int(r["key_id"]), int(r["estimate"])) for r in top.keys] == mod.read()[:3] and top.keys_tracked == len(
        mod.candidates)
    assert eng.sync() == 0
    eng.close()


def test_host_call_in_chunks(rl):
    """rl_hot_batch with m above max_batch: all of the call's adds, then the
    look at its keys -- one call of the model, not one per chunk"""
    calls = H.zipf_calls()
    key, cfg, n, dec = [np.concatenate([c[j] for c in calls]) for j in range(4)]
    eng = engine(rl, max_batch=4096, hot=(H.ZIPF_HOT_MIN, 64, 4096))
    mod = H.HotModel(64, H.ZIPF_HOT_MIN, H.NCFG)
    eng.hot_batch(key, cfg, n, dec)
    mod.call(key, cfg, n, dec)
    per_chunk = H.model_of([tuple(a[o:o + 4096] for a in (key, cfg, n, dec)) for o in range(0, key.size, 4096)], 64,
                           H.ZIPF_HOT_MIN)
    assert set(per_chunk.candidates) <= set(mod.candidates)
    h = eng.hot_read(top=4096)
    H.check_read(h, mod, "chunks")
    assert (h.info.batches, h.info.requests) == (1, key.size)
    eng.close()


# --- 2. merge edges ---------------------------------------------------------------------

def lds_home(keys):
    """rl_hot.h: the LDS slot a key's probe run starts at in k_hot_add"""
    return ((mix64(keys) >> U64(40)) & U64(H.LDS_KEYS - 1)).astype(np.int64)


def test_merge_edges(rl):
    """hot_min 1, width 2^16: every counted key is a candidate, so a read
    reports the model's full column sums.  One key in 1 .. 257 lanes; two keys
    lane by lane; 64 keys in a wave; more keys than the block's LDS table holds"""
    eng = engine(rl, hot=(1, 1 << 16, 4096))
    rng = np.random.default_rng(2)
    cases = {}
    for m in (1, 63, 64, 65, 255, 256, 257):
        cases[f"one key x {m}"] = (np.full(m, 4242 + m, U64), np.full(m, 2, np.uint32), np.full(m, 3, np.int64),
                                   rng.choice([0, 1, 2], m).astype(np.uint8))
    cases["two keys lane by lane"] = (np.tile(np.array([5, 6], U64), 150), np.tile(np.array([0, 3], np.uint32), 150),
                                      np.ones(300, np.int64), np.ones(300, np.uint8))
    cases["64 keys in a wave"] = (np.arange(9000, 9064).astype(U64), np.full(64, 1, np.uint32), np.ones(64, np.int64),
                                  np.zeros(64, np.uint8))
    # the straight-to-global path: 2105 distinct keys, 256 per block, and in the
    # first block 40 keys of one LDS home slot, of which a probe run of 8 holds 8
    ids = np.arange(1 << 30, (1 << 30) + 60000, dtype=U64)
    crowd = ids[lds_home(ids) == 7][:40]
    rest = ids[lds_home(ids) != 7][:2105 - 40]
    many = np.concatenate([crowd, rest])
    assert crowd.size == 40 and np.unique(many).size == 2105 >= 4 * H.LDS_KEYS and fits(many, 4096)
    cases["LDS run taken"] = (many, (many % U64(H.NCFG)).astype(np.uint32), np.ones(2105, np.int64),
                              rng.choice([0, 1], 2105).astype(np.uint8))
    # ... and the same keys twice more in another order: merged in LDS where they fit, global where not
    again = np.concatenate([many, many])[rng.permutation(4210)]
    cases["LDS run taken, repeated keys"] = (again, (again % U64(H.NCFG)).astype(np.uint32), np.ones(4210, np.int64),
                                             np.ones(4210, np.uint8))
    for what, (key, cfg, n, dec) in cases.items():
        mod = H.HotModel(1 << 16, 1, H.NCFG)
        one_call(mod, eng, key, cfg, n, dec)
        assert len(mod.candidates) == np.unique(key).size
        h = eng.hot_read(top=4096, clear=True)
        H.check_read(h, mod, what)
        assert (h.info.batches, h.info.requests, h.info.total) == (1, key.size, key.size), what
    # nothing to count, and null arrays
    assert rl.lib.rl_hot_batch_device(eng.h, 0, None, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_hot_batch(eng.h, 0, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_hot_batch_device(eng.h, 3, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_hot_batch(eng.h, 3, None, None, None, None) == rl.RL_EINVAL
    h = eng.hot_read(top=8)
    assert (h.info.batches, h.info.requests, h.info.total, h.keys_tracked) == (0, 0, 0, 0)
    eng.close()


def test_stride(rl):
    """more requests than the capped grid covers with one per thread, half of
    them one key"""
    cap = rl.HOT_GRID_CAP
    assert cap == rl.lib.rl_hot_grid_cap() == 1024 * 256
    m = cap + 257
    rng = np.random.default_rng(4)
    key = (U64(50000) + rng.integers(0, 400, m).astype(U64))
    key[rng.permutation(m)[:m // 2]] = U64(77)
    cfg = (key % U64(H.NCFG)).astype(np.uint32)
    n = np.ones(m, np.int64)
    dec = rng.choice([0, 1], m).astype(np.uint8)
    eng = engine(rl, hot=(300, 1 << 16, 4096))
    mod = H.HotModel(1 << 16, 300, H.NCFG)
    one_call(mod, eng, key, cfg, n, dec)
    assert mod.true[77] >= m // 2 and len(mod.candidates) > 1
    h = eng.hot_read(top=4096)
    H.check_read(h, mod, "stride")
    assert int(h.keys["key_id"][0]) == 77 and int(h.keys["estimate"][0]) == mod.true[77]
    eng.close()


# --- 3. threshold -----------------------------------------------------------------------

def test_threshold(rl):
    hm = 50
    a, b, c, d = 101, 202, 303, 404     # a: hm - 1 then + 1; b: stays at hm - 1; c: passes in call 1; d: filler
    assert H.distinct_columns([a, b, c, d], 1 << 16)
    eng = engine(rl, hot=(hm, 1 << 16, 4096))
    mod = H.HotModel(1 << 16, hm, H.NCFG)
    key = np.array([a] * (hm - 1) + [b] * (hm - 1) + [c] * (hm + 5) + [d] * 3, U64)
    key = key[np.random.default_rng(1).permutation(key.size)]
    one_call(mod, eng, key, np.zeros(key.size, np.uint32), np.ones(key.size, np.int64), np.ones(key.size, np.uint8))
    h = eng.hot_read(top=16)
    assert [(int(r["key_id"]), int(r["estimate"])) for r in h.keys] == [(c, hm + 5)] == mod.read()
    one_call(mod, eng, [a, d], [1, 1], [1, 1], [0, 0])
    h = eng.hot_read(top=16)
    # c had no request in call 2: still there, with the estimate read now
    assert [(int(r["key_id"]), int(r["estimate"])) for r in h.keys] == [(c, hm + 5), (a, hm)] == mod.read()
    H.check_read(h, mod, "threshold")
    one_call(mod, eng, [c, c, d], [0, 0, 0], [1, 1, 1], [2, 0, 1])
    h = eng.hot_read(top=16)
    assert [(int(r["key_id"]), int(r["estimate"])) for r in h.keys] == [(c, hm + 7), (a, hm)] == mod.read()
    assert b not in mod.candidates and mod.true[b] == hm - 1
    eng.close()


# --- 4. overflow ------------------------------------------------------------------------

def test_overflow(rl):
    """width 16, 16 records, hot_min 2: more candidates than records.  Which
    keys won is not asserted; a tracked key is a model candidate with the
    model's estimate"""
    rng = np.random.default_rng(6)
    key = (U64(7000) + rng.integers(0, 200, 3000).astype(U64))
    cfg = (key % U64(H.NCFG)).astype(np.uint32)
    eng = engine(rl, hot=(2, 16, 16))
    mod = H.HotModel(16, 2, H.NCFG)
    one_call(mod, eng, key[:1500], cfg[:1500], np.ones(1500, np.int64), np.ones(1500, np.uint8))
    one_call(mod, eng, key[1500:], cfg[1500:], np.ones(1500, np.int64), np.zeros(1500, np.uint8))
    assert len(mod.candidates) > 16
    h = eng.hot_read(top=64)
    assert h.info.dropped > 0 and 1 <= h.keys_tracked <= 16 and h.keys.size == h.keys_tracked == h.info.keys_tracked
    # 16 probes cover the whole table: a key finds a free record while there is one
    assert h.keys_tracked == 16
    want = dict(mod.read())
    for r in h.keys:
        assert int(r["key_id"]) in want and int(r["estimate"]) == want[int(r["key_id"])]
    assert (h.info.total, h.info.skipped) == (mod.total, mod.skipped) == (3000, 0)
    est = [int(x) for x in h.keys["estimate"]]
    assert est == sorted(est, reverse=True)
    # a clear resets dropped
    eng.hot_read(clear=True)
    assert eng.hot_read().info.dropped == 0
    eng.close()


# --- 5. what does not count -------------------------------------------------------------

@pytest.mark.parametrize("weight", [H.REQUESTS, H.UNITS])
def test_skips(rl, weight):
    """the reserved key, an unregistered config, decisions 3 and 200, and in
    units mode n <= 0: one more skipped each, and nothing else"""
    eng = engine(rl, hot=(1, 1 << 16, 4096, weight))
    rows = [(H.KEY_RESERVED, 0, 1, 1), (5, H.NCFG, 1, 1), (5, 0xffffffff, 1, 0), (5, 0, 1, 3), (5, 0, 1, 200)]
    if weight == H.UNITS:
        rows += [(5, 0, 0, 1), (5, 0, -4, 0), (5, 0, -(1 << 63), 1)]
    for j, (k, c, n, d) in enumerate(rows):
        hot_dev(eng, [k], [c], [n], [d])
        h = eng.hot_read(top=8)
        assert (h.info.skipped, h.info.total, h.keys_tracked, h.info.dropped, h.keys.size) == (j + 1, 0, 0, 0, 0), rows[j]
        assert (h.info.batches, h.info.requests) == (j + 1, j + 1)
    # among counted requests, in one wave
    mod = H.HotModel(1 << 16, 1, H.NCFG, weight)
    key = np.array([r[0] for r in rows] + [5, 6, 5], U64)
    cfg = np.array([r[1] for r in rows] + [0, 1, 2], np.uint32)
    n = np.array([r[2] for r in rows] + [2, 3, 4], np.int64)
    dec = np.array([r[3] for r in rows] + [0, 1, 2], np.uint8)
    eng.hot_read(clear=True)
    one_call(mod, eng, key, cfg, n, dec)
    assert mod.skipped == len(rows) and mod.total == (9 if weight == H.UNITS else 3)
    if weight == H.REQUESTS:       # n <= 0 counts in requests mode
        one_call(mod, eng, [9, 9], [0, 0], [0, -7], [1, 0])
        assert mod.true[9] == 2
    H.check_read(eng.hot_read(top=8), mod, "skips among counted")
    eng.close()


def test_units(rl):
    """weights are n: a wave group of one, of many, a key across waves and
    blocks, large n with sums below 2^63"""
    rng = np.random.default_rng(9)
    m = 1500
    key = (U64(300) + rng.integers(0, 40, m).astype(U64))
    key[:700:2] = U64(299)
    cfg = (key % U64(H.NCFG)).astype(np.uint32)
    n = rng.choice([1, 2, 7, 50, 1 << 40], m).astype(np.int64)
    n[5] = 1 << 61
    n[rng.random(m) < 0.05] = 0
    dec = rng.choice([0, 1, 2], m).astype(np.uint8)
    eng = engine(rl, hot=(100, 1 << 16, 4096, H.UNITS))
    mod = H.HotModel(1 << 16, 100, H.NCFG, H.UNITS)
    one_call(mod, eng, key, cfg, n, dec)
    one_call(mod, eng, key[::-1].copy(), cfg[::-1].copy(), n[::-1].copy(), dec[::-1].copy())
    assert mod.total < 1 << 63 and mod.skipped > 50 and H.distinct_columns(sorted(mod.true), 1 << 16)
    h = eng.hot_read(top=100)
    H.check_read(h, mod, "units")
    assert h.info.weight == 1 and all(int(r["estimate"]) == mod.true[int(r["key_id"])] for r in h.keys)
    eng.close()


# --- 6. read, clear, enable -------------------------------------------------------------

def test_read_and_clear(rl):
    calls = H.zipf_calls(seed=3, sizes=(900, 901))
    eng = engine(rl, hot=(20, 256, 1024))
    mod = H.HotModel(256, 20, H.NCFG)
    for c in calls:
        one_call(mod, eng, *c)
    a, b = eng.hot_read(top=1024), eng.hot_read(top=1024)
    assert a.keys.tobytes() == b.keys.tobytes() and bytes(a.info) == bytes(b.info)
    H.check_read(a, mod, "before clear")
    assert a.keys_tracked > 3
    # key_cap 0 and null outputs
    assert rl.lib.rl_hot_read(eng.h, None, 0, None, None, 0) == rl.RL_OK
    buf = np.zeros(4, rl.HOT_KEY)
    buf["key_id"] = 99
    tracked = C.c_uint64()
    assert rl.lib.rl_hot_read(eng.h, buf.ctypes.data_as(C.c_void_p), 0, C.byref(tracked), None, 0) == rl.RL_OK
    assert tracked.value == a.keys_tracked and (buf["key_id"] == 99).all()
    assert rl.lib.rl_hot_read(eng.h, None, 4, C.byref(tracked), None, 0) == rl.RL_OK
    info = rl.rl_hot_info()
    info.struct_size = 4
    assert rl.lib.rl_hot_read(eng.h, None, 0, None, C.byref(info), 0) == rl.RL_EINVAL
    short = rl.rl_hot_info()
    short.struct_size = 24                       # a caller built against a shorter struct: width and depth only
    assert rl.lib.rl_hot_read(eng.h, None, 0, None, C.byref(short), 0) == rl.RL_OK
    assert (short.struct_size, short.width, short.depth, short.key_slots) == (24, 256, 4, 0)
    c = eng.hot_read(top=1024, clear=True)
    assert c.keys.tobytes() == a.keys.tobytes()
    z = eng.hot_read(top=1024)
    i = z.info
    assert z.keys.size == 0 and z.keys_tracked == 0
    assert (i.keys_tracked, i.dropped, i.total, i.skipped, i.batches, i.requests) == (0, 0, 0, 0, 0, 0)
    assert (i.width, i.depth, i.key_slots, i.hot_min, i.weight) == (256, 4, 1024, 20, 0)
    # from zero again: the sketch is zero too, or the second call alone would not equal a fresh model
    mod.clear()
    one_call(mod, eng, *calls[1])
    H.check_read(eng.hot_read(top=1024), mod, "after clear")
    eng.close()


def test_enable(rl):
    eng = engine(rl)
    z8, z4, z1 = np.zeros(4, U64), np.zeros(4, np.uint32), np.zeros(4, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert rl.lib.rl_hot_batch(eng.h, 4, p(z8), p(z4), p(z8), p(z1)) == rl.RL_EINVAL
    assert rl.lib.rl_hot_batch_device(eng.h, 4, p(z8), p(z4), p(z8), p(z1), None) == rl.RL_EINVAL
    assert rl.lib.rl_hot_batch_device(eng.h, 0, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_hot_read(eng.h, None, 0, None, None, 0) == rl.RL_EINVAL
    with pytest.raises(rl.EngineError):
        eng.hot_read()
    bad = rl.rl_hot_opts(hot_min=1)
    bad.struct_size = 8
    assert rl.lib.rl_hot_enable(eng.h, C.byref(bad)) == rl.RL_EINVAL
    for kw in (dict(hot_min=0), dict(hot_min=1, width=(1 << 24) + 1), dict(hot_min=1, key_slots=(1 << 24) + 1),
               dict(hot_min=1, weight=2)):
        assert rl.lib.rl_hot_enable(eng.h, C.byref(rl.rl_hot_opts(**kw))) == rl.RL_EINVAL, kw
    eng.hot_enable(3, width=100, key_slots=5)            # rounded up
    i = eng.hot_read().info
    assert (i.width, i.key_slots, i.hot_min, i.depth) == (128, 16, 3, 4)
    assert rl.lib.rl_hot_enable(eng.h, C.byref(rl.rl_hot_opts(hot_min=1))) == rl.RL_EINVAL     # a second enable
    eng.close()
    # the defaults
    eng = engine(rl, hot=(1,))
    i = eng.hot_read().info
    assert (i.width, i.key_slots) == (1 << 18, 65536)
    eng.close()


def test_config_registered_after_enable(rl):
    eng = engine(rl, hot=(1, 1 << 16, 4096))
    mod = H.HotModel(1 << 16, 1, H.NCFG)
    one_call(mod, eng, [1, 2, 2], [0, H.NCFG, H.NCFG], [1, 1, 1], [1, 1, 0])
    assert mod.skipped == 2
    assert eng.register(3, 2, NS) == H.NCFG
    mod.ncfg += 1
    one_call(mod, eng, [2, 2, 3], [H.NCFG, H.NCFG, H.NCFG + 1], [1, 1, 1], [1, 0, 1])
    assert (mod.skipped, mod.true) == (3, {1: 1, 2: 2})
    H.check_read(eng.hot_read(top=8), mod, "new config")
    eng.close()


# --- 7. behind real batches -------------------------------------------------------------

def test_behind_batches_in_flight(rl):
    """RL_OPT_PIPELINE, device API, one stream, no host sync: three batches of
    20,000 with a token-bucket key of 4500 requests in each (the chain), an
    rl_hot_batch_device behind each.  The read equals the model fed with the
    decisions that came back."""
    import torch
    N, size = 12, 20_000
    configs, (key, ts, n, cfg, _), sizes = many_config_trace(17, N, nbatch=3, m=size, hot=4500)
    cfg = cfg.copy()
    cfg[::211] = N + 1                               # unregistered: RL_INVALID, skipped
    eng = engine(rl, configs, flags=rl.OPT_PIPELINE, hot=(300, 1 << 12, 4096))
    dev = torch.device("cuda", 0)
    parts = [slice(b * size, (b + 1) * size) for b in range(3)]
    ins = [to_dev(key[s], ts[s], n[s], cfg[s]) for s in parts]
    outs = [[torch.full((size,), 9, dtype=torch.uint8, device=dev)] +
            [torch.empty(size, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(size, dtype=torch.float64, device=dev)] for _ in parts]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for i, o in zip(ins, outs):
        eng.decide_device(size, i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), None,
                          *[x.data_ptr() for x in o], stream)
        eng.hot_batch_device(size, i[0].data_ptr(), i[3].data_ptr(), i[2].data_ptr(), o[0].data_ptr(), stream)
    h = eng.hot_read(top=4096)
    torch.cuda.synchronize()
    assert eng.sync() == 0
    mod = H.HotModel(1 << 12, 300, N)
    for s, o in zip(parts, outs):
        dec = o[0].cpu().numpy()
        assert dec.max() <= 3 and (dec == 3).sum() >= size // 211      # every byte written: no 9 left
        mod.call(key[s], cfg[s], n[s], dec)
    ids, cnt = np.unique(key, return_counts=True)
    hot_key = int(ids[np.argmax(cnt)])
    # of the hot key's 13,500 requests about 1 % have n = 0 and 1 in 211 the unregistered config: RL_INVALID
    assert cnt.max() >= 3 * 4500 and 3 * 4500 * 0.95 < mod.true[hot_key] < 3 * 4500 and mod.skipped > 200
    assert fits(list(mod.candidates), 4096) and len(mod.candidates) >= 7
    H.check_read(h, mod, "in flight")
    assert int(h.keys["key_id"][0]) == hot_key
    eng.close()


# --- 8. the engine is untouched ---------------------------------------------------------

def test_engine_untouched(rl):
    """the same trace on an engine with the top keys on (a call behind every
    batch) and on one without: every decide output bit for bit, and rl_stats;
    the tally, enabled beside it, reads the same as alone"""
    from tracegen import random_trace
    configs = CONFIG_SETS["mixed"]
    key, ts, n, cfg, _ = random_trace(61, 9000, 300, configs, big_n=True)
    cfg = cfg.copy()
    cfg[::131] = len(configs) + 2
    a = engine(rl, configs, hot=(40, 1 << 10, 4096), tally=True)
    b = engine(rl, configs, tally=True)
    for lo in range(0, 9000, 3000):
        s = slice(lo, lo + 3000)
        ra = a.decide(key[s], ts[s], n[s], cfg[s], check=False)
        rb = b.decide(key[s], ts[s], n[s], cfg[s], check=False)
        before = bytes(a.stats())
        a.tally(key[s], cfg[s], n[s], ra.decision)
        b.tally(key[s], cfg[s], n[s], rb.decision)
        a.hot_batch(key[s], cfg[s], n[s], ra.decision)
        hot_dev(a, key[s], cfg[s], n[s], ra.decision)
        a.hot_read(top=10, clear=lo == 3000)
        assert bytes(a.stats()) == before
        assert ra.status == rb.status
        for f in ("decision", "remaining", "retry_after_ns", "reset_at_ns"):
            assert getattr(ra, f).tobytes() == getattr(rb, f).tobytes(), f
        tb = (cfg[s] < 5) & (ra.decision <= 1)
        assert tb.sum() > 500 and ra.tokens[tb].tobytes() == rb.tokens[tb].tobytes()
    sa, sb = a.stats(), b.stats()
    for f, _ in rl.rl_stats._fields_:
        if f != "stamp_cycles":
            va, vb = getattr(sa, f), getattr(sb, f)
            assert (list(va) == list(vb)) if hasattr(va, "__len__") else va == vb, f
    ta, tb_ = a.tally_read(top=400), b.tally_read(top=400)
    assert ta.cfg.tobytes() == tb_.cfg.tobytes() and ta.keys.tobytes() == tb_.keys.tobytes()
    assert bytes(ta.info) == bytes(tb_.info) and ta.keys_tracked == tb_.keys_tracked > 10
    assert a.hot_read().info.batches == 2          # cleared after the second slice: one slice, two calls
    assert a.sync() == b.sync() == 0
    a.close()
    b.close()
