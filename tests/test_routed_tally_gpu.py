"""The routed usage tally and top keys on the GPU: k_tally_routed
(csrc/rl_tally.h) and k_hot_add_routed / k_hot_pick_routed (csrc/rl_hot.h)
behind rl_tally_routed_device / rl_hot_routed_device (include/rl_route.h), and
shard.RoutedPipeline(observe=) with usage() / top_keys() end to end.  The routed
kernels are pinned to the array-form kernels (Engine.tally_device /
hot_batch_device, themselves pinned in tests/test_tally_gpu.py and
tests/test_hot_gpu.py) over the same requests in merge order, and both to the
reference models (tally_cases.expected_tally, hot_cases.HotModel).  DESIGN.md
§10o."""
import numpy as np
import pytest

import hot_cases
import tally_cases
from routed_tally_cases import DROPPED, code
from test_routed_ops_gpu import Rig, _dev, _fingerprint
from test_routed_refund_gpu import merge_order, shape_order
from tracegen import CONFIG_SETS, T0, many_configs, skewed_trace

pytestmark = pytest.mark.gpu
CONFIGS = CONFIG_SETS["mixed"]
KEY_RESERVED = (1 << 64) - 1
ALL = 1 << 16          # a `top` that returns every tracked key
WIDTH = 1 << 12


def counting_rig(rl, max_m, configs=CONFIGS, key_slots=4096, hot_min=8, weight=0, **kw):
    rig = Rig(rl, 0, max_m, configs=configs, **kw)
    rig.eng.tally_enable(key_slots)
    rig.eng.hot_enable(hot_min, width=WIDTH, key_slots=4096, weight=weight)
    return rig


def array_engine(rl, configs=CONFIGS, key_slots=4096, hot_min=8, weight=0):
    """engine B: only its array-form tally and top keys are used"""
    eng = rl.Engine(profile=0, tb_capacity=1 << 10, win_capacity=1 << 10, max_batch=2048)
    for a, L, W in configs:
        eng.register(a, L, W)
    eng.tally_enable(key_slots)
    eng.hot_enable(hot_min, width=WIDTH, key_slots=4096, weight=weight)
    return eng


def set_decisions(rig, dec):
    """the step's result records as the test wants them: at world 1 a request's
    receive index is its position in the batch (one owner, batch order)"""
    rig.res.zero_()
    if len(dec):
        rig.res[:len(dec), 0] = rig.torch.from_numpy(np.asarray(dec, np.int64)).cuda()


def count_routed(rig, m_max=None, info=True, tally=True, hot=True):
    a = rig.args(m_max)[:6]
    if tally:
        rig.eng.tally_routed(*a, rig.info.data_ptr() if info else None, 1, rig.s)
    if hot:
        rig.eng.hot_routed(*a, stream=rig.s)


def count_arrays(eng, torch, key, cfg, n, dec, tally=True, hot=True):
    d = [_dev(torch, x) for x in (key, cfg, n, code(dec))]
    p = [t.data_ptr() for t in d]
    if tally:
        eng.tally_device(key.size, *p)
    if hot:
        eng.hot_batch_device(key.size, *p)
    torch.cuda.synchronize()


def same_reads(a, b, what, clear=True):
    """engine a's routed counts against engine b's array counts: every config
    row, every key record (as sets), every device-counted info word, every
    candidate and estimate -> (tally, hot) of a"""
    ta, tb = a.tally_read(top=ALL), b.tally_read(top=ALL, clear=clear)
    assert np.array_equal(ta.cfg["count"], tb.cfg["count"]) and np.array_equal(ta.cfg["units"], tb.cfg["units"]), what
    rows = lambda t: {(int(r["key_id"]), int(r["denied"]), int(r["units_denied"])) for r in t.keys}
    assert rows(ta) == rows(tb), what
    for f in ("keys_tracked", "untracked_requests", "untracked_units", "unknown_cfg", "bad_codes"):
        assert getattr(ta.info, f) == getattr(tb.info, f), (what, f)
    ha, hb = a.hot_read(top=ALL), b.hot_read(top=ALL, clear=clear)
    assert [(int(r["key_id"]), int(r["estimate"])) for r in ha.keys] == \
        [(int(r["key_id"]), int(r["estimate"])) for r in hb.keys], what
    for f in ("keys_tracked", "dropped", "total", "skipped"):
        assert getattr(ha.info, f) == getattr(hb.info, f), (what, f)
    if clear:
        a.tally_read(clear=True)
        a.hot_read(clear=True)
    return ta, ha


def check_models(t, h, calls, ncfg, hot_min, weight, what):
    """the reads against the reference models of the calls [(key, cfg, n, decision)]"""
    cat = [np.concatenate([c[f] for c in calls]) for f in range(4)]
    e = tally_cases.expected_tally(cat[0], cat[1], cat[2], code(cat[3]), ncfg)
    assert np.array_equal(t.cfg["count"], e.count) and np.array_equal(t.cfg["units"], e.units), what
    assert (t.info.unknown_cfg, t.info.bad_codes) == (e.unknown_cfg, e.bad_codes), what
    assert (t.info.untracked_requests, t.info.untracked_units) == tuple(e.reserved), what
    assert {int(r["key_id"]): (int(r["denied"]), int(r["units_denied"])) for r in t.keys} == \
        {k: (v[0], v[1]) for k, v in e.keys.items()}, what
    mod = hot_cases.HotModel(WIDTH, hot_min, ncfg, weight)
    for key, cfg, n, dec in calls:
        mod.call(key, cfg, n, code(dec))
    assert [(int(r["key_id"]), int(r["estimate"])) for r in h.keys] == mod.read(), what
    assert (h.info.total, h.info.skipped, h.info.dropped) == (mod.total, mod.skipped, 0), what
    for r in h.keys:
        assert int(r["estimate"]) >= mod.true[int(r["key_id"])], what       # never below the true weight
    return e, mod


# --- 1. the routed kernels against the array-form kernels ---------------------------------

@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_routed_equals_array_form(rl, in_order):
    """engine A routes a batch, decides it and counts the step; engine B counts
    the same requests as arrays in merge order with the decisions A returned:
    equal reads, equal to the models, at counts around the wave, the block and
    one merge tile, in both forms of the merge"""
    rig = counting_rig(rl, 4096)
    b = array_engine(rl)
    ncfg = len(CONFIGS)
    steps = requests = 0
    seen = set()
    for c in (0, 1, 63, 64, 65, 255, 257, 2049):
        key, ts, n, cfg, _ = skewed_trace(300 + c, max(c, 1), 30, CONFIGS)
        key, ts, n, cfg = (x[:c] for x in (key, ts, n, cfg))
        cfg = cfg.copy()
        cfg[5::41] = 99
        key, ts, n, cfg = shape_order(key, ts, n, cfg, in_order)
        rig.route(key, ts, n, cfg)
        rig.eng.decide_routed(*rig.args())
        count_routed(rig)
        dec = rig.results()[0]
        if c > 1:
            assert rig.identity_form() == in_order
        o = merge_order(ts)
        call = (key[o], cfg[o], n[o], dec[o].astype(np.int64))
        count_arrays(b, rig.torch, *call)
        steps, requests = steps + 1, requests + c
        ri = rig.eng.tally_routed_read()
        assert (ri.steps, ri.requests, ri.dropped_requests) == (1, c, 0)
        t, h = same_reads(rig.eng, b, f"count {c}")
        check_models(t, h, [call], ncfg, 8, 0, f"count {c}")
        assert t.routed.steps == 1 and t.routed.requests == c
        assert (t.info.batches, t.info.requests, h.info.batches, h.info.requests) == (0, 0, 0, 0)   # array calls only
        seen |= set(dec.tolist())
        ri = rig.eng.tally_routed_read()
        assert (ri.steps, ri.requests, ri.dropped_requests) == (0, 0, 0)                # the clearing read
    assert seen >= {0, 1, 3}
    assert rig.eng.sync() == rl.RL_OK
    b.close()
    rig.close()


# --- 2. contention and the LDS edges -------------------------------------------------------

def test_routed_tally_contention_and_lds_edges(rl):
    """one key holds a third of 5000 requests, denied after its first few; 300
    distinct denied keys (above TALLY_LDS_KEYS); 40 registered configs, so
    config ids straddle TALLY_LDS_CFGS = 32"""
    configs = many_configs(3, 40)
    rng = np.random.default_rng(3)
    m = 5000
    key = (rng.integers(0, 300, m) + 1000).astype(np.uint64)
    key[rng.random(m) < 1 / 3] = 7
    key[:300] = np.arange(300, dtype=np.uint64) + 1000
    cfg = (key % np.uint64(40)).astype(np.uint32)
    n = rng.choice([1, 2, 5], m).astype(np.int64)
    dec = rng.choice([0, 0, 1, 2, 3], m).astype(np.int64)
    dec[:300] = 0
    hot = np.nonzero(key == 7)[0]
    dec[hot[:4]], dec[hot[4:]] = 1, 0
    ts = T0 + np.arange(m, dtype=np.int64)
    assert hot.size > 1500 and tally_cases.LDS_CFGS == 32 and np.unique(key[dec == 0]).size == 301
    for in_order in (True, False):
        rig = counting_rig(rl, 8192, configs=configs)
        b = array_engine(rl, configs=configs)
        k2, t2, n2, c2 = shape_order(key, ts, n, cfg, in_order)
        rig.route(k2, t2, n2, c2)
        set_decisions(rig, dec)
        count_routed(rig)
        o = merge_order(t2)
        call = (k2[o], c2[o], n2[o], dec[o])
        count_arrays(b, rig.torch, *call)
        t, h = same_reads(rig.eng, b, f"in order {in_order}")
        e, _ = check_models(t, h, [call], 40, 8, 0, f"in order {in_order}")
        assert e.keys[7][0] == hot.size - 4 and (e.count[32:, 0] > 0).any() and (e.count[:32, 0] > 0).any()
        assert int(t.keys[0]["key_id"]) == 7
        assert rig.eng.sync() == rl.RL_OK
        b.close()
        rig.close()


@pytest.mark.parametrize("weight", [hot_cases.REQUESTS, hot_cases.UNITS])
def test_routed_hot_zipf(rl, weight):
    """hot_cases.zipf_calls (5000, 5037, 5074 requests, none a multiple of the
    wave or the block), both weights, steps alternating between the two forms
    of the merge: the array form's and the model's candidates and estimates,
    none below the true weight"""
    calls = hot_cases.zipf_calls()
    rig = counting_rig(rl, 8192, configs=CONFIGS[:hot_cases.NCFG], hot_min=hot_cases.ZIPF_HOT_MIN, weight=weight)
    b = array_engine(rl, configs=CONFIGS[:hot_cases.NCFG], hot_min=hot_cases.ZIPF_HOT_MIN, weight=weight)
    done = []
    for j, (key, cfg, n, dec) in enumerate(calls):
        ts = T0 + np.arange(key.size, dtype=np.int64)
        k2, t2, n2, c2 = shape_order(key, ts, n, cfg, j % 2 == 0)
        rig.route(k2, t2, n2, c2)
        set_decisions(rig, dec)
        count_routed(rig)
        o = merge_order(t2)
        done.append((k2[o], c2[o], n2[o], dec[o].astype(np.int64)))
        count_arrays(b, rig.torch, *done[-1])
    t, h = same_reads(rig.eng, b, f"weight {weight}")
    _, mod = check_models(t, h, done, hot_cases.NCFG, hot_cases.ZIPF_HOT_MIN, weight, f"weight {weight}")
    assert len(mod.candidates) >= 3 and mod.skipped > 0
    assert rig.eng.sync() == rl.RL_OK
    b.close()
    rig.close()


# --- 3. the grid stride -----------------------------------------------------------------

def test_routed_counts_grid_stride(rl):
    """1024 * 256 + 777 requests: every block strides to a second round, the
    last round partly filled"""
    m = rl.TALLY_GRID_CAP + 777
    assert m == 1024 * 256 + 777 and rl.HOT_GRID_CAP == rl.TALLY_GRID_CAP
    rng = np.random.default_rng(5)
    key = rng.integers(0, 5000, m).astype(np.uint64)
    key[rng.random(m) < 0.2] = 11
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    n = rng.choice([1, 2, 5], m).astype(np.int64)
    dec = rng.choice([0, 1, 1, 2, 3], m).astype(np.int64)
    ts = T0 + np.arange(m, dtype=np.int64)
    rig = counting_rig(rl, m, key_slots=1 << 14, hot_min=200, max_batch=8192)
    b = array_engine(rl, key_slots=1 << 14, hot_min=200)
    for in_order in (True, False):
        k2, t2, n2, c2 = shape_order(key, ts, n, cfg, in_order)
        rig.route(k2, t2, n2, c2)
        set_decisions(rig, dec)
        count_routed(rig)
        o = merge_order(t2)
        call = (k2[o], c2[o], n2[o], dec[o])
        count_arrays(b, rig.torch, *call)
        assert rig.eng.tally_routed_read().requests == m
        t, h = same_reads(rig.eng, b, f"stride, in order {in_order}")
        check_models(t, h, [call], len(CONFIGS), 200, 0, f"stride, in order {in_order}")
    assert rig.eng.sync() == rl.RL_OK
    b.close()
    rig.close()


# --- 4. a count above m_max ---------------------------------------------------------------

@pytest.mark.parametrize("in_order", [True, False], ids=["identity", "order"])
def test_routed_count_above_m_max(rl, in_order):
    """*count = m_max + 37: only the first m_max requests in merge order -- the
    ones the engine gave results -- are counted"""
    rng = np.random.default_rng(9)
    m, m_max = 300, 263
    key = rng.integers(0, 40, m).astype(np.uint64)
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    n = rng.choice([1, 2, 5], m).astype(np.int64)
    dec = rng.choice([0, 0, 1, 2, 3], m).astype(np.int64)
    ts = T0 + rng.permutation(m).astype(np.int64) * 1000
    key, ts, n, cfg = shape_order(key, ts, n, cfg, in_order)
    rig = counting_rig(rl, 2048, hot_min=2)
    rig.route(key, ts, n, cfg)
    set_decisions(rig, dec)
    count_routed(rig, m_max=m_max)
    o = merge_order(ts)[:m_max]
    t, h = rig.eng.tally_read(top=ALL), rig.eng.hot_read(top=ALL)
    check_models(t, h, [(key[o], cfg[o], n[o], dec[o])], len(CONFIGS), 2, 0, "the first m_max")
    assert t.routed.requests == m_max and t.routed.steps == 1
    assert rig.identity_form() == in_order
    assert rig.eng.sync() in (rl.RL_OK, rl.RL_EOVERFLOW)       # the flag a decide of this step would have raised
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 5. the key table overflows -------------------------------------------------------------

def test_routed_tally_key_table_overflow(rl):
    """key_slots = 16 against 200 denied keys: a key is tracked completely or
    not at all, and the untracked sums make up the rest"""
    rng = np.random.default_rng(13)
    m = 3000
    key = (rng.integers(0, 200, m) + 50).astype(np.uint64)
    key[:200] = np.arange(200, dtype=np.uint64) + 50
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    n = rng.choice([1, 2, 5], m).astype(np.int64)
    dec = rng.choice([0, 0, 1], m).astype(np.int64)
    dec[:200] = 0
    ts = T0 + np.arange(m, dtype=np.int64)
    e = tally_cases.expected_tally(key, cfg, n, code(dec), len(CONFIGS))
    assert len(e.keys) == 200
    for in_order in (True, False):
        rig = counting_rig(rl, 4096, key_slots=16)
        k2, t2, n2, c2 = shape_order(key, ts, n, cfg, in_order)
        rig.route(k2, t2, n2, c2)
        set_decisions(rig, dec)
        count_routed(rig, hot=False)
        t = rig.eng.tally_read(top=ALL)
        assert np.array_equal(t.cfg["count"], e.count) and np.array_equal(t.cfg["units"], e.units)
        assert t.info.key_slots == 16 and 0 < t.keys_tracked <= 16 and t.keys.size == t.keys_tracked
        for r in t.keys:
            assert (int(r["denied"]), int(r["units_denied"])) == tuple(e.keys[int(r["key_id"])][:2])
        assert int(t.keys["denied"].sum()) + t.info.untracked_requests == e.denied
        assert (int(t.keys["units_denied"].sum()) + t.info.untracked_units) & ((1 << 64) - 1) == e.units_denied
        assert rig.eng.sync() == rl.RL_OK
        rig.close()


# --- 6. classes -------------------------------------------------------------------------

def test_routed_classes(rl):
    """unknown cfg 99 adds to unknown_cfg; the reserved key is decided -- and so
    counted -- as RL_INVALID; a decision of 7 or -1 adds to bad_codes / skipped
    and nothing else"""
    key, ts, n, cfg, _ = skewed_trace(77, 1500, 40, CONFIGS)
    cfg, key = cfg.copy(), key.copy()
    cfg[3::50] = 99
    key[7::60] = np.uint64(KEY_RESERVED)
    key, ts, n, cfg = shape_order(key, ts, n, cfg, True)
    rig = counting_rig(rl, 2048)
    rig.route(key, ts, n, cfg)
    rig.eng.decide_routed(*rig.args())
    dec = rig.results()[0].astype(np.int64)
    assert (dec[key == np.uint64(KEY_RESERVED)] == 3).all()
    bad = np.nonzero((cfg != 99) & (key != np.uint64(KEY_RESERVED)))[0][10:30]
    dec[bad[::2]], dec[bad[1::2]] = 7, -1
    res = rig.res.cpu().numpy()
    res[bad[::2], 0], res[bad[1::2], 0] = 7, -1          # receive index = batch position at world 1
    rig.res.copy_(rig.torch.from_numpy(res))
    count_routed(rig)
    t, h = rig.eng.tally_read(top=ALL), rig.eng.hot_read(top=ALL)
    e, mod = check_models(t, h, [(key, cfg, n, dec)], len(CONFIGS), 8, 0, "classes")
    assert t.info.unknown_cfg == int((cfg == 99).sum()) > 0 and t.info.bad_codes == 20
    assert int(e.count[:, 3].sum()) >= int((key == np.uint64(KEY_RESERVED)).sum()) > 0
    assert int(t.cfg["count"].sum()) == key.size - t.info.unknown_cfg - 20
    assert h.info.skipped == mod.skipped >= t.info.unknown_cfg + 20
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 7. drops ---------------------------------------------------------------------------

def test_routed_tally_counts_sender_drops(rl):
    """a bucket of 2048 records against 2100 requests: dropped_requests equals
    the number of RL_SLOT_DROPPED slots; with recv_info NULL it stays 0"""
    import torch
    m = 2100
    r = rl.Router(0, 1, m, 2048)
    cap = r.capacity
    assert cap == 2048
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=cap)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    eng.tally_enable(1024)
    rng = np.random.default_rng(2)
    key = rng.integers(0, 50, m).astype(np.uint64)
    cfg = (key % np.uint64(len(CONFIGS))).astype(np.uint32)
    n = np.ones(m, np.int64)
    ts = T0 + np.arange(m, dtype=np.int64)
    ins = [_dev(torch, x) for x in (key, ts, n, cfg)]
    p = lambda t: t.data_ptr()
    send = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
    info = torch.zeros((1, 4), dtype=torch.int64, device="cuda")
    slot = torch.zeros(m, dtype=torch.int32, device="cuda")
    order = torch.zeros(cap, dtype=torch.int32, device="cuda")
    sms = torch.zeros(cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    r.pack(m, *[p(t) for t in ins], p(send), p(info), p(slot), s)
    r.merge(p(send), p(info), p(order), p(sms), p(cnt), s)
    eng.decide_routed(cap, p(cnt), p(send), p(order), p(sms), p(res), s, s)
    eng.tally_routed(cap, p(cnt), p(send), p(order), p(sms), p(res), None, 1, s)
    torch.cuda.synchronize()
    dropped = int((slot.cpu().numpy() == -1).sum())            # RL_SLOT_DROPPED as int32
    assert dropped == m - cap
    ri = eng.tally_routed_read()
    assert (ri.steps, ri.requests, ri.dropped_requests) == (1, cap, 0)
    eng.tally_routed(cap, p(cnt), p(send), p(order), p(sms), p(res), p(info), 1, s)
    ri = eng.tally_routed_read()
    assert (ri.steps, ri.requests, ri.dropped_requests) == (2, 2 * cap, dropped)
    t = eng.tally_read(top=ALL, clear=True)
    assert int(t.cfg["count"].sum()) == 2 * cap and t.routed.dropped_requests == dropped
    assert eng.tally_routed_read().dropped_requests == 0
    assert r.sync(None) == rl.RL_EOVERFLOW and eng.sync() == rl.RL_OK
    eng.close()
    r.close()


# --- 8. nothing else moves ------------------------------------------------------------------

def test_routed_counts_change_nothing_else(rl):
    """recv and res are byte-identical afterwards; the table fingerprint,
    rl_stats and the sticky status are what they were"""
    key, ts, n, cfg, _ = skewed_trace(91, 3000, 100, CONFIGS)
    rig = counting_rig(rl, 4096)
    rig.route(key, ts, n, cfg)
    rig.eng.decide_routed(*rig.args())
    rig.results()
    assert rig.eng.sync() == rl.RL_OK
    now_ms = int(ts.max()) // 1_000_000
    before = _fingerprint(rl, rig.eng, now_ms)
    bufs = lambda: [x.cpu().numpy().tobytes() for x in (rig.send, rig.res, rig.order, rig.sms, rig.cnt, rig.info)]
    b0 = bufs()
    for _ in range(2):
        count_routed(rig)
    rig.torch.cuda.synchronize()
    assert bufs() == b0
    assert rig.eng.sync() == rl.RL_OK
    assert _fingerprint(rl, rig.eng, now_ms) == before
    assert rig.eng.tally_routed_read().steps == 2 and rig.eng.tally_read().info.batches == 0
    assert _fingerprint(rl, rig.eng, now_ms) == before
    rig.close()


def test_routed_count_arguments(rl):
    """RL_EINVAL before the feature is enabled and for a null array with m_max >
    0; m_max = 0 is a no-op; recv_info may be null"""
    rig = Rig(rl, 0, 2048)
    p = lambda t: t.data_ptr()
    good = [rig.eng.h, 16, p(rig.cnt), p(rig.send), p(rig.order), p(rig.sms), p(rig.res)]
    t, h = rl.lib.rl_tally_routed_device, rl.lib.rl_hot_routed_device
    assert t(*good, p(rig.info), 1, None) == rl.RL_EINVAL and h(*good, None) == rl.RL_EINVAL
    assert t(rig.eng.h, 0, None, None, None, None, None, None, 0, None) == rl.RL_EINVAL       # not enabled
    info = rl.rl_tally_routed_info()
    assert rl.lib.rl_tally_routed_read(rig.eng.h, info) == rl.RL_EINVAL
    rig.eng.tally_enable(64)
    rig.eng.hot_enable(4, width=64, key_slots=64)
    for k in (2, 3, 4, 5, 6):
        bad = list(good)
        bad[k] = None
        assert t(*bad, p(rig.info), 1, None) == rl.RL_EINVAL and h(*bad, None) == rl.RL_EINVAL
    assert t(*(good[:1] + [1 << 32] + good[2:]), None, 0, None) == rl.RL_EINVAL
    assert t(rig.eng.h, 0, None, None, None, None, None, None, 0, None) == rl.RL_OK
    assert h(rig.eng.h, 0, None, None, None, None, None, None) == rl.RL_OK
    assert rig.eng.tally_routed_read().steps == 0
    assert t(*good, None, 0, None) == rl.RL_OK and h(*good, None) == rl.RL_OK        # a zero count
    ri = rig.eng.tally_routed_read()
    assert (ri.steps, ri.requests, ri.dropped_requests) == (1, 0, 0)
    assert rig.eng.sync() == rl.RL_OK
    rig.close()


# --- 9. the pipeline end to end -----------------------------------------------------------

HOT_ARGS = (WIDTH, 15, len(CONFIGS), 0)


def _pipeline_rank(rank, world, backend="nccl", exchange=None, m=3000):
    """one rank (routed_refund_cases.run_ranks) on cuda:0: the steps D P D R P D
    P through a pipeline without observe= and, on a fresh engine, through one
    with the tally and the top keys -> (ok, info)"""
    import torch
    import torch.distributed as dist

    import rl_amd
    import routed_op_cases as rc
    import routed_tally_cases as tc
    import shard
    torch.cuda.set_device(0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    pg_res = dist.new_group(backend=backend)
    in_place = not exchange and world == 1
    mine = rc.rank_batches(rank, CONFIGS, m=m, reset_n_none=in_place, peeks_in_order=in_place)
    ins = [tuple(None if x is None else _dev(torch, x) for x in bt) for bt in mine]
    info, decisions = {}, []
    for observed in (False, True):
        router = rl_amd.Router(0, world, m, m)
        eng = rl_amd.Engine(profile=0, tb_capacity=1 << 16, win_capacity=1 << 16, max_batch=world * router.capacity)
        for a, L, W in CONFIGS:
            eng.register(a, L, W)
        kw = {}
        if observed:
            eng.tally_enable(4096)
            eng.hot_enable(HOT_ARGS[1], width=WIDTH, key_slots=4096)
            kw = dict(observe=[eng.tally_routed, eng.hot_routed])
        pipe = shard.RoutedPipeline(router, eng.decide_routed, world, m, "cuda:0", pg_req=None, pg_res=pg_res,
                                    exchange=exchange, staged=backend == "gloo", decide_ev=eng.decide_routed_ev,
                                    peek=eng.peek_routed, peek_ev=eng.peek_routed_ev, reset=eng.reset_routed,
                                    reset_ev=eng.reset_routed_ev, **kw)
        outs = [(torch.empty(m, dtype=torch.uint8, device="cuda"),) +
                tuple(torch.empty(m, dtype=torch.int64, device="cuda") for _ in range(3)) for _ in mine]
        torch.cuda.synchronize()
        pipe.run(ins, outs, kinds=rc.KINDS)
        if observed:
            usage = pipe.usage(eng.tally_read, top=20)
            top = pipe.top_keys(eng.hot_read, top=20)
            info["local_steps"] = int(eng.tally_routed_read().steps)
            info["batches"] = int(eng.stats().batches)
        torch.cuda.synchronize()
        info["status"] = (eng.sync(), router.sync(None))
        decisions.append([[x.cpu().numpy().tobytes() for x in o] for o in outs])
        dec = [o[0].cpu().numpy() for o in outs]
        del pipe
        eng.close()
        router.close()
    info["identical"] = decisions[0] == decisions[1]
    # the model over the union: every rank's executed decide requests with the
    # decisions they were given, counted on their owners step by step
    every = [None] * world
    dist.all_gather_object(every, [(bt[0], bt[3], bt[2], d) for bt, d in zip(mine, dec)], group=pg_res)
    steps = [b for b, k in enumerate(rc.KINDS) if k == rc.D]
    calls = [[] for _ in range(world)]
    dropped = 0
    for b in steps:
        cat = [np.concatenate([every[r][b][f] for r in range(world)]) for f in range(4)]
        live = cat[3] != DROPPED
        dropped += int((~live).sum())
        own = shard.owner_of(cat[0], world)
        for w in range(world):
            sel = live & (own == w)
            calls[w].append((cat[0][sel], cat[1][sel], cat[2][sel], cat[3][sel].astype(np.int64)))
    allc = [c for w in range(world) for c in calls[w]]
    e = tally_cases.expected_tally(*[np.concatenate([c[f] for c in allc]) for f in range(3)],
                                   code(np.concatenate([c[3] for c in allc])), len(CONFIGS))
    mods = []
    for w in range(world):
        mod = hot_cases.HotModel(*HOT_ARGS)
        for c in calls[w]:
            mod.call(c[0], c[1], c[2], code(c[3]))
        mods.append(mod)
    routed = dict(steps=len(steps) * world, requests=sum(c[0].size for c in allc), dropped_requests=dropped)
    tc.check_usage(usage, e, routed, 20, f"rank {rank}")
    tc.check_top_keys(top, mods, 20, f"rank {rank}")
    info["denied_keys"], info["hot_keys"] = len(e.keys), sum(len(mod.candidates) for mod in mods)
    info["steps"] = len(steps)
    ok = info["identical"] and info["status"] == (0, 0) and info["local_steps"] == len(steps) and \
        info["batches"] == len(steps) and info["denied_keys"] > 20 and info["hot_keys"] > 0
    return ok, info


def _spawn(world, backend, **kw):
    import routed_refund_cases as rf
    return rf.run_ranks(__name__, "_pipeline_rank", world, limit=240, backend=backend, **kw)


def _check(res, world):
    for r in range(world):
        ok, info = res[r]
        assert ok, (r, info)


def test_pipeline_one_rank_in_place():
    """world 1 without the exchange: the kernels read the send buckets and the
    results in place (the RL_ORDER_IDENTITY form where a step's ts are in order)"""
    _check(_spawn(1, "nccl"), 1)


def test_pipeline_one_rank_rccl():
    """world 1 over the RCCL loopback: the counts run behind the result
    all-to-all and the unpack on U; the reads gather over the group"""
    _check(_spawn(1, "nccl", exchange=True), 1)


def test_pipeline_two_ranks_one_gpu():
    """two ranks (two engines, two routers) on the one GPU, collectives through
    host memory (gloo): merged orders of two sources, every key counted on its
    owner, both ranks read the same cluster-wide answer"""
    _check(_spawn(2, "gloo"), 2)
