"""Charge (rl_charge_batch) on the GPU, bit-exact against the composition on
the Python oracle (charge_cases.apply_charge) on both profiles: every output
field (`tokens` as bit patterns), Peek (n = 0) of every key, the stored values
themselves (a snapshot of the engine against the oracle's db) and the decisions
of the trace that follows."""
import ctypes as C

import numpy as np
import pytest

from charge_cases import KINDS, apply_charge, charge_case
from oracle import rl_oracle_py as po
from refund_cases import py_peek, warm
from reset_cases import KEY_RESERVED
from test_refund_gpu import Rig as RefundRig
from test_refund_gpu import assert_rows, engine_state
from tracegen import NS, T0

pytestmark = pytest.mark.gpu


def assert_charges(res, rows, what=""):
    """an engine result against apply_charge's rows: every field of every row,
    tokens as bit patterns"""
    want = [np.array([r[j] for r in rows], dt) for j, dt in enumerate((np.uint8, np.int64, np.int64, np.int64,
                                                                      np.float64))]
    got = (res.decision, res.charged, res.remaining, res.reset_at_ns, res.tokens)
    for name, g, w in zip(("decision", "charged", "remaining", "reset_at_ns", "tokens"), got, want):
        if g is None:
            continue
        g, w = (g.view(np.uint64), w.view(np.uint64)) if name == "tokens" else (g, w)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what} {name} at {bad[:10]}: gpu={g[bad[:10]]} ref={w[bad[:10]]}"


class Rig(RefundRig):
    """an engine and the Python oracle, fed the same decides and Charge calls"""

    def charge(self, key, ts, n, cfg, sms=None, what="", status=0, want_tokens=True):
        """one host call: every output field, the counters of a decide batch
        -> (result, (rows, info))"""
        st0 = self.eng.stats()
        res = self.eng.charge(key, ts, n, cfg, sms, want_tokens=want_tokens, check=False)
        assert res.status == status, self.eng.last_error()
        st1 = self.eng.stats()
        assert (st1.batches - st0.batches, st1.decisions - st0.decisions) == (1, len(key))
        assert self.eng.sync() == 0
        want = apply_charge(self.sim, np.asarray(key, np.uint64), ts, n, cfg, sms)
        assert_charges(res, want[0], what)
        return res, want


# --- parity: seeded cases, every algorithm ----------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(rl, kind, profile):
    """charge_cases.charge_case: decide the warm-up, one Charge call, Peek
    every key with n = 0, the stored state, the trace that follows"""
    configs, first_trace, (key, ts, n, cfg, sms), second, now_ms, cover = charge_case(kind, profile)
    r = Rig(rl, profile, configs)
    r.decide(first_trace, "warm-up")
    res, (rows, info) = r.charge(key, ts, n, cfg, sms, "call")
    cls = info["cls"]
    assert (cls == "full").sum() >= 20 and info["fresh"] and info["expired"]
    if kind in ("tb", "mixed"):
        assert min((cls == c).sum() for c in ("short", "empty")) >= 20 and (cls == "dup_denied").any()
    if kind != "tb":
        assert (cls == "over").sum() >= 20 and (cls == "error").any()
    r.check_state(now_ms, "after the call")
    r.check_keys(now_ms, "after the call")
    pk = np.array(sorted({int(k) for k in key.tolist() if k != np.uint64(KEY_RESERVED)} |
                         {int(k) for k in first_trace[0].tolist()}), np.uint64)
    pc = (pk % np.uint64(len(configs))).astype(np.uint32)
    t_end = int(ts[-1])
    got = r.eng.peek(pk, np.full(pk.size, t_end), np.zeros(pk.size, np.int64), pc, np.full(pk.size, now_ms))
    assert_rows(got, [py_peek(r.sim, int(k), t_end, int(c), now_ms) for k, c in zip(pk, pc)], "peek")
    r.decide(second, "the trace that follows")
    end_ms = int(second[4][-1]) if second[4] is not None else int(second[1][-1]) // 1_000_000
    r.check_keys(end_ms, "after")
    r.check_state(end_ms, "after")
    r.close()


# --- kernel shapes ----------------------------------------------------------------

SHAPE_CONFIGS = [(1, 10, 3600 * NS), (3, 5, 3600 * NS), (2, 8, 3600 * NS), (1, 3, 3600 * NS)]


def shape_call(m, t, seed):
    """m requests over about m / 3 keys of a bucket of 10, a fixed window of
    5, a sliding window of 8 and a bucket of 3: full and short charges,
    duplicates that are denied, windows pushed over, a few invalid requests"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, max(m // 3, 4), m).astype(np.uint64)
    cfg = (key % np.uint64(4)).astype(np.uint32)
    n = rng.choice([1, 2, 4, 7, 20], m).astype(np.int64)
    if m > 8:
        n[rng.integers(0, m, m // 50 + 1)] = 0
        key[rng.integers(0, m, m // 50 + 1)] = np.uint64(KEY_RESERVED)
    return key, t + np.arange(m, dtype=np.int64) * 1000, n, cfg


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4096, 4097])
def test_sizes(rl, m):
    """one lane, the wave's edge, and both sides of the size up to which the
    decide runs as one workgroup; a second call finds the buckets the first one
    emptied"""
    r = Rig(rl, 0, SHAPE_CONFIGS)
    seen = set()
    for j in range(3 if m == 1 else 2):
        key, ts, n, cfg = shape_call(m, T0 + j * NS, 20 + j)
        if m == 1:
            key, cfg, n = np.array([4], np.uint64), np.array([0], np.uint32), np.array([7], np.int64)
        res, (rows, info) = r.charge(key, ts, n, cfg, what=f"M = {m}, call {j}")
        seen |= set(info["cls"].tolist())
        r.check_state(0, f"M = {m}, call {j}")
    if m == 1:
        assert seen == {"full", "short", "empty"}          # 7 of 10, 3 of 3, none of 0
    else:
        assert {"full", "short", "empty", "dup_denied", "over", "invalid"} <= seen
    r.close()


def test_grid_stride(rl):
    """M = grid cap + 4096 + 37: the grid-stride loops of both kernels run twice"""
    cap = rl.CHARGE_GRID_CAP
    assert cap == 1024 * 256
    m = cap + 4096 + 37
    r = Rig(rl, 0, SHAPE_CONFIGS, tb=1 << 18, win=1 << 18, max_batch=1 << 19)
    assert r.eng.charge_max() == 1 << 19
    key, ts, n, cfg = shape_call(m, T0, 9)
    res, (rows, info) = r.charge(key, ts, n, cfg, what="stride")
    cls = info["cls"]
    for c in ("full", "short", "dup_denied", "over", "invalid"):
        assert (cls[cap:] == c).any() and (cls[:cap] == c).any(), c
    r.check_state(0, "stride")
    r.close()


# --- order in flight --------------------------------------------------------------

def test_order_in_flight(rl):
    """RL_OPT_PIPELINE, device API, no host sync between the calls: decide,
    Charge, Charge from a second stream, decide"""
    import torch
    configs, first_trace, (key, ts, n, cfg, sms), second, now_ms, _ = charge_case("mixed", 0)
    # the second call: the same requests behind the first one on both clocks
    span = int(ts[-1]) - int(ts[0]) + 1000
    span_ms = int(sms[-1]) - int(sms[0]) + 1
    shift = 2 * span + 2 * span_ms * 1_000_000
    second = (second[0], second[1] + shift, second[2], second[3], None)
    r = Rig(rl, 0, configs, flags=rl.OPT_PIPELINE)
    dev = torch.device("cuda", 0)

    def dev_in(*arrs):
        return [None if x is None else
                torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                                 np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                                 np.ascontiguousarray(x)).to(dev) for x in arrs]

    def dev_out(m):
        return ([torch.empty(m, dtype=torch.uint8, device=dev)] +
                [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
                [torch.empty(m, dtype=torch.float64, device=dev)])

    p = lambda t: None if t is None else t.data_ptr()
    D = [first_trace, second]
    d_in = [dev_in(*d) for d in D]
    d_out = [dev_out(d[0].size) for d in D]
    calls = [(key, ts, n, cfg, sms), (key, ts + span, n, cfg, sms + span_ms)]
    a_in = [dev_in(*c) for c in calls]
    a_out = [dev_out(key.size) for _ in calls]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()

    def decide(j, s):
        r.eng.decide_device(D[j][0].size, *[p(x) for x in d_in[j]], *[p(x) for x in d_out[j]], s.cuda_stream)

    def charge(j, s):
        r.eng.charge_device(key.size, *[p(x) for x in a_in[j]], *[p(x) for x in a_out[j]], s.cuda_stream)

    decide(0, streams[0])
    charge(0, streams[0])
    charge(1, streams[1])
    decide(1, streams[0])
    torch.cuda.synchronize()
    assert r.eng.sync() == 0, r.eng.last_error()
    st = r.eng.stats()
    assert (st.batches, st.decisions) == (4, D[0][0].size + D[1][0].size + 2 * key.size)
    assert_rows(rl.Decisions(*[x.cpu().numpy() for x in d_out[0]]), warm(r.sim, D[0]), "decide 0")
    for j, c in enumerate(calls):
        rows, info = apply_charge(r.sim, *c)
        assert_charges(rl.Charges(*[x.cpu().numpy() for x in a_out[j]]), rows, f"call {j}")
        assert (info["cls"] == "short").sum() >= 20
    assert_rows(rl.Decisions(*[x.cpu().numpy() for x in d_out[1]]), warm(r.sim, D[1]), "decide 1")
    r.check_state(int(second[1][-1]) // 1_000_000)
    r.close()


# --- limits -----------------------------------------------------------------------

def test_limits(rl):
    """m = 0, null arrays, m = rl_charge_max + 1, exactly the maximum, nullable tokens"""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, max_batch=1 << 12)
    h = r.eng.h
    assert r.eng.charge_max() == 1 << 12
    keys = np.arange(50, dtype=np.uint64)
    cfg = (keys % np.uint64(2)).astype(np.uint32)
    r.decide((keys, np.full(50, T0), np.full(50, 9), cfg, None))
    st0 = r.eng.stats()
    assert r.eng.charge([], [], [], []).charged.size == 0
    assert rl.lib.rl_charge_batch(h, 0, *[None] * 10) == rl.RL_OK
    assert rl.lib.rl_charge_batch_device(h, 0, *[None] * 11) == rl.RL_OK
    assert rl.lib.rl_charge_batch(h, 3, *[None] * 10) == rl.RL_EINVAL
    assert rl.lib.rl_charge_batch_device(h, 3, *[None] * 11) == rl.RL_EINVAL
    z = np.zeros((1 << 12) + 1, np.int64)
    a = z.ctypes.data_as(C.c_void_p)
    for hole in (2, 3, 4, 5, 7, 8, 9, 10):                  # every array but server_ms and tokens
        args = [h, 3] + [a] * 10
        args[hole] = None
        assert rl.lib.rl_charge_batch(*args) == rl.RL_EINVAL, hole
        assert rl.lib.rl_charge_batch_device(*args, None) == rl.RL_EINVAL, hole
    big = z.size
    assert rl.lib.rl_charge_batch(h, big, a, a, a, a, None, a, a, a, a, None) == rl.RL_EINVAL
    assert rl.lib.rl_charge_batch_device(h, big, a, a, a, a, None, a, a, a, a, None, None) == rl.RL_EINVAL
    st1 = r.eng.stats()
    assert (st0.batches, st0.decisions) == (st1.batches, st1.decisions)
    r.check_state(0, "nothing ran")
    # exactly the maximum, on fifty keys
    mk = np.tile(keys, 82)[:1 << 12]
    r.charge(mk, np.full(mk.size, T0), np.full(mk.size, 2, np.int64), (mk % np.uint64(2)).astype(np.uint32),
             what="the maximum")
    r.check_state(0, "the maximum")
    # the tokens are nullable
    res, _ = r.charge(keys, np.full(50, T0 + 7 * NS), np.full(50, 30, np.int64), cfg, what="no tokens",
                      want_tokens=False)
    assert res.tokens is None and (res.decision[cfg == 0] == po.DENIED).all()      # 30 of a bucket of 20
    assert (res.charged[cfg == 0] > 0).all() and (res.charged[cfg == 0] < 30).all()
    r.check_state(0, "no tokens array")
    r.close()


def test_full_table(rl):
    """tables too full to take every key: the rejected keys' rows carry the
    decide's code and charged = 0, the accepted keys stay exact"""
    configs = [(1, 20, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, tb=1 << 10, win=1 << 10)
    ids = np.random.default_rng(4).permutation(1 << 20)[:2600].astype(np.uint64)
    cfg = (np.arange(2600) % 2).astype(np.uint32)
    d0 = r.eng.decide(ids, np.full(2600, T0), np.full(2600, 5), cfg, check=False)
    assert d0.status == rl.RL_ENOMEM and r.eng.sync() == rl.RL_ENOMEM and r.eng.sync() == 0
    rejected = d0.decision >= po.ERROR
    assert 500 < rejected.sum() < 1100
    before = engine_state(r.eng, 0)
    res = r.eng.charge(ids, np.full(2600, T0), np.full(2600, 18), cfg, check=False)
    assert res.status == rl.RL_ENOMEM and r.eng.sync() == 0
    rej = res.decision >= po.ERROR
    assert np.array_equal(rej, rejected)
    assert np.array_equal(res.decision[rej], d0.decision[rej]) and (res.charged[rej] == 0).all()
    tb, ok = cfg == 0, ~rej
    # a bucket of 20 that gave 5 holds 15: 15 of 18 charged; a window of 100 at 5 records all 18
    assert (res.charged[ok & tb] == 15).all() and (res.decision[ok & tb] == po.DENIED).all()
    assert (res.remaining[ok & tb] == 0).all()
    assert (res.charged[ok & ~tb] == 18).all() and (res.decision[ok & ~tb] == po.ALLOWED).all()
    assert (res.remaining[ok & ~tb] == 77).all()
    after = engine_state(r.eng, 0)
    assert after.keys() == before.keys()
    for name, v in after.items():
        assert v[0] == (0.0 if name.startswith("tb:") else 23), (name, v)
    r.close()


# --- through the coalescer --------------------------------------------------------

@pytest.mark.parametrize("m_call", [300, 70_000])
def test_coalescer_between_decides(rl, m_call):
    """the engine behind the coalescer: decide, Charge, decide, nothing
    drained; below and above the size from which a launch is staged through the
    slot's device block.  With the tally on, its rows are the requests' asked n
    under the verb's decisions; with the top keys on, the requests are counted
    there too."""
    import threading
    import time

    from refund_cases import new_sim
    from tally_cases import expected_tally
    from test_charge_coalescer import charges_of
    from test_refund_coalescer import CONFIGS, rows_of, traces
    warm_tr, held, after = traces()
    mb = 1 << 17
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=mb, flags=rl.OPT_PIPELINE)
    sim = new_sim(0, CONFIGS)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=mb, tally_key_slots=1 << 12, hot_min=3)
    t_call = int(held[1][-1]) + 1000
    call = charges_of(warm_tr, m_call, t_call, 6)
    after = (after[0], after[1] + 2000, after[2], after[3])
    t0 = co.submit(*warm_tr)
    th = co.submit(*held)
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.charge(*call)))
    while co.stats().pending:                      # the decides are launched (not waited for)
        time.sleep(0.0005)
    thr.start()
    while co.stats_charge().charge_launches == 0 and co.stats().pending == 0:   # queued, or launched
        time.sleep(0.0005)
    t1 = co.submit(*after)
    thr.join()
    rc0, got0 = co.wait(t0, warm_tr[0].size)
    rch, goth = co.wait(th, 1)
    rc1, got1 = co.wait(t1, after[0].size)
    assert (rc0, rch, rc1, out["r"][0]) == (0, 0, 0, 0)
    st = co.stats_charge()
    rct, tally = co.tally()
    rch2, hot = co.hot(top=8)
    big = np.zeros(mb + 1, np.int64)
    assert co.charge(big.astype(np.uint64), big, big + 1, big.astype(np.uint32))[0] == -22
    co.close()
    assert eng.sync() == 0
    want0 = warm(sim, warm_tr + (None,))
    wanth = warm(sim, held + (None,))
    rows, info = apply_charge(sim, *call)
    want1 = warm(sim, after + (None,))
    res = out["r"][1]
    assert rows_of(got0, warm_tr[0].size) == [w[:4] for w in want0]
    assert rows_of(res, call[0].size) == [w[:4] for w in rows]
    assert {"full", "short", "dup_denied", "over"} <= set(info["cls"].tolist())
    assert rows_of(got1, after[0].size) == [w[:4] for w in want1]
    assert st.charge_launches == 1
    assert (st.submitted, st.decided) == (1200 + call[0].size,) * 2
    # the tally: every decide request and every charge, by the decision its row carries
    assert rct == 0
    every = [np.concatenate(x) for x in zip(warm_tr, held, call, after)]
    dec = np.array([w[0] for w in want0 + wanth + rows + want1], np.uint8)
    e = expected_tally(every[0], every[3], every[2], dec, len(CONFIGS))
    assert tally.cfg.shape[0] == len(CONFIGS)
    assert np.array_equal(tally.cfg["count"], e.count) and np.array_equal(tally.cfg["units"], e.units)
    # the top keys count the same launches: every decide request and every charge, once
    assert rch2 == 0 and hot.info.requests == st.decided and hot.info.batches == st.batches + st.charge_launches
    assert hot.keys.size == 8 and int(hot.keys["estimate"][0]) >= 3
    eng.close()
