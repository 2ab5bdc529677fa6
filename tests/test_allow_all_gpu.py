"""AllowAll (rl_allow_all_batch) on the GPU, bit-exact against the composition
on the Python oracle (allow_all_cases.apply_allow_all) on both profiles: every
member field (`tokens` as bit patterns), the verdicts, the rollback statuses,
Peek (n = 0) of every key, the stored values themselves (a snapshot of the
engine against the oracle's db) and the decisions of the trace that follows."""
import ctypes as C

import numpy as np
import pytest

from allow_all_cases import KINDS, MAX_GROUP, allow_all_case, apply_allow_all, group_spans
from oracle import rl_oracle_py as po
from refund_cases import DONE, INVALID, NOKEY, py_peek, warm
from test_refund_gpu import Rig as RefundRig
from test_refund_gpu import assert_rows, engine_state
from tracegen import NS, T0

pytestmark = pytest.mark.gpu


def assert_bytes(got, want, what):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    assert bad.size == 0, f"{what} at {bad[:10]}: gpu={np.asarray(got)[bad[:10]]} ref={np.asarray(want)[bad[:10]]}"


class Rig(RefundRig):
    """an engine and the Python oracle, fed the same decides and AllowAll calls"""

    def allow_all(self, key, ts, n, cfg, first, sms=None, what="", status=0):
        """one host call: every member field, verdict, rollback, the counters
        of a decide batch -> (result, (rows, verdict, g, rollback, info))"""
        st0 = self.eng.stats()
        res = self.eng.allow_all(key, ts, n, cfg, first, sms, check=False)
        assert res.status == status, self.eng.last_error()
        st1 = self.eng.stats()
        assert (st1.batches - st0.batches, st1.decisions - st0.decisions) == (1, len(key))
        assert self.eng.sync() == 0
        want = apply_allow_all(self.sim, np.asarray(key, np.uint64), ts, n, cfg, first, sms)
        self.check_call(res, res.verdict, res.rollback, want, what)
        return res, want

    @staticmethod
    def check_call(res, verdict, rollback, want, what=""):
        rows, v, g, rb, info = want
        assert_rows(res, rows, what)
        assert_bytes(verdict, v, f"{what} verdict")
        if rollback is not None:
            assert_bytes(rollback, rb, f"{what} rollback")


# --- parity: seeded cases, every algorithm ----------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(rl, kind, profile):
    """allow_all_cases.allow_all_case: decide the warm-up, one AllowAll call,
    Peek every key with n = 0, the stored state, the trace that follows"""
    configs, first_trace, (key, ts, n, cfg, sms, first), second, now_ms, cover = allow_all_case(kind, profile)
    r = Rig(rl, profile, configs)
    r.decide(first_trace, "warm-up")
    res, (rows, v, g, rb, info) = r.allow_all(key, ts, n, cfg, first, sms, "call")
    assert (v == po.ALLOWED).sum() > 40 and ((rb == NOKEY) & (g > 0)).any() and (rb == DONE).sum() > 100
    assert any(len(idx) >= 2 for idx in info["targets"].values())
    r.check_state(now_ms, "after the call")
    r.check_keys(now_ms, "after the call")
    pk = np.array(sorted({int(k) for k in key.tolist() if k != np.uint64((1 << 64) - 1)} |
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

SHAPE_CONFIGS = [(3, 10 ** 9, 3600 * NS), (1, 10 ** 9, 3600 * NS), (1, 5, 3600 * NS)]


def shape_call(first, deny_at, seed=3):
    """members for a grouping `first`: a member is either a taker (one of 3000
    keys on a fixed window or a bucket of limit 1e9, n = 1: always allowed) or,
    at the indices deny_at, a denier (a bucket of limit 5 asked for 6: always
    denied, and it takes nothing)"""
    m = len(first)
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 3000, m).astype(np.uint64)
    cfg = (key % np.uint64(2)).astype(np.uint32)
    n = np.ones(m, np.int64)
    deny_at = np.asarray(deny_at, np.int64)
    key[deny_at] = 5000 + deny_at % 50
    cfg[deny_at] = 2
    n[deny_at] = 6
    return key, np.full(m, T0 + 5), n, cfg, np.asarray(first, np.uint8)


def test_small_shapes(rl):
    """groups across lanes 63|64 and the block edge (members 250 to 260), a
    group ending at M - 1, first[0] == 0, runs of exactly 16 and 17, M = 1"""
    r = Rig(rl, 0, SHAPE_CONFIGS)
    m = 600
    first = np.zeros(m, np.uint8)
    heads = [0, 3, 10, 26, 43, 60, 69, 100, 116, 133, 250, 261, 300, 333, 592]
    first[heads] = 1
    first[0] = 0
    first[340:592:4] = 9                                   # groups of 4 up to the last one
    spans = group_spans(first.tolist())
    assert (60, 69) in spans and (250, 261) in spans and (592, 600) in spans
    assert (10, 26) in spans and (26, 43) in spans and (300, 333) in spans    # 16, 17 and 33 members
    deny = [1, 64, 255, 599, 30, 345, 350]
    key, ts, n, cfg, fb = shape_call(first, deny)
    res, (rows, v, g, rb, info) = r.allow_all(key, ts, n, cfg, fb, what="shapes")
    for h, e in spans:
        want = po.INVALID if e - h > MAX_GROUP else po.DENIED if any(h <= d < e for d in deny) else po.ALLOWED
        assert (v[h:e] == want).all(), (h, e)
    assert rb[60] == DONE and rb[64] == INVALID and rb[250] == DONE and rb[260] == DONE and rb[592] == DONE
    assert rb[10] == INVALID and rb[26] == DONE               # an allowed run of 16, a run of 17 rolled back
    r.check_state(0, "shapes")
    # M = 1: an allowed member; a denied window member gets its INCRBY back; a denied bucket asks nothing
    for k, c, nn, verdict, back in ((7, 1, 1, po.ALLOWED, INVALID), (8, 0, 10 ** 9 + 1, po.DENIED, DONE),
                                    (5001, 2, 6, po.DENIED, INVALID)):
        for f0 in (0, 1):
            res, _ = r.allow_all([k], [T0 + 9], [nn], [c], [f0], what="M = 1")
            assert (res.verdict[0], res.rollback[0]) == (verdict, back)
    r.check_state(0, "M = 1")
    r.close()


def test_grid_stride(rl):
    """M = grid cap + 4096 + 37: the grid-stride loop runs twice.  One-member
    groups mixed with 16-member groups, runs of 17 and 33 across the stride's
    seam, a ragged last group"""
    cap = rl.ALLOW_ALL_GRID_CAP
    assert cap == 1024 * 256
    m = cap + 4096 + 37
    r = Rig(rl, 0, SHAPE_CONFIGS, max_batch=1 << 19)
    assert r.eng.allow_all_max() == 1 << 19
    rng = np.random.default_rng(8)
    sizes = rng.choice([1, 1, 1, 16, 16, 5], m // 4)
    heads = np.concatenate([[0], np.cumsum(sizes)])
    first = np.zeros(m, np.uint8)
    first[heads[heads < m]] = 1
    # the seam: a run of 17 that straddles member `cap`, a run of 33 behind it, then 16
    first[cap - 40:cap + 80] = 0
    first[[cap - 40, cap - 24, cap - 8, cap + 9, cap + 42, cap + 58]] = 1
    first[m - 37:] = 0
    first[m - 37] = 1                                         # 37 members: too long, to the end
    spans = group_spans(first.tolist())
    for want in ((cap - 8, cap + 9), (cap + 9, cap + 42), (cap + 42, cap + 58), (m - 37, m)):
        assert want in spans
    deny = rng.integers(0, m, m // 40)
    deny = np.unique(np.concatenate([deny[(deny < cap - 24) | (deny >= cap - 8)], [cap - 30, cap + 50]]))
    key, ts, n, cfg, fb = shape_call(first, deny)
    res, (rows, v, g, rb, info) = r.allow_all(key, ts, n, cfg, fb, what="stride")
    assert (v[cap - 8:cap + 42] == po.INVALID).all() and (v[cap - 40:cap - 24] == po.DENIED).all()
    assert (v[cap + 42:cap + 58] == po.DENIED).all() and (v[m - 37:] == po.INVALID).all()
    assert (v[cap - 24:cap - 8] == po.ALLOWED).all()
    assert (v == po.ALLOWED).sum() > m // 4 and (rb == DONE).sum() > m // 8
    r.check_state(0, "stride")
    r.close()


# --- order in flight --------------------------------------------------------------

def test_order_in_flight(rl):
    """RL_OPT_PIPELINE, device API, no host sync between the calls: decide,
    AllowAll, AllowAll from a second stream, decide"""
    import torch
    configs, first_trace, (key, ts, n, cfg, sms, first), second, now_ms, _ = allow_all_case("mixed", 0)
    span = int(ts[-1]) - int(ts[0]) + 1000
    second = (second[0], second[1] + span, second[2], second[3], None)
    r = Rig(rl, 0, configs, flags=rl.OPT_PIPELINE)
    dev = torch.device("cuda", 0)

    def dev_in(*arrs):
        return [None if x is None else
                torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                                 np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                                 np.ascontiguousarray(x)).to(dev) for x in arrs]

    def dev_out(m, extra):
        return ([torch.empty(m, dtype=torch.uint8, device=dev)] +
                [torch.empty(m, dtype=torch.int64, device=dev) for _ in range(3)] +
                [torch.empty(m, dtype=torch.float64, device=dev)] +
                [torch.full((m,), 77, dtype=torch.uint8, device=dev) for _ in range(extra)])

    p = lambda t: None if t is None else t.data_ptr()
    D = [first_trace, second]
    d_in = [dev_in(*d) for d in D]
    d_out = [dev_out(d[0].size, 0) for d in D]
    calls = [(key, ts, n, cfg, sms, first), (key, ts + span, n, cfg, sms, first)]
    a_in = [dev_in(*c) for c in calls]
    a_out = [dev_out(key.size, 2) for _ in calls]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()

    def decide(j, s):
        i, o = d_in[j], d_out[j]
        r.eng.decide_device(D[j][0].size, *[p(x) for x in i], *[p(x) for x in o], s.cuda_stream)

    def allow_all(j, s):
        i, o = a_in[j], a_out[j]
        r.eng.allow_all_device(key.size, p(i[0]), p(i[1]), p(i[2]), p(i[3]), p(i[4]), p(i[5]),
                               *[p(x) for x in o], s.cuda_stream)

    decide(0, streams[0])
    allow_all(0, streams[0])
    allow_all(1, streams[1])
    decide(1, streams[0])
    torch.cuda.synchronize()
    assert r.eng.sync() == 0, r.eng.last_error()
    st = r.eng.stats()
    assert (st.batches, st.decisions) == (4, D[0][0].size + D[1][0].size + 2 * key.size)
    host = lambda o: rl.Decisions(*[x.cpu().numpy() for x in o[:5]])
    assert_rows(host(d_out[0]), warm(r.sim, D[0]), "decide 0")
    for j, c in enumerate(calls):
        want = apply_allow_all(r.sim, *c[:4], c[5], c[4])
        Rig.check_call(host(a_out[j]), a_out[j][5].cpu().numpy(), a_out[j][6].cpu().numpy(), want, f"call {j}")
        assert (want[3] == DONE).sum() > 100
    assert_rows(host(d_out[1]), warm(r.sim, D[1]), "decide 1")
    r.check_state(int(second[1][-1]) // 1_000_000)
    r.close()


# --- limits -----------------------------------------------------------------------

def test_limits(rl):
    """m = 0, null arrays, m = rl_allow_all_max + 1, a nullable rollback"""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, max_batch=1 << 12)
    h = r.eng.h
    assert r.eng.allow_all_max() == r.eng.refund_max() == 1 << 12
    keys = np.arange(50, dtype=np.uint64)
    cfg = (keys % np.uint64(2)).astype(np.uint32)
    r.decide((keys, np.full(50, T0), np.full(50, 9), cfg, None))
    st0 = r.eng.stats()
    assert r.eng.allow_all([], [], [], [], []).verdict.size == 0
    assert rl.lib.rl_allow_all_batch(h, 0, *[None] * 13) == rl.RL_OK
    assert rl.lib.rl_allow_all_batch_device(h, 0, *[None] * 14) == rl.RL_OK
    assert rl.lib.rl_allow_all_batch(h, 3, *[None] * 13) == rl.RL_EINVAL
    assert rl.lib.rl_allow_all_batch_device(h, 3, *[None] * 14) == rl.RL_EINVAL
    big = (1 << 12) + 1
    z = np.zeros(big, np.int64)
    a = z.ctypes.data_as(C.c_void_p)
    assert rl.lib.rl_allow_all_batch(h, big, a, a, a, a, None, a, a, a, a, a, None, a, None) == rl.RL_EINVAL
    assert rl.lib.rl_allow_all_batch_device(h, big, a, a, a, a, None, a, a, a, a, a, None, a, None, None) == rl.RL_EINVAL
    st1 = r.eng.stats()
    assert (st0.batches, st0.decisions) == (st1.batches, st1.decisions)
    r.check_state(0, "nothing ran")
    # exactly the maximum: 256 groups of 16 on fifty keys
    mk = np.tile(keys, 82)[:1 << 12]
    first = (np.arange(mk.size) % 16 == 0).astype(np.uint8)
    r.allow_all(mk, np.full(mk.size, T0), np.ones(mk.size, np.int64), (mk % np.uint64(2)).astype(np.uint32), first,
                what="the maximum")
    r.check_state(0, "the maximum")
    # the rollback is nullable, and so are the tokens
    args = (keys, np.full(50, T0 + 7), np.full(50, 30, np.int64), cfg, np.ones(50, np.uint8))
    res = r.eng.allow_all(*args, want_rollback=False, want_tokens=False)
    assert res.rollback is None
    rows, v, g, rb, _ = apply_allow_all(r.sim, *args)
    assert_bytes(res.verdict, v, "verdict")
    assert (v[cfg == 0] == po.DENIED).all()          # 30 of a bucket of 20
    r.check_state(0, "no rollback array")
    r.close()


def test_full_table(rl):
    """tables too full to take every key: a rejected member fails its group,
    and the accepted keys of those groups stay bit-exact"""
    configs = [(1, 20, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, tb=1 << 10, win=1 << 10)
    ids = np.random.default_rng(4).permutation(1 << 20)[:2600].astype(np.uint64)
    cfg = (np.arange(2600) % 2).astype(np.uint32)
    d0 = r.eng.decide(ids, np.full(2600, T0), np.full(2600, 5), cfg, check=False)
    assert d0.status == rl.RL_ENOMEM and r.eng.sync() == rl.RL_ENOMEM and r.eng.sync() == 0
    rejected = d0.decision >= po.ERROR
    assert 500 < rejected.sum() < 1100
    before = engine_state(r.eng, 0)
    # groups of two: an accepted key, then any key
    acc = np.nonzero(~rejected)[0][:1200]
    other = np.random.default_rng(5).permutation(2600)[:1200]
    idx = np.stack([acc, other], 1).ravel()
    first = (np.arange(idx.size) % 2 == 0).astype(np.uint8)
    res = r.eng.allow_all(ids[idx], np.full(idx.size, T0), np.full(idx.size, 3), cfg[idx], first, check=False)
    assert res.status == rl.RL_ENOMEM and r.eng.sync() == 0
    rej = res.decision >= po.ERROR
    assert np.array_equal(rej, rejected[idx]) and 150 < rej.sum()
    pair_fails = rej.reshape(-1, 2).any(1)
    assert (res.verdict.reshape(-1, 2)[pair_fails] >= po.ERROR).all()
    assert (res.verdict.reshape(-1, 2)[~pair_fails] == po.ALLOWED).all()
    assert (res.rollback[rej] == INVALID).all()
    assert (res.rollback[np.repeat(pair_fails, 2) & ~rej] == DONE).all()
    after = engine_state(r.eng, 0)
    assert after.keys() == before.keys()
    name = lambda k, c: "tb:%d" % k if c == 0 else "w:%d:%d" % (k, po.window_start(T0, 60 * NS))
    kept = np.zeros(2600, np.int64)                 # what the allowed groups keep, per request index
    np.add.at(kept, idx[np.repeat(~pair_fails, 2)], 3)
    for j in np.nonzero(~rejected)[0]:
        k = name(int(ids[j]), int(cfg[j]))
        want = before[k][0] - kept[j] if cfg[j] == 0 else before[k][0] + kept[j]
        assert after[k][0] == want and after[k][1:] == before[k][1:], k
    r.close()


# --- through the coalescer --------------------------------------------------------

@pytest.mark.parametrize("m_call", [300, 70_000])
def test_coalescer_between_decides(rl, m_call):
    """the engine behind the coalescer: decide, AllowAll, decide, nothing
    drained; below and above the size from which a launch is staged through the
    slot's device block.  With the tally on, its rows are the members' own
    decisions; with the top keys on, the members are counted there too."""
    import threading
    import time

    from refund_cases import new_sim
    from tally_cases import expected_tally
    from test_allow_all_coalescer import members_of
    from test_refund_coalescer import CONFIGS, rows_of, traces
    warm_tr, held, after = traces()
    mb = 1 << 17
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=mb, flags=rl.OPT_PIPELINE)
    sim = new_sim(0, CONFIGS)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=mb, tally_key_slots=1 << 12, hot_min=3)
    t_call = int(held[1][-1]) + 1000
    groups = m_call // 3
    call = members_of(warm_tr, groups, t_call, 6)
    after = (after[0], after[1] + 2000, after[2], after[3])
    t0 = co.submit(*warm_tr)
    th = co.submit(*held)
    out = {}
    thr = threading.Thread(target=lambda: out.update(r=co.allow_all(*call)))
    while co.stats().pending:                      # the decides are launched (not waited for)
        time.sleep(0.0005)
    thr.start()
    while co.stats().allow_all_launches == 0 and co.stats().pending == 0:   # queued, or launched
        time.sleep(0.0005)
    t1 = co.submit(*after)
    thr.join()
    rc0, got0 = co.wait(t0, warm_tr[0].size)
    rch, goth = co.wait(th, 1)
    rc1, got1 = co.wait(t1, after[0].size)
    assert (rc0, rch, rc1, out["r"][0]) == (0, 0, 0, 0)
    st = co.stats()
    rct, tally = co.tally()
    rch2, hot = co.hot(top=8)
    big = np.zeros(mb + 1, np.int64)
    assert co.allow_all(big.astype(np.uint64), big, big + 1, big.astype(np.uint32), big.astype(np.uint8))[0] == -22
    co.close()
    assert eng.sync() == 0
    want0 = warm(sim, warm_tr + (None,))
    wanth = warm(sim, held + (None,))
    rows, v, g, rb, _ = apply_allow_all(sim, *call)
    want1 = warm(sim, after + (None,))
    res = out["r"][1]
    assert rows_of(got0, warm_tr[0].size) == [w[:4] for w in want0]
    assert rows_of(res, call[0].size) == [w[:4] for w in rows]
    assert_bytes(res[4], v, "verdict")
    assert (v == po.ALLOWED).any() and (g > 0).sum() > 20
    assert rows_of(got1, after[0].size) == [w[:4] for w in want1]
    assert (st.allow_all_launches, st.allow_all_groups) == (1, groups)
    assert (st.submitted, st.decided) == (1200 + call[0].size,) * 2
    # the tally: every decide request and every member, by its own decision
    assert rct == 0
    every = [np.concatenate(x) for x in zip(warm_tr, held, call[:4], after)]
    dec = np.array([w[0] for w in want0 + wanth + rows + want1], np.uint8)
    e = expected_tally(every[0], every[3], every[2], dec, len(CONFIGS))
    assert tally.cfg.shape[0] == len(CONFIGS)
    assert np.array_equal(tally.cfg["count"], e.count) and np.array_equal(tally.cfg["units"], e.units)
    assert int(e.count[:, 0].sum()) > 100
    # the top keys count the same launches: every decide request and every member, once
    assert rch2 == 0 and hot.info.requests == st.decided and hot.info.batches == st.batches + st.allow_all_launches
    assert hot.keys.size == 8 and int(hot.keys["estimate"][0]) >= 3
    eng.close()
