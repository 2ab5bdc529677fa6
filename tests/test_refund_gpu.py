"""Refund (rl_refund_batch) on the GPU, bit-exact against the Python oracle on
both profiles.

The expected state is refund_cases.apply_refunds on the oracle's keyspace.  It
is compared through the per-request status, through Peek (n = 0) of every key,
through every field of the decisions of the trace that follows (`tokens` as
bit patterns), through rl_table_keys, and through the stored values themselves
(a snapshot of the engine against the oracle's db)."""
import ctypes as C

import numpy as np
import pytest

import rl_snapshot as snap
from oracle import rl_oracle_py as po
from refund_cases import (DONE, INT64_MAX, INVALID, KINDS, NOKEY, apply_refunds, bucket_counterexample, new_sim,
                          py_peek, refund_case, warm)
from reset_cases import KEY_RESERVED, engine_keys, py_keys
from tracegen import NS, T0

pytestmark = pytest.mark.gpu

M32 = (1 << 32) - 1


def assert_rows(res, rows, what=""):
    """an engine result against the Python oracle's rows, every field; tokens
    of token-bucket rows as bit patterns"""
    for i, (dec, rem, retry, reset, tok) in enumerate(rows):
        assert res.decision[i] == dec, f"{what} decision at {i}: gpu={res.decision[i]} ref={dec}"
        if dec == po.INVALID:
            continue
        got = (int(res.remaining[i]), int(res.retry_after_ns[i]), int(res.reset_at_ns[i]))
        assert got == (rem, retry, reset), f"{what} at {i}: gpu={got} ref={(rem, retry, reset)}"
        if tok == tok and dec <= 1:
            assert np.float64(tok).view(np.uint64) == res.tokens[i:i + 1].view(np.uint64)[0], f"{what} tokens at {i}"


def engine_state(eng, now_ms, profile=0):
    """{db key: value} of the engine's keys live at now_ms, in the Python
    oracle's naming: tb -> (tokens, last, when), window -> (count, when)"""
    p = snap.parse(eng.snapshot(now_ms))
    live = lambda when: when != snap.ABSENT and (when == snap.NO_EXPIRY or
                                                 (now_ms <= when if profile == 0 else now_ms < when))
    out = {}
    for k, tok, last, when in p["tb"].tolist():
        if live(when):
            out["tb:%d" % k] = (tok, last, when)
    for k, s in zip(p["win"]["key"].tolist(), p["win"]["s"]):
        for j in (0, 1):
            if live(int(s["when"][j])):
                out["w:%d:%d" % (k, s["ws"][j])] = (int(s["cnt"][j]), int(s["when"][j]))
    for k, ws, cnt, when in p["spill"].tolist():
        if live(when):
            out["w:%d:%d" % (k, ws)] = (cnt, when)
    return out


def oracle_state(sim, now_ms):
    out = {}
    for name, (val, when) in sim.db.items():
        if sim._expired(when, now_ms):
            continue
        w = snap.NO_EXPIRY if when is None else when
        out[name] = (val[0], val[1], w) if name.startswith("tb:") else (val, w)
    return out


def locations(eng):
    """{db key: 'slot0' | 'slot1' | 'spill'} of every window key that exists"""
    p = snap.parse(eng.snapshot(0))
    loc = {}
    for k, s in zip(p["win"]["key"].tolist(), p["win"]["s"]):
        for j in (0, 1):
            if s["when"][j] != snap.ABSENT:
                loc["w:%d:%d" % (k, s["ws"][j])] = f"slot{j}"
    for k, ws, when in zip(p["spill"]["key"].tolist(), p["spill"]["ws"].tolist(), p["spill"]["when"].tolist()):
        if when != snap.ABSENT:
            loc["w:%d:%d" % (k, ws)] = "spill"
    return loc


class Rig:
    """an engine and the Python oracle, fed the same decides and refunds"""

    def __init__(self, rl, profile, configs, tb=1 << 12, win=1 << 12, max_batch=1 << 15, flags=0):
        self.rl, self.profile, self.configs = rl, profile, configs
        self.eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch, flags=flags)
        self.sim = new_sim(profile, configs)
        for a, L, W in configs:
            self.eng.register(a, L, W)

    def decide(self, part, what=""):
        key, ts, n, cfg, sms = part
        assert_rows(self.eng.decide(key, ts, n, cfg, sms), warm(self.sim, part), what)

    def refund(self, key, ts, n, cfg, sms=None, what=""):
        """one host refund call: statuses, untouched counters and sticky
        status -> apply_refunds' info"""
        st0 = self.eng.stats()
        status = self.eng.refund(key, ts, n, cfg, sms)
        st1 = self.eng.stats()
        assert (st0.batches, st0.decisions, st0.light_batches) == (st1.batches, st1.decisions, st1.light_batches)
        assert self.eng.sync() == 0
        want, info = apply_refunds(self.sim, key, ts, n, cfg, sms)
        bad = np.nonzero(status != want)[0]
        assert bad.size == 0, f"{what} status at {bad[:10]}: gpu={status[bad[:10]]} ref={want[bad[:10]]}"
        return info

    def check_state(self, now_ms, what=""):
        got, want = engine_state(self.eng, now_ms, self.profile), oracle_state(self.sim, now_ms)
        assert got.keys() == want.keys(), f"{what}: {sorted(got.keys() ^ want.keys())[:6]}"
        for k in want:
            if k.startswith("tb:"):
                assert np.array([got[k][:2]]).view(np.uint64).tolist() == np.array([want[k][:2]]).view(np.uint64).tolist() \
                    and got[k][2] == want[k][2], f"{what} {k}: gpu={got[k]} ref={want[k]}"
            else:
                assert got[k] == want[k], f"{what} {k}: gpu={got[k]} ref={want[k]}"

    def check_keys(self, now_ms, what=""):
        got, want = engine_keys(self.rl, self.eng, now_ms), py_keys(self.sim, now_ms)
        assert got == want, f"{what}: engine only {sorted(got - want)[:5]}, oracle only {sorted(want - got)[:5]}"

    def close(self):
        self.eng.close()


# --- parity: seeded cases, every algorithm ----------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_parity(rl, kind, profile):
    """refund_cases.refund_case: decide the warm-up, refund, Peek every key
    with n = 0, decide the following trace."""
    configs, first, (rkey, rts, rn, rcfg, rsms), second, now_ms, cover = refund_case(kind, profile)
    r = Rig(rl, profile, configs)
    r.decide(first, "warm-up")
    loc = locations(r.eng)
    info = r.refund(rkey, rts, rn, rcfg, rsms, "refund")
    assert sum(len(v) >= 2 for v in info["targets"].values()) >= 50
    if kind == "skew":
        assert {loc[t] for t in info["targets"]} == {"slot0", "slot1", "spill"}
    r.check_state(now_ms, "after the refund")
    r.check_keys(now_ms, "after the refund")
    # Peek every key with n = 0, at the end of the warm-up
    nkeys = int(first[0].max()) + 1
    pk = np.arange(nkeys, dtype=np.uint64)
    pc = (pk % np.uint64(len(configs))).astype(np.uint32)
    t_end = int(first[1][-1])
    got = r.eng.peek(pk, np.full(nkeys, t_end), np.zeros(nkeys, np.int64), pc, np.full(nkeys, now_ms))
    assert_rows(got, [py_peek(r.sim, int(k), t_end, int(c), now_ms) for k, c in zip(pk, pc)], "peek")
    r.decide(second, "second half")
    end_ms = int(second[4][-1]) if second[4] is not None else int(second[1][-1]) // 1_000_000
    r.check_keys(end_ms, "after")
    r.check_state(end_ms, "after")
    r.close()


# --- the sum rule on the device ---------------------------------------------------

def test_bucket_sum_rule(rl):
    """t = 0.9763120008305, a = 4, b = 45 (and the first few t of the seeded
    search): one call stores q14(t + a + b), two calls q14(q14(t + a) + b)"""
    found = bucket_counterexample()[:6]
    assert found[0] == (0.9763120008305, 4, 45)
    configs = [(1, 10 ** 6, 60 * NS)]
    last, when = float(T0) / 1e9, T0 // 1_000_000 + 120_000
    res = []
    for calls in ("one", "two"):
        r = Rig(rl, 0, configs)
        tb = [(10 + j, t, last, when) for j, (t, a, b) in enumerate(found)]
        r.eng.restore(snap.build(tb=tb, profile=0, now_ms=0), 0)
        for k, t, _, w in tb:
            r.sim.db["tb:%d" % k] = [(t, last), w]
        keys = np.array([k for k, *_ in tb], np.uint64)
        a = np.array([x[1] for x in found], np.int64)
        b = np.array([x[2] for x in found], np.int64)
        z = np.zeros(keys.size, np.uint32)
        ts = np.full(keys.size, T0)
        if calls == "one":
            r.refund(np.concatenate([keys, keys]), np.concatenate([ts, ts]), np.concatenate([a, b]),
                     np.concatenate([z, z]))
        else:
            r.refund(keys, ts, a, z)
            r.refund(keys, ts, b, z)
        r.check_state(0, calls)
        st = engine_state(r.eng, 0)
        res.append([st["tb:%d" % k][0] for k in keys.tolist()])
        r.close()
    assert all(x != y for x, y in zip(*res))
    assert ("%.14g" % res[0][0], "%.14g" % res[1][0]) == ("49.97631200083", "49.976312000831")


# --- arithmetic edges -------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_arithmetic_edges(rl, profile):
    """n of 2^32 - 1, 2^32, 2^62 twice and INT64_MAX three times on buckets of
    limit 1 and 1e12 and on window counters; a window count exactly N (DEL) and
    N + 1 (a count of 1 stays)"""
    configs = [(1, 1, 60 * NS), (1, 10 ** 12, 60 * NS), (3, 100, 60 * NS), (2, 100, 60 * NS)]
    r = Rig(rl, profile, configs)
    amounts = [[M32], [1 << 32], [1 << 62, 1 << 62], [INT64_MAX] * 3, [M32, 1], [M32] * 3 + [(1 << 32) + 1]]
    nk = len(amounts)
    # buckets: limit 1 emptied, limit 1e12 down to 5 tokens
    k1, k2 = np.arange(nk, dtype=np.uint64) + np.uint64(100), np.arange(nk, dtype=np.uint64) + np.uint64(200)
    r.decide((k1, np.full(nk, T0), np.ones(nk, np.int64), np.zeros(nk, np.uint32), None))
    r.decide((k2, np.full(nk, T0), np.full(nk, 10 ** 12 - 5), np.ones(nk, np.uint32), None))
    # window counters (fixed and sliding) holding sum(amounts) + d: d = 0 is
    # DEL, d = 1 leaves a count of 1, d = -1 is DEL too; saturated sums delete
    wk, wn, wc, rk, rn_, rc = [], [], [], [], [], []
    kid = 300
    for c in (2, 3):
        for ns in amounts:
            for d in (0, 1, -1):
                have = min(sum(ns), INT64_MAX) + d
                if have > INT64_MAX:
                    have = INT64_MAX
                # INCRBY in two steps: one request's n is below 2^63 anyway
                for part in (have // 2, have - have // 2):
                    wk.append(kid); wn.append(part); wc.append(c)
                rk += [kid] * len(ns); rn_ += ns; rc += [c] * len(ns)
                kid += 1
    r.decide((np.array(wk, np.uint64), np.full(len(wk), T0), np.array(wn, np.int64), np.array(wc, np.uint32), None))
    for j, ns in enumerate(amounts):
        for k, c in ((k1[j], 0), (k2[j], 1)):
            rk += [int(k)] * len(ns); rn_ += ns; rc += [c] * len(ns)
    order = np.random.default_rng(5).permutation(len(rk))
    rk, rn_, rc = np.array(rk, np.uint64)[order], np.array(rn_, np.int64)[order], np.array(rc, np.uint32)[order]
    info = r.refund(rk, np.full(rk.size, T0 + 1000), rn_, rc)
    assert len(info["targets"]) == 2 * nk + 2 * 3 * nk
    assert len(info["deleted"]) >= 2 * 2 * nk - 4        # d = 0 and d = -1, and every saturated sum
    r.check_state(0, "edges")
    st = engine_state(r.eng, 0)
    left = sorted(v[0] for name, v in st.items() if name.startswith("w:"))
    assert left and set(left) == {1}                     # the d = 1 counters of the sums that did not saturate
    assert all(st["tb:%d" % k][0] == 1.0 for k in k1.tolist())
    assert st["tb:200"][0] == 5.0 + M32 and st["tb:202"][0] == 1e12
    # every key again
    r.decide((rk, np.full(rk.size, T0 + 2000), np.full(rk.size, 2), rc, None), "after")
    r.close()


# --- merge shapes -----------------------------------------------------------------

def test_merge_shapes(rl):
    """grid cap + 4096 + 37 refunds of n = 1 on three fixed-window counters:
    every lane of a wave on one key, key runs of 63 and 65 that straddle waves,
    block edges and the grid stride; then a wave of 64 distinct keys"""
    cap = rl.REFUND_GRID_CAP
    assert cap == 1024 * 256
    m = cap + 4096 + 37
    L = 10 ** 9
    configs = [(3, L, 3600 * NS)]
    r = Rig(rl, 0, configs, tb=1 << 6, win=1 << 10, max_batch=1 << 19)
    assert r.eng.refund_max() == 1 << 19
    keys = np.array([1, 2, 3], np.uint64)
    have = 10 ** 7
    r.decide((keys, np.full(3, T0), np.full(3, have), np.zeros(3, np.uint32), None))
    which = np.empty(m, np.int64)
    which[:20_000] = 0                                          # whole waves and blocks of one key
    runs = np.repeat(np.arange(1400) % 3, np.tile([63, 65], 700))  # 89600 requests in runs of 63 and 65
    which[20_000:20_000 + runs.size] = runs
    rest = m - 20_000 - runs.size
    which[20_000 + runs.size:] = np.random.default_rng(1).integers(0, 3, rest)
    which[cap - 130:cap + 130] = 1                              # one key across the stride's seam
    which[-37:] = 2                                             # the ragged tail
    rk = keys[which]
    status = r.eng.refund(rk, np.full(m, T0 + 5), np.ones(m, np.int64), np.zeros(m, np.uint32))
    assert (status == DONE).all()
    assert r.eng.sync() == 0
    cnt = np.bincount(which, minlength=3)
    assert cnt.sum() == m and cnt.min() > 50_000
    got = r.eng.peek(keys, np.full(3, T0 + 9), np.zeros(3, np.int64), np.zeros(3, np.uint32))
    assert (L - got.remaining).tolist() == (have - cnt).tolist()
    # a wave of 64 distinct keys, each with an amount of its own
    k64 = np.arange(64, dtype=np.uint64) + np.uint64(1000)
    r.decide((k64, np.full(64, T0), np.full(64, 1000), np.zeros(64, np.uint32), None))
    status = r.eng.refund(k64, np.full(64, T0 + 5), np.arange(64) + 1, np.zeros(64, np.uint32))
    assert (status == DONE).all()
    got = r.eng.peek(k64, np.full(64, T0 + 9), np.zeros(64, np.int64), np.zeros(64, np.uint32))
    assert (L - got.remaining).tolist() == (1000 - (np.arange(64) + 1)).tolist()
    # every lane its own key next to lanes that share one
    mix = np.concatenate([k64[:40], np.full(24, 1, np.uint64)])
    status = r.eng.refund(mix, np.full(64, T0 + 5), np.full(64, 2), np.zeros(64, np.uint32))
    assert (status == DONE).all()
    got = r.eng.peek(np.array([1000, 1039, 1040, 1], np.uint64), np.full(4, T0 + 9), np.zeros(4, np.int64),
                     np.zeros(4, np.uint32))
    assert (L - got.remaining).tolist() == [997, 958, 959, have - int(cnt[0]) - 48]
    r.close()


# --- nothing stored for NOKEY -----------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_nokey_stores_nothing(rl, profile):
    """a call of only never-seen and expired keys: used / live counts and the
    key set at an earlier clock are unchanged -- no insert, no lazy delete"""
    configs = [(1, 20, 12 * NS), (3, 5, 2 * NS), (2, 5, 2 * NS)]
    r = Rig(rl, profile, configs)
    keys = np.arange(90, dtype=np.uint64)
    cfg = (keys % np.uint64(3)).astype(np.uint32)
    r.decide((keys, np.full(90, T0), np.full(90, 2), cfg, None))
    now_ms = T0 // 1_000_000
    late = now_ms + 3_600_000
    info0 = r.eng.table_info(now_ms)
    keys0, state0 = engine_keys(rl, r.eng, now_ms), engine_state(r.eng, now_ms, profile)
    assert len(keys0) == 90
    fresh = keys + np.uint64(500)
    rk = np.concatenate([keys, fresh])
    rc = np.concatenate([cfg, cfg])
    rs = np.concatenate([np.full(90, late), np.full(90, now_ms)])
    info = r.refund(rk, np.full(180, T0), np.full(180, 3), rc, rs)
    assert not info["targets"] and len(info["expired"]) == 90
    info1 = r.eng.table_info(now_ms)
    for f in ("tb_used", "tb_live", "win_used", "win_live", "spill_used", "spill_live"):
        assert getattr(info0, f) == getattr(info1, f), f
    assert engine_keys(rl, r.eng, now_ms) == keys0 and engine_state(r.eng, now_ms, profile) == state0
    r.check_state(now_ms)
    r.close()


# --- order in flight --------------------------------------------------------------

@pytest.mark.parametrize("size", [6000, 700])
def test_order_in_flight(rl, size):
    """RL_OPT_PIPELINE, device API, no sync between the calls: decide, refund,
    decide (above and below the engine's single-workgroup cut).  The refund
    gives back what the first decide took from the keys the second one uses."""
    import torch
    from tracegen import CONFIG_SETS, random_trace
    configs = CONFIG_SETS["mixed"]
    tr = random_trace(71, 2 * size, 200, configs, big_n=True)
    D = [tuple(None if x is None else x[j * size:(j + 1) * size] for x in tr) for j in range(2)]
    # every key's last request of the first decide twice (its window is live at
    # the key's clock) and every second request (windows of any age), at the
    # store clock of the key's last request: a key's store clock never goes back
    k0, t0 = D[0][0], D[0][1]
    last = {int(k): i for i, k in enumerate(k0.tolist())}
    li = np.array(sorted(last.values()))
    pick = np.concatenate([li, li, np.arange(0, size, 2)])
    rk, rt = k0[pick], t0[pick]
    rn = np.maximum(D[0][2][pick], 1)
    rc = (rk % np.uint64(len(configs))).astype(np.uint32)
    rs = np.array([int(t0[last[int(k)]]) // 1_000_000 for k in rk.tolist()], np.int64)
    r = Rig(rl, 0, configs, flags=rl.OPT_PIPELINE)
    dev = torch.device("cuda", 0)

    def dev_in(*arrs):
        return [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                                 np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                                 np.ascontiguousarray(x)).to(dev) for x in arrs]

    ins = [dev_in(*d[:4]) for d in D]
    outs = [[torch.empty(size, dtype=torch.uint8, device=dev)] +
            [torch.empty(size, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(size, dtype=torch.float64, device=dev)] for _ in D]
    rin = dev_in(rk, rt, rn, rc, rs)
    rst = torch.full((rk.size,), 77, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def decide(j):
        i, o = ins[j], outs[j]
        r.eng.decide_device(size, i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), None,
                            *[x.data_ptr() for x in o], stream)

    decide(0)
    r.eng.refund_device(rk.size, rin[0].data_ptr(), rin[1].data_ptr(), rin[2].data_ptr(), rin[3].data_ptr(),
                        rin[4].data_ptr(), rst.data_ptr(), stream)
    decide(1)
    torch.cuda.synchronize()
    assert r.eng.sync() == 0, r.eng.last_error()
    st = r.eng.stats()
    assert (st.batches, st.decisions) == (2, 2 * size)
    host = lambda o: rl.Decisions(*[x.cpu().numpy() for x in o])
    assert_rows(host(outs[0]), warm(r.sim, D[0]), "decide 0")
    want, info = apply_refunds(r.sim, rk, rt, rn, rc, rs)
    assert np.array_equal(rst.cpu().numpy(), want) and (want == DONE).sum() > 200
    assert_rows(host(outs[1]), warm(r.sim, D[1]), "decide 1")
    r.check_state(int(tr[1][-1]) // 1_000_000)
    r.close()


# --- limits -----------------------------------------------------------------------

def test_limits(rl):
    """m = 0, null arrays, m = rl_refund_max + 1, a nullable status, untouched
    stats and sticky status, only invalid requests"""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, max_batch=1 << 12)
    h = r.eng.h
    assert r.eng.refund_max() == 1 << 12
    keys = np.arange(50, dtype=np.uint64)
    cfg = (keys % np.uint64(2)).astype(np.uint32)
    r.decide((keys, np.full(50, T0), np.full(50, 9), cfg, None))
    assert r.eng.refund([], [], [], []).size == 0
    assert rl.lib.rl_refund_batch(h, 0, None, None, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_refund_batch_device(h, 0, None, None, None, None, None, None, None) == rl.RL_OK
    assert rl.lib.rl_refund_batch(h, 3, None, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_refund_batch_device(h, 3, None, None, None, None, None, None, None) == rl.RL_EINVAL
    big = (1 << 12) + 1
    z = np.zeros(big, np.int64)
    args = [z.ctypes.data_as(C.c_void_p)] * 4
    assert rl.lib.rl_refund_batch(h, big, *args, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_refund_batch_device(h, big, *args, None, None, None) == rl.RL_EINVAL
    r.check_state(0, "nothing ran")
    # exactly the maximum: one call, every request on fifty keys
    mk = np.tile(keys, 82)[:1 << 12]
    info = r.refund(mk, np.full(mk.size, T0), np.ones(mk.size, np.int64), (mk % np.uint64(2)).astype(np.uint32))
    assert len(info["targets"]) == 50 and len(info["deleted"]) == 25
    r.check_state(0, "the maximum")
    # the status is nullable; only invalid requests
    assert r.eng.refund(keys, np.full(50, T0), np.ones(50, np.int64), cfg, want_status=False) is None
    apply_refunds(r.sim, keys, np.full(50, T0), np.ones(50, np.int64), cfg)
    assert r.eng.refund([KEY_RESERVED, 1, 2, 3], [T0] * 4, [1, 0, -1, 1], [0, 1, 0, 2]).tolist() == [INVALID] * 4
    assert r.eng.sync() == 0
    r.check_state(0, "after")
    r.close()


def test_full_table(rl):
    """tables too full to take every key: a refund finds the keys that have
    state (DONE) and ends its bounded probe for the others (NOKEY); the sticky
    status is the decide's, not the refund's"""
    configs = [(1, 20, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, 0, configs, tb=1 << 10, win=1 << 10)
    ids = np.random.default_rng(4).permutation(1 << 20)[:2600].astype(np.uint64)
    cfg = (np.arange(2600) % 2).astype(np.uint32)
    assert r.eng.decide(ids, np.full(2600, T0), np.full(2600, 5), cfg, check=False).status == rl.RL_ENOMEM
    assert r.eng.sync() == rl.RL_ENOMEM and r.eng.sync() == 0
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (1024, 1024)
    before = engine_state(r.eng, 0)
    status = r.eng.refund(ids, np.full(2600, T0), np.full(2600, 3), cfg)
    assert r.eng.sync() == 0
    name = lambda k, c: "tb:%d" % k if c == 0 else "w:%d:%d" % (k, po.window_start(T0, 60 * NS))
    have = np.array([name(int(k), int(c)) in before for k, c in zip(ids, cfg)])
    assert 1500 < have.sum() <= 2048
    assert np.array_equal(status, np.where(have, DONE, NOKEY))
    after = engine_state(r.eng, 0)
    assert after.keys() == before.keys()
    for k, v in before.items():
        assert after[k][0] == (min(v[0] + 3.0, 20.0) if k.startswith("tb:") else v[0] - 3), k
    r.close()
