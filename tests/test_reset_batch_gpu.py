"""Batched Reset (rl_reset_batch) on the GPU.

The expected state is the C oracle's after one `reset` per executed request.
It is compared in two ways: rl_table_keys(now_ms) against the oracle's live
keys as sets, and every field of the decisions of the trace that follows
(`tokens` as bit patterns)."""
import numpy as np
import pytest

import oracle
import rl_snapshot as snap
from reset_cases import (INVALID, KEY_RESERVED, KINDS, RESET_DONE, apply_resets, engine_keys, expected_status,
                         reset_case)
from tracegen import CONFIG_SETS, NS, T0, many_configs, random_trace

pytestmark = pytest.mark.gpu


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


class Rig:
    """an engine and the C oracle, fed the same decides and resets"""

    def __init__(self, rl, profile, configs, tb=1 << 12, win=1 << 12, max_batch=1 << 15, flags=0):
        self.rl, self.profile, self.configs = rl, profile, configs
        self.eng = rl.Engine(profile=profile, tb_capacity=tb, win_capacity=win, max_batch=max_batch, flags=flags)
        self.sim = oracle.OracleSim(profile)
        for a, L, W in configs:
            assert self.eng.register(a, L, W) == self.sim.add_config(a, L, W)

    def decide(self, part, what=""):
        key, ts, n, cfg, sms = part
        assert_same(self.eng.decide(key, ts, n, cfg, sms), self.sim.decide(key, ts, n, cfg, sms), self.configs, cfg,
                    what=what)

    def check_keys(self, now_ms, what=""):
        got, want = engine_keys(self.rl, self.eng, now_ms), set(self.sim.keys(now_ms))
        assert got == want, f"{what}: engine only {sorted(got - want)[:5]}, oracle only {sorted(want - got)[:5]}"
        return want

    def reset(self, key, ts, cfg, now_ms, what=""):
        """one host reset batch: statuses, untouched counters and sticky
        status, and the key set afterwards; -> the keys it deleted"""
        key, ts, cfg = np.asarray(key, np.uint64), np.asarray(ts, np.int64), np.asarray(cfg, np.uint32)
        before = set(self.sim.keys(now_ms))
        st0 = self.eng.stats()
        status = self.eng.reset_batch(key, ts, cfg)
        st1 = self.eng.stats()
        assert (st0.batches, st0.decisions, st0.sort_predicted, st0.light_batches) == \
               (st1.batches, st1.decisions, st1.sort_predicted, st1.light_batches)
        assert np.array_equal(status, expected_status(key, cfg, len(self.configs))), what
        assert self.eng.sync() == 0
        apply_resets(self.sim, key, ts, cfg, len(self.configs), now_ms)
        return before - self.check_keys(now_ms, what)

    def close(self):
        self.eng.close()


def locations(eng):
    """{(key, ws): 'slot0' | 'slot1' | 'spill'} of every window key that exists"""
    p = snap.parse(eng.snapshot(0))
    loc = {}
    for k, s in zip(p["win"]["key"].tolist(), p["win"]["s"]):
        for j in (0, 1):
            if s["when"][j] != snap.ABSENT:
                loc[(k, int(s["ws"][j]))] = f"slot{j}"
    for k, ws, when in zip(p["spill"]["key"].tolist(), p["spill"]["ws"].tolist(), p["spill"]["when"].tolist()):
        if when != snap.ABSENT:
            loc[(k, ws)] = "spill"
    return loc


# --- seeded cases, every algorithm ------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_cases(rl, kind, profile):
    """reset_cases.reset_case: resets at the warm-up's own request times (live
    windows of any age), one window later / earlier, far away, absent keys,
    duplicates.  The skewed-clock case must delete window keys in slot 0, in
    slot 1 and in the spill."""
    configs, first, (rkey, rts, rcfg), second, now_ms = reset_case(kind, 100 + profile, ff=kind in ("fw", "sw"))
    r = Rig(rl, profile, configs)
    r.decide(first, "first half")
    r.check_keys(now_ms, "before")
    loc = locations(r.eng)
    gone = r.reset(rkey, rts, rcfg, now_ms, "reset")
    assert len(gone) >= 5
    if kind == "skew":
        assert {loc[(k, ws)] for k, kind_, ws in gone if kind_ == 1} == {"slot0", "slot1", "spill"}
    r.decide(second, "second half")
    r.check_keys(int(second[4][-1]) if second[4] is not None else int(second[1][-1]) // 1_000_000, "after")
    r.close()


# --- launch shapes ----------------------------------------------------------------

def test_launch_shapes(rl):
    """m = 0, 1, 255, 256, 257, and around what the capped grid covers with one
    reset per thread (the stride).  Token-bucket keys; every shape has a key
    range of its own, and every fourth key of a range stays out of its batch."""
    cap = rl.RESET_GRID_CAP
    assert cap == 1024 * 256
    configs = [(1, 20, 12 * NS)]
    shapes = [0, 1, 255, 256, 257, cap - 1, cap, cap + 1]
    r = Rig(rl, 0, configs, tb=1 << 22, win=1 << 6, max_batch=1 << 19)
    total = sum(s + (s + 2) // 3 for s in shapes)
    ids = np.arange(total, dtype=np.uint64) + np.uint64(1000)
    for o in range(0, total, 1 << 19):
        k = ids[o:o + (1 << 19)]
        r.decide((k, np.full(k.size, T0), np.full(k.size, 3), np.zeros(k.size, np.uint32), None))
    now_ms = T0 // 1_000_000
    assert r.eng.table_info(now_ms).tb_live == total
    off, live = 0, total
    for m in shapes:
        span = ids[off:off + m + (m + 2) // 3]
        inside = np.ones(span.size, bool)
        inside[3::4] = False                      # every fourth key stays
        inside[np.nonzero(inside)[0][m:]] = False
        batch = span[inside]
        assert batch.size == m
        status = r.eng.reset_batch(batch, np.full(m, T0), np.zeros(m, np.uint32))
        assert status.size == m and (status == RESET_DONE).all()
        apply_resets(r.sim, batch, np.full(m, T0), np.zeros(m, np.uint32), 1, now_ms)
        live -= m
        assert r.eng.table_info(now_ms).tb_live == live, m
        off += span.size
    want = np.array(sorted(k for k, _, _ in r.sim.keys(now_ms)), np.uint64)
    assert want.size == live
    import ctypes as C
    from reset_cases import KEY_REC
    out, cnt = np.zeros(live, KEY_REC), C.c_uint64()
    assert rl.lib.rl_table_keys(r.eng.h, now_ms, out.ctypes.data_as(C.c_void_p), live, C.byref(cnt)) == 0
    assert cnt.value == live and np.array_equal(np.sort(out["key_id"]), want)
    # reset keys are fresh, the others carry on
    for o in range(0, total, 1 << 19):
        k = ids[o:o + (1 << 19)]
        r.decide((k, np.full(k.size, T0 + 1000), np.full(k.size, 18), np.zeros(k.size, np.uint32), None), "after")
    r.close()


# --- probe runs -------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_probe_runs(rl, profile):
    """1024-slot tables filled to ~90 %: keys share home slots and sit at the
    end of long runs.  Every third key is reset; the others keep their state."""
    configs = [(1, 20, 12 * NS), (2, 100, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, profile, configs, tb=1 << 10, win=1 << 10)
    info = r.eng.table_info(0)
    assert (info.tb_capacity, info.win_capacity) == (1024, 1024)
    nk = 920
    rng = np.random.default_rng(9 + profile)
    ids = rng.permutation(1 << 20)[:2 * nk].astype(np.uint64)
    cfg = np.concatenate([np.zeros(nk, np.uint32), 1 + (np.arange(nk) % 2).astype(np.uint32)])
    ts = T0 + np.arange(ids.size, dtype=np.int64) * 1000
    n = rng.choice([1, 2, 25, 120], ids.size).astype(np.int64)
    r.decide((ids, ts, n, cfg, None))
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (nk, nk)
    home = snap.mix64(ids[:nk]) & np.uint64(1023)
    assert np.unique(home).size < nk - 200           # shared home slots
    now_ms = int(ts[-1]) // 1_000_000
    sel = np.arange(ids.size) % 3 == 0
    gone = r.reset(ids[sel], np.full(int(sel.sum()), ts[-1]), cfg[sel], now_ms)
    assert {k for k, _, _ in gone} == set(ids[sel].tolist())
    info = r.eng.table_info(0)
    assert (info.tb_used, info.win_used) == (nk, nk)   # no key id leaves a table
    r.decide((ids, np.full(ids.size, ts[-1] + 5000), n, cfg, None), "after")
    r.close()


# --- per algorithm ----------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_token_bucket_present_absent_already_reset(rl, profile):
    configs = [(1, 20, 12 * NS)]
    r = Rig(rl, profile, configs)
    keys = np.arange(1, 41, dtype=np.uint64)
    one = lambda t, n: (keys, np.full(40, t), np.full(40, n), np.zeros(40, np.uint32), None)
    r.decide(one(T0, 15))
    now_ms = T0 // 1_000_000
    r.reset([3], [T0], [0], now_ms, "a single reset before")          # already reset when the batch runs
    batch = np.array([1, 2, 3, 1000, 1001, 4], np.uint64)             # present, already reset, absent
    gone = r.reset(batch, np.full(6, T0), np.zeros(6, np.uint32), now_ms, "batch")
    assert gone == {(1, 0, 0), (2, 0, 0), (4, 0, 0)}
    assert r.reset(batch, np.full(6, T0), np.zeros(6, np.uint32), now_ms, "again") == set()
    r.decide(one(T0 + 1000, 10), "after")     # 15 + 10 > 20: only the reset keys are allowed
    r.close()


def window_rig(rl, profile, alg):
    """keys 1..4 of a 60 s window limiter with the same history: windows w0,
    w1, w2 in turn, all alive (the server clock stands still), so w0 is in the
    spill and w1, w2 in the entry's slots"""
    configs = [(alg, 100, 60 * NS)]
    r = Rig(rl, profile, configs)
    w = [(T0 // (60 * NS) + 1 + j) * 60 * NS for j in range(4)]
    s0 = w[0] // 1_000_000
    keys = np.arange(1, 5, dtype=np.uint64)
    for j in range(3):
        r.decide((keys, np.full(4, w[j] + 5 * NS), np.full(4, 7 + j), np.zeros(4, np.uint32), np.full(4, s0)))
    loc = locations(r.eng)
    for k in (1, 2, 3, 4):
        assert loc[(k, w[0] // NS)] == "spill"
        assert {loc[(k, w[1] // NS)], loc[(k, w[2] // NS)]} == {"slot0", "slot1"}
    return r, w, s0, keys, loc


def window_after(r, w, s0, keys):
    """every key at every window again"""
    for j in (2, 1, 0, 3):
        r.decide((keys, np.full(4, w[j] + 6 * NS), np.full(4, 95), np.zeros(4, np.uint32), np.full(4, s0)), f"w{j}")


@pytest.mark.parametrize("profile", [0, 1])
def test_fixed_window_slots_and_spill(rl, profile):
    r, w, s0, keys, loc = window_rig(rl, profile, 3)
    # key 1: the newest window; key 2: the one before (the other slot); key 3:
    # the spilled one; key 4: a ts in a window that holds nothing
    ts = np.array([w[2] + 9 * NS, w[1] + 59 * NS, w[0], w[3] + NS], np.int64)
    gone = r.reset(keys, ts, np.zeros(4, np.uint32), s0)
    assert gone == {(1, 1, w[2] // NS), (2, 1, w[1] // NS), (3, 1, w[0] // NS)}
    assert {loc[(1, w[2] // NS)], loc[(2, w[1] // NS)], loc[(3, w[0] // NS)]} == {"slot0", "slot1", "spill"}
    window_after(r, w, s0, keys)
    r.close()


@pytest.mark.parametrize("profile", [0, 1])
def test_sliding_window_current_and_previous(rl, profile):
    r, w, s0, keys, loc = window_rig(rl, profile, 2)
    # key 1: current w2 + previous w1 (both slots); key 2: current w1 + previous
    # w0 (in the spill); key 3: one window later -- w3 holds nothing, w2 goes,
    # w1 and w0 stay; key 4: far from every window
    ts = np.array([w[2] + 9 * NS, w[1] + 30 * NS, w[3] + NS, w[3] + 3600 * NS], np.int64)
    gone = r.reset(keys, ts, np.zeros(4, np.uint32), s0)
    assert gone == {(1, 1, w[2] // NS), (1, 1, w[1] // NS), (2, 1, w[1] // NS), (2, 1, w[0] // NS),
                    (3, 1, w[2] // NS)}
    window_after(r, w, s0, keys)
    r.close()


def test_one_id_two_tables(rl):
    """the same key id under a token-bucket config and under a window config:
    a reset touches the table of its config only"""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS), (2, 100, 60 * NS)]
    r = Rig(rl, 0, configs)
    ids = np.array([5, 5, 6, 6, 7, 7], np.uint64)
    cfg = np.array([0, 1, 0, 2, 0, 1], np.uint32)
    r.decide((ids, np.full(6, T0), np.full(6, 15), cfg, None))
    now_ms = T0 // 1_000_000
    ws = T0 // (60 * NS) * 60
    gone = r.reset([5, 6], [T0, T0], [0, 2], now_ms)
    assert gone == {(5, 0, 0), (6, 1, ws)}
    gone = r.reset([7, 7], [T0, T0], [1, 0], now_ms)
    assert gone == {(7, 0, 0), (7, 1, ws)}
    r.decide((ids, np.full(6, T0 + 1000), np.full(6, 10), cfg, None), "after")
    r.close()


def test_single_resets_against_batch(rl):
    """the same resets through rl_reset one by one on one engine and through
    one rl_reset_batch on another (both run the one device routine, reset_one):
    the same keys afterwards, the same decisions from a following batch.  A
    token-bucket key, fixed-window keys in a slot and in the spill, sliding-
    window keys whose current or previous window is spilled."""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS), (2, 100, 60 * NS)]
    a, b = Rig(rl, 0, configs), Rig(rl, 0, configs)
    w = [(T0 // (60 * NS) + 1 + j) * 60 * NS for j in range(4)]
    s0 = w[0] // 1_000_000
    keys = np.arange(1, 25, dtype=np.uint64)
    cfg = (keys % np.uint64(3)).astype(np.uint32)
    for j in range(3):        # windows w0, w1, w2 all alive: w0 is in the spill
        part = (keys, np.full(24, w[j] + 5 * NS), np.full(24, 7 + j), cfg, np.full(24, s0))
        a.decide(part)
        b.decide(part)
    loc = locations(a.eng)
    assert loc == locations(b.eng)
    assert all(loc[(int(k), w[0] // NS)] == "spill" for k in keys[cfg != 0])
    #        TB   absent TB  FW slot  FW spill  SW w1+w0(spill)  SW w2+w1  SW w3: w2 only
    rkey = [3,    999,       4,       7,        5,               8,        11]
    rcfg = [0,    0,         1,       1,        2,               2,        2]
    rts = [T0,    T0,        w[2],    w[0] + NS, w[1] + 30 * NS, w[2] + NS, w[3] + NS]
    before = engine_keys(rl, a.eng, s0)
    for k, t, c in zip(rkey, rts, rcfg):
        a.eng.reset(c, k, t)
    assert (b.eng.reset_batch(rkey, rts, rcfg) == RESET_DONE).all()
    assert a.eng.sync() == 0 and b.eng.sync() == 0
    after = engine_keys(rl, a.eng, s0)
    assert after == engine_keys(rl, b.eng, s0)
    assert before - after == {(3, 0, 0), (4, 1, w[2] // NS), (7, 1, w[0] // NS), (5, 1, w[1] // NS),
                              (5, 1, w[0] // NS), (8, 1, w[2] // NS), (8, 1, w[1] // NS), (11, 1, w[2] // NS)}
    assert locations(a.eng) == locations(b.eng)
    apply_resets(a.sim, rkey, rts, rcfg, len(configs), s0)
    for j in (2, 1, 0, 3):    # every key at every window again: engine against engine, and against the oracle
        part = (keys, np.full(24, w[j] + 6 * NS), np.full(24, 95), cfg, np.full(24, s0))
        ra, rb = a.eng.decide(*part), b.eng.decide(*part)
        for f in ("decision", "remaining", "retry_after_ns", "reset_at_ns"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), f"w{j} {f}"
        assert np.array_equal(ra.tokens.view(np.uint64)[cfg == 0], rb.tokens.view(np.uint64)[cfg == 0]), f"w{j}"
        assert_same(ra, a.sim.decide(*part), configs, cfg, f"w{j}")
    a.close()
    b.close()


# --- duplicates -------------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
def test_duplicates_in_one_batch(rl, profile):
    """the same (key, ts, cfg) 64 times in one wave, per algorithm, and one
    sliding-window key at two ts in adjacent windows: the oracle's result"""
    configs = [(1, 20, 12 * NS), (2, 100, 60 * NS), (3, 100, 60 * NS)]
    r = Rig(rl, profile, configs)
    w = [(T0 // (60 * NS) + 1 + j) * 60 * NS for j in range(3)]
    s0 = w[0] // 1_000_000
    keys = np.arange(30, dtype=np.uint64)
    cfg = (keys % np.uint64(3)).astype(np.uint32)
    for j in range(3):
        r.decide((keys, np.full(30, w[j] + NS), np.full(30, 9), cfg, np.full(30, s0)))
    for k in (0, 1, 2):        # a token bucket, a sliding and a fixed window key
        rk = np.concatenate([np.full(64, k), [12 + k, 15 + k]]).astype(np.uint64)
        gone = r.reset(rk, np.full(66, w[2] + 2 * NS), (rk % np.uint64(3)).astype(np.uint32), s0, f"64 x key {k}")
        assert len(gone) == [3, 6, 3][k]
    # sliding-window key 4 at w2 and at w1: w2, w1 and w0 (spilled) all go
    rk = np.tile(np.array([4, 4], np.uint64), 32)
    rt = np.tile(np.array([w[2] + NS, w[1] + NS], np.int64), 32)
    gone = r.reset(rk, rt, np.ones(64, np.uint32), s0, "adjacent windows")
    assert gone == {(4, 1, x // NS) for x in w}
    for j in (2, 1, 0):
        r.decide((keys, np.full(30, w[j] + 3 * NS), np.full(30, 93), cfg, np.full(30, s0)), f"after, w{j}")
    r.close()


# --- invalid requests -------------------------------------------------------------

@pytest.mark.parametrize("N", [15, 40, 70])
def test_invalid_requests(rl, N):
    """cfg == N, N + 63 and the reserved key among valid requests, with 15, 40
    (> 32) and 70 (> 64) registered configs"""
    configs = CONFIG_SETS["mixed"] if N == 15 else many_configs(3, N)
    assert len(configs) == N
    r = Rig(rl, 0, configs)
    first = random_trace(17, 6000, 300, configs)
    second = random_trace(18, 3000, 300, configs)
    second = (second[0], second[1] + (first[1][-1] - T0), second[2], second[3], None)
    r.decide(first)
    now_ms = int(first[1][-1]) // 1_000_000
    rkey = first[0][-500:].copy()
    rts = first[1][-500:].copy()
    rcfg = first[3][-500:].copy()
    rcfg[::7] = N
    rcfg[3::7] = N + 63
    rkey[5::7] = np.uint64(KEY_RESERVED)
    st = expected_status(rkey, rcfg, N)
    assert (st == INVALID).sum() >= 200 and (st == RESET_DONE).sum() >= 200
    gone = r.reset(rkey, rts, rcfg, now_ms)       # statuses, stats and the sticky status: Rig.reset
    assert len(gone) > 20
    # status is nullable
    assert r.eng.reset_batch(rkey, rts, rcfg, want_status=False) is None
    assert r.eng.sync() == 0
    # only invalid requests, and none
    assert list(r.eng.reset_batch([KEY_RESERVED, 1], [T0, T0], [0, N])) == [INVALID, INVALID]
    assert r.eng.reset_batch([], [], []).size == 0
    assert rl.lib.rl_reset_batch(r.eng.h, 3, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_reset_batch_device(r.eng.h, 3, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_reset_batch_device(r.eng.h, 0, None, None, None, None, None) == rl.RL_OK
    assert r.eng.sync() == 0
    r.check_keys(now_ms)
    r.decide(second, "after")
    r.close()


# --- order in flight --------------------------------------------------------------

@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("size", [6000, 700])
@pytest.mark.parametrize("pipeline", [False, True])
def test_order_in_flight(rl, profile, size, pipeline):
    """device API, no sync between the calls: decide, reset batch, decide,
    reset batch, decide (above and below the engine's single-workgroup cut of
    4096).  Each reset batch deletes keys the decide before it wrote and the
    decide after it uses again, at the window of that decide."""
    import torch
    configs = CONFIG_SETS["mixed"]
    nkeys = 200
    tr = random_trace(61 + profile, 3 * size, nkeys, configs, big_n=True)
    D = [tuple(None if x is None else x[j * size:(j + 1) * size] for x in tr) for j in range(3)]
    R = []
    for j in (1, 2):           # before decide j: a third of its requests' (key, ts), and some of the last decide's
        sel = np.arange(size) % 3 == 0
        rk = np.concatenate([D[j][0][sel], D[j - 1][0][-50:]])
        rt = np.concatenate([D[j][1][sel], D[j - 1][1][-50:]])
        R.append((rk, rt, (rk % np.uint64(len(configs))).astype(np.uint32)))
    r = Rig(rl, profile, configs, flags=rl.OPT_PIPELINE if pipeline else 0)
    dev = torch.device("cuda", 0)

    def dev_in(*arrs):
        return [torch.from_numpy(np.ascontiguousarray(x).view(np.int64) if x.dtype == np.uint64 else
                                 np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else
                                 np.ascontiguousarray(x)).to(dev) for x in arrs]

    ins = [dev_in(*d[:4]) for d in D]
    outs = [[torch.empty(size, dtype=torch.uint8, device=dev)] +
            [torch.empty(size, dtype=torch.int64, device=dev) for _ in range(3)] +
            [torch.empty(size, dtype=torch.float64, device=dev)] for _ in D]
    rin = [dev_in(*x) for x in R]
    rst = [torch.full((x[0].size,), 77, dtype=torch.uint8, device=dev) for x in R]
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def decide(j):
        i, o = ins[j], outs[j]
        r.eng.decide_device(size, i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), i[3].data_ptr(), None,
                            *[x.data_ptr() for x in o], stream)

    def reset(j):
        i = rin[j]
        r.eng.reset_batch_device(i[0].numel(), i[0].data_ptr(), i[1].data_ptr(), i[2].data_ptr(), rst[j].data_ptr(),
                                 stream)

    decide(0); reset(0); decide(1); reset(1); decide(2)
    torch.cuda.synchronize()
    assert r.eng.sync() == 0, r.eng.last_error()
    st = r.eng.stats()
    assert (st.batches, st.decisions) == (3, 3 * size)
    host = lambda o: rl.Decisions(*[x.cpu().numpy() for x in o])
    for j in range(3):
        if j:
            apply_resets(r.sim, *R[j - 1], len(configs), 0)
            assert (rst[j - 1].cpu().numpy() == RESET_DONE).all()
        assert_same(host(outs[j]), r.sim.decide(*D[j][:4]), configs, D[j][3], f"decide {j}")
    r.check_keys(int(tr[1][-1]) // 1_000_000)
    r.close()


# --- host against device ----------------------------------------------------------

def test_host_against_device(rl):
    """the same batch through rl_reset_batch (larger than max_batch: chunked)
    and through rl_reset_batch_device on a second engine"""
    import torch
    configs = CONFIG_SETS["mixed"]
    first = random_trace(23, 4000, 3000, configs)
    second = random_trace(24, 4000, 3000, configs)
    second = (second[0], second[1] + (first[1][-1] - T0), second[2], second[3], None)
    now_ms = int(first[1][-1]) // 1_000_000
    m = 3 * 4096 + 5
    rng = np.random.default_rng(2)
    rkey = rng.integers(0, 4000, m).astype(np.uint64)
    rkey[rkey % np.uint64(3) == 1] += np.uint64(1)        # keys = 1 mod 3 are never reset
    rts = first[1][rng.integers(0, 4000, m)]
    rcfg = (rkey % np.uint64(len(configs))).astype(np.uint32)
    rcfg[::100] = len(configs)
    a = Rig(rl, 0, configs, max_batch=1 << 12)
    b = Rig(rl, 0, configs, max_batch=1 << 12)
    a.decide(first)
    b.decide(first)
    gone = a.reset(rkey, rts, rcfg, now_ms, "host, chunked")
    assert len(gone) >= 10      # live keys; the snapshots below compare expired ones too
    dev = torch.device("cuda", 0)
    dk = torch.from_numpy(rkey.view(np.int64)).to(dev)
    dt = torch.from_numpy(rts).to(dev)
    dc = torch.from_numpy(rcfg.view(np.int32)).to(dev)
    ds = torch.zeros(m, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    b.eng.reset_batch_device(m, dk.data_ptr(), dt.data_ptr(), dc.data_ptr(), ds.data_ptr(),
                             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert b.eng.sync() == 0
    assert np.array_equal(ds.cpu().numpy(), expected_status(rkey, rcfg, len(configs)))
    assert engine_keys(rl, b.eng, now_ms) == engine_keys(rl, a.eng, now_ms)
    fa, fb = snap.parse(a.eng.snapshot(0)), snap.parse(b.eng.snapshot(0))
    for sec in ("tb", "win", "spill"):
        order = lambda x: x[np.argsort(x["key"], kind="stable")] if sec != "spill" else \
            x[np.lexsort((x["when"], x["cnt"], x["ws"], x["key"]))]
        assert order(fa[sec]).tobytes() == order(fb[sec]).tobytes(), sec
    apply_resets(b.sim, rkey, rts, rcfg, len(configs), now_ms)
    a.decide(second, "host engine, after")
    b.decide(second, "device engine, after")
    a.close()
    b.close()
