"""Resets through the coalescer: a run of adjacent reset submissions at the
queue head is one launch (rl_coalescer_reset and rl_coalescer_reset_batch
alike).  CPU: the host-backend seam over the C oracle; GPU: the engine."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import oracle
from reset_cases import INVALID, KEY_RESERVED, RESET_DONE, expected_status
from tracegen import CONFIG_SETS, T0, random_trace

CONFIGS = CONFIG_SETS["mixed"]
N = len(CONFIGS)
EINVAL = -22


def arr(p, n, ct):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))


def new_sim():
    sim = oracle.OracleSim(0)
    for a, L, W in CONFIGS:
        sim.add_config(a, L, W)
    return sim


class Store:
    """the host backend over one C oracle; `gate` holds the batch function"""

    def __init__(self):
        self.sim = new_sim()
        self.gate = threading.Event()
        self.gate.set()
        self.entered = threading.Event()
        self.log = []

    def batch(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        self.entered.set()
        self.gate.wait()
        d, r, ra, rs, _ = self.sim.decide(arr(key, m, C.c_uint64).copy(), arr(ts, m, C.c_int64).copy(),
                                          arr(n, m, C.c_int64).copy(), arr(cfg, m, C.c_uint32).copy())
        arr(dec, m, C.c_uint8)[:], arr(rem, m, C.c_int64)[:] = d, r
        arr(retry, m, C.c_int64)[:], arr(reset, m, C.c_int64)[:] = ra, rs
        self.log.append(("batch", m))
        return 0

    def reset(self, user, cfg, key, ts):
        self.log.append(("reset", 1))
        if cfg >= N or key == KEY_RESERVED:
            return EINVAL
        self.sim.reset(cfg, key, ts)
        return 0

    def reset_batch(self, user, m, key, ts, cfg, status):
        k, t, c = arr(key, m, C.c_uint64), arr(ts, m, C.c_int64), arr(cfg, m, C.c_uint32)
        st = expected_status(k, c, N)
        for i in range(m):
            if st[i] == RESET_DONE:
                self.sim.reset(int(c[i]), int(k[i]), int(t[i]))
        arr(status, m, C.c_uint8)[:] = st
        self.log.append(("reset_batch", m))
        return 0


def traces():
    tr = random_trace(7, 1200, 300, CONFIGS)
    cut = lambda a, b: tuple(x[a:b] for x in tr[:4])
    return cut(0, 800), cut(800, 801), cut(801, 1200)


def held_resets(rl, with_batch_fn, K=200, bad=None):
    """warm up, hold one decide in the backend, queue K single resets behind
    it from K threads, release -> (store, coalescer stats before / after,
    reset return codes, the decisions after, the reference's decisions)"""
    warm, held, after = traces()
    store = Store()
    co = rl.Coalescer(store.batch, max_batch=4096, max_in_flight=1, reset=store.reset,
                      reset_batch=store.reset_batch if with_batch_fn else None)
    t = co.submit(*warm)
    assert co.wait(t, warm[0].size)[0] == 0
    st0 = co.stats()
    store.gate.clear()
    store.entered.clear()
    th = co.submit(*held)
    store.entered.wait()              # the submitter thread is inside the backend now
    rk = warm[0][-K:].copy()
    rt = warm[1][-K:]
    rc_ = (rk % np.uint64(N)).astype(np.uint32)
    if bad is not None:
        rc_[bad] = N
    rcs = [None] * K

    def one(i):
        rcs[i] = co.reset(int(rk[i]), int(rt[i]), int(rc_[i]))

    ths = [threading.Thread(target=one, args=(i,)) for i in range(K)]
    for x in ths:
        x.start()
    while co.stats().pending < K:     # every reset is queued behind the held batch
        time.sleep(0.0005)
    assert co.stats().reset_launches == st0.reset_launches
    store.gate.set()
    for x in ths:
        x.join()
    assert co.wait(th, 1)[0] == 0
    st1 = co.stats()
    t = co.submit(*after)
    rc, got = co.wait(t, after[0].size)
    assert rc == 0
    co.close()
    ref = new_sim()
    ref.decide(*warm)
    ref.decide(*held)
    for i in range(K):
        if rc_[i] < N:
            ref.reset(int(rc_[i]), int(rk[i]), int(rt[i]))
    want = ref.decide(*after)
    return store, st0, st1, rcs, got, want


def same(got, want):
    return all(np.array_equal(got[i], want[i]) for i in range(4))


def test_queued_single_resets_are_one_launch(rl):
    store, st0, st1, rcs, got, want = held_resets(rl, True)
    assert rcs == [0] * 200
    assert st1.reset_launches - st0.reset_launches == 1
    assert st1.resets - st0.resets == 200
    assert ("reset_batch", 200) in store.log and not any(w == "reset" for w, _ in store.log)
    # resets are no requests
    assert (st1.submitted, st1.decided) == (st0.submitted + 1, st0.decided + 1)
    assert same(got, want)


def test_per_key_fallback_without_reset_batch(rl):
    store, st0, st1, rcs, got, want = held_resets(rl, False)
    assert rcs == [0] * 200
    assert st1.reset_launches - st0.reset_launches == 1 and st1.resets - st0.resets == 200
    assert sum(1 for w, _ in store.log if w == "reset") == 200
    assert same(got, want)


@pytest.mark.parametrize("with_batch_fn", [True, False])
def test_invalid_reset_in_a_merged_run(rl, with_batch_fn):
    store, st0, st1, rcs, got, want = held_resets(rl, with_batch_fn, bad=77)
    assert rcs == [0] * 77 + [rl.RL_EINVAL] + [0] * 122
    assert st1.reset_launches - st0.reset_launches == 1 and st1.resets - st0.resets == 199
    assert same(got, want)


def test_reset_batch_submission(rl):
    """one submission, statuses, and one larger than max_batch split across launches"""
    warm, held, after = traces()
    store = Store()
    co = rl.Coalescer(store.batch, max_batch=64, reset=store.reset, reset_batch=store.reset_batch)
    t = co.submit(*warm)
    assert co.wait(t, warm[0].size)[0] == 0
    rk = warm[0][-150:].copy()
    rt = warm[1][-150:]
    rc_ = (rk % np.uint64(N)).astype(np.uint32)
    rc_[5], rk[9] = N + 63, np.uint64(KEY_RESERVED)
    rc, status = co.reset_batch(rk, rt, rc_)
    assert rc == 0 and np.array_equal(status, expected_status(rk, rc_, N))
    assert list(status[[5, 9]]) == [INVALID, INVALID]
    st = co.stats()
    assert (st.resets, st.reset_launches) == (148, 3)
    assert [x for x in store.log if x[0] != "batch"] == [("reset_batch", 64), ("reset_batch", 64), ("reset_batch", 22)]
    rc, none = co.reset_batch(rk[:0], rt[:0], rc_[:0])
    assert rc == 0 and none.size == 0 and co.stats().reset_launches == 3
    t = co.submit(*after)
    rc, got = co.wait(t, after[0].size)
    co.close()
    ref = new_sim()
    ref.decide(*warm)
    for i in range(150):
        if status[i] == RESET_DONE:
            ref.reset(int(rc_[i]), int(rk[i]), int(rt[i]))
    assert same(got, ref.decide(*after))


def test_old_struct_sizes_still_work(rl):
    """a caller compiled before `reset_batch`, `resets` and `reset_launches`
    existed passes the shorter structs"""
    store = Store()
    keep = (rl.BATCH_FN(store.batch), rl.RESET_FN(store.reset), rl.RESET_BATCH_FN(store.reset_batch))
    b = rl.rl_coalescer_backend(batch=keep[0], reset=keep[1], table_info=C.cast(None, rl.INFO_FN),
                                gc=C.cast(None, rl.GC_FN), user=None, peek=C.cast(None, rl.BATCH_FN),
                                reset_batch=keep[2])
    b.struct_size = rl.rl_coalescer_backend.reset_batch.offset
    o = rl.rl_coalescer_opts(max_batch=16)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_host_backend(C.byref(b), C.byref(o), C.byref(h)) == 0
    assert rl.lib.rl_coalescer_reset(h, 5, T0, 0) == 0
    assert rl.lib.rl_coalescer_reset(h, 5, T0, N) == rl.RL_EINVAL
    # the field past the caller's struct is not read: the per-key path
    assert [w for w, _ in store.log] == ["reset", "reset"]
    st = rl.rl_coalescer_stats()
    st.struct_size = rl.rl_coalescer_stats.resets.offset
    st.resets = st.reset_launches = 12345
    assert rl.lib.rl_coalescer_get_stats(h, C.byref(st)) == 0
    assert (st.resets, st.reset_launches, st.struct_size) == (12345, 12345, rl.rl_coalescer_stats.resets.offset)
    full = rl.rl_coalescer_stats()
    assert rl.lib.rl_coalescer_get_stats(h, C.byref(full)) == 0
    assert (full.resets, full.reset_launches) == (1, 2)
    assert rl.lib.rl_coalescer_destroy(h) == 0


@pytest.mark.gpu
def test_gpu_decides_reset_batches_and_single_resets_from_threads(rl):
    """Threads interleave decide submissions, reset_batch calls and single
    resets, each on keys of its own (so a key's times stay in order however
    the threads interleave).  Every decision equals the oracle replay in ticket
    order, a thread's resets placed after the decide it made before them."""
    eng = rl.Engine(profile=0, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 12, flags=rl.OPT_PIPELINE)
    for a, L, W in CONFIGS:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=1 << 12)
    nthreads, rounds, m = 4, 30, 25
    trs = []
    for i in range(nthreads):
        k, ts, n, cfg, _ = random_trace(91 + i, rounds * m, 30, CONFIGS)
        trs.append((k + np.uint64(1500 * i), ts, n, cfg))      # 1500 keeps key % 15
    events, lock, errs = [], threading.Lock(), []

    def worker(i):
        rng = np.random.default_rng(i)
        for j in range(rounds):
            part = tuple(x[j * m:(j + 1) * m] for x in trs[i])
            t = co.submit(*part)
            rc, out = co.wait(t, m)
            mine = [("decide", part, out)]
            if rc != 0:
                errs.append(rc)
            # a reset batch of some of the keys just used (with a duplicate and an invalid request) ...
            sel = rng.integers(0, m, 8)
            rk, rt = part[0][sel].copy(), part[1][sel]
            rcfg = part[3][sel].copy()
            rcfg[0] = N
            rc, status = co.reset_batch(rk, rt, rcfg)
            if rc != 0 or not np.array_equal(status, expected_status(rk, rcfg, N)):
                errs.append(("reset_batch", rc))
            mine.append(("resets", (rk, rt, rcfg)))
            # ... and a single one
            q = int(rng.integers(0, m))
            if co.reset(int(part[0][q]), int(part[1][q]), int(part[3][q])) != 0:
                errs.append("reset")
            mine.append(("resets", (part[0][q:q + 1], part[1][q:q + 1], part[3][q:q + 1])))
            with lock:
                events.extend((t, i, s, e) for s, e in enumerate(mine))

    ths = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    st = co.stats()
    co.close()
    assert not errs
    assert eng.sync() == 0
    eng.close()
    assert st.submitted == st.decided == nthreads * rounds * m
    assert st.resets == nthreads * rounds * 8 and 0 < st.reset_launches <= nthreads * rounds * 2
    sim = new_sim()
    for t, i, s, (what, *rest) in sorted(events, key=lambda e: e[:3]):
        if what == "resets":
            rk, rt, rcfg = rest[0]
            for a in range(rk.size):
                if rcfg[a] < N:
                    sim.reset(int(rcfg[a]), int(rk[a]), int(rt[a]))
            continue
        part, out = rest
        dec, rem, retry, reset, _ = sim.decide(*part)
        for name, a, b in zip(("decision", "remaining", "retry", "reset_at"), out, (dec, rem, retry, reset)):
            assert np.array_equal(a, b), f"ticket {t}: {name}"
