"""rl_coalescer_hot: over a host backend (CPU; the C oracle behind the test seam,
the coalescer's own host sketch) and, GPU-marked, over the engine with the
tally on beside it.  The model is fed the backend's batches: one call each."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import hot_cases as H
import oracle
from tally_cases import check_read as check_tally
from tally_cases import expected_tally
from test_tally_coalescer import CONFIGS, arr, reqs, wait_for
from tracegen import T0

U64 = np.uint64
HOST_NCFG = 1 << 16      # the host rule: a config id is known once a request of it was decided


class Backend:
    """rl_batch_fn over the C oracle, with a peek and a batched reset that
    only answer; `log` keeps every decide batch's (key, cfg, n, decision) in
    launch order; `gate`, when given, holds the first batch inside the backend"""

    def __init__(self, gate=None):
        self.sim = oracle.OracleSim(oracle.REDIS7)
        for a, L, W in CONFIGS:
            self.sim.add_config(a, L, W)
        self.log, self.gate, self.entered = [], gate, threading.Event()
        self.peeks = self.resets = 0

    def batch(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        k, t, nn, c = arr(key, m, np.uint64), arr(ts, m, np.int64), arr(n, m, np.int64), arr(cfg, m, np.uint32)
        if self.gate is not None and not self.log:
            self.entered.set()
            self.gate.wait(30)
        out = self.sim.decide(k.copy(), t.copy(), nn.copy(), c.copy())
        arr(dec, m, np.uint8)[:], arr(rem, m, np.int64)[:] = out[0], out[1]
        arr(retry, m, np.int64)[:], arr(reset, m, np.int64)[:] = out[2], out[3]
        self.log.append((k.copy(), c.copy(), nn.copy(), np.asarray(out[0], np.uint8).copy()))
        return 0

    def peek(self, user, m, key, ts, n, cfg, dec, rem, retry, reset):
        self.peeks += m
        arr(dec, m, np.uint8)[:] = 1
        for a in (rem, retry, reset):
            arr(a, m, np.int64)[:] = 0
        return 0

    def reset_batch(self, user, m, key, ts, cfg, status):
        self.resets += m
        arr(status, m, np.uint8)[:] = 1
        return 0

    def model(self, first, last, width, hot_min, weight=H.REQUESTS):
        return H.model_of(self.log[first:last], width, hot_min, HOST_NCFG, weight)


def coalescer(rl, be, **kw):
    return rl.Coalescer(be.batch, peek=be.peek, reset_batch=be.reset_batch, **kw)


def test_hot_between_two_submissions_counts_the_first_only(rl):
    """A is held inside the backend while the read and then B are queued behind
    it: the read runs between them in sequence order"""
    gate = threading.Event()
    be = Backend(gate)
    co = coalescer(rl, be, max_batch=64, max_in_flight=1, hot_min=3, hot_width=1 << 10, hot_key_slots=64)
    ta = co.submit(*reqs(np.arange(12) % 4, 2))            # each key three times
    assert be.entered.wait(30)
    got = []
    th = threading.Thread(target=lambda: got.append(co.hot(top=16)))
    th.start()
    wait_for(lambda: co.stats().pending >= 1, "the read to be queued")
    tb = co.submit(*reqs(np.arange(12) % 4, 2, t=T0 + 1))
    gate.set()
    th.join(30)
    rc, h = got[0]
    assert rc == 0 and co.wait(ta, 12)[0] == 0 and co.wait(tb, 12)[0] == 0
    assert len(be.log) == 2
    mod = be.model(0, 1, 1 << 10, 3)
    assert len(mod.candidates) == 4 and mod.total == 12
    H.check_read(h, mod, "between")
    i = h.info
    assert (i.batches, i.requests, i.width, i.depth, i.key_slots, i.hot_min, i.weight) == (1, 12, 1 << 10, 4, 64, 3, 0)
    rc, h = co.hot(top=16)
    H.check_read(h, be.model(0, 2, 1 << 10, 3), "both")
    assert [int(e) for e in h.keys["estimate"]] == [6, 6, 6, 6]
    co.close()


@pytest.mark.parametrize("weight", [H.REQUESTS, H.UNITS])
def test_threads_reads_and_dropped_requests(rl, weight):
    """eight submitting threads, some submissions with a deadline already past
    and some cancelled while the first batch is held, peeks and resets in
    between, and a thread that reads all along, clearing every third time.
    A read reports how many batches it has counted since the last clear: it
    equals the model fed with exactly those batches of the backend's log.
    Before each read the reader decides a request of a key of its own and
    waits for it: that request was submitted before the read, so it is in it."""
    gate = threading.Event()
    be = Backend(gate)
    width, hot_min = 64, 12                       # 40 keys in 64 columns: collisions, false positives
    co = coalescer(rl, be, max_batch=32, max_in_flight=2, hot_min=hot_min, hot_width=width, hot_key_slots=1024,
                   hot_weight=weight)
    first = co.submit(*reqs([0, 1, 2], 1))
    assert be.entered.wait(30)
    errs, reads, stop = [], [], threading.Event()

    def worker(i):
        rng = np.random.default_rng(i)
        tickets = []
        for j in range(40):
            m = int(rng.integers(1, 6))
            keys = rng.integers(0, 40, m).astype(U64)
            cfgs = (keys % U64(3)).astype(np.uint32)
            cfgs[rng.random(m) < 0.1] = 7                                  # unknown config
            n = rng.choice([1, 2, 0, 3], m).astype(np.int64)
            dl = 1 if j % 10 == 3 else 0                                   # a deadline long past
            t = co.submit(keys, np.full(m, T0 + j, np.int64), n, cfgs, deadline_ns=dl)
            if j % 10 == 7:
                co.cancel(t)
            if j % 10 == 9:                                                # blocks while the first batch is held
                rc1, _ = co.peek(keys, np.full(m, T0 + j, np.int64), n, cfgs)
                rc2, _ = co.reset_batch(keys + U64(1000), np.full(m, T0 + j, np.int64), cfgs)
                if rc1 or rc2:
                    errs.append((rc1, rc2))
            tickets.append((t, m))
        for t, m in tickets:
            rc, _ = co.wait(t, m)
            if rc not in (0, rl.RL_EDEADLINE, rl.RL_ECANCELED):
                errs.append(rc)

    def reader():
        j = 0
        while not stop.is_set() or j < 4:
            mark = 5000 + j
            rc, _ = co.decide(mark, T0 + j, 1, mark % 3)
            rc2, h = co.hot(top=1024, clear=j % 3 == 2)
            if rc or rc2:
                errs.append((rc, rc2))
                return
            reads.append((mark, j % 3 == 2, h))
            j += 1

    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for x in th:
        x.start()
    wait_for(lambda: co.stats().submitted >= 150, "150 submitted requests")
    rd = threading.Thread(target=reader)
    rd.start()
    gate.set()
    for x in th:
        x.join(60)
    stop.set()
    rd.join(60)
    assert not errs and co.wait(first, 3)[0] == 0 and not rd.is_alive()
    st = co.stats()
    assert st.expired > 0 and st.cancelled > 0 and st.pending == 0 and be.peeks > 0 and be.resets > 0
    rc, last = co.hot(top=1024)
    assert rc == 0
    reads.append((None, False, last))
    assert len(reads) >= 5
    base, counted, fp = 0, 0, 0
    for mark, cleared, h in reads:
        b = h.info.batches
        mod = be.model(base, base + b, width, hot_min, weight)
        H.check_read(h, mod, f"read at batch {base + b}")
        fp += len(set(mod.candidates) - mod.true_hot())
        if mark is not None:
            assert any((p[0] == U64(mark)).any() for p in be.log[:base + b]), "a request submitted before the read"
        if cleared:
            base += b
            counted += h.info.requests
    # every decided request was counted or skipped once; nothing else was
    assert base + last.info.batches == len(be.log)
    assert counted + last.info.requests == st.decided == st.submitted - st.expired - st.cancelled
    assert not any(((p[0] >= U64(1000)) & (p[0] < U64(5000))).any() for p in be.log)     # no reset key reached a batch
    assert fp > 0, "no read held a false positive: the trace does not test the sketch's collisions"
    co.close()


def test_host_table_overflow_and_clear(rl):
    """16 records, 40 qualifying keys one batch at a time: dropped is set,
    tracked keys carry the model's estimates; a clear zeroes everything"""
    be = Backend()
    co = coalescer(rl, be, max_batch=8, hot_min=1, hot_width=16, hot_key_slots=16)
    keys = (np.arange(40, dtype=U64) * U64(7919) + U64(5 << 20))
    for k in keys.tolist():
        assert co.decide(k, T0, 1, k % 3)[0] == 0
    rc, h = co.hot(top=64, clear=True)
    mod = be.model(0, None, 16, 1)
    assert rc == 0 and len(mod.candidates) == 40 and h.info.dropped > 0 and h.keys_tracked == 16
    want = dict(mod.read())
    assert all(int(r["estimate"]) == want[int(r["key_id"])] for r in h.keys)
    assert (h.info.total, h.info.requests, h.info.batches) == (40, 40, len(be.log))
    rc, z = co.hot(top=64)
    i = z.info
    assert rc == 0 and z.keys.size == 0 and (i.keys_tracked, i.dropped, i.total, i.skipped, i.batches, i.requests) == \
        (0, 0, 0, 0, 0, 0)
    co.close()


def test_off_by_default_and_old_opts_size(rl):
    be = Backend()
    co = coalescer(rl, be, max_batch=16)
    rc, h = co.hot()
    assert rc == rl.RL_EINVAL and h is None
    assert co.decide(1, T0, 1, 1)[0] == 0                  # goes on working
    co.close()
    # a caller compiled before the options passes the shorter struct: off, whatever the bytes behind say
    fn = rl.BATCH_FN(be.batch)
    o = rl.rl_coalescer_opts_hot(max_batch=16, hot_min=5, hot_width=64)
    for size in (rl.rl_coalescer_opts_hot.hot_width.offset, C.sizeof(rl.rl_coalescer_opts),
                 rl.rl_coalescer_opts_hot.hot_min.offset):
        o.struct_size = size
        h = C.c_void_p()
        assert rl.lib.rl_coalescer_create_with_backend(fn, None, C.byref(o), C.byref(h)) == 0
        assert rl.lib.rl_coalescer_hot(h, None, 0, None, None, 0) == rl.RL_EINVAL
        assert rl.lib.rl_coalescer_destroy(h) == 0
    o.struct_size = C.sizeof(o)
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_backend(fn, None, C.byref(o), C.byref(h)) == 0
    info = rl.rl_hot_info()
    assert rl.lib.rl_coalescer_hot(h, None, 0, None, C.byref(info), 0) == 0 and (info.width, info.hot_min) == (64, 5)
    assert rl.lib.rl_coalescer_destroy(h) == 0
    o.struct_size = C.sizeof(o) + 8
    assert rl.lib.rl_coalescer_create_with_backend(fn, None, C.byref(o), C.byref(h)) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_hot(None, None, 0, None, None, 0) == rl.RL_EINVAL
    for kw in (dict(hot_min=1, hot_width=(1 << 24) + 1), dict(hot_min=1, hot_key_slots=(1 << 24) + 1),
               dict(hot_min=1, hot_weight=2)):
        with pytest.raises(rl.EngineError):
            coalescer(rl, be, **kw)


@pytest.mark.gpu
def test_over_the_engine(rl):
    """the same over the GPU engine, the tally on beside it.  A is submitted, a
    thread reads, B is submitted; tickets are sequence numbers and the read
    takes one, so they tell where it was sequenced (test_tally_coalescer).
    The read's batches tell how the coalescer cut A and B into launches: the
    model is fed the same calls."""
    from tracegen import CONFIG_SETS, random_trace
    configs = CONFIG_SETS["mixed"]
    eng = rl.Engine(tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 17, flags=rl.OPT_PIPELINE)
    for a, L, W in configs:
        eng.register(a, L, W)
    width, hot_min = 256, 290
    co = rl.Coalescer(eng, max_batch=1 << 17, tally_key_slots=4096, hot_min=hot_min, hot_width=width,
                      hot_key_slots=4096)
    cut, total, between = 5000, 80_000, False
    for rnd in range(12):
        key, ts, n, cfg, _ = random_trace(91 + 10 * rnd, total, 300, configs, big_n=True)
        cfg = cfg.copy()
        cfg[::53] = len(configs) + 2
        ta = co.submit(key[:cut], ts[:cut], n[:cut], cfg[:cut])
        got, started = [], threading.Event()

        def read():
            started.set()
            got.append(co.hot(top=4096))
        th = threading.Thread(target=read)
        th.start()
        assert started.wait(30)
        end = time.perf_counter() + 0.0005          # let the call reach the queue
        while time.perf_counter() < end:
            pass
        tb = co.submit(key[cut:], ts[cut:], n[cut:], cfg[cut:])
        th.join(60)
        assert not th.is_alive()
        rc, a = co.wait(ta, cut)
        assert rc == 0
        rc, b = co.wait(tb, total - cut)
        assert rc == 0
        dec = np.concatenate([a[0], b[0]])
        A = (key[:cut], cfg[:cut], n[:cut], dec[:cut])
        B = (key[cut:], cfg[cut:], n[cut:], dec[cut:])
        AB = (key, cfg, n, dec)
        rc, h1 = got[0]
        assert rc == 0 and tb in (ta + cut, ta + cut + 1)
        if tb == ta + cut + 1:
            between = True
            assert (h1.info.requests, h1.info.batches) == (cut, 1)
            H.check_read(h1, H.model_of([A], width, hot_min, len(configs)), "A")
        else:
            assert h1.info.requests == total and h1.info.batches in (1, 2)
            H.check_read(h1, H.model_of([AB] if h1.info.batches == 1 else [A, B], width, hot_min, len(configs)),
                         "A + B, read behind")
        rc, h = co.hot(top=4096, clear=True)
        assert rc == 0 and h.info.requests == total and h.info.batches in (1, 2)
        mod = H.model_of([AB] if h.info.batches == 1 else [A, B], width, hot_min, len(configs))
        assert len(set(mod.candidates) - mod.true_hot()) > 0 and mod.skipped > total // 53
        H.check_read(h, mod, "A + B")
        # the tally beside it counted the same batches
        rc, t = co.tally(top=400, clear=True)
        assert rc == 0 and t.info.requests == total
        check_tally(t, expected_tally(key, cfg, n, dec, len(configs)), len(configs), "tally beside")
        if between:
            break
    assert between, "the read was never sequenced between the two submissions"
    # peeks and resets are not counted
    assert co.peek(key[:10], ts[:10], n[:10], cfg[:10])[0] == 0
    assert co.reset_batch(key[:10], ts[:10], cfg[:10])[0] == 0
    rc, z = co.hot(top=4)
    assert rc == 0 and (z.info.requests, z.info.total, z.info.skipped, z.keys_tracked) == (0, 0, 0, 0)
    co.close()
    assert eng.stats().decisions == (rnd + 1) * total
    eng.close()
