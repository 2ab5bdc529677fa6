"""rl_coalescer_tally: over a host backend (CPU; the C oracle behind the test
seam, the coalescer's own host tally) and, GPU-marked, over the engine."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import oracle
from table_cases import keys_with_home
from tally_cases import check_read, expected_tally, fits, host_table
from tracegen import NS, T0

CONFIGS = [(1, 5, 60 * NS), (2, 4, 60 * NS), (3, 3, 60 * NS)]
U64 = np.uint64


def wait_for(cond, what, seconds=30.0):
    """poll until cond(); a regression fails here instead of hanging the suite"""
    end = time.monotonic() + seconds
    while not cond():
        assert time.monotonic() < end, f"timed out waiting for {what}"


def arr(p, n, dtype):
    """the backend's view of a C array argument"""
    ct = {np.uint64: C.c_uint64, np.int64: C.c_int64, np.uint32: C.c_uint32, np.uint8: C.c_uint8}[dtype]
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))


class OracleBackend:
    """rl_batch_fn over the C oracle; `log` keeps every batch's (key, cfg, n,
    decision) in the order the coalescer launched them; `gate` (an Event),
    when set up, holds the first batch inside the backend"""

    def __init__(self, gate=None):
        self.sim = oracle.OracleSim(oracle.REDIS7)
        for a, L, W in CONFIGS:
            self.sim.add_config(a, L, W)
        self.log, self.gate, self.entered = [], gate, threading.Event()

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

    def expected(self, first=0, last=None, ncfg=len(CONFIGS)):
        parts = self.log[first:last]
        return expected_tally(*[np.concatenate([p[j] for p in parts]) for j in range(4)], ncfg)


def reqs(keys, n, cfgs=None, t=T0):
    keys = np.asarray(keys, U64)
    cfgs = (keys % U64(3)).astype(np.uint32) if cfgs is None else np.asarray(cfgs, np.uint32)
    return keys, np.full(keys.size, t, np.int64), np.full(keys.size, n, np.int64), cfgs


def test_tally_between_two_submissions_counts_the_first_only(rl):
    """A is held inside the backend while the tally and then B are queued
    behind it: the tally runs between them in sequence order"""
    gate = threading.Event()
    be = OracleBackend(gate)
    co = rl.Coalescer(be.batch, max_batch=64, max_in_flight=1, tally_key_slots=1024)
    ta = co.submit(*reqs(np.arange(12) % 4, 2))            # each key three times: 2 + 2 + 2 against limits 5, 4, 3
    assert be.entered.wait(30)
    got = []
    th = threading.Thread(target=lambda: got.append(co.tally(top=16)))
    th.start()
    wait_for(lambda: co.stats().pending >= 1, "the tally to be queued")
    tb = co.submit(*reqs(np.arange(12) % 4, 2, t=T0 + 1))
    gate.set()
    th.join(30)
    rc, t = got[0]
    assert rc == 0 and co.wait(ta, 12)[0] == 0 and co.wait(tb, 12)[0] == 0
    assert len(be.log) == 2
    e = be.expected(0, 1)
    assert e.denied > 0 and int(e.count[:, 1].sum()) > 0
    check_read(t, e, 3, "between")
    assert (t.info.batches, t.info.requests, t.info.key_slots) == (1, 12, 1024)
    rc, t = co.tally(top=16)
    check_read(t, be.expected(), 3, "both")
    assert (t.info.batches, t.info.requests) == (2, 24)
    co.close()


def test_eight_threads_and_dropped_requests(rl):
    """concurrent submissions, some with a deadline already past and some
    cancelled while the first batch is held: what was dropped unapplied is not
    counted, everything else is, once"""
    gate = threading.Event()
    be = OracleBackend(gate)
    co = rl.Coalescer(be.batch, max_batch=32, max_in_flight=2, tally_key_slots=1024)
    first = co.submit(*reqs([0, 1, 2], 1))        # a decided request of every config: all three are known
    assert be.entered.wait(30)
    errs = []

    def worker(i):
        rng = np.random.default_rng(i)
        tickets = []
        for j in range(40):
            m = int(rng.integers(1, 6))
            keys = rng.integers(0, 40, m).astype(U64)
            cfgs = (keys % U64(3)).astype(np.uint32)
            cfgs[rng.random(m) < 0.1] = 7                                  # unknown config
            n = rng.choice([1, 2, 0, 1 << 62], m).astype(np.int64)
            dl = 1 if j % 10 == 3 else 0                                   # a deadline long past
            t = co.submit(keys, np.full(m, T0 + j, np.int64), n, cfgs, deadline_ns=dl)
            if j % 10 == 7:
                co.cancel(t)
            tickets.append((t, m))
        for t, m in tickets:
            rc, _ = co.wait(t, m)
            if rc not in (0, rl.RL_EDEADLINE, rl.RL_ECANCELED):
                errs.append(rc)

    th = [threading.Thread(target=worker, args=(i,)) for i in range(8)]
    for x in th:
        x.start()
    wait_for(lambda: co.stats().submitted >= 200, "200 submitted requests")
    gate.set()
    for x in th:
        x.join(60)
    assert not errs and co.wait(first, 3)[0] == 0
    st = co.stats()
    assert st.expired > 0 and st.cancelled > 0 and st.pending == 0
    rc, t = co.tally(top=64)
    assert rc == 0
    total = int(t.cfg["count"].sum()) + t.info.unknown_cfg + t.info.bad_codes
    assert total == st.submitted - st.expired - st.cancelled == st.decided == t.info.requests
    assert t.info.batches == st.batches == len(be.log)
    e = be.expected()
    assert fits(list(e.keys), 1024) and e.unknown_cfg > 0
    check_read(t, e, 3, "threads")
    co.close()


def test_off_is_einval_and_old_opts_size(rl):
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=16)
    rc, t = co.tally()
    assert rc == rl.RL_EINVAL and t is None
    assert co.decide(1, T0, 1, 1)[0] == 0                  # goes on working
    co.close()
    # a caller compiled before tally_key_slots passes the shorter struct: off
    fn = rl.BATCH_FN(be.batch)
    o = rl.rl_coalescer_opts(max_batch=16, tally_key_slots=64)
    o.struct_size = rl.rl_coalescer_opts.tally_key_slots.offset
    h = C.c_void_p()
    assert rl.lib.rl_coalescer_create_with_backend(fn, None, C.byref(o), C.byref(h)) == 0
    assert rl.lib.rl_coalescer_tally(h, None, 0, None, None, 0, None, None, 0) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_destroy(h) == 0
    o.struct_size = 60
    assert rl.lib.rl_coalescer_create_with_backend(fn, None, C.byref(o), C.byref(h)) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_tally(None, None, 0, None, None, 0, None, None, 0) == rl.RL_EINVAL
    with pytest.raises(rl.EngineError):
        rl.Coalescer(be.batch, tally_key_slots=(1 << 24) + 1)


def test_fewer_rows_than_configs(rl):
    """a read with room for fewer rows than there are configs returns those
    rows and the config count's worth of nothing else: no error, also with clear"""
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=16, tally_key_slots=16)
    for k in (0, 1, 2):
        assert co.decide(k, T0, 1, k)[0] == 0
    rc, t = co.tally(top=4, clear=True, max_configs=2)
    assert rc == 0 and t.cfg.size == 2 and t.cfg["count"][:, 1].tolist() == [1, 1] and t.info.requests == 3
    rc, t = co.tally(max_configs=8)
    assert rc == 0 and t.cfg.size == 3 and not t.cfg["count"].any()
    co.close()


def test_host_key_table_and_clear(rl):
    """16 records: eight keys of one home slot are all tracked; of 40 keys that
    come one at a time, exactly those the sequential table rule admits"""
    be = OracleBackend()
    co = rl.Coalescer(be.batch, max_batch=1, tally_key_slots=16)     # max_batch 1: the arrival order is the tally's
    for k in keys_with_home(15, 9, 8, start=3 << 20).tolist():
        for j in range(2):
            assert co.decide(k, T0 + j, 3, k % 3)[0] == 0            # n = 3 against limits 5, 4, 3: allowed, then denied
    rc, t = co.tally(top=16, clear=True)
    e = be.expected()
    assert rc == 0 and len(e.keys) == 8 and fits(list(e.keys), 16)
    check_read(t, e, 3, "one home slot")
    rc, z = co.tally(top=16)
    assert rc == 0 and not z.cfg["count"].any() and z.keys_tracked == 0 and z.cfg.size == 3
    assert (z.info.requests, z.info.batches, z.info.untracked_requests) == (0, 0, 0)
    mark = len(be.log)
    order = (np.arange(40, dtype=U64) * U64(7919) + U64(5 << 20)).tolist()
    for k in order:
        assert co.decide(k, T0 + 5, 9, k % 3)[0] == 0                # n = 9 > every limit: denied
    rc, t = co.tally(top=64)
    e = be.expected(mark)
    assert rc == 0 and e.denied == 40
    want = host_table(order, 16)
    assert len(want) == 16 and {int(k) for k in t.keys["key_id"]} == want and t.keys_tracked == 16
    assert (t.info.untracked_requests, t.info.untracked_units) == (24, 24 * 9)
    assert np.array_equal(t.cfg["count"], e.count) and np.array_equal(t.cfg["units"], e.units)
    co.close()


@pytest.mark.gpu
@pytest.mark.parametrize("profile", [0, 1])
def test_over_the_engine(rl, profile):
    """the same over the GPU engine.  A is submitted, a thread calls the tally,
    B is submitted.  Tickets are sequence numbers and the tally takes one, so
    they tell where the tally was sequenced: tb == ta + |A| + 1 means between A
    and B, and then it must have counted A and nothing of B; tb == ta + |A|
    means behind B, and then it must have counted both.  Rounds repeat (a few
    ms each) until one has the tally in between; A is below the coalescer's
    zero-copy cut, B above it.  Getting the tally in between rests on timing (a
    0.5 ms spin after the reading thread starts, twelve rounds): on a machine
    loaded enough to delay that thread every time, the test fails with "never
    sequenced between" without a fault in the code -- no round can pass with a
    wrong count."""
    from tracegen import CONFIG_SETS, random_trace
    configs = CONFIG_SETS["mixed"]
    eng = rl.Engine(profile=profile, tb_capacity=1 << 12, win_capacity=1 << 12, max_batch=1 << 17,
                    flags=rl.OPT_PIPELINE)
    for a, L, W in configs:
        eng.register(a, L, W)
    co = rl.Coalescer(eng, max_batch=1 << 17, tally_key_slots=4096)
    cut, total, between = 5000, 80_000, False
    for rnd in range(12):
        key, ts, n, cfg, _ = random_trace(71 + profile + 10 * rnd, total, 300, configs, big_n=True)
        cfg = cfg.copy()
        cfg[::53] = len(configs) + 2
        ta = co.submit(key[:cut], ts[:cut], n[:cut], cfg[:cut])
        got, started = [], threading.Event()

        def read():
            started.set()
            got.append(co.tally(top=400))
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
        rc, t1 = got[0]
        assert rc == 0 and tb in (ta + cut, ta + cut + 1)
        if tb == ta + cut + 1:
            between = True
            assert t1.info.requests == cut
            check_read(t1, expected_tally(key[:cut], cfg[:cut], n[:cut], dec[:cut], len(configs)), len(configs), "A")
        else:
            assert t1.info.requests == total
            check_read(t1, expected_tally(key, cfg, n, dec, len(configs)), len(configs), "A + B, tally behind")
        rc, t = co.tally(top=400, clear=True)
        assert rc == 0 and t.info.requests == total
        check_read(t, expected_tally(key, cfg, n, dec, len(configs)), len(configs), "A + B")
        if between:
            break
    assert between, "the tally was never sequenced between the two submissions"
    # peeks and resets are not counted
    assert co.peek(key[:10], ts[:10], n[:10], cfg[:10])[0] == 0
    assert co.reset_batch(key[:10], ts[:10], cfg[:10])[0] == 0
    rc, z = co.tally(top=4)
    assert rc == 0 and z.info.requests == 0 and not z.cfg["count"].any() and z.keys_tracked == 0
    co.close()
    assert eng.stats().decisions == (rnd + 1) * total
    eng.close()
