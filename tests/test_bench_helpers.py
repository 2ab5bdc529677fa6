"""bench.py's host-side arithmetic (CPU): the hot-owner bound the N > 1 line
reports, and the replay-timeline words it reads back (10-ns realtime ticks,
low 32 bits, so every difference must survive a wrap of the counter)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_hot_owner_bound_is_batch_over_chain_time(bench):
    # chain rate / hot share = (hot / t) / (hot / m) = m / t, whatever the share
    for hot, us, m in ((123847, 290.0, 1_000_000), (247051, 538.36, 2_000_000), (1, 0.5, 10)):
        b = bench.hot_owner_bound(hot, us, m)
        assert b["bound_decisions_per_s"] == pytest.approx(m / (us * 1e-6), rel=1e-12)
        assert b["hot_share"] == pytest.approx(hot / m)
        assert b["chain_steps_per_s"] == pytest.approx(hot / (us * 1e-6))
        assert b["hot_key_requests_per_step"] == hot


@pytest.mark.parametrize("hot,us", [(0, 10.0), (100, 0.0), (-1, 5.0)])
def test_hot_owner_bound_absent_without_a_chain(bench, hot, us):
    assert bench.hot_owner_bound(hot, us, 1000) is None


def test_steps_past_the_pool_replay_it_later_in_time(bench):
    # 3 pool batches, 8 steps, 2 batches after the timed region: step b is pool
    # batch b mod 3, b // 3 spans later; the tail moves by the last step's shift
    import numpy as np
    import torch
    m, span = 5, 1000
    dev = torch.device("cpu")
    mk = lambda i: (torch.full((m,), i), torch.arange(m) + 300 * i + 1, torch.ones(m, dtype=torch.int64),
                    torch.zeros(m, dtype=torch.int32))
    batches = [mk(i) for i in range(5)]
    before = [t.clone() for _, t, _, _ in batches]
    steps = bench.resident_steps(batches, 3, 8, span, dev)
    assert len(steps) == 10
    for b, (k, t, n, c) in enumerate(steps[:8]):
        assert k is batches[b % 3][0] and n is batches[b % 3][2] and c is batches[b % 3][3]
        assert torch.equal(t, before[b % 3] + (b // 3) * span)
    for i in (3, 4):
        assert steps[5 + i][0] is batches[i][0] and torch.equal(steps[5 + i][1], before[i] + 2 * span)
    ts = np.concatenate([t.numpy() for _, t, _, _ in steps])
    assert np.all(np.diff(ts) > 0)                                      # time never goes backwards
    assert all(torch.equal(t, t0) for (_, t, _, _), t0 in zip(batches, before))   # the pool itself is untouched
    # a run inside the pool is the trace as generated
    assert all(a is b for x, y in zip(bench.resident_steps(batches, 3, 3, span, dev), batches[:3] + batches[3:])
               for a, b in zip(x, y))


def test_dump_outputs_float_arrays_under_the_size_cap(bench, tmp_path, monkeypatch):
    import numpy as np
    import torch
    m = 1000
    arrays = {"decision": (torch.arange(m) % 2).to(torch.uint8), "remaining": torch.arange(m) - 3,
              "tokens": torch.arange(m, dtype=torch.float64) / 7}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = {f: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["decision.npy", "remaining.npy", "tokens.npy"]
    assert got["decision.npy"].dtype == np.float32 and got["remaining.npy"].dtype == np.float64
    assert all(np.array_equal(got[k + ".npy"], v.numpy().astype(got[k + ".npy"].dtype)) for k, v in arrays.items())
    # too large for the cap: the same seeded sample of rows on every call
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 2800)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    s1 = {f: np.load(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")}
    s2 = {f: np.load(tmp_path / "s2" / f) for f in os.listdir(tmp_path / "s2")}
    assert sorted(s1) == ["decision.npy", "remaining.npy", "sample_index.npy", "tokens.npy"]
    assert sum(a.nbytes for a in s1.values()) <= 2800 and all(np.array_equal(s1[k], s2[k]) for k in s1)
    idx = s1["sample_index.npy"].astype(np.int64)
    assert idx.size == 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(s1["tokens.npy"], arrays["tokens"].numpy()[idx])


@pytest.mark.parametrize("start", [0, 12345, 0xffffffff - 500, 0xffffffff])
def test_timeline_words_wrap(bench, start):
    dbgw = [0] * 96
    dbgw[13] = ~start & 0xffffffff               # the kernel keeps the first block's start complemented
    dbgw[16] = (start + 264) & 0xffffffff        # hot segment start, 2.64 us in
    dbgw[17] = (start + 29368) & 0xffffffff      # hot segment end, 293.68 us in
    dbgw[51] = (start + 239) & 0xffffffff        # a stamps-build word
    assert bench.hot_chain_us(dbgw) == pytest.approx(291.04)
    assert bench._rel_us(dbgw, 51) == pytest.approx(2.39)
    assert bench._rel_us(dbgw, 52) is None       # unset: a product build
