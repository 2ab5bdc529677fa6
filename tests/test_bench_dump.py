"""A plain `bench.py` run (GPU): the line it prints, and `--dump-outputs`.

One run with more steps than the 64-batch trace pool, so the last timed step is
a replayed pool batch moved one pass later in time.  The dumped arrays are what
that step returned; the CPU oracle decides the same 72 batches and must agree
bit for bit (the arrays are float32 / float64, which hold every value here
exactly: see bench.py's docstring)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = 64


def test_plain_run_line_and_dumped_outputs(tmp_path, oracle_mod):
    import traces
    steps, warmup, m = 70, 2, 20_000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--batch", str(m), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stderr.decode()[-3000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["n_gpus"] == 1
    assert d["unit"] == "decisions/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(m / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert d["roofline"]["launches_timed"] > 0
    # what takes work of its own is behind --full
    for k in ("latency", "stages_ms_per_batch", "cpu_baseline", "secondary"):
        assert k not in d

    gen = traces.TokenBucketZipf(batch=m, seed=3)
    pool = [gen.next_batch() for _ in range(POOL)]
    span = gen.t - traces.T0
    sim = oracle_mod.OracleSim(oracle_mod.REDIS7)
    for a, L, W in gen.configs:
        sim.add_config(a, L, W)
    for b in range(warmup + steps):
        key, ts, n, cfg = pool[b % POOL]
        dec, rem, retry, reset, tok = sim.decide(key, ts + (b // POOL) * span, n, cfg)
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["decision", "remaining", "reset_at_ns_minus_t0", "retry_after_ns", "tokens"]
    assert got["decision"].dtype == np.float32 and all(got[k].dtype == np.float64 for k in got if k != "decision")
    assert all(a.shape == (m,) for a in got.values())
    assert 0 < int((dec == 1).sum()) < m
    assert np.array_equal(got["decision"], dec.astype(np.float32))
    assert np.array_equal(got["remaining"], rem.astype(np.float64))
    assert np.array_equal(got["retry_after_ns"], retry.astype(np.float64))
    assert np.array_equal(got["reset_at_ns_minus_t0"], (reset - traces.T0).astype(np.float64))
    assert np.array_equal(got["tokens"].view(np.uint64), tok.view(np.uint64))
