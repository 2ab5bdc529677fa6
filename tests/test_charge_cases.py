"""Charge's expectation on the Python oracle (charge_cases.py): the builder's
coverage on both profiles, the single-time-stamp bound on a directed case, and
the equivalence of a one-request call with Peek + AllowN."""
import copy

import numpy as np
import pytest

from charge_cases import KINDS, apply_charge, charge_case
from oracle import rl_oracle_py as po
from refund_cases import new_sim, py_peek
from reset_cases import KEY_RESERVED
from tracegen import CONFIG_SETS, NS, T0


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_builder_coverage(kind, profile):
    """the seeds meet the counts the builder asserts, on the oracle alone"""
    configs, first, (key, ts, n, cfg, sms), second, now_ms, cover = charge_case(kind, profile)
    assert (sms is None) == (kind == "tb")
    rows = cover["rows"]
    assert len(rows) == key.size
    for (dec, got, rem, reset, tok), nn, c in zip(rows, n.tolist(), cover["cls"].tolist()):
        assert 0 <= got <= max(nn, 0)
        if c == "full":
            assert (dec, got) == (po.ALLOWED, nn)
        elif c in ("short", "empty", "dup_denied"):
            assert dec == po.DENIED and got < nn
        elif c == "over":
            assert (dec, got, rem) == (po.DENIED, nn, 0)
        elif c == "invalid":
            assert (dec, got, rem, reset, tok) == (po.INVALID, 0, 0, 0, 0.0)
    # the clocks never go back from the warm-up through the call to the trace that follows
    clock = lambda tr: tr[4] if tr[4] is not None else tr[1] // 1_000_000
    c0, c1, c2 = clock(first), clock((key, ts, n, cfg, sms)), clock(second)
    assert c0[-1] <= c1[0] and (np.diff(c1) >= 0).all() and c1[-1] <= c2[0]
    assert first[1][-1] < ts[0] and ts[-1] < second[1][0]


def test_single_time_stamp_bound():
    """one time stamp, buckets asked many times: a bucket that refused any ask
    (charged < n) ends with fewer whole tokens than that ask, and the tokens
    taken are the sum of `charged`"""
    configs = [(1, 20, 12 * NS), (1, 5, 60 * NS), (1, 1000, 3600 * NS)]
    rng = np.random.default_rng(11)
    m = 400
    key = rng.integers(0, 12, m).astype(np.uint64)
    cfg = (key % np.uint64(3)).astype(np.uint32)
    n = rng.choice([1, 2, 3, 7, 30, 400], m).astype(np.int64)
    t = T0 + 5 * NS
    for profile in (0, 1):
        sim = new_sim(profile, configs)
        for k in range(12):                       # buckets part empty before the call
            sim.decide(k, T0, 1 + k % 4, k % 3)
        before = {k: py_peek(sim, k, t, k % 3, t // 1_000_000)[4] for k in range(12)}
        rows, info = apply_charge(sim, key, np.full(m, t), n, cfg)
        refused = 0
        for k in range(12):
            left = py_peek(sim, k, t, k % 3, t // 1_000_000)
            idx = np.nonzero(key == np.uint64(k))[0]
            took = sum(rows[i][1] for i in idx)
            assert abs(before[k] - took - left[4]) < 1e-6
            for i in idx:
                if rows[i][1] < n[i]:
                    refused += 1
                    assert rows[i][0] == po.DENIED and left[1] < n[i], (k, i)
        assert refused > 100 and (info["cls"] == "dup_denied").sum() > 20 and (info["cls"] == "short").sum() >= 3


@pytest.mark.parametrize("kind", KINDS)
def test_one_request_is_peek_then_allow(kind):
    """a call of one request is Peek(key, 0) and AllowN(key, min(n, r)) for a
    bucket, AllowN(key, n) for a window"""
    configs = CONFIG_SETS[kind]
    sim = new_sim(0, configs)
    rng = np.random.default_rng(5)
    t = T0
    seen = set()
    for step in range(1500):
        t += int(rng.choice([1000, 5_000_000, 200_000_000]))
        k = int(rng.integers(0, 40))
        c = k % len(configs)
        nn = int(rng.choice([1, 2, 7, 50, 0, -1, 1 << 62]))
        if step % 97 == 0:
            k = KEY_RESERVED
        ref = copy.deepcopy(sim)
        rows, info = apply_charge(sim, [k], [t], [nn], [c])
        row = rows[0]
        if nn <= 0 or k == KEY_RESERVED:
            want = (po.INVALID, 0, 0, 0, 0.0)
        elif configs[c][0] == po.TOKEN_BUCKET:
            peek = py_peek(ref, k, t, c, t // 1_000_000)
            take = min(nn, peek[1])
            if take == 0:
                want = (po.DENIED, 0, 0, peek[3], peek[4])
            else:
                d = ref.decide(k, t, take, c)
                assert d[0] == po.ALLOWED         # Peek's parity with AllowN: exact for a bucket asked once
                want = (po.ALLOWED if take == nn else po.DENIED, take, d[1], d[3], d[4])
        else:
            d = ref.decide(k, t, nn, c)
            want = (d[0], nn if d[0] <= po.ALLOWED else 0, d[1], d[3], 0.0)
        assert row == want, (step, row, want)
        assert sim.db == ref.db
        seen.add(info["cls"][0])
    assert {"full", "invalid"} <= seen and ("short" in seen or "over" in seen)
