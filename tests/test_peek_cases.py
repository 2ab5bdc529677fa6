"""tests/peek_cases.py checked against the Python oracle itself (CPU): the
helper changes nothing, equals a decide on a copy for n >= 1, and for n == 0
reports exactly the quota a decide could still take."""
import copy

import numpy as np
import pytest

from oracle import rl_oracle_py as po
from peek_cases import peek_expected, peek_one, sim_decide
from tracegen import CONFIG_SETS, NS, T0, random_trace, skewed_trace


def warm_sim(kind, profile, seed, m=2000, nkeys=24, ff=False, skew=False):
    configs = CONFIG_SETS[kind]
    sim = po.Sim(profile)
    for a, L, W in configs:
        sim.add_config(a, L, W)
    tr = skewed_trace(seed, m, nkeys, configs) if skew else random_trace(seed, m, nkeys, configs, fastforward=ff,
                                                                         big_n=True)
    sim_decide(sim, *tr)
    return sim, configs, tr


def probes(configs, tr, nkeys=24, extra=4):
    """(key, ts, cfg, server_ms) of every warmed key and a few unseen ones, at
    the trace's last time and a little later"""
    key, ts, n, cfg, sms = tr
    out = []
    for k in range(nkeys + extra):
        for dt in (0, 250_000_000, 3 * NS):
            t = int(ts[-1]) + dt
            s = None if sms is None else int(sms[-1]) + dt // 1_000_000
            out.append((k, t, k % len(configs), s))
    return out


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["tb", "sw", "fw", "mixed"])
def test_helper_changes_nothing_and_equals_decide_on_a_copy(kind, profile):
    sim, configs, tr = warm_sim(kind, profile, 5 + profile, ff=kind != "tb", skew=kind == "mixed")
    before = copy.deepcopy(sim.db)
    for k, t, c, s in probes(configs, tr):
        for n in (1, 2, 7, 1 << 62):
            got = peek_one(sim, k, t, n, c, s)
            want = copy.deepcopy(sim).decide(k, t, n, c, s)
            assert repr(got) == repr(want), (k, t, n, c, s)   # repr: nan tokens of the window rows compare equal
        peek_one(sim, k, t, 0, c, s)
    assert sim.db == before
    # invalid peeks
    assert peek_one(sim, 1, T0, -1, 0)[0] == po.INVALID
    assert peek_one(sim, 1, T0, 1, len(configs))[0] == po.INVALID
    assert peek_one(sim, (1 << 64) - 1, T0, 1, 0)[0] == po.INVALID
    assert sim.db == before


def check_status(sim, k, t, c, s):
    """peek n == 0: allowed for a token bucket; `remaining` is the largest n'
    a decide on a copy allows, and n' + 1 is denied"""
    dec, rem, retry, reset, tok = peek_one(sim, k, t, 0, c, s)
    alg, L, W = sim.cfgs[c]
    if alg == po.TOKEN_BUCKET:
        assert dec == po.ALLOWED and retry == 0
    assert 0 <= rem <= L
    if rem >= 1:
        assert copy.deepcopy(sim).decide(k, t, rem, c, s)[0] == po.ALLOWED, (k, t, c, rem)
    assert copy.deepcopy(sim).decide(k, t, rem + 1, c, s)[0] == po.DENIED, (k, t, c, rem)
    # the same reset time as a request that runs
    assert reset == copy.deepcopy(sim).decide(k, t, 1, c, s)[3]


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", ["tb", "fw"])
def test_status_query_is_what_is_left(kind, profile):
    sim, configs, tr = warm_sim(kind, profile, 21 + profile, ff=kind == "fw")
    seen = set()
    for k, t, c, s in probes(configs, tr):
        check_status(sim, k, t, c, s)
        seen.add(c)
    assert seen == set(range(len(CONFIG_SETS[kind])))   # every config of the set


@pytest.mark.parametrize("profile", [0, 1])
def test_status_query_sliding_window_integer_weights(profile):
    """Sliding window: remaining = limit - int64(prev * (1 - progress) + curr)
    truncates the weighted count, so `remaining` more requests fit only when
    the weighted previous count is an integer.  Checked on those states only:
    no live previous window, or a time exactly at a window start."""
    sim, configs, tr = warm_sim("sw", profile, 33 + profile)
    key, ts, n, cfg, sms = tr
    checked = with_prev = 0
    for k in range(28):
        c = k % len(configs)
        alg, L, W = configs[c]
        last = int(ts[-1])
        # the trace's end and later, and the whole seconds after it (a window
        # of whole seconds starts on one: progress == 0 there)
        for t in [last, last + 250_000_000, last + 200 * NS] + [(last // NS + j) * NS for j in range(1, 4)]:
            ws = po.window_start(t, W)
            ent = sim.db.get("w:%d:%d" % (k, ws - po.go_f2i(po.duration_seconds(W))))
            prev_live = ent is not None and not sim._expired(ent[1], t // 1_000_000)
            if prev_live and ws * NS != t:
                continue   # a fractional weighted previous count
            check_status(sim, k, t, c, None)
            checked += 1
            with_prev += prev_live
    assert checked > 40 and with_prev > 0


def test_peek_expected_arrays():
    sim, configs, tr = warm_sim("mixed", 0, 3)
    key, ts, n, cfg, sms = tr
    before = copy.deepcopy(sim.db)
    dec, rem, retry, reset, tok = peek_expected(sim, key[:50], ts[:50] + 10 * NS, n[:50], cfg[:50])
    assert sim.db == before
    for i in range(50):
        want = copy.deepcopy(sim).decide(int(key[i]), int(ts[i]) + 10 * NS, int(n[i]), int(cfg[i])) \
            if n[i] >= 1 else None
        if want is not None:
            assert (dec[i], rem[i], retry[i], reset[i]) == want[:4]
            assert np.isnan(tok[i]) == np.isnan(want[4]) and (np.isnan(tok[i]) or tok[i] == want[4])
