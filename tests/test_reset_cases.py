"""tests/reset_cases.py on the oracles alone (CPU): the C and the Python oracle
agree on every case, the cases delete something and leave something, and --
what k_reset_batch's design rests on -- a permutation of one batch's resets
leaves identical keys and identical later decisions."""
import copy

import numpy as np
import pytest

import oracle
from reset_cases import (INVALID, KEY_RESERVED, KINDS, RESET_DONE, apply_resets, expected_status, new_sims, py_decide_rows,
                         py_keys, reset_case)


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_c_oracle_equals_python_oracle(kind, profile):
    configs, first, (rkey, rts, rcfg), second, now_ms = reset_case(kind, 11 + profile, m=1500, nkeys=30,
                                                                   ff=kind in ("fw", "sw"))
    csim, psim = new_sims(oracle, profile, configs)
    csim.decide(*first)
    py_decide_rows(psim, first)
    before = set(csim.keys(now_ms))
    assert before == py_keys(psim, now_ms)
    apply_resets(csim, rkey, rts, rcfg, len(configs), now_ms)
    apply_resets(psim, rkey, rts, rcfg, len(configs))
    after = set(csim.keys(now_ms))
    assert after == py_keys(psim, now_ms)
    # the case is not vacuous: keys went, keys stayed
    assert after < before and len(before - after) >= 3 and len(after) >= 5
    if kind != "tb":
        assert any(k[1] == 1 for k in before - after)
    dec, rem, retry, reset, tok = csim.decide(*second)
    rows = py_decide_rows(psim, second)
    for i, row in enumerate(rows):
        d, r, ra, rs, t = row
        assert (dec[i], rem[i], retry[i], reset[i]) == (d, r, ra, rs), i
        if d <= 1 and configs[second[3][i]][0] == 1:
            assert np.float64(t).view(np.uint64) == tok[i:i + 1].view(np.uint64)[0], i


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_resets_of_one_batch_commute(kind, profile):
    configs, first, (rkey, rts, rcfg), second, now_ms = reset_case(kind, 31 + profile, m=1500, nkeys=30)
    _, base = new_sims(oracle, profile, configs)
    py_decide_rows(base, first)
    rng = np.random.default_rng(7)
    want_keys = want_rows = None
    for trial in range(4):
        sim = copy.deepcopy(base)
        order = None if trial == 0 else rng.permutation(rkey.size)
        apply_resets(sim, rkey, rts, rcfg, len(configs), order=order)
        if trial == 3:      # and idempotent: the whole batch a second time
            apply_resets(sim, rkey, rts, rcfg, len(configs))
        keys, rows = py_keys(sim, now_ms), py_decide_rows(sim, second)
        if trial == 0:
            want_keys, want_rows = keys, rows
        assert keys == want_keys and rows == want_rows, trial
    # the C oracle as well
    want = None
    for trial in range(3):
        csim, _ = new_sims(oracle, profile, configs)
        csim.decide(*first)
        apply_resets(csim, rkey, rts, rcfg, len(configs), now_ms, None if trial == 0 else rng.permutation(rkey.size))
        got = (set(csim.keys(now_ms)), [x.tobytes() for x in csim.decide(*second)[:4]])
        want = want or got
        assert got == want


def test_invalid_requests_are_skipped():
    configs, first, (rkey, rts, rcfg), second, now_ms = reset_case("mixed", 5, m=800, nkeys=20)
    N = len(configs)
    rkey, rcfg = rkey.copy(), rcfg.copy()
    rcfg[::7] = N
    rcfg[3::7] = N + 63
    rkey[5::7] = np.uint64(KEY_RESERVED)
    st = expected_status(rkey, rcfg, N)
    assert set(st) == {RESET_DONE, INVALID} and (st == INVALID).sum() >= 3 * (rkey.size // 7)
    csim, psim = new_sims(oracle, 0, configs)
    csim.decide(*first)
    py_decide_rows(psim, first)
    apply_resets(csim, rkey, rts, rcfg, N, now_ms)
    apply_resets(psim, rkey, rts, rcfg, N)
    assert set(csim.keys(now_ms)) == py_keys(psim, now_ms)
