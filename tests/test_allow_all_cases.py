"""AllowAll on the CPU: the seeded cases meet the coverage their builder
asserts, the composition on the Python oracle has the properties the contract
states, and a plain-Python model of the settle kernel's two bounded scans
agrees with the "maximal run" definition of a group."""
import copy
import itertools

import numpy as np
import pytest

from allow_all_cases import (KINDS, MAX_GROUP, allow_all_case, apply_allow_all, group_spans, run_group, scan_group,
                             settle)
from oracle import rl_oracle_py as po
from refund_cases import DONE, INVALID, NOKEY, new_sim, warm
from tracegen import NS, T0


def agree(first, cap):
    """scan_group against run_group for every member of one byte pattern"""
    for i in range(len(first)):
        h, e = run_group(first, i)
        want = (h, e) if e - h <= cap else None
        assert scan_group(first, i, cap) == want, (first, i, cap)


@pytest.mark.parametrize("cap", [MAX_GROUP, 3])
def test_scans_exhaustive(cap):
    """every byte pattern of length <= 12 (a byte is zero or not); with the cap
    of 16 no run is too long, with a cap of 3 most are"""
    for m in range(1, 13):
        for bits in itertools.product((0, 1), repeat=m):
            agree(bits, cap)


def test_scans_long_runs():
    """random patterns of length 70 that hold runs of 15, 16, 17, 32 and 33"""
    rng = np.random.default_rng(11)
    seen = set()
    for _ in range(300):
        runs = rng.permutation([15, 16, 17, 32, 33, 1, 2]).tolist()
        first = np.zeros(70, np.uint8)
        at = int(rng.integers(0, 2))          # first[0] == 0 starts a group too
        first[0] = at
        pos = 0
        for r in runs:
            if pos >= 70:
                break
            if pos:
                first[pos] = rng.choice([1, 7, 255])
            seen.add(min(r, 70 - pos))
            pos += r
        agree(first.tolist(), MAX_GROUP)
        spans = group_spans(first.tolist())
        assert spans == sorted({run_group(first.tolist(), i) for i in range(70)})
    assert {15, 16, 17, 32, 33} <= seen


@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_case_coverage(kind, profile):
    """the committed seeds meet the builder's coverage on both profiles"""
    configs, first_trace, (key, ts, n, cfg, sms, first), second, now_ms, cover = allow_all_case(kind, profile)
    assert cover["transient"] and cover["nokey"] >= 1 and sorted(cover["long_runs"]) == [17, 33]
    assert (sms is None) == (kind == "tb")
    # a failed check takes nothing: every member that took something in a
    # failed group asks all of it back, and nobody else asks anything
    v, g, dec = cover["verdict"], cover["g"], cover["decision"]
    ok = v == po.ALLOWED
    assert (g[ok] == 0).all() and (cover["rollback"][g == 0] == INVALID).all()
    assert set(np.unique(cover["rollback"][g > 0]).tolist()) <= {DONE, NOKEY}
    assert ((g == 0) | (g == n)).all()
    assert (g[(dec == po.ERROR) | (dec == po.INVALID)] == 0).all()
    # the second trace starts after the call on the request clock
    assert int(second[1][0]) > int(ts[-1])


def test_failed_check_takes_nothing():
    """a failed group leaves window counters and (up to %.14g) buckets as it
    found them; an allowed group keeps what it took"""
    configs = [(1, 20, 12 * NS), (3, 100, 60 * NS), (2, 100, 60 * NS)]
    sim = new_sim(0, configs)
    keys = np.array([1, 2, 3], np.uint64)
    cfg = np.array([0, 1, 2], np.uint32)
    warm(sim, (keys, np.full(3, T0), np.full(3, 5), cfg, None))
    before = copy.deepcopy(sim.db)
    # bucket allowed, fixed window allowed, sliding window denied (5 + 96 > 100)
    rows, v, g, rb, info = apply_allow_all(sim, keys, np.full(3, T0 + 1000), [3, 10, 96], cfg, [1, 0, 0])
    assert [r[0] for r in rows] == [po.ALLOWED, po.ALLOWED, po.DENIED]
    assert v.tolist() == [po.DENIED] * 3 and g.tolist() == [3, 10, 96] and rb.tolist() == [DONE] * 3
    assert sim.db["w:2:%d" % po.window_start(T0, 60 * NS)][0] == before["w:2:%d" % po.window_start(T0, 60 * NS)][0]
    assert sim.db["w:3:%d" % po.window_start(T0, 60 * NS)][0] == 5
    assert abs(sim.db["tb:1"][0][0] - before["tb:1"][0][0]) < 1e-4      # the refill of 1 us stays
    # the same members, each a group of its own: AllowN, plus the give-back of
    # the denied window member's INCRBY
    rows, v, g, rb, _ = apply_allow_all(sim, keys, np.full(3, T0 + 2000), [3, 10, 96], cfg, [1, 1, 1])
    assert v.tolist() == [po.ALLOWED, po.ALLOWED, po.DENIED] and g.tolist() == [0, 0, 96]
    assert rb.tolist() == [INVALID, INVALID, DONE]
    assert sim.db["w:2:%d" % po.window_start(T0, 60 * NS)][0] == 15
    assert sim.db["w:3:%d" % po.window_start(T0, 60 * NS)][0] == 5


def test_conservative_two_groups():
    """the worked example of §10k: [A 15 of 20, B over its limit] fails, and
    [A 15] behind it in the same call is denied on A's transient take; in a
    call of its own it is allowed.  Never the other way round."""
    configs = [(1, 20, 12 * NS)]
    t = np.full(3, T0)
    one = new_sim(0, configs)
    _, v, g, _, _ = apply_allow_all(one, [1, 2, 1], t, [15, 40, 15], [0, 0, 0], [1, 0, 1])
    assert v.tolist() == [po.DENIED] * 3 and g.tolist() == [15, 0, 0]
    assert one.db["tb:1"][0][0] == 20.0
    two = new_sim(0, configs)
    _, va, _, _, _ = apply_allow_all(two, [1, 2], t[:2], [15, 40], [0, 0], [1, 0])
    _, vb, _, _, _ = apply_allow_all(two, [1], t[:1], [15], [0], [1])
    assert va.tolist() == [po.DENIED] * 2 and vb.tolist() == [po.ALLOWED]


def test_settle_precedence():
    """INVALID > ERROR > DENIED > ALLOWED; ERROR and INVALID members ask
    nothing back; a run of 17 is INVALID and still gives back what it took"""
    sim = new_sim(0, [(1, 20, 12 * NS), (3, 100, 60 * NS)])
    A, D, E, I = po.ALLOWED, po.DENIED, po.ERROR, po.INVALID
    first = [1, 0, 1, 0, 1, 0, 0, 1, 0]
    dec = [A, A, A, D, D, E, A, E, I]
    cfg = [0, 1] * 4 + [0]
    v, g = settle(sim, first, [2] * 9, cfg, dec)
    assert v.tolist() == [A, A, D, D, E, E, E, I, I]
    assert g.tolist() == [0, 0, 2, 2, 0, 0, 2, 0, 0]      # member 4: a denied bucket took nothing
    v, g = settle(sim, [1] + [0] * 16, [1] * 17, [1] * 17, [A] * 17)
    assert v.tolist() == [I] * 17 and g.tolist() == [1] * 17
    v, g = settle(sim, [1] + [0] * 15, [1] * 16, [1] * 16, [A] * 16)
    assert v.tolist() == [A] * 16 and g.tolist() == [0] * 16
