"""Directed traces for the token-bucket chain replay (k_tb_chain), built by
construction with the Python oracle's arithmetic (oracle/rl_oracle_py.py,
Sim._tb: now = t / 1e9, add = (now - last) * rate, last stored as "%.14g" of
now under Redis 7 -- 1e-4 s resolution -- and no clamp of negative elapsed
time), and for every trace a predicate over the oracle's own per-step record
that states what the trace is claimed to contain.  Nothing here calls the
engine.

A batch that holds one key with more than 4096 requests is one chain segment
that starts at sorted position 0: an offset in the segment is the index in the
batch, the first window starts at the segment start and tiles start at
multiples of CH_TILE.

Every case uses key ids of its own and configuration ids into CONFIGS, so all
cases can share one engine and one oracle.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from oracle import rl_oracle_py as rpy
from tracegen import CONFIG_SETS, NS, T0

# the chain's structural constants (csrc/rl_tb_window.h, rl_engine.hip)
CH_TILE, CH_W, CH_SERIAL, CH_NE, HUGE_MIN, HEAVY_MIN = 384, 2304, 64, 64, 4096, 32
L = 4700                                    # one key's requests in a directed batch: two windows and 92 steps

# CONFIG_SETS["tb"], then a bucket that refills 1000 tokens per microsecond
# (every step clamps) and one whose capacity leaves room for adds of ten times
# the balance (the magnitude edge)
CONFIGS = list(CONFIG_SETS["tb"]) + [(1, 10 ** 9, NS), (1, 10 ** 6, 1000 * NS)]
C_20_12, C_10_1, C_3_03, C_7_15, C_FLOOD, C_WIDE = 0, 2, 3, 4, 5, 6


@dataclass
class Case:
    name: str
    batches: list            # [(key, ts, n, cfg, server_ms or None)]; the last one is the batch under test
    claim: dict = field(default_factory=dict)
    small_max0: bool = False  # needs RL_SMALL_MAX=0 to reach the chain (a batch of <= 4096 requests)

    @property
    def test_batch(self):
        return self.batches[-1]


def _batch(key, ts, n, cfg, sms=None):
    m = len(ts)
    return (np.full(m, key, np.uint64) if np.isscalar(key) else np.asarray(key, np.uint64),
            np.asarray(ts, np.int64), np.asarray(n, np.int64),
            np.full(m, cfg, np.uint32) if np.isscalar(cfg) else np.asarray(cfg, np.uint32),
            None if sms is None else np.asarray(sms, np.int64))


# --- the oracle's per-step record ------------------------------------------------

@dataclass
class Record:
    out: list                # per batch (decision, remaining, retry, reset_at, tokens) arrays
    dec: np.ndarray          # the batch under test, per request:
    stored: np.ndarray       # stored tokens after the step
    before: np.ndarray       # stored tokens before the step (the capacity when the key is absent)
    add: np.ndarray          # (now - last) * rate (0 when the key is absent)
    clamp: np.ndarray        # tokens + add >= capacity
    absent: np.ndarray       # the key was absent or expired


def replay(case, profile):
    """The Python oracle over every batch of the case, with the per-step
    record of the batch under test."""
    sim = rpy.Sim(profile)
    for c in CONFIGS:
        sim.add_config(*c)
    rates = [float(lim) / rpy.duration_seconds(win) for _, lim, win in CONFIGS]
    caps = [float(lim) for _, lim, _ in CONFIGS]
    outs, rec = [], None
    for bi, (key, ts, n, cfg, sms) in enumerate(case.batches):
        m = len(ts)
        kl, tl, nl, cl = key.tolist(), ts.tolist(), n.tolist(), cfg.tolist()
        sl = [None] * m if sms is None else sms.tolist()
        res = [sim.decide(kl[i], tl[i], nl[i], cl[i], sl[i]) for i in range(m)] if bi < len(case.batches) - 1 else []
        if bi == len(case.batches) - 1:
            stored, before, add, clamp, absent = [], [], [], [], []
            db = sim.db
            for i in range(m):
                k = "tb:%d" % kl[i]
                s_ms = sl[i] if sl[i] is not None else tl[i] // 1_000_000
                ent = db.get(k)
                if ent is None or sim._expired(ent[1], s_ms):
                    absent.append(True), before.append(caps[cl[i]]), add.append(0.0), clamp.append(True)
                else:
                    tokens, last = ent[0]
                    a = (float(tl[i]) / 1e9 - last) * rates[cl[i]]
                    absent.append(False), before.append(tokens), add.append(a)
                    clamp.append(not (tokens + a < caps[cl[i]]))
                res.append(sim.decide(kl[i], tl[i], nl[i], cl[i], sl[i]))
                ent = db.get(k)                 # (a TTL of 0 s deletes the key at once)
                stored.append(ent[0][0] if ent is not None else math.nan)
            rec = (np.array(stored), np.array(before), np.array(add), np.array(clamp, bool), np.array(absent, bool))
        cols = list(zip(*res))
        outs.append((np.array(cols[0], np.uint8), np.array(cols[1], np.int64), np.array(cols[2], np.int64),
                     np.array(cols[3], np.int64), np.array(cols[4], np.float64)))
    return Record(outs, outs[-1][0], *rec)


def decade(x):
    return math.floor(math.log10(abs(x))) if x != 0 and math.isfinite(x) else None


def one_decade(values):
    ds = {decade(float(v)) for v in values if v > 0}
    return len(ds) <= 1 and all(v > 0 for v in values)


def near_distance(add, E):
    """|frac(add * 10^(13 - E)) - 1/2|, exactly."""
    f = Fraction(float(add)) * Fraction(10) ** (13 - E)
    return abs(f - math.floor(f) - Fraction(1, 2))


# --- (a), (b): a steady state with one event, or one burst of allows -------------

STEADY_GAP = 10           # ns
EDGE_OFFSETS = [0, 1, 5, 6, 383, 384, 385, 2303, 2304, 2305, 4607, L - 1]
EDGE_KINDS = {            # gap (ns), n of the event step
    "allow": (1 * NS, 1),
    "clamp_allow": (20 * NS, 1),
    "clamp_deny": (20 * NS, 1 << 62),
    "expiry": (25 * NS, 1),            # above the 24 s TTL of (20, 12 s)
    "back": (-5 * NS, 1),
    "zero": (0, 1),
}


def _steady_prime(key):
    # T0 is a multiple of 1e-4 s, and so is every gap below but the steady one:
    # last_refill's rounding error starts at 0 and grows by 10 ns per step, which
    # lets the balance drift up by rate * sum(error) < 0.2 tokens over L steps
    # (0.55 -> 0.73: one decade, one binade, below n = 1 throughout)
    return _batch(key, [T0, T0 + 330_000_000], [20, 1], C_20_12)


def _steady(key, events, absent=False):
    gaps = np.full(L, STEADY_GAP, np.int64)
    n = np.ones(L, np.int64)
    for o, (g, nn) in events.items():
        gaps[o], n[o] = g, nn
    ts = T0 + 330_000_000 + np.cumsum(gaps)
    main = _batch(key, ts, n, C_20_12)
    return [main] if absent else [_steady_prime(key), main]


def edge_case(key, kind, o):
    return Case(f"edge-{kind}-{o}", _steady(key, {o: EDGE_KINDS[kind]}), {"family": "a", "kind": kind, "o": o})


def edge_absent_case(key):
    return Case("edge-absent-0", _steady(key, {}, absent=True), {"family": "a", "kind": "absent", "o": 0})


def check_edge(case, rec):
    kind, o = case.claim["kind"], case.claim["o"]
    calm = ~(rec.dec == 1) & ~rec.clamp & ~rec.absent
    assert calm[:o].all(), f"{case.name}: an allow, clamp or expiry before the event"
    if kind != "absent":
        assert one_decade(np.concatenate([rec.before[:1], rec.stored[:o]])), \
            f"{case.name}: the balance leaves its decade before the event"
    d, c, a = bool(rec.dec[o] == 1), bool(rec.clamp[o]), bool(rec.absent[o])
    if kind == "allow":
        assert d and not c and not a
    elif kind == "clamp_allow":
        assert d and c and not a
    elif kind == "clamp_deny":
        assert not d and c and not a
    elif kind in ("expiry", "absent"):
        assert a and d
    elif kind == "back":
        assert not d and rec.stored[o] < -7.0 and (rec.stored[o:] < 0).all() and not (rec.dec[o:] == 1).any()
    elif kind == "zero":
        ts = case.test_batch[1]
        prev = ts[o - 1] if o else case.batches[0][1][-1]
        assert ts[o] == prev and calm[o]
    else:
        raise AssertionError(kind)


BURST_LENGTHS = [CH_SERIAL - 1, CH_SERIAL, CH_SERIAL + 1, 2 * CH_SERIAL + 1]
BURST_STARTS = [0, CH_W - 32]
BURST_GAP = 600_000_000   # (20 / 12 s) * 0.6 s = 1 token: each burst step allows and returns to the steady balance


def burst_case(key, start, B):
    ev = {start + i: (BURST_GAP, 1) for i in range(B)}
    return Case(f"burst-{B}-at-{start}", _steady(key, ev), {"family": "b", "start": start, "B": B})


def flood_case(key):
    # 100 us apart, on last_refill's "%.14g" grid: every add is exactly 1e5 tokens (at 1 us gaps the
    # rounding of last_refill makes elapsed time negative on most steps, and those do not clamp)
    ts = T0 + 100_000 * np.arange(1, L + 1)
    return Case("burst-every-step", [_batch(key, ts, np.ones(L, np.int64), C_FLOOD)],
                {"family": "b", "start": 0, "B": L, "all_clamp": True})


def check_burst(case, rec):
    s, B = case.claim["start"], case.claim["B"]
    allowed = rec.dec == 1
    assert allowed[s:s + B].all() and allowed.sum() == B, f"{case.name}: the run of allows is not {B} at {s}"
    if case.claim.get("all_clamp"):
        assert rec.clamp.all()


# --- (c): near-step density in one-decade windows (Redis-7 profile) -------------

NEAR_MAX, FAR_MIN = Fraction(1, 1000), Fraction(3, 100)
# "Band" steps: inside the kernel's near band, yet so far from the half unit that no rounding can flip
# them.  The first window of a segment is summarized with dmax = 1e14 digits, so its band is
# 10^13 * 2^(4 - 53) = 0.01776 (ch_produce); the roundings of strtod and of the sum move a step by at
# most 2 * 2^(1 - 53) * 10^13 = 0.0044 units while the balance is below 4 tokens.  A band step is
# listed as near by the producers and resolves to its nominal result: a tile of them fills the near
# list without making the near fixed point iterate.
BAND_LO, BAND_HI = Fraction(8, 1000), Fraction(15, 1000)
FAR, NEAR, BAND = 0, 1, 2
DENSITY_N = 19            # above the balance throughout: no allow


def _q14(x):
    return float("%.14g" % x)


def density_case(key, name, near, seed):
    """Timestamps chosen by search so that step i is near (its add within 0.001
    of a half unit of the balance's decade) where near[i] == NEAR, a band step
    where near[i] == BAND, and far (more than 0.03 away) everywhere else.  The
    balance starts at 2 tokens and climbs ~5e-4 per step: decade 0 for the
    whole segment."""
    near = np.asarray(near, np.int8)
    rng = np.random.default_rng(seed)
    rate = 20.0 / 12.0
    tok, t = 2.0, T0
    last = _q14(float(t) / 1e9)
    ts = np.empty(L, np.int64)
    for i in range(L):
        span = 1_200_000 if near[i] else 600_000
        while True:
            cand = t + np.arange(4_000, span, 119, dtype=np.int64)
            now = cand.astype(np.float64) / 1e9
            add = (now - last) * rate
            pr = add * 1e13
            d = np.abs(pr - np.floor(pr) - 0.5)
            # margins over the double product's error (< 1e-5 at |pr| < 2e10)
            idx = np.nonzero(d < 0.0009 if near[i] == NEAR else (d > 0.0081) & (d < 0.0149) if near[i] == BAND
                             else d > 0.031)[0]
            if near[i] and idx.size:          # the shortest few: keeps the climb of an all-near tile small
                idx = idx[:4]
            if idx.size:
                break
            span *= 2
        j = int(rng.choice(idx))
        t = int(cand[j])
        ts[i] = t
        tok = _q14(tok + float(add[j]))
        last = _q14(float(now[j]))
        assert 1.0 <= tok < 10.0
    prime = _batch(key, [T0], [18], C_20_12)
    return Case(name, [prime, _batch(key, ts, np.full(L, DENSITY_N, np.int64), C_20_12)],
                {"family": "c", "near": near == NEAR, "band": near == BAND})


def _near_tiles(tiles, count, seed, kind=NEAR):
    rng = np.random.default_rng(seed)
    near = np.zeros(L, np.int8)
    for t in tiles:
        near[t * CH_TILE + rng.choice(CH_TILE, count, replace=False)] = kind
    return near


def density_cases(key0):
    run70 = np.zeros(L, np.int8)
    run70[CH_TILE - 35:CH_TILE + 35] = NEAR
    specs = [("near-63", _near_tiles([1, 8], 63, 1)), ("near-64", _near_tiles([1, 8], 64, 2)),
             ("near-65", _near_tiles([1, 8], 65, 3)), ("near-384", _near_tiles([1], CH_TILE, 4)),
             ("near-6x64", _near_tiles(range(6), 64, 5)), ("near-run70", run70),
             # the two sides of the near list's capacity with steps that never flip: the 64-step
             # tile commits from its summary, the 65-step tile overflows the list
             ("band-64", _near_tiles([1], CH_NE, 6, BAND)), ("band-65", _near_tiles([1], CH_NE + 1, 7, BAND))]
    return [density_case(key0 + i, name, near, 40 + i) for i, (name, near) in enumerate(specs)]


def tile_near_counts(rec):
    """(per-tile near counts aligned to the segment start, steps that are
    neither near nor far), from the oracle's adds and balances."""
    m = len(rec.add)
    near, band, vague = np.zeros(m, bool), np.zeros(m, bool), 0
    for i in range(m):
        d = near_distance(rec.add[i], decade(rec.before[i]))
        near[i] = d < NEAR_MAX
        band[i] = BAND_LO <= d <= BAND_HI
        vague += int(NEAR_MAX <= d <= FAR_MIN and not band[i])
    return [int((near | band)[o:o + CH_TILE].sum()) for o in range(0, m, CH_TILE)], vague, near, band


def flips(rec):
    """Per step, the stored digits' change minus the nominal increment
    rint(add * 10^13) (balances in decade 0): nonzero where the roundings of
    the script step moved the result off the nominal one."""
    out = np.zeros(len(rec.add), np.int64)
    for i in range(len(rec.add)):
        d0, d1 = round(Fraction(float(rec.before[i])) * 10 ** 13), round(Fraction(float(rec.stored[i])) * 10 ** 13)
        out[i] = d1 - d0 - round(Fraction(float(rec.add[i])) * 10 ** 13)
    return out


def check_density(case, rec):
    want, wband = case.claim["near"], case.claim["band"]
    counts, vague, near, band = tile_near_counts(rec)
    assert vague == 0, f"{case.name}: {vague} steps neither near nor far"
    assert np.array_equal(near, want), f"{case.name}: near steps not as designated"
    assert np.array_equal(band, wband), f"{case.name}: band steps not as designated"
    assert counts == [int((want | wband)[o:o + CH_TILE].sum()) for o in range(0, L, CH_TILE)]
    if wband.any():
        # band steps only in the first window and below 4 tokens, where the band and the bound on
        # the roundings are the ones stated above; and no step of the segment flips
        assert not wband[CH_W:].any() and rec.stored[wband].max() < 4.0
        assert not flips(rec).any(), f"{case.name}: a step leaves its nominal result"
    assert one_decade(np.concatenate([rec.before[:1], rec.stored])), f"{case.name}: more than one decade"
    assert not (rec.dec == 1).any() and not rec.clamp.any() and not rec.absent.any()


# --- (d): hot keys under clock skew at chain length ------------------------------

SKEWS_NS = (0, -2_500_000_000, -7 * NS, 4 * NS, -130 * NS)   # tracegen.skewed_trace's
SKEW_CFGS = (C_20_12, C_10_1, C_7_15)


def skew_case(key0, seed=3, m=40_000):
    """Three hot token-bucket keys, each on a config of its own, stamped by
    five app servers with skewed clocks; server_ms is the store's own clock
    (true time).  As tracegen.skewed_trace, at chain length."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 3, m)
    gaps = rng.choice([0, 1000, 250_000, 50_000_000, 700_000_000], m, p=[0.1, 0.4, 0.2, 0.25, 0.05])
    true_t = T0 + np.cumsum(gaps).astype(np.int64)
    ts = true_t + np.asarray(SKEWS_NS, np.int64)[rng.integers(0, len(SKEWS_NS), m)]
    n = rng.choice([1, 1, 1, 2, 3, 7], m).astype(np.int64)
    cfg = np.asarray(SKEW_CFGS, np.uint32)[which]
    return Case("skew-hot", [_batch(key0 + which.astype(np.uint64), ts, n, cfg, true_t // 1_000_000)],
                {"family": "d", "keys": [key0, key0 + 1, key0 + 2]})


def check_skew(case, rec):
    key = case.test_batch[0]
    hit = []
    for k in case.claim["keys"]:
        st = rec.stored[key == k]
        assert st.size >= 12_000, f"{case.name}: key {k} has {st.size} requests"
        sg = np.sign(st[st != 0])
        flips = int((sg[1:] != sg[:-1]).sum())
        mag = np.abs(st)
        ok = (mag[:-1] > 0) & (mag[1:] > 0)
        drop = np.floor(np.log10(mag[:-1][ok])) - np.floor(np.log10(mag[1:][ok]))
        hit.append(int((st < 0).sum()) >= 1000 and flips >= 100 and bool((drop >= 2).any()))
    assert any(hit), f"{case.name}: no key with 1000 negative balances, 100 sign changes and a two-decade fall"


# --- (e): the magnitude edge ------------------------------------------------------

def magnitude_case(key, name, start, skew_s):
    """Two app servers skew_s seconds apart, two requests from each in turn, on
    a bucket that refills 1000 tokens / s: adds of +a, ~0, -a, ~0 with
    a = 1000 * skew_s tokens, several times the balance.  A producer lane's
    six steps then sum to +-a.  With a above 2^46 units of the start decade
    and every step below 2^49, ch_produce's condition for its int64 tile scan
    holds; that the branch is taken is inferred from that condition, no debug
    word counts it.

    start = 1500, skew 8 s: the balance moves between 1500 and 9500 tokens,
    one decade (a = 8e13 units), so one-decade windows commit tiles whose sums
    came from that scan.  start = 2000, skew 20 s: 2000 to 22000 tokens, a
    decade crossed on every big step (multi-decade windows on Redis 7)."""
    true_t = T0 + 10_000 * np.arange(1, L + 1)
    ahead = (np.arange(L) % 4) < 2
    ts = true_t + np.where(ahead, skew_s * NS, 0)
    prime = _batch(key, [T0], [10 ** 6 - start], C_WIDE, [T0 // 1_000_000])
    return Case(name, [prime, _batch(key, ts, np.full(L, 999_999, np.int64), C_WIDE, true_t // 1_000_000)],
                {"family": "e", "one_decade": name == "magnitude-one-decade"})


def check_magnitude(case, rec):
    assert not (rec.dec == 1).any() and not rec.clamp.any() and not rec.absent.any()
    found = False
    for o in range(0, L - CH_TILE + 1, CH_TILE):
        E0 = decade(rec.before[o])
        if E0 is None:
            continue
        u = [abs(Fraction(float(a))) * Fraction(10) ** (13 - E0) for a in rec.add[o:o + CH_TILE]]
        if max(u) < 2 ** 49 and sum(u) > 2 ** 53:
            # of the tile's adds, half are the clock steps between the servers: 1 to 1000 times the
            # balance at the tile's start
            big = sum(1 for a in rec.add[o:o + CH_TILE] if 1.0 <= abs(a) / abs(rec.before[o]) <= 1000.0)
            found = found or big >= CH_TILE // 4
    assert found, f"{case.name}: no aligned tile with every step below 2^49 units and their sum above 2^53"
    if case.claim["one_decade"]:
        assert one_decade(np.concatenate([rec.before[:1], rec.stored]))
        E0 = decade(rec.before[0])
        assert max(abs(float(a)) for a in rec.add) * 10.0 ** (13 - E0) > 2.0 ** 46


# --- (f): segment lengths and starts ----------------------------------------------

LENGTH_CFGS = (C_20_12, C_10_1, C_7_15)      # refills of 0.08, 0.45 and 0.2 tokens per request of a key
ODD_BATCHES = [[4097, 4607, 4609], [4991, 4993, 6911], [6913, 8191, 8193]]
EVEN_BATCHES = [[4096, 4608, 4992], [6912, 8192, 4096], [4096]]
THRESHOLD_BATCH = [HEAVY_MIN - 1, HEAVY_MIN, HEAVY_MIN + 1, HUGE_MIN - 1, HUGE_MIN, HUGE_MIN + 1]


def lengths_case(key0, name, counts, seed, small_max0=False):
    """Keys with exactly these request counts, interleaved at random; random
    gaps (15 ms mean) and n in {1, 1, 1, 2}: allows mixed with denials."""
    rng = np.random.default_rng(seed)
    which = np.concatenate([np.full(c, i) for i, c in enumerate(counts)])
    which = which[rng.permutation(which.size)]
    m = which.size
    ts = T0 + np.cumsum(np.rint(rng.exponential(15_000_000, m))).astype(np.int64)
    n = rng.choice([1, 1, 1, 2], m).astype(np.int64)
    cfg = np.asarray(LENGTH_CFGS, np.uint32)[which % 3]
    return Case(name, [_batch(key0 + which.astype(np.uint64), ts, n, cfg)],
                {"family": "f", "counts": {key0 + i: c for i, c in enumerate(counts)}}, small_max0)


def check_lengths(case, rec):
    key = case.test_batch[0]
    if case.claim.get("expires"):
        assert rec.absent.all() and (rec.dec == 1).all()
        return
    ks, cs = np.unique(key, return_counts=True)
    assert dict(zip(ks.tolist(), cs.tolist())) == case.claim["counts"]
    for k, c in case.claim["counts"].items():
        if c >= HUGE_MIN:
            d = rec.dec[key == k]
            assert (d == 1).sum() >= 100 and (d == 0).sum() >= 100, f"{case.name}: key {k} lacks allows or denials"
            assert not rec.absent[key == k][1:].any(), f"{case.name}: key {k} expires inside its segment"


def expiry_case(key):
    """An extra segment on (3, 300 ms), whose TTL of 0 s deletes the key after
    every request: each step finds it absent and is allowed."""
    rng = np.random.default_rng(95)
    ts = T0 + np.cumsum(np.rint(rng.exponential(15_000_000, L))).astype(np.int64)
    return Case("lengths-every-step-expires", [_batch(key, ts, np.ones(L, np.int64), C_3_03)],
                {"family": "f", "counts": {key: L}, "expires": True})


# --- all cases ----------------------------------------------------------------------

CHECKS = {"a": check_edge, "b": check_burst, "c": check_density, "d": check_skew, "e": check_magnitude,
          "f": check_lengths}


def check(case, rec):
    CHECKS[case.claim["family"]](case, rec)


@functools.lru_cache(maxsize=None)
def all_cases():
    """{family: [Case]} -- every case with key ids of its own."""
    key = iter(range(10_000, 1 << 20, 16))
    out = {"a": [], "b": [], "c": [], "d": [], "e": [], "f": []}
    for kind in EDGE_KINDS:
        for o in EDGE_OFFSETS:
            out["a"].append(edge_case(next(key), kind, o))
    out["a"].append(edge_absent_case(next(key)))
    for s in BURST_STARTS:
        for B in BURST_LENGTHS:
            out["b"].append(burst_case(next(key), s, B))
    out["b"].append(flood_case(next(key)))
    out["c"] = density_cases(next(key))
    out["d"].append(skew_case(next(key)))
    out["e"].append(magnitude_case(next(key), "magnitude-one-decade", 1500, 8))
    out["e"].append(magnitude_case(next(key), "magnitude", 2000, 20))
    for i, counts in enumerate(ODD_BATCHES):
        out["f"].append(lengths_case(next(key), f"lengths-odd-{i}", counts, 70 + i))
    for i, counts in enumerate(EVEN_BATCHES):
        out["f"].append(lengths_case(next(key), f"lengths-even-{i}", counts, 80 + i, small_max0=sum(counts) <= 4096))
    out["f"].append(lengths_case(next(key), "lengths-thresholds", THRESHOLD_BATCH, 90))
    out["f"].append(expiry_case(next(key)))
    return out
