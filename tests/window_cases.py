"""Directed traces for the fixed- and sliding-window replay (wave_win_segment,
fw_step / sw_step, csrc/rl_replay_wave.h and csrc/rl_window.h), built by
construction, and for every trace a predicate over the Python oracle's own
per-request record (oracle/rl_oracle_py.py: Sim._fw, Sim._sw, Sim.db) that
states what the trace is claimed to contain.  Nothing here calls the engine.

A case is a list of batches (key, ts, n, cfg, server_ms); the last one is the
batch under test.  Every case uses key ids of its own and configuration ids
into CONFIGS, so one engine and one oracle serve a whole family.

  g  run geometry: where a window run ends relative to the lane and chunk grid
     of the wave shortcut, segment lengths around HEAVY_MIN and SMALL_MAX, and a
     sliding-window run whose decisions go deny -> allow -> deny
  b  bail-outs of the shortcut, each at offsets 1, 6, 383, 384 and 385 of a run
     of 400 requests, with a short tail that reads the state the serial replay
     left
  s  sliding-window weighted counts whose exact value p (1 - el / W) + cc is an
     integer at (or one below) the limit, so that one ulp decides: S_LIGHT, one
     key per point (sw_step, and Peek), and S_RUNS, a client pacing exactly at
     the limit (the shortcut's copy of the formula)
  c  state carried from an earlier batch into the batch under test

Left out, and why:
  * A config change inside one key's segment.  The engine's contract
    (include/rl_engine.h, rl_config_register) keys state by key id alone and has
    callers give each (config, key) an id of its own, so one id never meets two
    configs; no trace of the suite does it either.
  * The previous-key-died-mid-run branch of the shortcut (`pdead`).  The current
    key's expiry is its creation clock + ttl_c and is never moved later except
    by a TTL re-set, which bails out; the previous key's expiry is the clock of
    the run's latest request + ttl_p, and ttl_p = int(2 W) >= ttl_c = int(W).
    With a server clock that never goes back (the engine's contract,
    csrc/rl_window.h) the previous key can therefore only be found dead by a
    request that finds the current key dead too, and that check comes first.
    check() asserts on every sliding-window case that the previous key, once
    found by a run, is found by every later request of that run the current key
    lives through.
  * W = 1.5 s in family s: the previous window's key is found from every other
    window only, and only while a late first request keeps it alive (family b
    states this); the straddles use windows of whole seconds.
  * The 2^53 twins of the TTL re-set need a count of 1 or 2 before the big
    request, so they exist at offset 1 only.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

from oracle import rl_oracle_py as rpy
from tracegen import NS, T0

# the shortcut's structural constants
CHUNK = 384        # requests per pass of wave_win_segment: 64 lanes * CH_K (csrc/rl_tb_window.h)
K = 6              # CH_K, requests per lane (csrc/rl_tb_window.h, RL_CH_K)
HEAVY_MIN = 32     # rl_engine::heavy_min (csrc/rl_engine_impl.h; RL_HEAVY_MIN): segments this long take a wave
SMALL_MAX = 4096   # SMALL_MAX (csrc/rl_engine.hip; RL_SMALL_MAX): batches up to this size run as k_small
assert CHUNK == 64 * K

MS = 1_000_000
DAY = 86400 * NS
YEAR = 365 * DAY
FW, SW = rpy.FIXED_WINDOW, rpy.SLIDING_WINDOW

# straddle windows (family s, light shape): (2, 100, W) each
S_LIGHT_WINDOWS = (2 * NS, 3 * NS, 7 * NS, 12 * NS, 60 * NS, DAY)
S_LIMIT = 100
# straddle runs (family s, run shape): (W, L, p), config (2, L, W) each -- see search_runs()
S_RUNS = (
    (2 * NS, 250, 250),
    (3 * NS, 250, 250),
    (YEAR, 219, 219),
    (YEAR, 250, 250),
    (YEAR, 500, 500),
)

CONFIGS = [
    (FW, 100, 60 * NS), (SW, 100, 60 * NS),              # allowed for a while
    (FW, 5, 2 * NS), (SW, 5, 2 * NS),                    # allow turns to deny inside a run
    (FW, 3, 1_500_000_000), (SW, 3, 1_500_000_000),      # ttl_c = 1 s, shorter than the window
    (FW, 4, 700_000_000), (SW, 4, 700_000_000),          # ttl_c = 0
    (FW, 2, 300_000_000), (SW, 2, 300_000_000),
] + [(SW, S_LIMIT, w) for w in S_LIGHT_WINDOWS if w != 60 * NS] + [(SW, lim, w) for w, lim, _ in S_RUNS]
FW_HI, SW_HI, FW_LO, SW_LO, FW_15, SW_15, FW_07, SW_07, FW_03, SW_03 = range(10)


def cfg_of(alg, limit, window):
    return CONFIGS.index((alg, limit, window))


def ttl_c(window):
    return rpy.go_f2i(rpy.duration_seconds(window))


def win_ns(window, i):
    """Start (ns) of the i-th whole window after T0 (i = 0: the first one that
    starts after T0).  Go's Truncate counts from year 1."""
    return T0 - (T0 + rpy.UNIX_TO_INTERNAL * NS) % window + (i + 1) * window


@dataclass
class Case:
    name: str
    batches: list            # [(key, ts, n, cfg, server_ms or None)]; the last one is the batch under test
    claim: dict = field(default_factory=dict)
    small_max0: bool = False  # a batch of <= SMALL_MAX requests meant for the full launch sequence as well

    @property
    def test_batch(self):
        return self.batches[-1]


def _batch(key, ts, n, cfg, sms=None):
    m = len(ts)
    return (np.full(m, key, np.uint64) if np.isscalar(key) else np.asarray(key, np.uint64),
            np.asarray(ts, np.int64),
            np.full(m, n, np.int64) if np.isscalar(n) else np.asarray(n, np.int64),
            np.full(m, cfg, np.uint32) if np.isscalar(cfg) else np.asarray(cfg, np.uint32),
            None if sms is None else np.asarray(sms, np.int64))


# --- the oracle's per-request record ------------------------------------------------

@dataclass
class Record:
    out: list                # per batch (decision, remaining, retry, reset_at, tokens) arrays
    # the batch under test, per request (lists; None where there is no such key):
    dec: np.ndarray
    rem: np.ndarray
    ws: list                 # window start (s) of the request: the current window key
    s_ms: list               # the server clock of the request
    cur_before: list         # current key's count / expiry (ms) before the request; None: absent or expired
    when_before: list
    cur_after: list          # ... and after it; None: deleted at once (a TTL of 0 s)
    when_after: list
    prev_cnt: list           # SW: the previous window key's count as the request found it; None: not found
    prev_when: list          # ... and its expiry after the request
    created: np.ndarray      # INCRBY created the current key
    ttl_set: np.ndarray      # the script (re)set the current key's TTL: float(cur) == float(n)
    err: np.ndarray          # the script errored (INCRBY overflow)
    # where the engine keeps the window keys, by _Entry's model of wk_create (csrc/rl_window.h):
    cur_in_entry: np.ndarray   # after the request, the current key is one of the entry's two slots
    prev_in_spill: np.ndarray  # SW: the previous key the request found lives in the spill


class _Entry:
    """Model of where one user key's window keys live (csrc/rl_window.h,
    wk_find / wk_create): two slots in the table entry, every other live key in
    the spill.  INCRBY's new key takes the first free or expired slot other
    than the previous window's; with none, the older slot key moves to the
    spill, unless the new key is older still and goes there itself."""

    def __init__(self):
        self.slots = [None, None]
        self.spill = set()

    def create(self, ws, pws, alive):
        for k in (0, 1):
            if self.slots[k] is not None and not alive(self.slots[k]):
                self.slots[k] = None
        self.spill = {w for w in self.spill if alive(w) and w != ws}
        keep = self.slots.index(pws) if pws is not None and pws in self.slots else -1
        cand = [k for k in (0, 1) if k != keep]
        for k in cand:
            if self.slots[k] is None:
                self.slots[k] = ws
                return
        best = min(cand, key=lambda k: self.slots[k])
        if self.slots[best] > ws:
            self.spill.add(ws)
        else:
            self.spill.add(self.slots[best])
            self.slots[best] = ws


def replay(case, profile):
    """The Python oracle over every batch of the case, with the per-request
    record of the batch under test."""
    sim = rpy.Sim(profile)
    for c in CONFIGS:
        sim.add_config(*c)
    db, entries, outs = sim.db, {}, []
    cols = None
    for bi, (key, ts, n, cfg, sms) in enumerate(case.batches):
        m = len(ts)
        last = bi == len(case.batches) - 1
        kl, tl, nl, cl = key.tolist(), ts.tolist(), n.tolist(), cfg.tolist()
        sl = (ts // 1_000_000).tolist() if sms is None else sms.tolist()
        res = []
        if last:
            cols = {f: [] for f in ("ws", "s_ms", "cur_before", "when_before", "cur_after", "when_after", "prev_cnt",
                                    "prev_when", "created", "ttl_set", "err", "cur_in_entry", "prev_in_spill")}
        for i in range(m):
            k, t, nn, s = kl[i], tl[i], nl[i], sl[i]
            alg, _, W = CONFIGS[cl[i]]
            ws = rpy.window_start(t, W)
            pws = ws - ttl_c(W) if alg == SW else None

            def live(w):
                ent = db.get("w:%d:%d" % (k, w))
                return ent if ent is not None and not sim._expired(ent[1], s) else None

            def alive(w):
                return live(w) is not None

            cb = live(ws)
            pb = live(pws) if alg == SW else None
            cur_before, when_before = (cb[0], cb[1]) if cb else (None, None)
            prev_cnt = pb[0] if pb else None
            ent = entries.setdefault(k, _Entry())
            p_spill = pb is not None and pws in ent.spill
            # liveness as the request finds it decides the placement: evaluate before the step
            if cb is None:
                held = {w: alive(w) for w in ent.slots + list(ent.spill) if w is not None}
            r = sim.decide(k, t, nn, cl[i], s)
            res.append(r)
            err = r[0] == rpy.ERROR
            created = cb is None and not err
            if created:
                ent.create(ws, pws if pb is not None else None, lambda w: held.get(w, False))
            if last:
                ca = db.get("w:%d:%d" % (k, ws))
                pa = db.get("w:%d:%d" % (k, pws)) if pb is not None else None
                cols["ws"].append(ws), cols["s_ms"].append(s)
                cols["cur_before"].append(cur_before), cols["when_before"].append(when_before)
                cols["cur_after"].append(ca[0] if ca else None), cols["when_after"].append(ca[1] if ca else None)
                cols["prev_cnt"].append(prev_cnt), cols["prev_when"].append(pa[1] if pa else None)
                cols["created"].append(created), cols["err"].append(err)
                cols["ttl_set"].append(not err and float((cur_before or 0) + nn) == float(nn))
                cols["cur_in_entry"].append(ws in ent.slots), cols["prev_in_spill"].append(p_spill)
        z = list(zip(*res))
        outs.append((np.array(z[0], np.uint8), np.array(z[1], np.int64), np.array(z[2], np.int64),
                     np.array(z[3], np.int64), np.array(z[4], np.float64)))
    for f in ("created", "ttl_set", "err", "cur_in_entry", "prev_in_spill"):
        cols[f] = np.array(cols[f], bool)
    return Record(outs, outs[-1][0], outs[-1][1], **cols)


# --- the shortcut's rules, restated ---------------------------------------------------

@dataclass
class Bail:
    check: str          # which check handed the rest of the segment to the serial replay
    at: int             # the request (index in the batch) that failed it
    serial_from: int    # the first request replayed serially


@dataclass
class Plan:
    label: list         # per request of the batch: "first", "run" or "serial"
    bail: dict          # per key: Bail or None


def plan(case, rec):
    """A model of wave_win_segment (csrc/rl_replay_wave.h), in plain Python: which
    requests of the batch under test the wave takes exactly as a run's first
    ("first"), which it applies from the prefix sum ("run"), and which it
    leaves to lane 0's serial replay ("serial"), with the check that bailed
    out.  It reads the sorted batch and the oracle's record only.

    It MUST BE KEPT IN STEP with wave_win_segment, and it proves nothing about
    the kernel by itself: the predicates use it to state that a case reaches
    the path it was built for, the GPU tests compare results.

    The rules.  A segment shorter than HEAVY_MIN is replayed serially ("light");
    so is one whose config has ttl_c == 0 ("ttl_c").  Otherwise, run by run: the
    first request is exact; it bails out when the script errored
    ("first-error"), when the current key is not in the entry afterwards
    ("cur-spill") or when SW's previous key lives in the spill ("prev-spill").
    The run's other requests -- same config, same window -- are applied CHUNK at
    a time; a chunk bails out as a whole, from its first request, when any
    request of it finds the current key expired ("expired"), overflows INCRBY
    ("overflow") or would set the TTL again ("ttl-reset")."""
    key, ts, n, cfg, _ = case.test_batch
    m = len(ts)
    label, bails = [None] * m, {}
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    for idx in np.split(order, bounds):
        idx = idx.tolist()
        c0 = int(cfg[idx[0]])
        alg, _, W = CONFIGS[c0]
        ln, bail, pos = len(idx), None, 0
        if ln < HEAVY_MIN:
            bail = Bail("light", idx[0], 0)
        elif ttl_c(W) <= 0:
            bail = Bail("ttl_c", idx[0], 0)
        while bail is None and pos < ln:
            i0 = idx[pos]
            if int(cfg[i0]) != c0:
                bail = Bail("config", i0, pos)
                break
            label[i0] = "first"
            pos += 1
            if rec.err[i0]:
                bail = Bail("first-error", i0, pos)
            elif not rec.cur_in_entry[i0]:
                bail = Bail("cur-spill", i0, pos)
            elif alg == SW and rec.prev_in_spill[i0]:
                bail = Bail("prev-spill", i0, pos)
            run_end = False
            while bail is None and not run_end and pos < ln:
                lim = 0
                while lim < CHUNK and pos + lim < ln:
                    i = idx[pos + lim]
                    if int(cfg[i]) != c0 or rec.ws[i] != rec.ws[i0]:
                        run_end = True
                        break
                    lim += 1
                for i in idx[pos:pos + lim]:
                    bad = "expired" if rec.cur_before[i] is None else "overflow" if rec.err[i] else \
                        "ttl-reset" if rec.ttl_set[i] else None
                    if bad:
                        bail = Bail(bad, i, pos)
                        break
                if bail is None:
                    for i in idx[pos:pos + lim]:
                        label[i] = "run"
                    pos += lim
                if lim == 0:
                    break
        if bail is not None:
            for i in idx[bail.serial_from:]:
                label[i] = "serial"
            bail.serial_from = idx[bail.serial_from] if bail.serial_from < ln else m
        bails[int(key[idx[0]])] = bail
    return Plan(label, bails)


def _labels(pl, lo, hi):
    return "".join(x[0] for x in pl.label[lo:hi])      # f / r / s per request


def _rle(dec):
    d = np.asarray(dec)
    return d[np.r_[True, d[1:] != d[:-1]]].tolist()


# --- (g) run geometry -------------------------------------------------------------------

G_RS = (0, 1, 5, 6, 7, 383, 384, 385, 768, 769)
G_B = 40


def two_runs_case(key, cfg, r):
    """Runs A (1 + r requests, half a second into a window) and B (G_B requests,
    from the next window's start), 1 ms apart: the window change falls at
    offset 1 + r."""
    _, _, W = CONFIGS[cfg]
    ts = np.r_[win_ns(W, 0) + 500 * MS + MS * np.arange(1 + r), win_ns(W, 1) + MS * np.arange(G_B)]
    return Case(f"g-two-runs-cfg{cfg}-r{r}", [_batch(key, ts, 1, cfg)],
                {"family": "g", "kind": "two-runs", "cfg": cfg, "runs": [1 + r, G_B]})


def new_windows_case(key, cfg):
    _, _, W = CONFIGS[cfg]
    ts = [win_ns(W, i) for i in range(HEAVY_MIN)]
    return Case(f"g-new-windows-cfg{cfg}", [_batch(key, ts, 1, cfg)],
                {"family": "g", "kind": "new-windows", "cfg": cfg, "runs": [1] * HEAVY_MIN})


def length_case(key, cfg, ln, gap=1_000_000):
    """One segment of ln requests: the short ones from a window start on, the
    long ones (20 ms gap) from the middle of a 60 s window, so that they cross
    into the next one at offset 1500 while SW's previous key still lives."""
    _, _, W = CONFIGS[cfg]
    ts = win_ns(W, 0) + (30 * NS + 7 * MS if ln > CHUNK else 0) + gap * np.arange(ln)
    w1 = int(np.searchsorted(ts, win_ns(W, 1)))
    runs = [w1, ln - w1] if w1 < ln else [ln]
    return Case(f"g-length-cfg{cfg}-{ln}", [_batch(key, ts, 1, cfg)],
                {"family": "g", "kind": "length", "cfg": cfg, "runs": runs}, small_max0=ln == SMALL_MAX)


def deny_allow_deny_case(key):
    """SW (100, 60 s): the previous window holds 100.  The run's first two
    requests are denied (101, 100.33 > 100), then one request a second is
    slower than the previous count decays (1.67 / s) and is allowed, then a
    burst 1 ms apart runs into the limit again."""
    W = 60 * NS
    w1 = win_ns(W, 1)
    paced = w1 + NS * np.arange(21)
    burst = paced[-1] + 1_000_000 * np.arange(1, 31)
    return Case("g-deny-allow-deny", [_batch(key, [w1 - 1], 100, SW_HI), _batch(key, np.r_[paced, burst], 1, SW_HI)],
                {"family": "g", "kind": "dad", "cfg": SW_HI, "runs": [51]})


def check_g(case, rec, pl):
    kind, cfg = case.claim["kind"], case.claim["cfg"]
    alg, L, _ = CONFIGS[cfg]
    runs = case.claim["runs"]
    m = len(rec.dec)
    assert sum(runs) == m
    (_, bail), = pl.bail.items()
    if m < HEAVY_MIN:
        assert bail.check == "light" and _labels(pl, 0, m) == "s" * m
    else:
        assert bail is None, f"{case.name}: bails out: {bail}"
        assert _labels(pl, 0, m) == "".join("f" + "r" * (r - 1) for r in runs), f"{case.name}: labels"
    o = 0
    for ri, r in enumerate(runs):
        assert len(set(rec.ws[o:o + r])) == 1 and (o == 0 or rec.ws[o] != rec.ws[o - 1]), f"{case.name}: run {ri}"
        if kind != "dad" and (alg == FW or ri == 0):
            # a fresh window and (SW) no previous count: allowed up to the limit, denied after it
            want = (np.arange(1, r + 1) <= L).astype(np.uint8)
            assert np.array_equal(rec.dec[o:o + r], want), f"{case.name}: run {ri}"
        if alg == SW and kind in ("two-runs", "length") and ri > 0:
            assert rec.prev_cnt[o:o + r] == [runs[ri - 1]] * r
        o += r
    if kind == "dad":
        assert rec.prev_cnt == [100] * m and _rle(rec.dec) == [0, 1, 0], f"{case.name}: {_rle(rec.dec)}"
        assert rec.dec[:3].tolist() == [0, 0, 1] and rec.dec[20] == 1 and rec.dec[-1] == 0


# --- (b) bail-outs --------------------------------------------------------------------------

B_OFFSETS = (1, 6, 383, 384, 385)
B_RUN, B_TAIL = 400, 8
B_M = B_RUN + B_TAIL


def _b_frame(cfg):
    """A run of B_RUN requests and B_TAIL more, 1 ms apart, one second into a
    window; for SW a batch before it that leaves 3 in the previous window."""
    alg, _, W = CONFIGS[cfg]
    w1 = win_ns(W, 1)
    ts = w1 + NS + MS * np.arange(B_M)
    prime = [_batch(0, [w1 - NS], 3, cfg)] if alg == SW else []
    return prime, ts, np.ones(B_M, np.int64)


def _b_case(name, key, cfg, prime, ts, n, sms, **claim):
    batches = [(np.full(len(b[1]), key, np.uint64),) + b[1:] for b in prime] + [_batch(key, ts, n, cfg, sms)]
    return Case(name, batches, dict(family="b", cfg=cfg, **claim))


def overflow_case(key, cfg, o):
    """2^62 from the run's first request, 2^62 again at o: INCRBY overflows, the
    script errors and the count stays."""
    prime, ts, n = _b_frame(cfg)
    n[0] = n[o] = 1 << 62
    return _b_case(f"b-overflow-cfg{cfg}-o{o}", key, cfg, prime, ts, n, None, kind="overflow", o=o, check="overflow")


def overflow_first_case(key, cfg):
    """The overflow on a run's first request: an earlier batch left 2^62."""
    _, _, W = CONFIGS[cfg]
    ts = win_ns(W, 1) + NS + MS * np.arange(1 + G_B)
    n = np.ones(G_B, np.int64)
    n[0] = 1 << 62
    return Case(f"b-overflow-first-cfg{cfg}", [_batch(key, ts[:1], 1 << 62, cfg), _batch(key, ts[1:], n, cfg)],
                {"family": "b", "cfg": cfg, "kind": "overflow", "o": 0, "check": "first-error"})


FF = 30_000      # ms the store's clock jumps ahead at the offset under test


def ttl_twin_case(key, cfg, o, big, before):
    """The count is `before` when n = big arrives at o, with the store's clock
    FF ms ahead from there on: Lua compares doubles, so the TTL is set again
    when before + big rounds to big.  The tail's first request comes 5 ms after
    the key's first expiry (long before a re-set one), still in the window."""
    _, _, W = CONFIGS[cfg]
    prime, ts, n = _b_frame(cfg)
    n[0] = before - (o - 1)
    n[o] = big
    sms = ts // MS
    sms[o:] += FF
    sms[B_RUN:] = sms[0] + ttl_c(W) * 1000 + 5 + np.arange(B_TAIL)
    reset = float(before + big) == float(big)
    return _b_case(f"b-ttl-{before}-cfg{cfg}-o{o}", key, cfg, prime, ts, n, sms, kind="ttl", o=o, reset=reset,
                   before=before, check="ttl-reset" if reset else "expired")


def expire_case(key, cfg, o, past):
    """The current key expires at o, with ts still in its window: the store's
    clock reaches the key's expiry (`when`) exactly -- alive under Redis 7,
    dead under miniredis -- or passes it by 1 ms."""
    _, _, W = CONFIGS[cfg]
    prime, ts, n = _b_frame(cfg)
    sms = ts // MS
    sms[o:] = sms[0] + ttl_c(W) * 1000 + past + np.arange(B_M - o)
    return _b_case(f"b-expire-{'past' if past else 'at'}-cfg{cfg}-o{o}", key, cfg, prime, ts, n, sms,
                   kind="expire", o=o, past=past, check="expired")


def expire_natural_case(key, cfg, o):
    """W = 1.5 s: ttl_c = 1 s is shorter than the window, so the key dies inside
    it on the requests' own clock (no server_ms)."""
    _, _, W = CONFIGS[cfg]
    ts = win_ns(W, 0) + MS * np.arange(B_M)
    ts[o:] += (1001 - o) * MS
    return _b_case(f"b-expire-natural-cfg{cfg}-o{o}", key, cfg, [], ts, np.ones(B_M, np.int64), None,
                   kind="expire", o=o, past=1, check="expired")


def _spill_prime(key, cfg, skew):
    """Window keys w1 < w2 < w3 of one user key, created in this order, all alive:
    the entry keeps w2 and w3, w1 moves to the spill.  SW: w2's requests keep w1
    alive (ttl_p).  FW (skew): the three app servers' clocks are a window apart
    while the store's clock moves 1 ms."""
    _, _, W = CONFIGS[cfg]
    w2, w3 = win_ns(W, 2), win_ns(W, 3)
    ts = [w2 - MS, w2 + 59 * NS, w3]
    return _batch(key, ts, [2, 3, 4], cfg, [w3 // MS + i for i in range(3)] if skew else None)


def prev_spill_case(key, o):
    """SW: o requests in w3, then the key's time steps back into w2, whose
    previous window w1 lives in the spill, for a run of G_B requests; a tail in
    w3 again.  The store's clock goes on."""
    W = 60 * NS
    w2, w3 = win_ns(W, 2), win_ns(W, 3)
    ts = np.r_[w3 + 10 * MS + MS * np.arange(o), w2 + 59 * NS + 500 * MS + MS * np.arange(G_B),
               w3 + NS + MS * np.arange(B_TAIL)]
    sms = w3 // MS + 10 + np.arange(len(ts))
    return Case(f"b-prev-spill-o{o}", [_spill_prime(key, SW_HI, False), _batch(key, ts, 1, SW_HI, sms)],
                {"family": "b", "cfg": SW_HI, "kind": "prev-spill", "o": o, "check": "prev-spill"})


def ttl0_case(key, cfg):
    _, _, W = CONFIGS[cfg]
    ts = win_ns(W, 0) + MS * np.arange(G_B)
    return Case(f"b-ttl0-cfg{cfg}", [_batch(key, ts, 1, cfg)], {"family": "b", "cfg": cfg, "kind": "ttl0", "o": 0,
                                                                "check": "ttl_c"})


def half_windows_case(key):
    """SW, W = 1.5 s, a request every 100 ms over six windows.  Window keys are
    named by whole seconds: pws = ws - 1 is the previous window's key only from
    a window that starts on a half second."""
    W = 1_500_000_000
    ts = win_ns(W, 0) + 100 * MS * np.arange(90)
    return Case("b-half-windows", [_batch(key, ts, 1, SW_15)], {"family": "b", "cfg": SW_15, "kind": "half", "o": None,
                                                                "check": "expired"})


def check_b(case, rec, pl, profile):
    cl = case.claim
    kind, o, cfg = cl["kind"], cl["o"], cl["cfg"]
    alg, L, W = CONFIGS[cfg]
    (_, bail), = pl.bail.items()
    m = len(rec.dec)
    assert bail is not None, f"{case.name}: no bail-out"
    want = o
    if kind == "expire" and not cl["past"] and profile == rpy.REDIS7:
        want = o + 1                      # `when` itself is alive under Redis 7: the next request finds the key gone
    if kind == "ttl" and not cl["reset"]:
        want = B_RUN                      # the twin without the re-set runs on until the tail finds the key gone
    if kind == "prev-spill":
        # the bail-out follows the exact first request of the run in w2; the o requests before it are a run in w3
        assert _labels(pl, 0, m) == "f" + "r" * (o - 1) + "f" + "s" * (m - o - 1), f"{case.name}: {_labels(pl, 0, m)}"
        assert rec.prev_in_spill[o] and rec.prev_cnt[o] == 2 and rec.cur_before[o] == 3 and rec.cur_in_entry[o]
        assert not rec.prev_in_spill[:o].any() and rec.prev_cnt[:o] == [3] * o
    if kind == "half":
        starts = [rpy.window_start(int(t), W) * NS == (int(t) - (int(t) + rpy.UNIX_TO_INTERNAL * NS) % W)
                  for t in case.test_batch[1]]          # the request's window starts on a whole second
        found = [p is not None for p in rec.prev_cnt]
        assert not any(f and s for f, s in zip(found, starts)), f"{case.name}: previous count found from a whole second"
        halves = sorted({w for w, s in zip(rec.ws, starts) if not s})
        assert len(halves) == 3 and all(any(f for f, w in zip(found, rec.ws) if w == h) for h in halves)
        assert bail.check == "expired"
        return
    assert bail.check == cl["check"], f"{case.name}: bails out on {bail}"
    assert bail.at == want, f"{case.name}: bails out at {bail.at}, not {want}"
    if kind == "overflow":
        assert rec.dec[o] == rpy.ERROR and rec.err.sum() == 1
        assert rec.cur_after[o] == rec.cur_before[o] == (1 << 62) + max(o - 1, 0)
        assert rec.cur_after[m - 1] == (1 << 62) + m - 2 + (o == 0)      # every other request of the batch counted
    elif kind == "ttl":
        t0 = B_RUN
        assert rec.ttl_set[o] == cl["reset"] and rec.ttl_set[1:].sum() == int(cl["reset"]) + int(not cl["reset"])
        assert rec.cur_before[o] == cl["before"]
        assert rec.s_ms[t0] > rec.when_after[0] and rec.ws[t0] == rec.ws[0]
        if cl["reset"]:
            assert rec.when_after[o] == rec.s_ms[o] + ttl_c(W) * 1000 >= rec.s_ms[m - 1]
            assert not rec.created[1:].any() and rec.cur_before[t0] is not None
        else:
            assert rec.when_after[o] == rec.when_after[0]
            assert rec.created[t0] and rec.created[1:].sum() == 1 and rec.cur_after[t0] == 1
    elif kind == "expire":
        assert rec.created[want] and rec.created.sum() == 2 and rec.cur_after[want] == 1, f"{case.name}: expiry"
        assert rec.ws[want] == rec.ws[0] == rec.ws[m - 1]
        assert rec.s_ms[o] == rec.when_after[0] + cl["past"] or case.test_batch[4] is None
        assert rec.dec[want] == 1 and (want <= L or rec.dec[want - 1] == 0)
    elif kind == "ttl0":
        assert rec.created.all() and (rec.dec == 1).all() and all(c is None for c in rec.cur_after)
        assert _labels(pl, 0, m) == "s" * m
    if kind in ("overflow", "ttl", "expire"):
        # nothing bails out before: the chunks before the failing one are applied as a run
        first = 1 + (bail.at - 1) // CHUNK * CHUNK if bail.at > 0 else 0
        if cl["check"] == "first-error":
            first = 1
        assert bail.serial_from == first, f"{case.name}: serial from {bail.serial_from}, not {first}"
        assert _labels(pl, 0, m) == ("f" + "r" * (first - 1) + "s" * (m - first))


# --- (s) weighted-count straddles ------------------------------------------------------------

def weighted(p, el, W, cc):
    """The reference arithmetic (slidingwindow.go calculateWeightedCount, as
    Sim._sw): a division, a subtraction, a product and a sum, each rounded."""
    progress = float(el) / float(W)
    w = float(p) * (1.0 - progress)
    return w + float(cc)


def visible(w, limit):
    """What a caller sees of a weighted count: (allowed, remaining)."""
    return w <= float(limit), max(0, rpy.wrap64(limit - rpy.go_f2i(w)))


def exact(p, el, W, cc):
    return Fraction(p) * (1 - Fraction(el, W)) + cc


def side(p, el, W, cc):
    """-1 / 0 / 1: the reference arithmetic lands below / on / above the exact
    value (an integer at every point of family s)."""
    w, x = Fraction(weighted(p, el, W, cc)), exact(p, el, W, cc)
    return (w > x) - (w < x)


def twice_rounded(p, el, W, cc):
    """The product's rounding error is large enough that the sum, rounded once
    from the unrounded product, would differ from the reference's."""
    one_minus = 1.0 - float(el) / float(W)
    q = Fraction(float(p)) * Fraction(one_minus) + cc
    return float(q) != weighted(p, el, W, cc)


S_CCS, S_PMAX, S_ON_EVERY = (1, 5, 50), 400, 10


def search_light():
    """Every (W, L, p, el, cc) with W in S_LIGHT_WINDOWS, L = S_LIMIT, cc in
    S_CCS, k = L - cc or L - cc - 1 (the exact weighted count k + cc is L or
    L - 1: one ulp shows in the decision or in `remaining`; at L + 1 nothing
    would show), k < p <= S_PMAX and el = W (p - k) / p a whole number of ns.
    Kept: every point where the reference arithmetic lands off the integer or
    is twice_rounded, and every S_ON_EVERY-th of the others."""
    out, on = [], 0
    for W in S_LIGHT_WINDOWS:
        for cc in S_CCS:
            for k in (S_LIMIT - cc - 1, S_LIMIT - cc):
                for p in range(k + 1, S_PMAX + 1):
                    if (W * (p - k)) % p:
                        continue
                    pt = (W, S_LIMIT, p, W * (p - k) // p, cc)
                    if side(*pt[2:4], W, cc) or twice_rounded(*pt[2:4], W, cc):
                        out.append(pt)
                    else:
                        on += 1
                        if on % S_ON_EVERY == 0:
                            out.append(pt)
    return tuple(out)


RUN_WINDOWS = (2 * NS, 3 * NS, YEAR)
RUN_P, RUN_P_LONG = range(33, CHUNK + 1), range(CHUNK + 2, 2 * CHUNK + 2)


def run_points(W, L, p):
    """The run shape: request j = 1 .. p - 1 at el_j = W j / p with the current
    count cc_j = L - (p - j): the exact weighted count is L throughout."""
    return [(p, W * j // p, W, L - (p - j)) for j in range(1, p)]


def search_runs():
    """(W, L, p) with L = p and p a divisor of W.  Scored by the number of
    requests where the reference arithmetic lands off the limit or is
    twice_rounded.  Per window of RUN_WINDOWS the best p of RUN_P (one heavy
    segment in one chunk), ties to the larger p; for the longest window also the
    second best and the best of RUN_P_LONG (a run that spans chunks).
    Searched: W in RUN_WINDOWS, p in 33 .. 769."""
    def score(W, p):
        return sum(1 for q in run_points(W, p, p) if side(*q) or twice_rounded(*q))

    out = []
    for W in RUN_WINDOWS:
        ranked = sorted((p for p in RUN_P if W % p == 0), key=lambda p: (score(W, p), p), reverse=True)
        picks = ranked[:2] if W == RUN_WINDOWS[-1] else ranked[:1]
        if W == RUN_WINDOWS[-1]:
            picks.append(max((p for p in RUN_P_LONG if W % p == 0), key=lambda p: (score(W, p), p)))
        out += [(W, p, p) for p in sorted(picks)]
    return tuple(out)


# (W, L, p, el, cc): search_light()'s result (tests/test_window_cases.py re-derives it)
S_LIGHT = (
    (2000000000, 100, 175, 880000000, 1), (2000000000, 100, 245, 1200000000, 1),
    (2000000000, 100, 350, 1440000000, 1), (2000000000, 100, 125, 416000000, 1), (2000000000, 100, 150, 680000000, 1),
    (2000000000, 100, 180, 900000000, 1), (2000000000, 100, 220, 1100000000, 1),
    (2000000000, 100, 225, 1120000000, 1), (2000000000, 100, 240, 1175000000, 1),
    (2000000000, 100, 300, 1340000000, 1), (2000000000, 100, 320, 1381250000, 1),
    (2000000000, 100, 330, 1400000000, 1), (2000000000, 100, 360, 1450000000, 1),
    (2000000000, 100, 400, 1505000000, 1), (2000000000, 100, 100, 120000000, 5),
    (2000000000, 100, 320, 1412500000, 5), (2000000000, 100, 400, 1530000000, 5),
    (2000000000, 100, 304, 1375000000, 5), (2000000000, 100, 400, 1525000000, 5),
    (2000000000, 100, 112, 1125000000, 50), (2000000000, 100, 245, 1600000000, 50),
    (2000000000, 100, 250, 1608000000, 50), (2000000000, 100, 280, 1650000000, 50),
    (2000000000, 100, 320, 1693750000, 50), (2000000000, 100, 350, 1720000000, 50),
    (2000000000, 100, 400, 1755000000, 50), (2000000000, 100, 250, 1600000000, 50),
    (2000000000, 100, 320, 1687500000, 50), (3000000000, 100, 147, 1000000000, 1),
    (3000000000, 100, 160, 1162500000, 1), (3000000000, 100, 168, 1250000000, 1),
    (3000000000, 100, 175, 1320000000, 1), (3000000000, 100, 192, 1468750000, 1),
    (3000000000, 100, 294, 2000000000, 1), (3000000000, 100, 300, 2020000000, 1),
    (3000000000, 100, 336, 2125000000, 1), (3000000000, 100, 350, 2160000000, 1),
    (3000000000, 100, 375, 2216000000, 1), (3000000000, 100, 384, 2234375000, 1),
    (3000000000, 100, 132, 750000000, 1), (3000000000, 100, 135, 800000000, 1), (3000000000, 100, 150, 1020000000, 1),
    (3000000000, 100, 180, 1350000000, 1), (3000000000, 100, 216, 1625000000, 1),
    (3000000000, 100, 220, 1650000000, 1), (3000000000, 100, 225, 1680000000, 1),
    (3000000000, 100, 256, 1839843750, 1), (3000000000, 100, 270, 1900000000, 1),
    (3000000000, 100, 297, 2000000000, 1), (3000000000, 100, 300, 2010000000, 1),
    (3000000000, 100, 320, 2071875000, 1), (3000000000, 100, 330, 2100000000, 1),
    (3000000000, 100, 360, 2175000000, 1), (3000000000, 100, 400, 2257500000, 1),
    (3000000000, 100, 120, 650000000, 5), (3000000000, 100, 141, 1000000000, 5),
    (3000000000, 100, 240, 1825000000, 5), (3000000000, 100, 256, 1898437500, 5),
    (3000000000, 100, 282, 2000000000, 5), (3000000000, 100, 320, 2118750000, 5),
    (3000000000, 100, 375, 2248000000, 5), (3000000000, 100, 384, 2265625000, 5),
    (3000000000, 100, 150, 1100000000, 5), (3000000000, 100, 228, 1750000000, 5),
    (3000000000, 100, 240, 1812500000, 5), (3000000000, 100, 285, 2000000000, 5),
    (3000000000, 100, 320, 2109375000, 5), (3000000000, 100, 375, 2240000000, 5),
    (3000000000, 100, 384, 2257812500, 5), (3000000000, 100, 400, 2287500000, 5),
    (3000000000, 100, 96, 1468750000, 50), (3000000000, 100, 150, 2020000000, 50),
    (3000000000, 100, 210, 2300000000, 50), (3000000000, 100, 240, 2387500000, 50),
    (3000000000, 100, 245, 2400000000, 50), (3000000000, 100, 250, 2412000000, 50),
    (3000000000, 100, 280, 2475000000, 50), (3000000000, 100, 294, 2500000000, 50),
    (3000000000, 100, 320, 2540625000, 50), (3000000000, 100, 336, 2562500000, 50),
    (3000000000, 100, 350, 2580000000, 50), (3000000000, 100, 375, 2608000000, 50),
    (3000000000, 100, 384, 2617187500, 50), (3000000000, 100, 400, 2632500000, 50),
    (3000000000, 100, 128, 1828125000, 50), (3000000000, 100, 240, 2375000000, 50),
    (3000000000, 100, 250, 2400000000, 50), (3000000000, 100, 300, 2500000000, 50),
    (3000000000, 100, 375, 2600000000, 50), (3000000000, 100, 384, 2609375000, 50),
    (7000000000, 100, 125, 1512000000, 1), (7000000000, 100, 175, 3080000000, 1),
    (7000000000, 100, 280, 4550000000, 1), (7000000000, 100, 350, 5040000000, 1),
    (7000000000, 100, 125, 1456000000, 1), (7000000000, 100, 140, 2050000000, 1),
    (7000000000, 100, 150, 2380000000, 1), (7000000000, 100, 154, 2500000000, 1),
    (7000000000, 100, 180, 3150000000, 1), (7000000000, 100, 192, 3390625000, 1),
    (7000000000, 100, 220, 3850000000, 1), (7000000000, 100, 225, 3920000000, 1),
    (7000000000, 100, 231, 4000000000, 1), (7000000000, 100, 252, 4250000000, 1),
    (7000000000, 100, 280, 4525000000, 1), (7000000000, 100, 288, 4593750000, 1),
    (7000000000, 100, 300, 4690000000, 1), (7000000000, 100, 308, 4750000000, 1),
    (7000000000, 100, 320, 4834375000, 1), (7000000000, 100, 330, 4900000000, 1),
    (7000000000, 100, 336, 4937500000, 1), (7000000000, 100, 350, 5020000000, 1),
    (7000000000, 100, 360, 5075000000, 1), (7000000000, 100, 385, 5200000000, 1),
    (7000000000, 100, 400, 5267500000, 1), (7000000000, 100, 140, 2300000000, 5),
    (7000000000, 100, 160, 2887500000, 5), (7000000000, 100, 224, 4062500000, 5),
    (7000000000, 100, 280, 4650000000, 5), (7000000000, 100, 320, 4943750000, 5),
    (7000000000, 100, 400, 5355000000, 5), (7000000000, 100, 175, 3200000000, 5),
    (7000000000, 100, 200, 3675000000, 5), (7000000000, 100, 224, 4031250000, 5),
    (7000000000, 100, 266, 4500000000, 5), (7000000000, 100, 350, 5100000000, 5),
    (7000000000, 100, 400, 5337500000, 5), (7000000000, 100, 70, 2100000000, 50),
    (7000000000, 100, 196, 5250000000, 50), (7000000000, 100, 245, 5600000000, 50),
    (7000000000, 100, 250, 5628000000, 50), (7000000000, 100, 280, 5775000000, 50),
    (7000000000, 100, 320, 5928125000, 50), (7000000000, 100, 343, 6000000000, 50),
    (7000000000, 100, 400, 6142500000, 50), (7000000000, 100, 100, 3500000000, 50),
    (7000000000, 100, 250, 5600000000, 50), (7000000000, 100, 280, 5750000000, 50),
    (7000000000, 100, 320, 5906250000, 50), (7000000000, 100, 350, 6000000000, 50),
    (12000000000, 100, 147, 4000000000, 1), (12000000000, 100, 160, 4650000000, 1),
    (12000000000, 100, 168, 5000000000, 1), (12000000000, 100, 175, 5280000000, 1),
    (12000000000, 100, 192, 5875000000, 1), (12000000000, 100, 294, 8000000000, 1),
    (12000000000, 100, 300, 8080000000, 1), (12000000000, 100, 336, 8500000000, 1),
    (12000000000, 100, 350, 8640000000, 1), (12000000000, 100, 375, 8864000000, 1),
    (12000000000, 100, 384, 8937500000, 1), (12000000000, 100, 132, 3000000000, 1),
    (12000000000, 100, 135, 3200000000, 1), (12000000000, 100, 150, 4080000000, 1),
    (12000000000, 100, 180, 5400000000, 1), (12000000000, 100, 216, 6500000000, 1),
    (12000000000, 100, 220, 6600000000, 1), (12000000000, 100, 225, 6720000000, 1),
    (12000000000, 100, 256, 7359375000, 1), (12000000000, 100, 270, 7600000000, 1),
    (12000000000, 100, 297, 8000000000, 1), (12000000000, 100, 300, 8040000000, 1),
    (12000000000, 100, 320, 8287500000, 1), (12000000000, 100, 330, 8400000000, 1),
    (12000000000, 100, 360, 8700000000, 1), (12000000000, 100, 400, 9030000000, 1),
    (12000000000, 100, 120, 2600000000, 5), (12000000000, 100, 141, 4000000000, 5),
    (12000000000, 100, 240, 7300000000, 5), (12000000000, 100, 256, 7593750000, 5),
    (12000000000, 100, 282, 8000000000, 5), (12000000000, 100, 320, 8475000000, 5),
    (12000000000, 100, 375, 8992000000, 5), (12000000000, 100, 384, 9062500000, 5),
    (12000000000, 100, 150, 4400000000, 5), (12000000000, 100, 228, 7000000000, 5),
    (12000000000, 100, 240, 7250000000, 5), (12000000000, 100, 285, 8000000000, 5),
    (12000000000, 100, 320, 8437500000, 5), (12000000000, 100, 375, 8960000000, 5),
    (12000000000, 100, 384, 9031250000, 5), (12000000000, 100, 400, 9150000000, 5),
    (12000000000, 100, 96, 5875000000, 50), (12000000000, 100, 150, 8080000000, 50),
    (12000000000, 100, 210, 9200000000, 50), (12000000000, 100, 240, 9550000000, 50),
    (12000000000, 100, 245, 9600000000, 50), (12000000000, 100, 250, 9648000000, 50),
    (12000000000, 100, 280, 9900000000, 50), (12000000000, 100, 294, 10000000000, 50),
    (12000000000, 100, 320, 10162500000, 50), (12000000000, 100, 336, 10250000000, 50),
    (12000000000, 100, 350, 10320000000, 50), (12000000000, 100, 375, 10432000000, 50),
    (12000000000, 100, 384, 10468750000, 50), (12000000000, 100, 400, 10530000000, 50),
    (12000000000, 100, 128, 7312500000, 50), (12000000000, 100, 240, 9500000000, 50),
    (12000000000, 100, 250, 9600000000, 50), (12000000000, 100, 300, 10000000000, 50),
    (12000000000, 100, 375, 10400000000, 50), (12000000000, 100, 384, 10437500000, 50),
    (60000000000, 100, 112, 7500000000, 1), (60000000000, 100, 147, 20000000000, 1),
    (60000000000, 100, 168, 25000000000, 1), (60000000000, 100, 175, 26400000000, 1),
    (60000000000, 100, 192, 29375000000, 1), (60000000000, 100, 224, 33750000000, 1),
    (60000000000, 100, 294, 40000000000, 1), (60000000000, 100, 336, 42500000000, 1),
    (60000000000, 100, 350, 43200000000, 1), (60000000000, 100, 375, 44320000000, 1),
    (60000000000, 100, 384, 44687500000, 1), (60000000000, 100, 100, 600000000, 1),
    (60000000000, 100, 135, 16000000000, 1), (60000000000, 100, 150, 20400000000, 1),
    (60000000000, 100, 176, 26250000000, 1), (60000000000, 100, 180, 27000000000, 1),
    (60000000000, 100, 216, 32500000000, 1), (60000000000, 100, 220, 33000000000, 1),
    (60000000000, 100, 225, 33600000000, 1), (60000000000, 100, 270, 38000000000, 1),
    (60000000000, 100, 297, 40000000000, 1), (60000000000, 100, 300, 40200000000, 1),
    (60000000000, 100, 320, 41437500000, 1), (60000000000, 100, 330, 42000000000, 1),
    (60000000000, 100, 352, 43125000000, 1), (60000000000, 100, 360, 43500000000, 1),
    (60000000000, 100, 400, 45150000000, 1), (60000000000, 100, 141, 20000000000, 5),
    (60000000000, 100, 160, 24750000000, 5), (60000000000, 100, 240, 36500000000, 5),
    (60000000000, 100, 282, 40000000000, 5), (60000000000, 100, 320, 42375000000, 5),
    (60000000000, 100, 375, 44960000000, 5), (60000000000, 100, 384, 45312500000, 5),
    (60000000000, 100, 96, 625000000, 5), (60000000000, 100, 192, 30312500000, 5),
    (60000000000, 100, 228, 35000000000, 5), (60000000000, 100, 240, 36250000000, 5),
    (60000000000, 100, 285, 40000000000, 5), (60000000000, 100, 375, 44800000000, 5),
    (60000000000, 100, 384, 45156250000, 5), (60000000000, 100, 400, 45750000000, 5),
    (60000000000, 100, 60, 11000000000, 50), (60000000000, 100, 112, 33750000000, 50),
    (60000000000, 100, 192, 44687500000, 50), (60000000000, 100, 210, 46000000000, 50),
    (60000000000, 100, 240, 47750000000, 50), (60000000000, 100, 245, 48000000000, 50),
    (60000000000, 100, 250, 48240000000, 50), (60000000000, 100, 280, 49500000000, 50),
    (60000000000, 100, 294, 50000000000, 50), (60000000000, 100, 320, 50812500000, 50),
    (60000000000, 100, 336, 51250000000, 50), (60000000000, 100, 375, 52160000000, 50),
    (60000000000, 100, 384, 52343750000, 50), (60000000000, 100, 400, 52650000000, 50),
    (60000000000, 100, 75, 20000000000, 50), (60000000000, 100, 200, 45000000000, 50),
    (60000000000, 100, 240, 47500000000, 50), (60000000000, 100, 250, 48000000000, 50),
    (60000000000, 100, 300, 50000000000, 50), (60000000000, 100, 375, 52000000000, 50),
    (60000000000, 100, 384, 52187500000, 50), (86400000000000, 100, 126, 19200000000000, 1),
    (86400000000000, 100, 135, 23680000000000, 1), (86400000000000, 100, 147, 28800000000000, 1),
    (86400000000000, 100, 168, 36000000000000, 1), (86400000000000, 100, 175, 38016000000000, 1),
    (86400000000000, 100, 180, 39360000000000, 1), (86400000000000, 100, 189, 41600000000000, 1),
    (86400000000000, 100, 192, 42300000000000, 1), (86400000000000, 100, 224, 48600000000000, 1),
    (86400000000000, 100, 252, 52800000000000, 1), (86400000000000, 100, 270, 55040000000000, 1),
    (86400000000000, 100, 294, 57600000000000, 1), (86400000000000, 100, 320, 59940000000000, 1),
    (86400000000000, 100, 336, 61200000000000, 1), (86400000000000, 100, 350, 62208000000000, 1),
    (86400000000000, 100, 360, 62880000000000, 1), (86400000000000, 100, 375, 63820800000000, 1),
    (86400000000000, 100, 378, 64000000000000, 1), (86400000000000, 100, 384, 64350000000000, 1),
    (86400000000000, 100, 135, 23040000000000, 1), (86400000000000, 100, 144, 27000000000000, 1),
    (86400000000000, 100, 150, 29376000000000, 1), (86400000000000, 100, 162, 33600000000000, 1),
    (86400000000000, 100, 180, 38880000000000, 1), (86400000000000, 100, 216, 46800000000000, 1),
    (86400000000000, 100, 220, 47520000000000, 1), (86400000000000, 100, 225, 48384000000000, 1),
    (86400000000000, 100, 243, 51200000000000, 1), (86400000000000, 100, 264, 54000000000000, 1),
    (86400000000000, 100, 270, 54720000000000, 1), (86400000000000, 100, 297, 57600000000000, 1),
    (86400000000000, 100, 300, 57888000000000, 1), (86400000000000, 100, 320, 59670000000000, 1),
    (86400000000000, 100, 324, 60000000000000, 1), (86400000000000, 100, 330, 60480000000000, 1),
    (86400000000000, 100, 360, 62640000000000, 1), (86400000000000, 100, 400, 65016000000000, 1),
    (86400000000000, 100, 120, 18720000000000, 5), (86400000000000, 100, 141, 28800000000000, 5),
    (86400000000000, 100, 180, 41280000000000, 5), (86400000000000, 100, 216, 48800000000000, 5),
    (86400000000000, 100, 225, 50304000000000, 5), (86400000000000, 100, 240, 52560000000000, 5),
    (86400000000000, 100, 270, 56320000000000, 5), (86400000000000, 100, 282, 57600000000000, 5),
    (86400000000000, 100, 288, 58200000000000, 5), (86400000000000, 100, 320, 61020000000000, 5),
    (86400000000000, 100, 360, 63840000000000, 5), (86400000000000, 100, 375, 64742400000000, 5),
    (86400000000000, 100, 384, 65250000000000, 5), (86400000000000, 100, 114, 14400000000000, 5),
    (86400000000000, 100, 180, 40800000000000, 5), (86400000000000, 100, 216, 48400000000000, 5),
    (86400000000000, 100, 225, 49920000000000, 5), (86400000000000, 100, 228, 50400000000000, 5),
    (86400000000000, 100, 240, 52200000000000, 5), (86400000000000, 100, 285, 57600000000000, 5),
    (86400000000000, 100, 288, 57900000000000, 5), (86400000000000, 100, 342, 62400000000000, 5),
    (86400000000000, 100, 360, 63600000000000, 5), (86400000000000, 100, 375, 64512000000000, 5),
    (86400000000000, 100, 384, 65025000000000, 5), (86400000000000, 100, 400, 65880000000000, 5),
    (86400000000000, 100, 75, 29952000000000, 50), (86400000000000, 100, 120, 51120000000000, 50),
    (86400000000000, 100, 168, 61200000000000, 50), (86400000000000, 100, 189, 64000000000000, 50),
    (86400000000000, 100, 210, 66240000000000, 50), (86400000000000, 100, 225, 67584000000000, 50),
    (86400000000000, 100, 240, 68760000000000, 50), (86400000000000, 100, 245, 69120000000000, 50),
    (86400000000000, 100, 250, 69465600000000, 50), (86400000000000, 100, 270, 70720000000000, 50),
    (86400000000000, 100, 280, 71280000000000, 50), (86400000000000, 100, 288, 71700000000000, 50),
    (86400000000000, 100, 294, 72000000000000, 50), (86400000000000, 100, 320, 73170000000000, 50),
    (86400000000000, 100, 336, 73800000000000, 50), (86400000000000, 100, 360, 74640000000000, 50),
    (86400000000000, 100, 375, 75110400000000, 50), (86400000000000, 100, 378, 75200000000000, 50),
    (86400000000000, 100, 384, 75375000000000, 50), (86400000000000, 100, 400, 75816000000000, 50),
    (86400000000000, 100, 80, 32400000000000, 50), (86400000000000, 100, 150, 57600000000000, 50),
    (86400000000000, 100, 240, 68400000000000, 50), (86400000000000, 100, 250, 69120000000000, 50),
    (86400000000000, 100, 270, 70400000000000, 50), (86400000000000, 100, 288, 71400000000000, 50),
    (86400000000000, 100, 300, 72000000000000, 50), (86400000000000, 100, 360, 74400000000000, 50),
    (86400000000000, 100, 375, 74880000000000, 50), (86400000000000, 100, 384, 75150000000000, 50),
)


def light_case(key0):
    """One key per point of S_LIGHT.  First batch: n = p at the last ns of the
    window before (denied when p > L, but counted).  Batch under test: n = cc
    at el into the window."""
    pts = S_LIGHT
    w1 = np.array([win_ns(W, 1) for W, *_ in pts], np.int64)
    keys = key0 + np.arange(len(pts), dtype=np.uint64)
    cfg = [cfg_of(SW, L, W) for W, L, *_ in pts]
    el = np.array([el for *_, el, _ in pts], np.int64)
    return Case("s-light", [_batch(keys, w1 - 1, [p for _, _, p, _, _ in pts], cfg),
                            _batch(keys, w1 + el, [cc for *_, cc in pts], cfg)],
                {"family": "s", "kind": "light", "points": pts})


def run_case(key, W, L, p, cut=None):
    w1 = win_ns(W, 1)
    pts = run_points(W, L, p)
    ts = w1 + np.array([el for _, el, _, _ in pts], np.int64)
    n = np.ones(p - 1, np.int64)
    n[0] = L - p + 1
    cfg = cfg_of(SW, L, W)
    batches = [_batch(key, [w1 - 1], p, cfg)]
    if cut:
        batches.append(_batch(key, ts[:cut], n[:cut], cfg))
    batches.append(_batch(key, ts[cut or 0:], n[cut or 0:], cfg))
    return Case(f"s-run-{W // NS}s-{p}" + (f"-cut{cut}" if cut else ""), batches,
                {"family": "c" if cut else "s", "kind": "run", "run": (W, L, p), "cut": cut or 0})


def check_s(case, rec, pl):
    if case.claim["kind"] == "light":
        pts = case.claim["points"]
        assert len(pts) == len(rec.dec)
        for i, (W, L, p, el, cc) in enumerate(pts):
            x = exact(p, el, W, cc)
            assert x.denominator == 1 and L - 1 <= x <= L and 0 < el < W, f"{case.name}: point {i}"
            assert rec.prev_cnt[i] == p and rec.created[i] and rec.cur_after[i] == cc, f"{case.name}: point {i}"
            assert (bool(rec.dec[i]), int(rec.rem[i])) == visible(weighted(p, el, W, cc), L)
        assert all(b.check == "light" for b in pl.bail.values())
        return
    W, L, p = case.claim["run"]
    cut = case.claim["cut"]
    pts = run_points(W, L, p)[cut:]
    m = len(pts)
    assert m == len(rec.dec) >= HEAVY_MIN
    (_, bail), = pl.bail.items()
    assert bail is None and _labels(pl, 0, m) == "f" + "r" * (m - 1), f"{case.name}: {bail}"
    for i, q in enumerate(pts):
        assert exact(*q) == L and rec.prev_cnt[i] == p and rec.cur_after[i] == q[3], f"{case.name}: request {i}"
        assert (bool(rec.dec[i]), int(rec.rem[i])) == visible(weighted(*q), L)
    if cut:
        assert side(*pts[0]) != 0 and not rec.created[0]     # the batch under test opens on a straddle


def side_counts(points):
    """{-1: below, 0: on, 1: above} over (p, el, W, cc) points."""
    out = {-1: 0, 0: 0, 1: 0}
    for q in points:
        out[side(*q)] += 1
    return out


def light_points():
    return [(p, el, W, cc, L) for W, L, p, el, cc in S_LIGHT]


def all_run_points():
    return [q + (L,) for W, L, p in S_RUNS for q in run_points(W, L, p)]


# --- (c) state carried between batches ---------------------------------------------------------

def carried_run_case(key, cfg):
    """20 requests of a window in one batch, 50 more of it in the next: the
    heavy segment's first request finds the key with a count."""
    _, _, W = CONFIGS[cfg]
    ts = win_ns(W, 1) + MS * np.arange(70)
    return Case(f"c-carried-run-cfg{cfg}", [_batch(key, ts[:20], 1, cfg), _batch(key, ts[20:], 1, cfg)],
                {"family": "c", "kind": "carried", "cfg": cfg, "before": 20, "prev": None})


def carried_prev_case(key):
    """SW: the previous window's 60 were written by an earlier batch."""
    w1 = win_ns(60 * NS, 1)
    return Case("c-carried-prev",
                [_batch(key, [w1 - NS], 60, SW_HI), _batch(key, w1 + 10 * NS + MS * np.arange(50), 1, SW_HI)],
                {"family": "c", "kind": "carried", "cfg": SW_HI, "before": None, "prev": 60})


def spilled_older_case(key, cfg):
    """The key's oldest window w1 sits in the spill when the batch starts
    (_spill_prime).  SW: a run in w3 -- nothing of the spill is touched.  FW
    (skewed app servers): a run in w3, then the key's time steps back into w1:
    the current key is the spilled one."""
    alg, _, W = CONFIGS[cfg]
    w1, w3 = win_ns(W, 1), win_ns(W, 3)
    ts = w3 + 10 * MS + MS * np.arange(G_B)
    if alg == FW:
        ts = np.r_[ts, w1 + 30 * NS + MS * np.arange(G_B)]
    sms = w3 // MS + 10 + np.arange(len(ts))
    return Case(f"c-spilled-older-cfg{cfg}", [_spill_prime(key, cfg, alg == FW), _batch(key, ts, 1, cfg, sms)],
                {"family": "c", "kind": "spilled", "cfg": cfg})


def check_c(case, rec, pl):
    kind = case.claim["kind"]
    if kind == "run":
        return check_s(case, rec, pl)
    alg, _, _ = CONFIGS[case.claim["cfg"]]
    (_, bail), = pl.bail.items()
    m = len(rec.dec)
    if kind == "carried":
        assert bail is None and _labels(pl, 0, m) == "f" + "r" * (m - 1)
        assert rec.cur_before[0] == case.claim["before"] and not rec.created[1:].any()
        assert rec.prev_cnt == [case.claim["prev"]] * m
        assert bool(rec.created[0]) == (case.claim["before"] is None)
    elif alg == SW:
        assert bail is None and _labels(pl, 0, m) == "f" + "r" * (m - 1)
        assert rec.cur_before[0] == 4 and rec.prev_cnt == [3] * m and not rec.prev_in_spill.any()
    else:
        assert _labels(pl, 0, m) == "f" + "r" * (G_B - 1) + "f" + "s" * (G_B - 1)
        assert bail.check == "cur-spill" and bail.at == G_B and not rec.cur_in_entry[G_B]
        assert rec.cur_before[0] == 4 and rec.cur_before[G_B] == 2 and rec.cur_after[m - 1] == 2 + G_B
        assert not rec.created.any() and rec.cur_in_entry[:G_B].all()


# --- all cases ---------------------------------------------------------------------------------

def check(case, rec, profile):
    """The case's predicate on the oracle's record (AssertionError when the
    trace does not contain what it was built for)."""
    pl = plan(case, rec)
    fam = case.claim["family"]
    if fam == "b":
        check_b(case, rec, pl, profile)
    else:
        {"g": check_g, "s": check_s, "c": check_c}[fam](case, rec, pl)
    # the shortcut's `pdead` branch (module docstring): inside a window run, the previous count a request
    # finds changes only where the current key is found dead as well
    for i in range(1, len(rec.dec)):
        if case.test_batch[0][i] == case.test_batch[0][i - 1] and rec.ws[i] == rec.ws[i - 1] and \
                rec.prev_cnt[i - 1] is not None and rec.prev_cnt[i] is None:
            assert rec.cur_before[i] is None, f"{case.name}: previous key dies alone at {i}"
    return pl


@functools.lru_cache(maxsize=None)
def all_cases():
    """{family: [Case]} -- every case with key ids of its own."""
    key = iter(range(20_000, 1 << 20, 16))
    out = {"g": [], "b": [], "s": [], "c": []}
    for cfg in (FW_HI, SW_HI, FW_LO, SW_LO):
        for r in G_RS:
            out["g"].append(two_runs_case(next(key), cfg, r))
    for cfg in (FW_LO, SW_LO):
        out["g"].append(new_windows_case(next(key), cfg))
    for cfg in (FW_HI, SW_HI):
        for ln in (HEAVY_MIN - 1, HEAVY_MIN, HEAVY_MIN + 1):
            out["g"].append(length_case(next(key), cfg, ln))
        for ln in (SMALL_MAX, SMALL_MAX + 1):
            out["g"].append(length_case(next(key), cfg, ln, gap=20 * MS))
    out["g"].append(deny_allow_deny_case(next(key)))

    for cfg in (FW_HI, SW_HI):
        for o in B_OFFSETS:
            out["b"].append(overflow_case(next(key), cfg, o))
            out["b"].append(ttl_twin_case(next(key), cfg, o, 1 << 62, 512))
            out["b"].append(ttl_twin_case(next(key), cfg, o, 1 << 62, 513))
            out["b"].append(expire_case(next(key), cfg, o, 0))
            out["b"].append(expire_case(next(key), cfg, o, 1))
        out["b"].append(overflow_first_case(next(key), cfg))
        out["b"].append(ttl_twin_case(next(key), cfg, 1, 1 << 53, 1))
        out["b"].append(ttl_twin_case(next(key), cfg, 1, 1 << 53, 2))
    for cfg in (FW_15, SW_15):
        for o in B_OFFSETS:
            out["b"].append(expire_natural_case(next(key), cfg, o))
    for o in B_OFFSETS:
        out["b"].append(prev_spill_case(next(key), o))
    for cfg in (FW_07, SW_07, FW_03, SW_03):
        out["b"].append(ttl0_case(next(key), cfg))
    out["b"].append(half_windows_case(next(key)))

    out["s"].append(light_case(next(key) + (1 << 20)))
    for W, L, p in S_RUNS:
        out["s"].append(run_case(next(key), W, L, p))

    for cfg in (FW_HI, SW_HI):
        out["c"].append(carried_run_case(next(key), cfg))
        out["c"].append(spilled_older_case(next(key), cfg))
    out["c"].append(carried_prev_case(next(key)))
    W, L, p = S_RUNS[0]
    pts = run_points(W, L, p)
    cut = next(j for j in range(1, p - 1 - HEAVY_MIN) if side(*pts[j]))
    out["c"].append(run_case(next(key), W, L, p, cut=cut))
    return out
