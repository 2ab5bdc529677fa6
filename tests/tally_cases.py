"""Reference for the usage tally (rl_tally_*, include/rl_engine.h;
csrc/rl_tally.h): what a finished batch (key, cfg, n, decision) adds to the
per-config counters, the global counters and the throttled-key table.  No GPU
here: test_tally_cases.py checks the numpy version against a brute-force one,
the GPU tests and the coalescer's host tally are compared with it."""
from dataclasses import dataclass, field

import numpy as np

from table_cases import mix64

U64 = np.uint64
M64 = (1 << 64) - 1
KEY_RESERVED = M64
DENIED, ALLOWED, ERROR, INVALID = 0, 1, 2, 3
PROBES = 64          # rl_tally.h TALLY_PROBES
LDS_CFGS = 32        # rl_tally.h TALLY_LDS_CFGS: config ids below it accumulate in LDS


@dataclass
class Expected:
    count: np.ndarray            # [ncfg, 4] uint64
    units: np.ndarray            # [ncfg, 2] uint64, modulo 2^64
    unknown_cfg: int = 0
    bad_codes: int = 0
    keys: dict = field(default_factory=dict)    # key id -> [denied, units_denied mod 2^64, {cfg ids}]
    reserved: list = field(default_factory=lambda: [0, 0])   # denied requests / units of KEY_RESERVED: never tracked

    @property
    def denied(self):
        return sum(v[0] for v in self.keys.values()) + self.reserved[0]

    @property
    def units_denied(self):
        return (sum(v[1] for v in self.keys.values()) + self.reserved[1]) & M64


def _arrays(key, cfg, n, dec):
    key = np.asarray(key, U64)
    cfg = np.asarray(cfg, np.uint32)
    n = np.asarray(n, np.int64)
    dec = np.asarray(dec, np.uint8)
    assert key.size == cfg.size == n.size == dec.size
    return key, cfg, n, dec


def expected_tally(key, cfg, n, dec, ncfg) -> Expected:
    """the tally of the requests, in any order and any split into batches"""
    key, cfg, n, dec = _arrays(key, cfg, n, dec)
    known = cfg < ncfg
    good = known & (dec <= 3)
    e = Expected(np.zeros((ncfg, 4), U64), np.zeros((ncfg, 2), U64))
    e.unknown_cfg = int((~known).sum())
    e.bad_codes = int((known & (dec > 3)).sum())
    u = np.where(n > 0, n, 0).astype(U64)
    with np.errstate(over="ignore"):
        for d in range(4):
            sel = good & (dec == d)
            e.count[:, d] = np.bincount(cfg[sel], minlength=ncfg).astype(U64)
            if d < 2:
                np.add.at(e.units[:, d], cfg[sel], u[sel])      # uint64: wraps
        den = good & (dec == DENIED)
        ids, inv = np.unique(key[den], return_inverse=True)
        cnt = np.bincount(inv, minlength=ids.size)
        us = np.zeros(ids.size, U64)
        np.add.at(us, inv, u[den])
    cfgs = [set() for _ in range(ids.size)]
    for j, c in zip(inv.tolist(), cfg[den].tolist()):
        cfgs[j].add(c)
    for j, k in enumerate(ids.tolist()):
        if k == KEY_RESERVED:
            e.reserved = [int(cnt[j]), int(us[j])]
        else:
            e.keys[k] = [int(cnt[j]), int(us[j]), cfgs[j]]
    return e


def brute_tally(key, cfg, n, dec, ncfg) -> Expected:
    """the same, one request at a time with Python integers"""
    key, cfg, n, dec = _arrays(key, cfg, n, dec)
    count = [[0] * 4 for _ in range(ncfg)]
    units = [[0] * 2 for _ in range(ncfg)]
    e = Expected(None, None)
    for k, c, x, d in zip(key.tolist(), cfg.tolist(), n.tolist(), dec.tolist()):
        if c >= ncfg:
            e.unknown_cfg += 1
            continue
        if d > 3:
            e.bad_codes += 1
            continue
        count[c][d] += 1
        x = x if x > 0 else 0
        if d < 2:
            units[c][d] = (units[c][d] + x) & M64
        if d == DENIED:
            if k == KEY_RESERVED:
                e.reserved = [e.reserved[0] + 1, (e.reserved[1] + x) & M64]
            else:
                r = e.keys.setdefault(k, [0, 0, set()])
                r[0] += 1
                r[1] = (r[1] + x) & M64
                r[2].add(c)
    e.count = np.array(count, U64).reshape(ncfg, 4)
    e.units = np.array(units, U64).reshape(ncfg, 2)
    return e


def fill(keys, slots):
    """the occupied slots of a `slots`-record table after inserting the distinct
    keys by unbounded linear probing from mix64(key) & (slots - 1) -> bool[slots],
    or None when they do not all fit.  The occupied set does not depend on the
    insertion order."""
    assert slots & (slots - 1) == 0
    keys = np.unique(np.asarray(keys, U64))
    if keys.size > slots:
        return None
    occ = np.zeros(slots, bool)
    for h in (mix64(keys) & U64(slots - 1)).astype(np.int64).tolist():
        while occ[h]:
            h = (h + 1) & (slots - 1)
        occ[h] = True
    return occ


def fits(denied_keys, slots):
    """every maximal run of occupied slots is at most min(slots, PROBES) long:
    then every key ends less than the probe bound from its home slot, whatever
    the order, and the table tracks all of them"""
    occ = fill(denied_keys, slots)
    if occ is None:
        return False
    if occ.all():
        return slots <= min(slots, PROBES)
    free = np.nonzero(~occ)[0]
    gaps = np.diff(np.concatenate([free, [free[0] + slots]])) - 1      # runs between free slots, cyclic
    return int(gaps.max()) <= min(slots, PROBES)


def host_table(keys_in_order, slots):
    """the keys a bounded-probe table tracks when the distinct keys arrive in
    this order (a sequential tally: the coalescer's host version) -> set"""
    probes, occ, tracked = min(slots, PROBES), {}, set()
    for k in keys_in_order:
        k = int(k)
        if k in tracked or k == KEY_RESERVED:
            continue
        h = int(mix64(k)[0]) & (slots - 1)
        for _ in range(probes):
            if h not in occ:
                occ[h] = k
                tracked.add(k)
                break
            h = (h + 1) & (slots - 1)
    return tracked


def check_read(t, e, ncfg, what=""):
    """a tally read `t` (rl_amd.Tally with every tracked key in t.keys) against
    Expected `e`, all of whose keys fit the table"""
    assert t.cfg.size == ncfg, what
    assert np.array_equal(t.cfg["count"], e.count), f"{what} count: {t.cfg['count'].tolist()} != {e.count.tolist()}"
    assert np.array_equal(t.cfg["units"], e.units), f"{what} units"
    assert (t.info.unknown_cfg, t.info.bad_codes) == (e.unknown_cfg, e.bad_codes), what
    assert (t.info.untracked_requests, t.info.untracked_units) == tuple(e.reserved), what
    assert t.keys_tracked == t.info.keys_tracked == len(e.keys), what
    got = {int(r["key_id"]): (int(r["denied"]), int(r["units_denied"])) for r in t.keys}
    assert got == {k: (v[0], v[1]) for k, v in e.keys.items()}, what
    for r in t.keys:
        assert int(r["cfg_id"]) in e.keys[int(r["key_id"])][2], what
    order = sorted(e.keys, key=lambda k: (-e.keys[k][0], k))
    assert [int(k) for k in t.keys["key_id"]] == order, f"{what} order"
