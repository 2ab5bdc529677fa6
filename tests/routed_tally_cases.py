"""Cases and models for the routed usage tally and top keys (include/rl_route.h
rl_tally_routed_device / rl_hot_routed_device, shard.RoutedPipeline(observe=),
shard.merge_tallies / merge_hots) -- TEST INFRASTRUCTURE ONLY.

  tally_part_of / hot_part_of   a reference model (tally_cases.Expected,
      hot_cases.HotModel) as the plain dict one rank's read travels as
  NumpyObserver        the two owner-side counters over host pointers: an
      observe= callable that recounts from the very buffers it is handed, and
      the reads shard.RoutedPipeline.usage / top_keys take
  expected_steps       ONE shared store over every rank's steps of the kinds
      D P R F C and A (allow_all): what every request was answered, and the
      order in which every owner saw its share
  union_model          the tally and the per-owner top-keys models over the
      executed requests of the observed steps
  check_usage / check_top_keys  a cluster read against them
"""
import numpy as np

import routed_allow_all_cases as ra
import routed_charge_cases as cc
import routed_op_cases as rc
import routed_refund_cases as rf
import shard
from hot_cases import HotModel
from route_ops import _arr
from tally_cases import expected_tally

U64 = np.uint64
D, P, R, F, C, A = cc.D, cc.P, cc.R, cc.F, cc.C, ra.A
DROPPED = rc.DROPPED
KINDS = [D, P, D, C, R, D, F, D, A]           # A takes two step numbers
OBSERVED = (D, A)

# rl_amd.TALLY_CFG / TALLY_KEY / HOT_KEY (test_routed_tally_abi.py pins them equal)
TALLY_CFG = np.dtype([("count", np.uint64, 4), ("units", np.uint64, 2)])
TALLY_KEY = np.dtype([("key_id", np.uint64), ("denied", np.uint64), ("units_denied", np.uint64),
                      ("cfg_id", np.uint32), ("pad_", np.uint32)])
HOT_KEY = np.dtype([("key_id", np.uint64), ("estimate", np.uint64), ("cfg_id", np.uint32), ("pad_", np.uint32)])


def code(dec):
    """an int64 decision as the counting kernels class it: 0..3, else a bad code (255)"""
    dec = np.asarray(dec, np.int64)
    return np.where((dec >= 0) & (dec <= 3), dec, 255).astype(np.uint8)


def tally_part_of(e, top, routed=None):
    """tally_cases.Expected as one rank's read with every key tracked: the
    `top` most denied keys (denied descending, key id ascending), each with the
    lowest config id that denied it"""
    cfg = np.zeros(e.count.shape[0], TALLY_CFG)
    cfg["count"], cfg["units"] = e.count, e.units
    ids = sorted(e.keys, key=lambda k: (-e.keys[k][0], k))[:top]
    keys = np.zeros(len(ids), TALLY_KEY)
    for i, k in enumerate(ids):
        keys[i] = (k, e.keys[k][0], e.keys[k][1], min(e.keys[k][2]), 0)
    info = dict(key_slots=0, keys_tracked=len(e.keys), untracked_requests=e.reserved[0],
                untracked_units=e.reserved[1], unknown_cfg=e.unknown_cfg, bad_codes=e.bad_codes, batches=0,
                requests=0)
    return dict(cfg=cfg, keys=keys, info=info, routed=dict(routed or dict(steps=0, requests=0, dropped_requests=0)))


def hot_part_of(mod, top):
    """hot_cases.HotModel as one rank's read with every candidate in the
    table: the `top` largest estimates (then key id), each with the lowest
    config id the model saw it hot with"""
    rows = mod.read()[:top]
    keys = np.zeros(len(rows), HOT_KEY)
    for i, (k, est) in enumerate(rows):
        keys[i] = (k, est, min(mod.candidates[k]), 0)
    info = dict(width=mod.width, depth=4, key_slots=0, hot_min=mod.hot_min, weight=mod.weight,
                keys_tracked=len(mod.candidates), dropped=0, total=mod.total, skipped=mod.skipped, batches=0,
                requests=0)
    return dict(keys=keys, info=info)


class NumpyObserver:
    """what an owner's engine counts of the routed steps it is shown, over host
    pointers: __call__ is an observe= callable (the signature of
    Engine.tally_routed), tally_read / hot_read are the `read` of
    RoutedPipeline.usage / top_keys.  calls[j]: the (key, cfg, n, decision
    int64) of the j-th step shown, in merge order."""

    def __init__(self, world, cap, ncfg, width=4096, hot_min=20, weight=0):
        self.world, self.cap, self.ncfg = world, cap, ncfg
        self.hot_args = (width, hot_min, ncfg, weight)
        self.calls, self.streams = [], []
        self.steps = self.dropped = 0

    def __call__(self, m_max, count, recv, order, sms, res, rcnt, world, stream):
        assert world == self.world and m_max == world * self.cap
        cnt = min(int(_arr(count, 1, np.int32)[0]), m_max)
        o = _arr(order, max(cnt, 1), np.int32)[:cnt].astype(np.int64)
        rec = _arr(recv, 4 * world * self.cap, np.int64).reshape(world * self.cap, 4)[o]
        dec = _arr(res, 4 * world * self.cap, np.int64).reshape(world * self.cap, 4)[o, 0]
        self.calls.append((rec[:, 0].copy().view(U64), (rec[:, 3] & 0xffffffff).astype(np.uint32), rec[:, 2].copy(),
                           dec.copy()))
        self.steps += 1
        if rcnt:
            self.dropped += int((_arr(rcnt, 4 * world, np.int64).reshape(world, 4)[:, 3] >> 1).sum())
        self.streams.append(stream)

    def _all(self):
        if not self.calls:
            return [np.zeros(0, t) for t in (U64, np.uint32, np.int64, np.int64)]
        return [np.concatenate([c[f] for c in self.calls]) for f in range(4)]

    def tally_read(self, top=0, clear=False):
        key, cfg, n, dec = self._all()
        part = tally_part_of(expected_tally(key, cfg, n, code(dec), self.ncfg), top,
                             dict(steps=self.steps, requests=key.size, dropped_requests=self.dropped))
        if clear:
            self.calls, self.steps, self.dropped = [], 0, 0
        return part

    def hot_read(self, top=0, clear=False):
        mod = HotModel(*self.hot_args)
        for key, cfg, n, dec in self.calls:
            mod.call(key, cfg, n, code(dec))
        part = hot_part_of(mod, top)
        if clear:
            self.calls, self.steps, self.dropped = [], 0, 0
        return part


# --- ONE shared store -----------------------------------------------------------------

def expected_steps(all_batches, kinds, configs, cap=None, profile=0):
    """every rank's steps on ONE shared store (routed_charge_cases /
    routed_allow_all_cases restated for the six kinds together).
    all_batches[r][b] = (key, ts, n or None, cfg), with `first` appended for A.
    -> per step dict(op, key, cfg, n, src, rows, seen): rows[i] the four result
    fields of request i of the union (rank-major; RL_DROPPED for a request
    dropped at its sender) -- of the member decide step for A -- and seen[w] the
    union indices owner w executed, in its merge order"""
    ref = rf.new_sim(configs, profile)
    algs = [c[0] for c in ref.cfgs]
    world = len(all_batches)
    clock = -(1 << 63)
    steps = []
    for b, op in enumerate(kinds):
        parts = [all_batches[r][b] for r in range(world)]
        parts = [tuple(np.zeros(p[0].size, np.int64) if (f == 2 and p[2] is None) else p[f] for f in range(len(p)))
                 for p in parts]
        U, src, pos, o, sms, clock, sent, _ = ra._merge([p[:4] for p in parts], world, cap, clock)
        full = np.zeros((U[0].size, 4), np.int64)
        full[:, 0] = DROPPED
        if op == A:
            full[o] = rc.step_rows(ref, D, U[0][o], U[1][o], U[2][o], U[3][o], sms)
            settled = [ra.settle_routed(algs, parts[r][4], parts[r][2], parts[r][3], full[src == r, 0])
                       for r in range(world)]
            gparts = [(parts[r][0], parts[r][1], settled[r][1], parts[r][3]) for r in range(world)]
            U2, _, _, o2, sms2, clock, _, _ = ra._merge(gparts, world, cap, clock, sel=[s[2] for s in settled])
            rf.refund_rows(ref, U2[0][o2], U2[1][o2], U2[2][o2], U2[3][o2], sms2)
        else:
            full[o] = cc.step_rows(ref, op, U[0][o], U[1][o], U[2][o], U[3][o], sms)
        own = shard.owner_of(U[0].astype(U64), world)
        steps.append(dict(op=op, key=U[0].astype(U64), cfg=U[3].astype(np.uint32), n=U[2], src=src, rows=full,
                          seen=[o[own[o] == w] for w in range(world)]))
    return steps


def observed_calls(steps, owner):
    """the (key, cfg, n, decision) an observer on `owner` is shown, step by step"""
    return [tuple(s[f][s["seen"][owner]] for f in ("key", "cfg", "n")) + (s["rows"][s["seen"][owner], 0],)
            for s in steps if s["op"] in OBSERVED]


def union_model(steps, world, ncfg, hot_args):
    """-> (tally_cases.Expected over every executed request of the observed
    steps; one HotModel per owner, fed step by step; the routed info of the
    cluster): what the owners' counters hold between them"""
    calls = [observed_calls(steps, w) for w in range(world)]
    allc = [c for w in range(world) for c in calls[w]]
    cat = [np.concatenate([c[f] for c in allc]) for f in range(4)]
    e = expected_tally(cat[0], cat[1], cat[2], code(cat[3]), ncfg)
    mods = []
    for w in range(world):
        mod = HotModel(*hot_args)
        for key, cfg, n, dec in calls[w]:
            mod.call(key, cfg, n, code(dec))
        mods.append(mod)
    nobs = sum(1 for s in steps if s["op"] in OBSERVED)
    routed = dict(steps=nobs * world, requests=int(cat[0].size),
                  dropped_requests=sum(int((s["rows"][:, 0] == DROPPED).sum()) for s in steps if s["op"] in OBSERVED))
    return e, mods, routed


def check_usage(got, e, routed, top, what=""):
    """a cluster read (shard.merge_tallies' dict) against the model"""
    assert np.array_equal(got["cfg"]["count"], e.count), f"{what} count"
    assert np.array_equal(got["cfg"]["units"], e.units), f"{what} units"
    i = got["info"]
    assert (i["unknown_cfg"], i["bad_codes"]) == (e.unknown_cfg, e.bad_codes), what
    assert (i["untracked_requests"], i["untracked_units"]) == tuple(e.reserved), what
    assert got["keys_tracked"] == i["keys_tracked"] == len(e.keys), what
    order = sorted(e.keys, key=lambda k: (-e.keys[k][0], k))[:top]
    assert [int(k) for k in got["keys"]["key_id"]] == order, f"{what} order"
    for r in got["keys"]:
        k = int(r["key_id"])
        assert (int(r["denied"]), int(r["units_denied"])) == (e.keys[k][0], e.keys[k][1]), what
        assert int(r["cfg_id"]) in e.keys[k][2], what
    assert got["routed"] == routed, f"{what}: routed info {got['routed']} != {routed}"


def check_top_keys(got, mods, top, what=""):
    """a cluster read (shard.merge_hots' dict) against the owners' models: their
    key sets are disjoint, so the cluster's list is their lists sorted together"""
    want = sorted((x for mod in mods for x in mod.read()), key=lambda x: (-x[1], x[0]))
    assert [(int(r["key_id"]), int(r["estimate"])) for r in got["keys"]] == want[:top], f"{what} keys"
    for r in got["keys"]:
        assert any(int(r["cfg_id"]) in mod.candidates.get(int(r["key_id"]), ()) for mod in mods), what
    i = got["info"]
    assert i["total"] == sum(mod.total for mod in mods) and i["skipped"] == sum(mod.skipped for mod in mods), what
    assert got["keys_tracked"] == i["keys_tracked"] == len(want) and i["dropped"] == 0, what
    assert (i["width"], i["hot_min"], i["weight"]) == (mods[0].width, mods[0].hot_min, mods[0].weight), what


# --- the pipeline case ------------------------------------------------------------------

def rank_batches(rank, world, configs, m=600, nkeys=150):
    """one app server's steps of KINDS: routed_charge_cases.rank_batches for
    the eight plain kinds and routed_allow_all_cases' members for A"""
    plain = cc.rank_batches(rank, configs, kinds=KINDS[:-1], m=m, nkeys=nkeys)
    return plain + [ra.rank_steps("mixed", rank, world, nkeys=nkeys)[0][1]]
