"""Cases and expectations for routed steps of five kinds -- decide, peek, reset,
refund and charge (include/rl_route.h, shard.RoutedPipeline) -- TEST
INFRASTRUCTURE ONLY.

Built on routed_refund_cases / routed_op_cases (the four earlier kinds) and
charge_cases.apply_charge (the Charge contract on the Python oracle, DESIGN.md
§10m).

  oracle_charge           rl_charge_routed_device over host pointers: the
      merged batch as ONE apply_charge call in merge order
  routed_expectations     routed_refund_cases.routed_expectations' merge
      restated with a charge kind: ONE shared store over every rank's steps, a
      charge step one apply_charge call over the step's merged batch;
      optionally the coverage of the charge steps
  rank_batches            one app server's steps of the kinds D C P D C R C F D
  charge_coverage         the coverage record of a set of ranks, asserted
"""
import numpy as np

import routed_op_cases as rc
import routed_refund_cases as rf
import shard
from charge_cases import apply_charge
from peek_cases import KEY_RESERVED
from route_ops import _arr
from tracegen import T0

D, P, R, F, C = shard.OP_DECIDE, shard.OP_PEEK, shard.OP_RESET, shard.OP_REFUND, shard.OP_CHARGE
KINDS = [D, C, P, D, C, R, C, F, D]
DROPPED = rc.DROPPED
BAD_CFG = rc.BAD_CFG
ALLOWED, DENIED, INVALID = 1, 0, 3
# every class of apply_charge but "error" (an INCRBY overflow needs three times
# 2^62 on one counter: charge_cases pins it on the array form)
CLASSES = ("invalid", "full", "short", "empty", "dup_denied", "over")
# amounts from 1 to more than any limit of CONFIG_SETS["mixed"] (at most 100)
AMOUNTS = np.array([1, 1, 1, 2, 3, 7, 50, 1 << 40], np.int64)
# the seed base of rank_batches: checked on the CPU (test_routed_charge.py) to
# meet the coverage charge_coverage asserts
SEED = 6300

new_sim, host_tensors, mismatches, run_ranks = rf.new_sim, rf.host_tensors, rf.mismatches, rf.run_ranks


def charge_rows(sim, key, ts, n, cfg, sms):
    """the result records of one merged charge step, in merge order, applied to
    sim as one call -> (rows, apply_charge's info).  A row is (decision,
    remaining, charged, reset_at): `charged` in the retry_after field."""
    m = len(key)
    out = np.zeros((m, 4), np.int64)
    if m == 0:
        return out, {"np": np.zeros(0, np.int64), "cls": np.zeros(0, "<U10"), "fresh": [], "expired": []}
    rows, info = apply_charge(sim, key, ts, n, cfg, sms)
    for i, (dec, got, rem, reset, _tok) in enumerate(rows):
        out[i] = (dec, rem, got, reset)
    return out, info


def step_rows(sim, op, key, ts, n, cfg, sms):
    if op == C:
        return charge_rows(sim, key, ts, n, cfg, sms)[0]
    return rf.step_rows(sim, op, key, ts, n, cfg, sms)


def oracle_charge(sim, world, cap):
    """rl_charge_routed_device over host pointers: request p is recv[order[p]]
    at store clock sms[p]; the merged batch is ONE apply_charge call in merge
    order.  Rows (decision, remaining, charged, reset_at)."""
    def call(m_max, count, recv, order, sms, res, stream, out_stream=None):
        cnt = int(_arr(count, 1, np.int32)[0])
        if cnt == 0:
            return
        o = _arr(order, cnt, np.int32).astype(np.int64)
        rec = _arr(recv, 4 * world * cap, np.int64).reshape(world * cap, 4)[o]
        rows = charge_rows(sim, rec[:, 0].view(np.uint64), rec[:, 1], rec[:, 2],
                           (rec[:, 3] & 0xffffffff).astype(np.uint32), _arr(sms, cnt, np.int64))[0]
        _arr(res, 4 * world * cap, np.int64).reshape(world * cap, 4)[o] = rows
    return call


def new_cover():
    return {"cls": set(), "cross_rank_dup": 0, "window_over": 0, "dropped": 0, "requests": 0}


def routed_expectations(all_batches, kinds, rank, configs, profile=0, cap=None, cover=None):
    """routed_refund_cases.routed_expectations with the charge kind:
    all_batches[r][b] = (key, ts, n or None, cfg); per step, `rank`'s four
    result fields in its batch order.  A charge step is ONE apply_charge call
    over the merged batch on the one shared store (a request past `cap` for its
    owner is dropped: RL_DROPPED, never recorded, but it still advances the
    clock).  cover (new_cover()): what the charge steps met -- apply_charge's
    classes, buckets charged by two or more ranks in one step with a
    contributor that was dup_denied, windows over their limit."""
    ref = new_sim(configs, profile)
    world = len(all_batches)
    outs = []
    clock = -(1 << 63)
    for b, op in enumerate(kinds):
        parts = [all_batches[r][b] for r in range(world)]
        parts = [(p[0], p[1], np.zeros(p[0].size, np.int64) if p[2] is None else p[2], p[3]) for p in parts]
        U = [np.concatenate([p[f] for p in parts]) for f in range(4)]
        src = np.concatenate([np.full(p[0].size, r) for r, p in enumerate(parts)])
        pos = np.concatenate([np.arange(p[0].size) for p in parts])
        own = shard.owner_of(U[0].astype(np.uint64), world)
        arrive = np.empty_like(U[1])
        sent = np.ones(U[0].size, bool)
        for r in range(world):
            for w in range(world):
                idx = np.nonzero((src == r) & (own == w))[0]
                if cap is not None and idx.size > cap:
                    sent[idx[cap:]] = False
                    idx = idx[:cap]
                if idx.size:
                    arrive[idx] = np.maximum.accumulate(U[1][idx])
        live = np.nonzero(sent)[0]
        o = live[np.lexsort((pos[live], src[live], arrive[live]))]
        sms = np.maximum(arrive[o] // 1_000_000, clock)
        if U[1].size:
            clock = max(clock, int(U[1].max()) // 1_000_000)
        full = np.zeros((U[0].size, 4), np.int64)
        full[:, 0] = DROPPED
        if op == C:
            rows, info = charge_rows(ref, U[0][o], U[1][o], U[2][o], U[3][o], sms)
            full[o] = rows
            if cover is not None:
                cls = info["cls"]
                cover["cls"] |= set(cls.tolist())
                cover["dropped"] += int((~sent).sum())
                cover["requests"] += int(o.size)
                cover["window_over"] += int((cls == "over").sum())
                bucket = np.isin(cls, ("full", "short", "empty", "dup_denied"))
                by_key = {}
                for i in np.nonzero(bucket)[0]:
                    by_key.setdefault(int(U[0][o[i]]), []).append(i)
                for idx in by_key.values():
                    if len({int(src[o[i]]) for i in idx}) >= 2 and any(cls[i] == "dup_denied" for i in idx):
                        cover["cross_rank_dup"] += 1
        else:
            full[o] = rf.step_rows(ref, op, U[0][o], U[1][o], U[2][o], U[3][o], sms)
        mine = src == rank
        outs.append([full[mine, f] for f in range(4)])
    return outs


def rank_batches(rank, configs, kinds=KINDS, m=1500, nkeys=400, reset_n_none=False, in_order=False):
    """one app server's steps, as routed_refund_cases.rank_batches (its own
    arrival order, its clock skewed against the other ranks' by up to 3 s, some
    requests out of time order and some stamped windows behind, keys shared by
    all ranks; in_order: the peek, refund and charge steps' ts sorted, which at
    world 1 takes the merge's RL_ORDER_IDENTITY form), with
      charge  the keys every rank decides on, so most buckets are charged by
              several requests and ranks in a step; amounts from 1 to 2^40, more
              than any limit; keys never seen; a few n <= 0, unknown cfgs and
              the reserved key id"""
    rng = np.random.default_rng(SEED + rank)
    t = T0 + [0, -3_000_000_000, 1_200_000_000, -700_000_000][rank % 4]
    ncfg = len(configs)
    out, last = [], None
    for op in kinds:
        key = rng.integers(0, nkeys, m).astype(np.uint64)
        ts = t + np.cumsum(rng.choice([0, 1, 500, 90_000, 2_000_000], m)).astype(np.int64)
        ts[rng.random(m) < 0.05] -= 5_000_000
        ts += rng.choice([0, 0, 0, 0, 0, 0, 0, 0, -7_000_000_000, -130_000_000_000], m)
        t = int(ts.max()) + 1
        if op == D:
            n = rng.choice([1, 1, 2, 5], m).astype(np.int64)
        elif op == P:
            n = rng.choice([0, 1, 2, 5], m).astype(np.int64)
            n[rng.random(m) < 0.01] = -1
        elif op == F:
            n = rng.choice([1, 1, 1, 2, 3], m).astype(np.int64)
            n[rng.random(m) < 0.01] = rng.choice([0, -1, -5])
        elif op == C:
            n = rng.choice(AMOUNTS, m, p=[0.25, 0.15, 0.1, 0.15, 0.1, 0.12, 0.11, 0.02])
            n[0], n[1] = 1, 1 << 40
        else:
            n = rng.integers(-3, 1 << 40, m).astype(np.int64)
        if op in (R, F):
            if last is not None:
                pick = rng.integers(0, last[0].size, m // 2)
                key[:m // 2], ts[:m // 2] = last[0][pick], last[1][pick]
            key[m // 2:m // 2 + 40] = key[m // 2 - 1]                 # one target many times in a row
            ts[m // 2:m // 2 + 40] = ts[m // 2 - 1]
        if op in (R, F, C):
            key[-30:] = np.arange(30, dtype=np.uint64) + np.uint64(10 * nkeys)   # never seen
        if op == C:
            n[rng.random(m) < 0.01] = rng.choice([0, -1, -5])
        if in_order and op in (P, F, C):
            o = np.argsort(ts, kind="stable")
            key, ts, n = key[o], ts[o], n[o]
        cfg = (key % np.uint64(ncfg)).astype(np.uint32)
        if op != D:
            cfg[rng.random(m) < 0.01] = BAD_CFG
            key[rng.random(m) < 0.01] = np.uint64(KEY_RESERVED)
        if op == D:
            last = (key, ts)
        out.append((key, ts, None if (op == R and reset_n_none) else n, cfg))
    return out


def charge_coverage(all_batches, configs, kinds=KINDS, cap=None):
    """the coverage record of these ranks' steps, asserted: every class of
    apply_charge but "error"; a window over its limit; and, with two ranks or
    more, a bucket charged by two ranks in one step, one contributor of which
    is dup_denied"""
    cover = new_cover()
    routed_expectations(all_batches, kinds, 0, configs, cap=cap, cover=cover)
    missing = [c for c in CLASSES if c not in cover["cls"]]
    assert not missing, (missing, cover)
    assert "error" not in cover["cls"], cover
    assert cover["window_over"] > 0, cover
    if len(all_batches) > 1:
        assert cover["cross_rank_dup"] > 0, cover
    return cover
