"""Cases and expectations for routed steps of the three kinds (decide, peek,
reset: include/rl_route.h, shard.RoutedPipeline) -- TEST INFRASTRUCTURE ONLY.

Built on route_ops (the routing kernels' CPU restatement), peek_cases and
reset_cases, with the Python oracle (oracle.rl_oracle_py.Sim) as the store: it
is the one oracle whose state a peek can put back.

  py_decide / oracle_peek / oracle_reset   the owner's engine over host
      pointers, with route_ops.oracle_decide's signature
  routed_expectations                      ONE shared store over every rank's
      steps, each step merged in (arrival, source rank, source position)
      order under the store clock of route_ops.shared_limiter_expectations
  rank_batches                             one app server's steps of the kinds
      D P D R P D P
"""
import numpy as np

import shard
from oracle import rl_oracle_py as po
from peek_cases import KEY_RESERVED, peek_one
from reset_cases import apply_resets, expected_status
from route_ops import _arr
from tracegen import T0

D, P, R = shard.OP_DECIDE, shard.OP_PEEK, shard.OP_RESET
KINDS = [D, P, D, R, P, D, P]
DROPPED = 4
BAD_CFG = 99


def new_sim(configs, profile=0):
    sim = po.Sim(profile)
    for a, L, W in configs:
        sim.add_config(a, L, W)
    return sim


def decide_row(sim, key, ts, n, cfg, sms):
    """one request of a decide step: the four Result fields (the engine
    rejects the reserved key id, which the oracle does not know)"""
    if int(key) == KEY_RESERVED:
        return (po.INVALID, 0, 0, 0)
    return sim.decide(int(key), int(ts), int(n), int(cfg), int(sms))[:4]


def step_rows(sim, op, key, ts, n, cfg, sms):
    """the result records of one merged step, in merge order, applied to sim"""
    m = len(key)
    if op == R:
        ncfg = len(sim.cfgs)
        st = expected_status(key, cfg, ncfg).astype(np.int64)
        apply_resets(sim, key, ts, cfg, ncfg)
        return np.stack([st, np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)], 1)
    one = decide_row if op == D else (lambda *a: peek_one(*a)[:4])
    out = np.zeros((m, 4), np.int64)
    for i in range(m):
        out[i] = one(sim, key[i], ts[i], n[i], cfg[i], sms[i])
    return out


def _engine(sim, world, cap, op):
    def call(m_max, count, recv, order, sms, res, stream, out_stream=None):
        cnt = int(_arr(count, 1, np.int32)[0])
        if cnt == 0:
            return
        o = _arr(order, cnt, np.int32).astype(np.int64)
        rec = _arr(recv, 4 * world * cap, np.int64).reshape(world * cap, 4)[o]
        rows = step_rows(sim, op, rec[:, 0].view(np.uint64), rec[:, 1], rec[:, 2],
                         (rec[:, 3] & 0xffffffff).astype(np.uint32), _arr(sms, cnt, np.int64))
        _arr(res, 4 * world * cap, np.int64).reshape(world * cap, 4)[o] = rows
    return call


def py_decide(sim, world, cap):
    """rl_decide_routed_device over host pointers, on the Python oracle"""
    return _engine(sim, world, cap, D)


def oracle_peek(sim, world, cap):
    """rl_peek_routed_device over host pointers: request p is recv[order[p]]
    at store clock sms[p]; sim is left as it was"""
    return _engine(sim, world, cap, P)


def oracle_reset(sim, world, cap):
    """rl_reset_routed_device over host pointers: every received request
    deletes its key"""
    return _engine(sim, world, cap, R)


def routed_expectations(all_batches, kinds, rank, configs, profile=0, cap=None):
    """shared_limiter_expectations with a kind per step: all_batches[r][b] =
    (key, ts, n or None, cfg); per step, `rank`'s four result fields in its
    batch order.  A peek row is peek_one at the request's store clock, a reset
    step is apply_resets; a request past `cap` for its owner is dropped
    (RL_DROPPED, never reaches the store) but still advances the clock."""
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
        full[o] = step_rows(ref, op, U[0][o], U[1][o], U[2][o], U[3][o], sms)
        mine = src == rank
        outs.append([full[mine, f] for f in range(4)])
    return outs


def rank_batches(rank, configs, kinds=KINDS, m=1500, nkeys=400, reset_n_none=False, peeks_in_order=False):
    """one app server's steps: its own arrival order, its clock skewed against
    the other ranks' (time goes back across ranks by up to 3 s), some requests
    out of time order (peeks_in_order: not in the peek steps, which at world 1
    then take the merge's RL_ORDER_IDENTITY form), keys shared by all ranks.
      decide  n in {1, 1, 2, 5}
      peek    n in {0, 1, 2, 5}; a few rows with n = -1, an unknown cfg or the
              reserved key id
      reset   half of them the (key, ts, cfg) of requests of this rank's last
              decide step (the window keys those created, wherever they live),
              the rest at the rank's current time; duplicates; keys never seen;
              a few unknown cfgs and the reserved key id; n is noise (ignored)
              or None"""
    rng = np.random.default_rng(4100 + rank)
    t = T0 + [0, -3_000_000_000, 1_200_000_000, -700_000_000][rank % 4]
    ncfg = len(configs)
    out, last = [], None
    for op in kinds:
        key = rng.integers(0, nkeys, m).astype(np.uint64)
        ts = t + np.cumsum(rng.choice([0, 1, 500, 90_000, 2_000_000], m)).astype(np.int64)
        ts[rng.random(m) < 0.05] -= 5_000_000
        # a few requests stamped by a server whose clock is windows behind: a
        # key then has more live windows than its table entry holds (the spill)
        ts += rng.choice([0, 0, 0, 0, 0, 0, 0, 0, -7_000_000_000, -130_000_000_000], m)
        if op == P and peeks_in_order:
            ts = np.sort(ts)
        t = int(ts.max()) + 1
        if op == D:
            n = rng.choice([1, 1, 2, 5], m).astype(np.int64)
        elif op == P:
            n = rng.choice([0, 1, 2, 5], m).astype(np.int64)
            n[rng.random(m) < 0.01] = -1
        else:
            n = rng.integers(-3, 1 << 40, m).astype(np.int64)
            if last is not None:
                pick = rng.integers(0, last[0].size, m // 2)
                key[:m // 2], ts[:m // 2] = last[0][pick], last[1][pick]
            key[m // 2:m // 2 + 40] = key[m // 2 - 1]                 # one reset many times in a row
            ts[m // 2:m // 2 + 40] = ts[m // 2 - 1]
            key[-30:] = np.arange(30, dtype=np.uint64) + np.uint64(10 * nkeys)   # never seen
        cfg = (key % np.uint64(ncfg)).astype(np.uint32)
        if op != D:
            cfg[rng.random(m) < 0.01] = BAD_CFG
            key[rng.random(m) < 0.01] = np.uint64(KEY_RESERVED)
        if op == D:
            last = (key, ts)
        out.append((key, ts, None if (op == R and reset_n_none) else n, cfg))
    return out


def host_tensors(torch, batch):
    """(key, ts, n, cfg) arrays as the pipeline's tensors (n may be None)"""
    key, ts, n, cfg = batch
    return (torch.from_numpy(key.view(np.int64)), torch.from_numpy(ts),
            None if n is None else torch.from_numpy(n), torch.from_numpy(cfg.view(np.int32)))


def mismatches(outs, exp):
    """[(step, field, first bad rows)] of a rank's outputs against routed_expectations"""
    bad = []
    for b, (ob, eb) in enumerate(zip(outs, exp)):
        for f, (o, e) in enumerate(zip(ob, eb)):
            g = (o.cpu().numpy() if hasattr(o, "cpu") else np.asarray(o)).astype(np.int64)
            w = np.nonzero(g != np.asarray(e, np.int64))[0]
            if w.size:
                bad.append((b, f, w[:5].tolist(), g[w[:5]].tolist(), np.asarray(e)[w[:5]].tolist()))
    return bad
