"""Cases and expectations for the routed AllowAll (shard.RoutedPipeline.allow_all,
include/rl_route.h) -- TEST INFRASTRUCTURE ONLY.

Built on route_ops (the routing kernels' CPU restatement), routed_refund_cases
(the four step kinds on the Python oracle) and allow_all_cases (the groups).

  RouteOpsSel             NumpyRouteOps with pack_sel and the skipped slot
  settle_routed           the routed settle in plain Python: the kernel's two
      bounded scans (allow_all_cases.scan_group) or the "maximal run"
      definition (allow_all_cases.group_spans), the severity order with DROPPED
  numpy_settle            rl_allow_all_settle_device over host pointers
  routed_expectations     routed_refund_cases.routed_expectations' merge with a
      fifth kind A: a decide step of all ranks' members, the settle rule per
      rank, ONE refund step with n = g of the selected members
  rank_steps / case       one rank's steps D A D P and their coverage
  run_kinds               the steps through a pipeline (A takes two numbers)
"""
import numpy as np

import routed_op_cases as rc
import routed_refund_cases as rf
import shard
from allow_all_cases import MAX_GROUP, group_spans, scan_group
from oracle import rl_oracle_py as po
from route_ops import CAP_ALIGN, DROPPED_SLOT, NumpyRouteOps, _arr
from tracegen import CONFIG_SETS, T0

D, P, R, F = rf.D, rf.P, rf.R, rf.F
A = "allow_all"                 # a compound: two step numbers
KINDS = [D, A, D, P]
DROPPED = rc.DROPPED            # 4
SKIPPED_SLOT = -2               # RL_SLOT_SKIPPED as int32
DONE, NOKEY, INVALID = rf.DONE, rf.NOKEY, rf.INVALID
CASE_KINDS = ["tb", "fw", "sw", "mixed"]

# severity of a decision code in the routed settle:
# ALLOWED < DENIED < ERROR < DROPPED < INVALID; a byte of 5 or more is INVALID
SEVERITY = {po.ALLOWED: 0, po.DENIED: 1, po.ERROR: 2, DROPPED: 3, po.INVALID: 4}
BY_SEVERITY = {v: k for k, v in SEVERITY.items()}


def severity(d):
    return SEVERITY.get(int(d), 4)


# --- the routing kernels' restatement, with the selection ---------------------------

class RouteOpsSel(NumpyRouteOps):
    """NumpyRouteOps plus rl_route_pack_sel and the skipped slot.  align: the
    capacity's rounding (the HIP merge's tile; 1 lets a CPU case use a small
    bucket)."""

    def __init__(self, world, cap, align=CAP_ALIGN):
        super().__init__(world, cap)
        self.capacity = (cap + align - 1) // align * align
        self.sel_dropped = 0        # selected requests pack_sel had to drop

    def pack_sel(self, m, key, ts, n, cfg, sel, send, scnt, slot, stream):
        cap = self.capacity
        k = _arr(key, m, np.int64).view(np.uint64)
        own = shard.owner_of(k, self.world)
        pick = _arr(sel, m, np.uint8) != 0
        snd = _arr(send, 4 * self.world * cap, np.int64).reshape(self.world * cap, 4)
        c = _arr(cfg, m, np.int32).view(np.uint32).astype(np.int64)
        t = _arr(ts, m, np.int64)
        rec = np.stack([k.view(np.int64), t, _arr(n, m, np.int64), c | (np.arange(m, dtype=np.int64) << 32)], 1)
        info = _arr(scnt, 4 * self.world, np.int64).reshape(self.world, 4)
        sl = _arr(slot, m, np.int32)
        sl[~pick] = SKIPPED_SLOT
        unsorted = int(m > 1 and bool(np.any(t[1:] < t[:-1])))     # the whole batch
        for o in range(self.world):
            idx = np.nonzero((own == o) & pick)[0]
            keep = idx[:cap]
            snd[o * cap:o * cap + keep.size] = rec[keep]
            sl[keep] = o * cap + np.arange(keep.size, dtype=np.int32)
            sl[idx[cap:]] = DROPPED_SLOT
            self.overflow |= idx.size > cap
            self.sel_dropped += idx.size - keep.size
            info[o] = [keep.size, t.min() if m else (1 << 63) - 1, t.max() if m else -(1 << 63),
                       2 * (idx.size - keep.size) + unsorted]

    def unpack(self, m, slot, back, dec, rem, retry, reset, stream):
        s = _arr(slot, m, np.int32)
        b = _arr(back, 4 * self.world * self.capacity, np.int64).reshape(self.world * self.capacity, 4)
        dropped, skipped = s == DROPPED_SLOT, s == SKIPPED_SLOT
        r = b[np.where(dropped | skipped, 0, s).astype(np.int64)]
        r[dropped] = [DROPPED, 0, 0, 0]
        r[skipped] = [po.INVALID, 0, 0, 0]          # nothing was asked
        _arr(dec, m, np.uint8)[:] = r[:, 0]
        _arr(rem, m, np.int64)[:] = r[:, 1]
        _arr(retry, m, np.int64)[:] = r[:, 2]
        _arr(reset, m, np.int64)[:] = r[:, 3]


# --- the settle ---------------------------------------------------------------------

def settle_routed(algs, first, n, cfg, decisions, scans=True):
    """the routed settle -> (verdict, g, sel), member by member.  algs[c]: the
    algorithm of config c.  scans: the kernel's two bounded scans
    (scan_group), else the definition (group_spans: a run above MAX_GROUP is
    INVALID)."""
    m = len(first)
    verdict = np.empty(m, np.uint8)
    g = np.zeros(m, np.int64)
    if scans:
        for i in range(m):
            span = scan_group(first, i)
            verdict[i] = po.INVALID if span is None else BY_SEVERITY[max(severity(decisions[j])
                                                                         for j in range(*span))]
    else:
        for h, e in group_spans(first):
            verdict[h:e] = po.INVALID if e - h > MAX_GROUP else BY_SEVERITY[max(severity(d) for d in decisions[h:e])]
    for i in np.nonzero(verdict != po.ALLOWED)[0].tolist():
        c, d = int(cfg[i]), int(decisions[i])
        if 0 <= c < len(algs):
            took = d == po.ALLOWED if algs[c] == po.TOKEN_BUCKET else d in (po.ALLOWED, po.DENIED)
            if took:
                g[i] = int(n[i])
    return verdict, g, (g > 0).astype(np.uint8)


def numpy_settle(sim):
    """rl_allow_all_settle_device over host pointers"""
    def call(m, first, cfg, n, dec, verdict, g, sel, stream):
        algs = [c[0] for c in sim.cfgs]
        v, gg, ss = settle_routed(algs, _arr(first, m, np.uint8), _arr(n, m, np.int64),
                                  _arr(cfg, m, np.int32).view(np.uint32), _arr(dec, m, np.uint8))
        _arr(verdict, m, np.uint8)[:] = v
        _arr(g, m, np.int64)[:] = gg
        _arr(sel, m, np.uint8)[:] = ss
    return call


# --- ONE shared store ---------------------------------------------------------------

def _merge(parts, world, cap, clock, sel=None):
    """one step's merge: parts[r] = (key, ts, n, cfg) -> (U, src, pos, o, sms,
    clock after, sent).  sel[r]: only those requests are sent (pack_sel); the
    clock still advances by every request's ts."""
    U = [np.concatenate([p[f] for p in parts]) for f in range(4)]
    src = np.concatenate([np.full(p[0].size, r) for r, p in enumerate(parts)])
    pos = np.concatenate([np.arange(p[0].size) for p in parts])
    picked = np.ones(U[0].size, bool) if sel is None else np.concatenate(sel).astype(bool)
    own = shard.owner_of(U[0].astype(np.uint64), world)
    arrive = np.zeros_like(U[1])
    sent = picked.copy()
    for r in range(world):
        for w in range(world):
            idx = np.nonzero((src == r) & (own == w) & picked)[0]
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
    return U, src, pos, o, sms, clock, sent, picked


def routed_expectations(all_batches, kinds, rank, configs, profile=0, cap=None, cover=None, sim_out=None):
    """ONE shared store over every rank's steps.  all_batches[r][b] = (key, ts,
    n or None, cfg) for the kinds D, P, R, F and (key, ts, n, cfg, first) for A.
    Per step, `rank`'s result fields in its batch order: four, and for A six --
    decision, remaining, retry_after, reset_at of the decide step, verdict,
    rollback.  A is the oracle composition: a decide step of all ranks' members
    in merge order, the settle rule on each rank's unpacked decisions (a member
    past `cap` for its owner: RL_DROPPED), and ONE refund step of the members
    with g > 0, n = g, at the refund step's store clock; rollback RL_INVALID
    for a member not selected.  cover (a list): one dict per A step, with every
    rank's decisions, verdict, g and rollback and the refund step's info.
    sim_out (a list): receives the store."""
    ref = rf.new_sim(configs, profile)
    algs = [c[0] for c in ref.cfgs]
    world = len(all_batches)
    outs = []
    clock = -(1 << 63)
    for b, op in enumerate(kinds):
        parts = [all_batches[r][b] for r in range(world)]
        parts = [tuple(np.zeros(p[0].size, np.int64) if (f == 2 and p[2] is None) else p[f] for f in range(len(p)))
                 for p in parts]
        U, src, pos, o, sms, clock, sent, _ = _merge([p[:4] for p in parts], world, cap, clock)
        full = np.zeros((U[0].size, 4), np.int64)
        full[:, 0] = DROPPED
        mine = src == rank
        if op != A:
            full[o] = rf.step_rows(ref, op, U[0][o], U[1][o], U[2][o], U[3][o], sms)
            outs.append([full[mine, f] for f in range(4)])
            continue
        full[o] = rc.step_rows(ref, D, U[0][o], U[1][o], U[2][o], U[3][o], sms)
        settled = [settle_routed(algs, parts[r][4], parts[r][2], parts[r][3], full[src == r, 0]) for r in range(world)]
        gparts = [(parts[r][0], parts[r][1], settled[r][1], parts[r][3]) for r in range(world)]
        U2, _, _, o2, sms2, clock, sent2, picked = _merge(gparts, world, cap, clock, sel=[s[2] for s in settled])
        back = np.zeros((U[0].size, 4), np.int64)
        back[:, 0] = np.where(picked, DROPPED, po.INVALID)
        rows, info = rf.refund_rows(ref, U2[0][o2], U2[1][o2], U2[2][o2], U2[3][o2], sms2)
        back[o2] = rows
        outs.append([full[mine, f] for f in range(4)] + [settled[rank][0].astype(np.int64), back[mine, 0]])
        if cover is not None:
            cover.append({
                "decision": [full[src == r, 0] for r in range(world)],
                "verdict": [s[0] for s in settled], "g": [s[1] for s in settled],
                "rollback": [back[src == r, 0] for r in range(world)],
                "decide_dropped": int((~sent).sum()), "refund_dropped": int((picked & ~sent2).sum()),
                "multi_rank_targets": sum(1 for idx in info["targets"].values()
                                          if len({int(src[o2[i]]) for i in idx}) >= 2),
                "refunds": int(picked.sum()),
            })
    if sim_out is not None:
        sim_out.append(ref)
    return outs


# --- the case -----------------------------------------------------------------------

def _members(rng, rank, world, configs, nkeys, t0):
    """one rank's AllowAll members: ~310 groups of 1 to 16 over nkeys keys, a
    run of 17 (rank 0), and the directed cross-rank groups"""
    ncfg = len(configs)
    sizes = rng.choice(np.arange(1, 17), 310, p=np.array([8, 8, 5, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2]) / 39.0)
    amounts = np.array([1, 1, 1, 1, 2, 3], np.int64)
    groups = []
    for s in sizes.tolist():
        gk = rng.integers(0, nkeys, s).astype(np.uint64)
        groups.append([gk, rng.choice(amounts, s), (gk % np.uint64(ncfg)).astype(np.uint32)])
    if rank == 0:
        gk = rng.integers(0, nkeys, 17).astype(np.uint64)
        groups.insert(100, [gk, np.ones(17, np.int64), (gk % np.uint64(ncfg)).astype(np.uint32)])
    # a member that is not executed, per rank: n = 0 and an unknown config
    groups[7][1][0] = 0
    groups[9][2][-1] = ncfg + 2
    # Transient takes across ranks, on keys of config 0 nobody else uses: rank 0
    # asks [X_j, Y_j] early -- X_j has all its quota, Y_j is asked for twice its
    # limit -- so X_j's take is given back in the refund step; the last rank asks
    # [X_j] late and is denied on that take
    L0 = configs[0][1]
    take = np.int64(3 * L0 // 4)
    directed = []
    for j in range(8):
        X, Y = np.uint64(ncfg * (300 + 2 * j)), np.uint64(ncfg * (301 + 2 * j))
        if rank == 0:
            groups.insert(2 + j, [np.array([X, Y]), np.array([take, 2 * L0], np.int64), np.zeros(2, np.uint32)])
            directed.append(2 + j)
        if rank == world - 1 and world > 1:
            groups.append([np.array([X]), np.array([take], np.int64), np.zeros(1, np.uint32)])
            directed.append(len(groups) - 1)
    # one target refunded from every rank: [Z, Y0] fails everywhere, and Z's
    # takes meet in one record of the refund step
    Z, Y0 = np.uint64(ncfg * 400), np.uint64(ncfg * 401)
    groups.insert(20, [np.array([Z, Y0]), np.array([1, 2 * L0], np.int64), np.zeros(2, np.uint32)])
    key = np.concatenate([g[0] for g in groups]).astype(np.uint64)
    n = np.concatenate([g[1] for g in groups]).astype(np.int64)
    cfg = np.concatenate([g[2] for g in groups]).astype(np.uint32)
    first = np.zeros(key.size, np.uint8)
    heads = np.cumsum([0] + [g[0].size for g in groups[:-1]])
    first[heads] = rng.choice([1, 1, 2, 255], heads.size)
    first[0] = 0                                    # member 0 starts a group whatever its byte
    ts = t0 + np.cumsum(rng.choice([0, 1000, 250_000, 2_000_000], key.size, p=[0.1, 0.5, 0.2, 0.2])).astype(np.int64)
    return (key, ts, n, cfg, first), [int(heads[d]) for d in directed]


def rank_steps(kind, rank, world, m=600, nkeys=120, seed=0):
    """one rank's steps D A D P -> (batches, heads of the directed groups of A).
    The ranks' clocks differ by microseconds, so every rank's A members
    interleave in the merge; a few requests of the D steps are out of time
    order."""
    configs = CONFIG_SETS[kind]
    rng = np.random.default_rng(7300 + 17 * seed + rank)
    ncfg = len(configs)
    t = T0 + 1000 * rank
    out, directed = [], None
    for op in KINDS:
        if op == A:
            batch, directed = _members(rng, rank, world, configs, nkeys, t)
            out.append(batch)
            t = int(batch[1].max()) + 1
            continue
        key = rng.integers(0, nkeys, m).astype(np.uint64)
        ts = t + np.cumsum(rng.choice([0, 1, 500, 90_000, 1_000_000], m)).astype(np.int64)
        ts[rng.random(m) < 0.05] -= 300_000
        t = int(ts.max()) + 1
        n = (rng.choice([1, 1, 2, 5], m) if op == D else rng.choice([0, 1, 2, 5], m)).astype(np.int64)
        out.append((key, ts, n, (key % np.uint64(ncfg)).astype(np.uint32)))
    return out, directed


def case(kind, world, cap=None, seed=0, check=True):
    """every rank's steps D A D P of one kind -> (configs, all_batches, cover):
    cover is the A step's (routed_expectations) plus the counts asserted here
    (check): at least 20 allowed groups and 20 failed groups per denying
    algorithm, 10 groups whose members' owners differ, a window member that was
    denied and rolled back, a NOKEY rollback, a target refunded by two ranks
    (world > 1), the run of 17, and (world > 1) at least 5 groups of the last
    rank denied only on rank 0's transient take -- allowed when the store is run
    without rank 0's members."""
    configs = CONFIG_SETS[kind]
    ncfg = len(configs)
    steps = [rank_steps(kind, r, world, seed=seed) for r in range(world)]
    all_batches = [s[0] for s in steps]
    cov = []
    routed_expectations(all_batches, KINDS, 0, configs, cap=cap, cover=cov)
    c = cov[0]
    alg_name = {po.TOKEN_BUCKET: "tb", po.SLIDING_WINDOW: "sw", po.FIXED_WINDOW: "fw"}
    algs = sorted({alg_name[a] for a, _, _ in configs})
    stat = {"allowed": 0, "failed_by": {a: 0 for a in algs}, "cross_owner": 0, "win_denied_done": 0,
            "nokey": 0, "long_runs": [], "dropped_groups": 0, "dropped_takers_back": 0, "transient": 0}
    for r in range(world):
        key, ts, n, cfg, first = all_batches[r][1]
        dec, v, g, rb = c["decision"][r], c["verdict"][r], c["g"][r], c["rollback"][r]
        own = shard.owner_of(key, world)
        alg_of = lambda j: alg_name[configs[int(cfg[j])][0]] if int(cfg[j]) < ncfg else None
        stat["nokey"] += int(((rb == NOKEY) & (g > 0)).sum())
        for h, e in group_spans(first):
            assert (v[h:e] == v[h]).all()
            if e - h > MAX_GROUP:
                assert v[h] == po.INVALID
                stat["long_runs"].append(e - h)
                continue
            stat["cross_owner"] += len(set(own[h:e].tolist())) > 1
            if v[h] == po.ALLOWED:
                stat["allowed"] += 1
                assert (g[h:e] == 0).all() and (rb[h:e] == po.INVALID).all()
            if v[h] == po.DENIED:
                for a in {alg_of(j) for j in range(h, e) if dec[j] == po.DENIED}:
                    stat["failed_by"][a] += 1
            if v[h] == DROPPED:
                stat["dropped_groups"] += 1
                assert (dec[h:e] == DROPPED).any() and not (dec[h:e] == po.INVALID).any()
                stat["dropped_takers_back"] += int(((g[h:e] > 0) & (rb[h:e] == DONE)).sum())
            stat["win_denied_done"] += sum(1 for j in range(h, e) if alg_of(j) in ("fw", "sw") and
                                           dec[j] == po.DENIED and g[j] > 0 and rb[j] == DONE)
    if world > 1:
        # without rank 0's members the last rank's directed groups pass
        alone = [list(bs) for bs in all_batches]
        alone[0][1] = tuple(x[:0] for x in all_batches[0][1])
        cov2 = []
        routed_expectations(alone, KINDS, 0, configs, cap=cap, cover=cov2)
        last = world - 1
        for h in steps[last][1]:
            stat["transient"] += int(c["verdict"][last][h] == po.DENIED and cov2[0]["verdict"][last][h] == po.ALLOWED)
    cover = dict(c, **stat)
    if check:
        assert all(1400 <= b[1][0].size <= 1800 for b in all_batches), [b[1][0].size for b in all_batches]
        assert stat["allowed"] >= 20, stat
        assert all(x >= 20 for x in stat["failed_by"].values()), stat
        assert stat["cross_owner"] >= (10 if world > 1 else 0), stat
        assert stat["nokey"] >= 1, stat
        assert stat["long_runs"] == [17], stat
        if kind != "tb":
            assert stat["win_denied_done"] >= 1, stat
        if world > 1:
            assert stat["transient"] >= 5, stat
            assert c["multi_rank_targets"] >= 1, c["multi_rank_targets"]
        assert c["refund_dropped"] == 0      # pack_sel cannot drop a give-back at the sender
    return configs, all_batches, cover


# --- through a pipeline ---------------------------------------------------------------

def host_tensors(torch, batch):
    """a step's arrays as the pipeline's tensors; an A batch carries `first`"""
    t = rc.host_tensors(torch, batch[:4])
    return t if len(batch) == 4 else t + (torch.from_numpy(batch[4]),)


def new_outs(torch, kinds, batches, device="cpu"):
    """per step the output tensors: dec, rem, retry, reset, and for A verdict
    and rollback too"""
    outs = []
    for k, b in zip(kinds, batches):
        m = b[0].size
        u8 = lambda: torch.empty(m, dtype=torch.uint8, device=device)
        i64 = lambda: torch.empty(m, dtype=torch.int64, device=device)
        outs.append((u8(), i64(), i64(), i64()) + ((u8(), u8()) if k == A else ()))
    return outs


def run_kinds(pipe, kinds, ins, outs):
    """the steps through the pipeline, numbered in order (A takes two numbers)
    -> the step number after the last"""
    b = 0
    for k, i, o in zip(kinds, ins, outs):
        if k == A:
            pipe.allow_all(b, *i, *o[:4], o[4], o[5])
            b += 2
        else:
            pipe.step(b, *i, *o, op=k)
            b += 1
    pipe.flush()
    return b


mismatches = rc.mismatches
