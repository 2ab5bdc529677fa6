"""Key-space sharding across GPUs (one process per GPU, torch.distributed).

Each rank owns the keys with owner(key) == rank (a 64-bit mix of the key id,
mod world size, include/rl_route.h) and keeps their state in its own HBM
tables.  Two ways to feed it:

  * routed ingress (RoutedPipeline, bench.py --gpus N): every rank receives
    arbitrary requests; the routing kernels group them by owner into
    fixed-capacity buckets, an equal-split all-to-all moves the buckets to
    their owners, the owner merges and decides, and the inverse all-to-all
    returns the results -- with no host read anywhere in the step.  On MI355X
    the "nccl" backend is RCCL over xGMI, where all-to-all drives all 7
    point-to-point links at once;
  * sharded ingress (bench.py --ingress sharded): every rank receives only
    requests of the keys it owns; no data-path collective (N replicas).

Order: the reference's N app servers share one Redis, which applies a key's
requests in arrival order.  The owner replays the union of the ranks'
requests ordered by (ts, source rank, source position), a deterministic total
order consistent with each rank's own order, under one monotone store clock.
"""
from __future__ import annotations

import collections
import warnings

import numpy as np
import torch
import torch.distributed as dist

_M1 = np.uint64(0xbf58476d1ce4e5b9)
_M2 = np.uint64(0x94d049bb133111eb)


def mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finalizer (same function as rl_table.h mix64)."""
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= _M1
        x ^= x >> np.uint64(27)
        x *= _M2
        x ^= x >> np.uint64(31)
    return x


def owner_of(key: np.ndarray, world: int) -> np.ndarray:
    # high bits: the table uses the low bits of the same hash for slots
    return ((mix64(key) >> np.uint64(32)) % np.uint64(world)).astype(np.int64)


# --- cluster-wide reads of the usage tally and the top keys ----------------------
#
# Every rank counts the routed steps it OWNS (rl_tally_routed_device,
# rl_hot_routed_device), so the ranks' reads are over disjoint key sets and a
# cluster read is a merge of small lists: `top` records per rank.

_M64 = (1 << 64) - 1


def _fields(x):
    """an info record -- a dict, or a ctypes struct of counters -- as a dict of ints"""
    if x is None:
        return {}
    if isinstance(x, dict):
        return {k: int(v) for k, v in x.items()}
    return {k: int(getattr(x, k)) for k, _ in x._fields_ if k not in ("struct_size", "pad_")}


def tally_part(t):
    """one rank's tally read (rl_amd.Tally, or anything with its cfg, keys,
    info and routed) as a plain dict that travels between ranks"""
    if isinstance(t, dict):
        return t
    return dict(cfg=np.array(t.cfg), keys=np.array(t.keys), info=_fields(t.info),
                routed=_fields(getattr(t, "routed", None)))


def hot_part(h):
    """one rank's top-keys read (rl_amd.Hot) as a plain dict"""
    if isinstance(h, dict):
        return h
    return dict(keys=np.array(h.keys), info=_fields(h.info))


def _sum_fields(dicts, skip=()):
    out = {}
    for d in dicts:
        for k, v in d.items():
            if k not in skip:
                out[k] = (out.get(k, 0) + int(v)) & _M64
    return out


def _unite(parts, value_fields, order_field, top):
    """the parts' key records united by key_id: a key two parts report has its
    value fields summed (modulo 2^64) and keeps the first part's other fields;
    ordered by order_field descending, then key id ascending, cut to `top`"""
    dt = parts[0]["keys"].dtype
    recs = {}
    for part in parts:
        for r in part["keys"]:
            k = int(r["key_id"])
            if k in recs:
                for f in value_fields:
                    recs[k][f] = (int(recs[k][f]) + int(r[f])) & _M64
            else:
                recs[k] = {f: r[f] for f in dt.names}
    ids = sorted(recs, key=lambda k: (-int(recs[k][order_field]), k))[:max(0, int(top))]
    out = np.zeros(len(ids), dt)
    for i, k in enumerate(ids):
        for f in dt.names:
            out[f][i] = recs[k][f]
    return out


def merge_tallies(parts, top):
    """the ranks' tally reads (tally_part dicts or rl_amd.Tally, in rank order)
    as one: config rows summed modulo 2^64, info fields and the routed info
    summed, key lists united -- a key id reported by two ranks is summed and
    keeps the lowest rank's cfg, which cannot happen under the owner partition
    -- ordered by denied descending, then key id ascending, cut to `top`.
    -> dict(cfg, keys, keys_tracked, info, routed)"""
    parts = [tally_part(p) for p in parts]
    rows = max(p["cfg"].size for p in parts)
    cfg = np.zeros(rows, parts[0]["cfg"].dtype)
    with np.errstate(over="ignore"):
        for p in parts:
            for f in cfg.dtype.names:
                cfg[f][:p["cfg"].size] += p["cfg"][f]      # uint64: wraps
    info = _sum_fields([p["info"] for p in parts])
    return dict(cfg=cfg, keys=_unite(parts, ("denied", "units_denied"), "denied", top),
                keys_tracked=info.get("keys_tracked", 0), info=info,
                routed=_sum_fields([p.get("routed") or {} for p in parts]))


_HOT_SAME = ("width", "depth", "hot_min", "weight")


def merge_hots(parts, top):
    """the ranks' top-keys reads (hot_part dicts or rl_amd.Hot, in rank order)
    as one: keys united, ordered by estimate descending, then key id ascending,
    cut to `top`; total, skipped, keys_tracked (and key_slots, batches,
    requests) summed; dropped non-zero if any part's is; width, depth, hot_min
    and weight must agree on all parts, else ValueError -- estimates of
    different sketches do not compare.  -> dict(keys, keys_tracked, info)"""
    parts = [hot_part(p) for p in parts]
    for f in _HOT_SAME:
        vals = {p["info"].get(f) for p in parts}
        if len(vals) > 1:
            raise ValueError(f"merge_hots: the parts' {f} differ: {sorted(vals, key=str)}")
    info = _sum_fields([p["info"] for p in parts], skip=_HOT_SAME + ("dropped",))
    info.update({f: parts[0]["info"][f] for f in _HOT_SAME if f in parts[0]["info"]})
    info["dropped"] = int(any(p["info"].get("dropped", 0) for p in parts))
    return dict(keys=_unite(parts, ("estimate",), "estimate", top), keys_tracked=info.get("keys_tracked", 0),
                info=info)


# --- the native routed pipeline (include/rl_route.h) ---------------------------

INFO = 4   # RL_ROUTE_INFO

# the kind of a routed step (every rank runs a step with the same kind)
OP_DECIDE, OP_PEEK, OP_RESET, OP_REFUND, OP_CHARGE = 0, 1, 2, 3, 4
_OP_NAMES = {OP_DECIDE: "decide", OP_PEEK: "peek", OP_RESET: "reset", OP_REFUND: "refund", OP_CHARGE: "charge"}


def _ctx(stream):
    import contextlib
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


class RoutedPipeline:
    """One rank of the routed decision path: every rank accepts requests for
    any key; the routing kernels (include/rl_route.h: `ops`, an rl_amd.Router)
    pack them into one fixed-capacity bucket per owner GPU, two equal-split
    RCCL all-to-alls over xGMI (torch.distributed "nccl" process groups) move
    the buckets to their owners and the result buckets back, and the owner's
    engine decides its keys in the order one shared store sees them -- by
    arrival time, ties by (source rank, source position).

    Nothing in a step is read by the host: every split of every collective is
    `ops.capacity` records, the owner's merge takes the received counts from
    the received info rows in device memory, and the engine reads the merged
    batch's size from device memory too (rl_decide_routed_device).  A request
    past its owner's capacity is dropped (decision RL_DROPPED, ops.sync()
    reports RL_EOVERFLOW); size `cap` for the key skew (a uniform hash
    partition needs ~max_batch / world plus a margin, a Zipf hot key more).

    Streams (two, each on a hardware queue of its own): the request stream R
    runs every step's pack, request-side collectives and merge in step order
    (the router's scratch and store clock are sequential) and hands the
    merged batch to the engine; the result stream U takes the engine's
    results, runs the result all-to-all and the unpack.  So R goes on with
    the next step while the engine decides this one.  `depth` buffer sets
    rotate; a set is rewritten only after the step that used it `depth`
    steps earlier has unpacked.  (Round 3-4 ran each step's merge, engine
    call, result exchange and unpack on one of `depth` step streams: with the
    engine's three streams that made up to nine queues, and the engine's
    grouping of step b waited for step b - depth's unpack on the same step
    stream.)

    Collective order (the first N > 1 run must not deadlock).  The request
    collectives run on the request group (`pg_req`), the result collective on
    `pg_res`: two communicators, two internal streams.  RCCL, like NCCL,
    guarantees progress only when every rank runs the collectives of its
    communicators in one consistent order (or every pending collective kernel
    can be resident at once).  So the GPU order is made the host's issue
    order, the same on every rank: each collective first waits for the last
    one issued on the other group.  The result side of step b is issued
    `lookahead` steps late, after step b + lookahead's request side, so the
    one order is Req(0..L), Res(0), Req(L+1), Res(1), ...: a step's request
    exchange never waits for the engine of the step before it, and its merge
    and grouping wait only for the engine of step b - L - 1, which the
    engine's three buffer sets make it wait for anyway at L = 1.
    allow_all(b, ...) is two steps whose second is packed from the first's
    results, so step b's result side cannot wait: the call first issues every
    pending result side, then Req(b), Res(b) at once, Req(b + 1), and defers
    Res(b + 1) by the usual rule -- ... Res(pending), Req(b), Res(b),
    Req(b + 1), then as above.  Every rank calls allow_all at the same step
    number, so this too is one order on every rank, and each collective still
    waits for the last one issued on the other group.

    decide(m_max, count, recv, order, sms, res, in_stream, out_stream) runs
    the owner's engine on the merged batch (rl_decide_routed_device_io;
    device pointers): the grouping waits for in_stream, out_stream waits for
    the results.
    exchange: run the collectives (world > 1 always; at world 1 they are
    loopback copies over a one-rank group, e.g. to exercise RCCL; without them
    the buckets and results are read in place).

    Step kinds (include/rl_route.h): step(..., op=OP_PEEK) asks what a decide
    step would answer and changes nothing; step(..., op=OP_RESET) deletes the
    requests' keys (n may be None); step(..., op=OP_REFUND) gives quota back
    (rl_refund_routed_device: all ranks' refunds of one target in the step are
    summed on the owner and applied once; decision REFUND_DONE, REFUND_NOKEY or
    INVALID); step(..., op=OP_CHARGE) records usage known after the fact
    (rl_charge_routed_device: the merged batch is one Charge call in merge
    order; dec / rem / reset as for a decide, and the `retry` output array
    receives `charged`).  Such a step is packed, exchanged, merged
    and unpacked exactly as a decide step -- same buffer sets, collectives,
    collective order and lookahead -- and only the owner's engine call differs:
    peek / reset / refund / charge (the signature of decide:
    rl_peek_routed_device / rl_reset_routed_device / rl_refund_routed_device /
    rl_charge_routed_device with out_stream) or peek_ev / reset_ev / refund_ev /
    charge_ev (that of decide_ev).  Every rank must give a
    step the same kind.  The engine orders
    the step after every step issued before it and before every later one.

    allow_all(b, ...) (settle=: Engine.allow_all_settle) checks each request
    against several limiters, all or nothing, wherever their keys live: decide
    step b, the settle on U, and refund step b + 1 packed with ops.pack_sel from
    the settle's give-backs (include/rl_route.h).

    observe= (a list of callables f(m_max, count, recv, order, sms, res, rcnt,
    world, stream): Engine.tally_routed, Engine.hot_routed) counts every decide
    step, and the member decide step of allow_all, on the keys' owner: the calls
    are enqueued on U in the step's result side, after the result all-to-all and
    the unpack -- the results leave first -- and before the buffer set's ev_done,
    so the set is not rewritten under them (on a CPU pipeline: inline after the
    unpack).  Peek, reset, refund and charge steps are not counted, nor are
    allow_all's give-backs.  Without observe the pipeline issues exactly the
    calls it issues otherwise.  usage() / top_keys() read the cluster's counts
    (DESIGN.md §10o)."""

    def __init__(self, ops, decide, world, max_batch, device, pg_req=None, pg_res=None, depth=4, exchange=None,
                 staged=False, lookahead=None, ordered=True, decide_ev=None, *, peek=None, peek_ev=None, reset=None,
                 reset_ev=None, refund=None, refund_ev=None, settle=None, charge=None, charge_ev=None, observe=None):
        self.ops, self.decide, self.world = ops, decide, world
        # observe: callables f(m_max, count, recv, order, sms, res, rcnt, world,
        # stream) run on U over every finished decide step (Engine.tally_routed,
        # Engine.hot_routed; device pointers)
        self.observe = list(observe or ())
        # settle(m, first, cfg, n, dec, verdict, g, sel, stream): the sender's
        # settle of allow_all (rl_allow_all_settle_device; device pointers)
        self.settle = settle
        self._aa = None               # allow_all's scratch (g, sel, the refund step's unused outputs)
        self.dev = torch.device(device)
        self.cuda = self.dev.type == "cuda"
        self.pg_req, self.pg_res = pg_req, pg_res
        self.depth = depth
        self.exchange = world > 1 if exchange is None else bool(exchange)
        if world > 1 and not self.exchange:
            raise ValueError("world > 1 needs the exchange")
        self.staged = staged          # all-to-alls through host memory (gloo with device tensors)
        self.max_batch = max_batch
        self.cap = cap = ops.capacity
        tot = world * cap
        self.m_max = tot              # the merged batch's bound (the engine's max_batch must hold it)
        d = self.dev
        # streams on hardware queues of their own (ops.dedicated_stream): the
        # step streams wait on the engine's events, and a waiting stream would
        # block every stream that shares its hardware queue
        mk = getattr(ops, "dedicated_stream", None)

        def new_stream():
            if not self.cuda:
                return None
            return mk() if mk is not None else torch.cuda.Stream(d)

        self.R = new_stream()
        self.U = new_stream()
        # decide_ev(m_max, count, recv, order, sms, res, in_stream, event):
        # the engine records its results' completion into `event` instead of
        # making U wait at call time -- with the result side issued
        # `lookahead` steps late, a wait made at call time would queue U
        # behind this step's engine before the result exchanges issued in
        # between, and serialize the engine's steps
        self.decide_ev = decide_ev if self.cuda else None
        # per step kind: (call with out_stream, call with event); a peek,
        # reset, refund or charge step takes the event form when it is given, like the
        # decide
        self._calls = {
            OP_DECIDE: (decide, self.decide_ev),
            OP_PEEK: (peek, peek_ev if self.cuda else None),
            OP_RESET: (reset, reset_ev if self.cuda else None),
            OP_REFUND: (refund, refund_ev if self.cuda else None),
            OP_CHARGE: (charge, charge_ev if self.cuda else None),
        }
        with_events = any(ev is not None for _, ev in self._calls.values())
        self._zero_n = None           # n of a reset step given without one
        self.slots = []
        for _ in range(depth):
            s = dict(
                send=torch.empty((tot, 4), dtype=torch.int64, device=d),
                slot=torch.empty(max_batch, dtype=torch.int32, device=d),
                # info rows (include/rl_route.h RL_ROUTE_INFO): {sent, earliest ts, latest ts, dropped}
                scnt=torch.zeros((world, INFO), dtype=torch.int64, device=d),   # per owner
                rcnt=torch.zeros((world, INFO), dtype=torch.int64, device=d) if self.exchange else None,
                recv=torch.empty((tot, 4), dtype=torch.int64, device=d) if self.exchange else None,
                order=torch.empty(tot, dtype=torch.int32, device=d),
                sms=torch.empty(tot, dtype=torch.int64, device=d),
                count=torch.zeros(1, dtype=torch.int32, device=d),
                res=torch.empty((tot, 4), dtype=torch.int64, device=d),
                back=torch.empty((tot, 4), dtype=torch.int64, device=d) if self.exchange else None,
                ev_done=None,
                ev_res=None,
            )
            if with_events:
                s["ev_res"] = torch.cuda.Event()
                s["ev_res"].record(self.R)    # materialize the event: the engine records it from now on
            self.slots.append(s)
        # result sides issued `lookahead` steps late (exchange only: without
        # collectives there is nothing to order).  Default 1, except on CUDA
        # without decide_ev: there the decide call makes U wait for this
        # step's engine at call time, so a late result side would queue step
        # b-1's result collective behind engine(b) and serialize the steps
        if lookahead is None:
            lookahead = 0 if (self.cuda and self.decide_ev is None) else 1
        elif lookahead > 0 and self.cuda and self.decide_ev is None and self.exchange:
            warnings.warn("RoutedPipeline: lookahead > 0 without decide_ev serializes the engine's steps on CUDA")
        self.lookahead = max(0, int(lookahead)) if self.exchange else 0
        if depth <= self.lookahead:
            raise ValueError("depth must exceed lookahead (a buffer set is reused after its step unpacked)")
        self.ordered = bool(ordered)  # False: no cross-group waits (A/B only: the order is then unconstrained)
        self._pend = []               # (b, slot, m, dec, rem, retry, reset, by event): result side not issued yet
        self._ev_req = None           # after the last request-side collective issued (stream R)
        self._ev_res = None           # after the last result-side collective issued (stream U)
        # ("req" | "res", step): the collective issue order, the last 4096 (tests)
        self.order_log = collections.deque(maxlen=4096)
        self.collectives = 0          # all-to-alls issued (tests: the exchange really ran)
        self.wait_s = 0.0             # host time spent waiting on the device: none by construction
        self.host_prof = {}

    @staticmethod
    def _p(t):
        return t.data_ptr()

    @staticmethod
    def _sp(stream):
        return stream.cuda_stream if stream is not None else None

    def _a2a(self, out, inp, group):
        """equal-split all-to-all (every split the same size: nothing to size)"""
        self.collectives += 1
        if self.staged:
            o = torch.empty(out.shape, dtype=out.dtype)
            dist.all_to_all_single(o, inp.cpu(), group=group)
            out.copy_(o, non_blocking=False)
        else:
            dist.all_to_all_single(out, inp, group=group)

    def _record(self, stream):
        if stream is None:
            return None
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def step(self, b, key, ts, n, cfg, dec, rem, retry, reset, op=OP_DECIDE):
        """route and decide batch b (device tensors: key/ts/n int64, cfg int32,
        complete now); its results reach dec/rem/retry/reset (the caller's
        order) once its result side is issued -- at once without the
        exchange, else `lookahead` steps later or at flush().  Returns the
        [(b', stream)] whose result sides this call issued: b' is complete on
        `stream`.  op: the step's kind, the same on every rank (OP_PEEK: the
        answers with nothing changed; OP_RESET: the keys deleted, n ignored
        and may be None; OP_REFUND: n units given back per request; OP_CHARGE:
        n units of usage recorded per request, `retry` receives `charged`)."""
        if op not in self._calls:
            raise ValueError(f"RoutedPipeline: unknown step kind {op!r}")
        call, call_ev = self._calls[op]
        if call is None and call_ev is None:
            raise ValueError(f"RoutedPipeline: a {_OP_NAMES[op]} step needs the pipeline built with "
                             f"{_OP_NAMES[op]}= or {_OP_NAMES[op]}_ev=")
        m = key.numel()
        assert m <= self.max_batch
        if n is None:
            if op != OP_RESET:
                raise ValueError("RoutedPipeline: only a reset step may leave n out")
            if self._zero_n is None:
                self._zero_n = torch.zeros(self.max_batch, dtype=torch.int64, device=self.dev)
            n = self._zero_n[:m]
        self._request_side(b, key, ts, n, cfg, call, call_ev)
        self._pend.append((b, self.slots[b % self.depth], m, dec, rem, retry, reset, call_ev is not None,
                           op == OP_DECIDE))
        done = []
        while len(self._pend) > self.lookahead:
            done.append(self._result_side(*self._pend.pop(0)))
        return done

    def _request_side(self, b, key, ts, n, cfg, call, call_ev, sel=None, after=None):
        """pack (of the requests with sel != 0, when given), request exchange,
        merge and the owner's engine call of step b, on R (after the event
        `after`, when given)"""
        s = self.slots[b % self.depth]
        m = key.numel()
        p, sp = self._p, self._sp
        R = self.R
        recv = s["recv"] if self.exchange else s["send"]
        rcnt = s["rcnt"] if self.exchange else s["scnt"]
        with _ctx(R):
            if s["ev_done"] is not None:
                R.wait_event(s["ev_done"])   # the set's previous step has unpacked
            if after is not None:
                R.wait_event(after)
            if sel is None:
                self.ops.pack(m, p(key), p(ts), p(n), p(cfg), p(s["send"]), p(s["scnt"]), p(s["slot"]), sp(R))
            else:
                self.ops.pack_sel(m, p(key), p(ts), p(n), p(cfg), p(sel), p(s["send"]), p(s["scnt"]), p(s["slot"]),
                                  sp(R))
            if self.exchange:
                if self._ev_res is not None and self.ordered and self.pg_res is not self.pg_req:
                    R.wait_event(self._ev_res)   # after the last result collective issued
                self._a2a(s["rcnt"], s["scnt"], self.pg_req)
                self._a2a(s["recv"], s["send"], self.pg_req)
                self.order_log.append(("req", b))
                self._ev_req = self._record(R)
            self.ops.merge(p(recv), p(rcnt), p(s["order"]), p(s["sms"]), p(s["count"]), sp(R))
            # the engine's grouping waits for R; U waits for its results
            if call_ev is not None:
                call_ev(self.m_max, p(s["count"]), p(recv), p(s["order"]), p(s["sms"]), p(s["res"]), sp(R),
                        s["ev_res"].cuda_event)
            else:
                call(self.m_max, p(s["count"]), p(recv), p(s["order"]), p(s["sms"]), p(s["res"]), sp(R),
                     sp(self.U))

    def allow_all(self, b, key, ts, n, cfg, first, dec, rem, retry, reset, verdict, rollback):
        """a routed AllowAll (include/rl_route.h) of the M members (key, ts, n,
        cfg; `first` uint8: member i starts a group when i == 0 or first[i] !=
        0) as the steps b and b + 1: a decide step, whose results reach
        dec/rem/retry/reset at once, the settle into `verdict` (uint8), and a
        refund step of the give-backs, whose statuses reach `rollback` (uint8)
        once step b + 1's result side is issued, as any step's.  Every rank
        calls it at the same step number.  Nothing is read by the host.
        Returns the [(b', stream)] whose result sides this call issued."""
        call, call_ev = self._calls[OP_DECIDE]
        rcall, rcall_ev = self._calls[OP_REFUND]
        if self.settle is None:
            raise ValueError("RoutedPipeline: allow_all needs the pipeline built with settle=")
        if call is None and call_ev is None:
            raise ValueError("RoutedPipeline: allow_all needs a decide call")
        if rcall is None and rcall_ev is None:
            raise ValueError("RoutedPipeline: allow_all needs the pipeline built with refund= or refund_ev=")
        if self.depth < 2:
            raise ValueError("RoutedPipeline: allow_all needs depth >= 2 (its two steps hold a buffer set each)")
        m = key.numel()
        assert m <= self.max_batch
        if self._aa is None:
            d, M = self.dev, self.max_batch
            self._aa = dict(g=torch.zeros(M, dtype=torch.int64, device=d),
                            sel=torch.zeros(M, dtype=torch.uint8, device=d),
                            out=[torch.empty(M, dtype=torch.int64, device=d) for _ in range(3)],
                            ev_packed=None)
        A = self._aa
        p, sp, U = self._p, self._sp, self.U
        done = self.flush()                       # Res(pending): the same order on every rank
        self._request_side(b, key, ts, n, cfg, call, call_ev)
        done.append(self._result_side(b, self.slots[b % self.depth], m, dec, rem, retry, reset, call_ev is not None,
                                      True))
        with _ctx(U):
            if A["ev_packed"] is not None:
                U.wait_event(A["ev_packed"])      # the previous call's pack has read g and sel
            self.settle(m, p(first), p(cfg), p(n), p(dec), p(verdict), p(A["g"]), p(A["sel"]), sp(U))
            settled = self._record(U)
        self._request_side(b + 1, key, ts, A["g"][:m], cfg, rcall, rcall_ev, sel=A["sel"], after=settled)
        A["ev_packed"] = self._record(self.R)
        self._pend.append((b + 1, self.slots[(b + 1) % self.depth], m, rollback, *(o[:m] for o in A["out"]),
                           rcall_ev is not None))
        while len(self._pend) > self.lookahead:
            done.append(self._result_side(*self._pend.pop(0)))
        return done

    def _result_side(self, b, s, m, dec, rem, retry, reset, by_event, observed=False):
        """result exchange and unpack of step b on U; observed: a decide step,
        which the observe= callables then count on its owner -- behind the
        exchange and the unpack, so the results leave first, and before
        ev_done, so the buffer set is not rewritten under them"""
        p, sp, U = self._p, self._sp, self.U
        with _ctx(U):
            if by_event:
                U.wait_event(s["ev_res"])        # this step's results (recorded by the engine)
            if self.exchange:
                if self._ev_req is not None and self.ordered and self.pg_res is not self.pg_req:
                    U.wait_event(self._ev_req)   # after the last request collective issued
                self._a2a(s["back"], s["res"], self.pg_res)
                self.order_log.append(("res", b))
                self._ev_res = self._record(U)
            self.ops.unpack(m, p(s["slot"]), p(s["back"] if self.exchange else s["res"]), p(dec), p(rem), p(retry),
                            p(reset), sp(U))
            if observed and self.observe:
                recv = s["recv"] if self.exchange else s["send"]
                rcnt = s["rcnt"] if self.exchange else s["scnt"]
                for f in self.observe:
                    f(self.m_max, p(s["count"]), p(recv), p(s["order"]), p(s["sms"]), p(s["res"]), p(rcnt),
                      self.world, sp(U))
            if U is not None:
                s["ev_done"] = torch.cuda.Event()
                s["ev_done"].record(U)
        return b, U

    def flush(self):
        """issue every deferred result side; returns [(b, stream)]"""
        done = []
        while self._pend:
            done.append(self._result_side(*self._pend.pop(0)))
        return done

    def _gather(self, read, top, clear, part_of, merge):
        self.flush()
        if self.U is not None:
            self.U.synchronize()      # every observe call has been enqueued on U: the local read sees them all
        part = part_of(read(top=top, clear=clear))
        if self.world == 1 and self.pg_res is None:
            return merge([part], top)
        parts = [None] * self.world
        dist.all_gather_object(parts, part, group=self.pg_res)
        return merge(parts, top)

    def usage(self, read, top=0, clear=False):
        """the cluster's usage tally (observe=[Engine.tally_routed]; read:
        Engine.tally_read): a collective -- every rank calls it at the same
        point.  Issues every deferred result side, waits for U, reads this
        rank's tally with the caller's `top` (and `clear`), gathers the ranks'
        reads over pg_res (world 1 without a group: no collective) and returns
        merge_tallies of them, the same on every rank.  The cluster's `top`
        most denied keys are among the ranks' local `top`: a key's denials are
        all on its owner."""
        return self._gather(read, top, clear, tally_part, merge_tallies)

    def top_keys(self, read, top=0, clear=False):
        """the cluster's top keys (observe=[Engine.hot_routed]; read:
        Engine.hot_read): a collective like usage(), merged by merge_hots"""
        return self._gather(read, top, clear, hot_part, merge_hots)

    def run(self, batches, outs, done=None, kinds=None):
        """all batches through the pipeline: batches[b] = (key, ts, n, cfg),
        outs[b] = (dec, rem, retry, reset); `done(b, stream)` after each;
        kinds[b] (default: every step decides) is step b's kind"""
        for b in range(len(batches)):
            op = OP_DECIDE if kinds is None else kinds[b]
            for bd, S in self.step(b, *batches[b], *outs[b], op=op):
                if done is not None:
                    done(bd, S)
        for bd, S in self.flush():
            if done is not None:
                done(bd, S)
