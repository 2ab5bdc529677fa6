"""The rate limiter's gRPC server (api/proto/ratelimiter.proto): the service
the reference plans in cmd/server/main.go:13-17 and docs/ARCHITECTURE.md
:287-304 -- per-tenant limiter instances, Allow / AllowN / Reset, a health
check, graceful shutdown -- backed by the MI355X engine through the request
coalescer (include/rl_coalescer.h): every RPC's requests join the next GPU
batch, and AllowBatch hands many requests to one batch at once.

Semantics per RPC follow the Go limiter (internal/ratelimiter):
  * time.Now() is read when the request arrives (tokenbucket.go:97,
    slidingwindow.go:73, fixedwindow.go:71);
  * n <= 0 -> INVALID_ARGUMENT "invalid n: must be greater than 0" (ErrInvalidN,
    errors.go:16; tokenbucket.go:91-93);
  * a storage (engine) error -> fail-open: {Allowed: true, Limit, Remaining 0,
    RetryAfter 0, ResetAt} (tokenbucket.go:100-112 and twins), fail-closed:
    UNAVAILABLE "failed to check rate limit: <err>";
  * keys are FormatKey(prefix, key) (config.go:81-87; prefix "" -> "ratelimit"),
    hashed to the engine's key ids on the host (rl_hash_keys_host).  As in
    Redis, the formatted key is the only namespace: two limiters with one
    prefix share state (a fixed and a sliding window of one length share
    their window counters, fixedwindow.go:139-141 / slidingwindow.go:150-152);
    --isolate-limiters gives every limiter a namespace of its own instead;
  * contexts (interface.go:75): the RPC deadline becomes the coalescer
    submission's deadline -- a request still queued when it passes is never
    applied -- and an expired or cancelled request takes the error branch
    (fail-open result, or DEADLINE_EXCEEDED / CANCELLED "failed to check rate
    limit: context ...");
  * the tables are collected from the serving path: the coalescer counts and
    GCs them between batches (rl_coalescer_opts.gc_*), so a long-running
    server never fills them.

Two front ends serve the same handlers' semantics: the native one (default,
include/rl_grpc.h: C++ event loops speaking HTTP/2 + protobuf themselves,
every RPC submitted to the coalescer as it arrives) and the Python one
(--frontend python: grpcio's server over RateLimiterService below, which
also documents the semantics the native server restates).

Run: python rl_server.py --address 127.0.0.1:8080 --limiter api:token_bucket:20:12s ...
"""
from __future__ import annotations

import argparse
import os
import re
import signal
import sys
import threading
import time
from concurrent import futures

import grpc
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import rl_amd  # noqa: E402
import rl_grpc  # noqa: E402

NS = 1_000_000_000
ERR_INVALID_N = "invalid n: must be greater than 0"            # errors.go:16
KEY_SEED = 0


def parse_duration(s: str) -> int:
    """Go time.ParseDuration subset: '1h2m3.5s', '500ms', '12s' -> ns"""
    units = {"ns": 1, "us": 1000, "µs": 1000, "ms": 1_000_000, "s": NS, "m": 60 * NS, "h": 3600 * NS}
    parts = re.findall(r"(\d+(?:\.\d*)?)(ns|us|µs|ms|s|m|h)", s)
    if not parts or "".join(a + b for a, b in parts) != s:
        raise ValueError(f"invalid duration {s!r}")
    return int(round(sum(float(a) * units[b] for a, b in parts)))


def _go_f2i(x: float) -> int:
    if not (x < 9223372036854775808.0) or not (x >= -9223372036854775808.0):
        return -(1 << 63)
    return int(x)


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= 1 << 63 else v


def reset_at_ns(alg: int, limit: int, window_ns: int, t: int) -> int:
    """Result.ResetAt of a request at t, as the fail-open path computes it
    (tokenbucket.go:161-165; fixedwindow.go:144-146; slidingwindow.go:155-157)"""
    if alg == rl_amd.TOKEN_BUCKET:
        wsec = float(window_ns // NS) + float(window_ns % NS) / 1e9
        rate = float(limit) / wsec
        now = float(t) / 1e9
        sec = _go_f2i(now)
        nsec = _go_f2i((now - float(sec)) * 1e9)
        return _wrap64(sec * NS + nsec + _go_f2i(float(limit) / rate * 1e9))
    r = (t + 62135596800 * NS) % window_ns           # time.Truncate is relative to year 1
    ws = (t - r) // NS
    return _wrap64(ws * NS + window_ns)


class Limiter:
    """One configured limiter instance (a reference Config, interface.go:46-70)."""

    def __init__(self, name, algorithm, limit, window_ns, prefix="", fail_open=False):
        err = rl_amd.config_validate(algorithm, limit, window_ns)
        if err:
            raise ValueError(f"invalid config: {err}")
        self.name = name
        self.alg = rl_amd.ALG_BY_NAME[algorithm]
        self.limit, self.window_ns = limit, window_ns
        self.prefix = (prefix or "ratelimit").encode()      # WithDefaults, config.go:62-64
        self.fail_open = fail_open
        self.cfg_id = None

    @staticmethod
    def parse(spec: str) -> "Limiter":
        """name:algorithm:limit:window[:prefix[:fail_open]]"""
        f = spec.split(":")
        if len(f) < 4:
            raise ValueError(f"limiter spec {spec!r}: name:algorithm:limit:window[:prefix[:fail_open]]")
        return Limiter(f[0], f[1], int(f[2]), parse_duration(f[3]), f[4] if len(f) > 4 else "",
                       len(f) > 5 and f[5].lower() in ("1", "true", "open", "fail_open"))


class RateLimiterService:
    """The RPC handlers over a coalescer (GPU engine, or the test seam's host
    backend).  `register(alg, limit, window_ns) -> cfg_id` registers a config
    with the backend; `clock()` -> Unix ns (time.Now())."""

    def __init__(self, limiters, coalescer, register, clock=time.time_ns, isolate=False, tally=False,
                 names_cap=4096, hot=False):
        # tally: serve RateLimiterMetrics.Usage from the coalescer's usage
        # tally (created with tally_key_slots), and remember the names of the
        # last names_cap keys a denied response went out for (newest wins)
        # hot: serve RateLimiterTopKeys.TopKeys from the coalescer's top keys
        # (created with hot_min).  The watch set is the key ids of the latest
        # TopKeys response, names_cap at most: a request of one of them records
        # its name in the same map, so a hot key that is never denied is named
        # from the second scrape on
        self.tally = tally
        self.hot = hot
        self.watch = frozenset()
        self.names_cap = names_cap
        self.names = {}                      # key id -> name, in insertion order
        self.names_lock = threading.Lock()
        self.a = rl_grpc.api("ratelimiter.proto")
        self.h = rl_grpc.api("health.proto")
        self.co = coalescer
        self.clock = clock
        self.isolate = isolate
        self.by_name = {}
        for lim in limiters:
            lim.cfg_id = register(lim.alg, lim.limit, lim.window_ns)
            self.by_name[lim.name] = lim
        self.serving = True

    # -- helpers -------------------------------------------------------------
    def _limiter(self, name, ctx):
        lim = self.by_name.get(name)
        if lim is None:
            ctx.abort(grpc.StatusCode.NOT_FOUND, f"unknown limiter {name!r}")
        return lim

    def _ids(self, lim, keys, m) -> np.ndarray:
        """FormatKey(prefix, key) hashed: the formatted key is the namespace
        (Redis), or one namespace per limiter with --isolate-limiters"""
        return rl_amd.hash_keys_host(keys, KEY_SEED, lim.prefix, cfg=[lim.cfg_id] * m if self.isolate else None)

    def _key_id(self, lim, key: str) -> int:
        return int(self._ids(lim, [key.encode()], 1)[0])

    @staticmethod
    def _deadline(ctx) -> int:
        """the RPC deadline on the coalescer's clock (0 = none)"""
        rem = ctx.time_remaining() if ctx is not None else None
        if rem is None or rem > 1e6:   # no deadline (gRPC reports an infinite one as huge)
            return 0
        return max(1, rl_amd.now_ns() + int(rem * 1e9))

    # rl_coalescer status -> (go error text, gRPC code) of the error branch
    _CTX_ERR = {rl_amd.RL_EDEADLINE: ("context deadline exceeded", grpc.StatusCode.DEADLINE_EXCEEDED),
                rl_amd.RL_ECANCELED: ("context canceled", grpc.StatusCode.CANCELLED)}

    def _result(self, lim, t, rc, dec, rem, retry, reset):
        """AllowResponse, or (None, fail-closed error text, gRPC code)"""
        if rc == rl_amd.RL_OK and dec in (rl_amd.ALLOWED, rl_amd.DENIED):
            return self.a.AllowResponse(allowed=dec == rl_amd.ALLOWED, limit=lim.limit, remaining=rem,
                                        retry_after_ns=retry, reset_at_unix_ns=reset), None, None
        if rc in self._CTX_ERR:
            err, code = self._CTX_ERR[rc]
        else:
            err = f"engine status {rc}" if rc != rl_amd.RL_OK else "script error (INCRBY overflow)"
            code = grpc.StatusCode.UNAVAILABLE
        if lim.fail_open:
            return self.a.AllowResponse(allowed=True, limit=lim.limit, remaining=0, retry_after_ns=0,
                                        reset_at_unix_ns=reset_at_ns(lim.alg, lim.limit, lim.window_ns, t)), \
                None, None
        return None, f"failed to check rate limit: {err}", code

    def _allow_n(self, name, key, n, ctx):
        lim = self._limiter(name, ctx)
        if n <= 0:
            ctx.abort(grpc.StatusCode.INVALID_ARGUMENT, ERR_INVALID_N)
        t = self.clock()
        kid = self._key_id(lim, key)
        rc, (dec, rem, retry, reset) = self.co.decide(kid, t, n, lim.cfg_id, deadline_ns=self._deadline(ctx))
        if rc == rl_amd.RL_OK and ((dec == rl_amd.DENIED and self.tally) or kid in self.watch):
            self._remember(kid, key)
        res, err, code = self._result(lim, t, rc, dec, rem, retry, reset)
        if err:
            ctx.abort(code, err)
        return res

    def _remember(self, kid: int, key: str):
        """the name of a key a denied response goes out for (Usage reports
        it), or of a key in the watch set (TopKeys does)"""
        if not (self.tally or self.hot) or self.names_cap <= 0:
            return
        with self.names_lock:
            self.names.pop(kid, None)
            self.names[kid] = key
            while len(self.names) > self.names_cap:
                del self.names[next(iter(self.names))]

    # -- RPCs ----------------------------------------------------------------
    def Usage(self, req, ctx):
        """one rl_coalescer_tally, in sequence order (blocks this handler
        thread, not the server)"""
        if not self.tally:
            ctx.abort(grpc.StatusCode.FAILED_PRECONDITION, "usage tally is off")
        top = min(req.top, 1 << 16)
        # rows for this server's limiters: up to their highest config id
        rows = 1 + max((lim.cfg_id for lim in self.by_name.values()), default=0)
        rc, t = self.co.tally(top=top, clear=req.clear, max_configs=rows)
        if rc == rl_amd.RL_EINVAL:
            ctx.abort(grpc.StatusCode.FAILED_PRECONDITION, "usage tally is off")
        if rc != rl_amd.RL_OK:
            ctx.abort(grpc.StatusCode.UNAVAILABLE, f"failed to read usage: engine status {rc}")
        by_cfg = {lim.cfg_id: lim for lim in reversed(list(self.by_name.values()))}
        out = self.a.UsageResponse(untracked_requests=t.info.untracked_requests, keys_tracked=t.keys_tracked)
        for lim in self.by_name.values():
            c = t.cfg[lim.cfg_id] if lim.cfg_id < t.cfg.size else None
            out.limiters.add(limiter=lim.name, **({} if c is None else dict(
                allowed=int(c["count"][rl_amd.ALLOWED]), denied=int(c["count"][rl_amd.DENIED]),
                errors=int(c["count"][rl_amd.ERROR]), invalid=int(c["count"][rl_amd.INVALID]),
                units_allowed=int(c["units"][1]), units_denied=int(c["units"][0]))))
        with self.names_lock:
            names = {int(r["key_id"]): self.names.get(int(r["key_id"]), "") for r in t.keys}
        for r in t.keys:
            lim = by_cfg.get(int(r["cfg_id"]))
            out.keys.add(limiter=lim.name if lim else "", key_hash=int(r["key_id"]), key=names[int(r["key_id"])],
                         denied=int(r["denied"]), units_denied=int(r["units_denied"]))
        return out

    def TopKeys(self, req, ctx):
        """one rl_coalescer_hot, in sequence order (blocks this handler thread,
        not the server); its keys become the watch set"""
        if not self.hot:
            ctx.abort(grpc.StatusCode.FAILED_PRECONDITION, "top keys are off")
        rc, h = self.co.hot(top=min(req.top, 1 << 16), clear=req.clear)
        if rc == rl_amd.RL_EINVAL:
            ctx.abort(grpc.StatusCode.FAILED_PRECONDITION, "top keys are off")
        if rc != rl_amd.RL_OK:
            ctx.abort(grpc.StatusCode.UNAVAILABLE, f"failed to read top keys: engine status {rc}")
        by_cfg = {lim.cfg_id: lim for lim in reversed(list(self.by_name.values()))}
        i = h.info
        out = self.a.TopKeysResponse(total=i.total, keys_tracked=h.keys_tracked, dropped=i.dropped, width=i.width,
                                     hot_min=i.hot_min, weight=i.weight)
        ids = [int(r["key_id"]) for r in h.keys]
        with self.names_lock:
            names = {k: self.names.get(k, "") for k in ids}
        for r, k in zip(h.keys, ids):
            lim = by_cfg.get(int(r["cfg_id"]))
            out.keys.add(limiter=lim.name if lim else "", key_hash=k, key=names[k], estimate=int(r["estimate"]))
        self.watch = frozenset(ids[:max(self.names_cap, 0)])
        return out

    def Allow(self, req, ctx):
        return self._allow_n(req.limiter, req.key, 1, ctx)

    def AllowN(self, req, ctx):
        return self._allow_n(req.limiter, req.key, req.n, ctx)

    def Peek(self, req, ctx):
        """the AllowResponse AllowN(key, n) would get now, with nothing changed
        (rl_coalescer_peek); an omitted n (0) asks how much is left.  Blocks
        like Reset: queued in sequence order, no deadline of its own."""
        lim = self._limiter(req.limiter, ctx)
        if req.n < 0:
            ctx.abort(grpc.StatusCode.INVALID_ARGUMENT, ERR_INVALID_N)
        t = self.clock()
        rc, (dec, rem, retry, reset) = self.co.peek([self._key_id(lim, req.key)], [t], [req.n], [lim.cfg_id])
        res, err, code = self._result(lim, t, rc, int(dec[0]), int(rem[0]), int(retry[0]), int(reset[0]))
        if err:
            ctx.abort(code, err)
        return res

    def Reset(self, req, ctx):
        lim = self._limiter(req.limiter, ctx)
        rc = self.co.reset(self._key_id(lim, req.key), self.clock(), lim.cfg_id)
        if rc != rl_amd.RL_OK:
            ctx.abort(grpc.StatusCode.UNAVAILABLE, f"failed to reset rate limit: engine status {rc}")
        return self.a.ResetResponse()

    def ResetBatch(self, req, ctx):
        """many Reset calls: one reset_batch submission to the coalescer; an
        unknown limiter is that entry's error string"""
        rs = req.requests
        t = self.clock()
        errors = [""] * len(rs)
        idx, keys, cfg = [], [], []
        groups = {}
        for i, r in enumerate(rs):
            lim = self.by_name.get(r.limiter)
            if lim is None:
                errors[i] = f"unknown limiter {r.limiter!r}"
                continue
            groups.setdefault(r.limiter, []).append(len(idx))
            idx.append(i)
            keys.append(r.key.encode())
            cfg.append(lim.cfg_id)
        if idx:
            kid = np.empty(len(idx), np.uint64)
            for name, pos in groups.items():
                kid[pos] = self._ids(self.by_name[name], [keys[p] for p in pos], len(pos))
            rc, status = self.co.reset_batch(kid, np.full(len(idx), t, np.int64), np.array(cfg, np.uint32))
            for j, i in enumerate(idx):
                if rc != rl_amd.RL_OK:
                    errors[i] = f"failed to reset rate limit: engine status {rc}"
                elif status[j] != rl_amd.RESET_DONE:
                    errors[i] = f"failed to reset rate limit: engine status {rl_amd.RL_EINVAL}"
        return self.a.ResetBatchResponse(errors=errors)

    @staticmethod
    def _refund_ts(r, t):
        """the time that picks the refund's window: just inside the window
        whose reset time the client passes back, or now"""
        return r.window_reset_at_unix_ns - 1 if r.window_reset_at_unix_ns else t

    def Refund(self, req, ctx):
        """give n units back (rl_coalescer_refund): one submission, applied in
        sequence order.  Blocks like Reset; a storage error is the RPC's error,
        never a fail-open answer."""
        lim = self._limiter(req.limiter, ctx)
        if req.n <= 0:
            ctx.abort(grpc.StatusCode.INVALID_ARGUMENT, ERR_INVALID_N)
        rc, status = self.co.refund([self._key_id(lim, req.key)], [self._refund_ts(req, self.clock())], [req.n],
                                    [lim.cfg_id])
        if rc != rl_amd.RL_OK:
            ctx.abort(grpc.StatusCode.UNAVAILABLE, f"failed to refund rate limit: engine status {rc}")
        return self.a.RefundResponse(applied=int(status[0]) == rl_amd.REFUND_DONE)

    def RefundBatch(self, req, ctx):
        """many refunds: one refund submission to the coalescer (one engine
        call: refunds of one key and window are summed); an unknown limiter or
        n <= 0 is that entry's error string"""
        rs = req.requests
        t = self.clock()
        out = [None] * len(rs)
        idx, keys, cfg, ns, ts = [], [], [], [], []
        groups = {}
        for i, r in enumerate(rs):
            lim = self.by_name.get(r.limiter)
            if lim is None:
                out[i] = self.a.RefundResult(error=f"unknown limiter {r.limiter!r}")
            elif r.n <= 0:
                out[i] = self.a.RefundResult(error=ERR_INVALID_N)
            else:
                groups.setdefault(r.limiter, []).append(len(idx))
                idx.append(i)
                keys.append(r.key.encode())
                cfg.append(lim.cfg_id)
                ns.append(r.n)
                ts.append(self._refund_ts(r, t))
        if idx:
            kid = np.empty(len(idx), np.uint64)
            for name, pos in groups.items():
                kid[pos] = self._ids(self.by_name[name], [keys[p] for p in pos], len(pos))
            rc, status = self.co.refund(kid, np.array(ts, np.int64), np.array(ns, np.int64), np.array(cfg, np.uint32))
            for j, i in enumerate(idx):
                if rc != rl_amd.RL_OK:
                    out[i] = self.a.RefundResult(error=f"failed to refund rate limit: engine status {rc}")
                else:
                    out[i] = self.a.RefundResult(applied=int(status[j]) == rl_amd.REFUND_DONE)
        return self.a.RefundBatchResponse(results=out)

    # --- RateLimiterMulti: all-or-nothing checks across limiters ---

    def _group_error(self, checks):
        """why a group of checks cannot run, or None"""
        if not 1 <= len(checks) <= 16:
            return f"checks: need 1 to 16, got {len(checks)}"
        for r in checks:
            if r.limiter not in self.by_name:
                return f"unknown limiter {r.limiter!r}"
            if r.n <= 0:
                return ERR_INVALID_N
        return None

    def _allow_all(self, groups, ctx):
        """one rl_coalescer_allow_all submission for the groups that can run ->
        per group (error text | None, gRPC code, AllowAllResponse)"""
        t = self.clock()
        out = [None] * len(groups)
        run, keys, cfg, ns, first, names = [], [], [], [], [], {}
        for g, checks in enumerate(groups):
            err = self._group_error(checks)
            if err:
                res = [self.a.AllowResponse(error=err) for _ in range(max(1, len(checks)))]
                out[g] = (err, grpc.StatusCode.INVALID_ARGUMENT,
                          self.a.AllowAllResponse(allowed=False, results=res, denied_by=-1))
                continue
            run.append(g)
            for j, r in enumerate(checks):
                names.setdefault(r.limiter, []).append(len(keys))
                keys.append(r.key.encode())
                cfg.append(self.by_name[r.limiter].cfg_id)
                ns.append(r.n)
                first.append(1 if j == 0 else 0)
        if run:
            kid = np.empty(len(keys), np.uint64)
            for name, pos in names.items():
                kid[pos] = self._ids(self.by_name[name], [keys[p] for p in pos], len(pos))
            rc, (dec, rem, retry, reset, verdict) = self.co.allow_all(
                kid, np.full(len(keys), t, np.int64), np.array(ns, np.int64), np.array(cfg, np.uint32),
                np.array(first, np.uint8), deadline_ns=self._deadline(ctx))
            at = 0
            for g in run:
                results, rolled, bad = [], [], None
                for r in groups[g]:
                    lim = self.by_name[r.limiter]
                    res, err, code = self._result(lim, t, rc, int(dec[at]), int(rem[at]), int(retry[at]), int(reset[at]))
                    if res is None:
                        bad = bad or (err, code)
                        res = self.a.AllowResponse(error=err)
                    results.append(res)
                    took = dec[at] == rl_amd.ALLOWED or (dec[at] == rl_amd.DENIED and lim.alg != rl_amd.TOKEN_BUCKET)
                    rolled.append(bool(rc == rl_amd.RL_OK and verdict[at] != rl_amd.ALLOWED and took))
                    at += 1
                by = next((j for j, x in enumerate(results) if not x.allowed), -1)
                out[g] = (bad[0] if bad else None, bad[1] if bad else None,
                          self.a.AllowAllResponse(allowed=by < 0, results=results, denied_by=by, rolled_back=rolled))
        return out

    def AllowAll(self, req, ctx):
        """one request against 1 to 16 limiters, all or nothing
        (rl_coalescer_allow_all): one submission, one group"""
        err, code, res = self._allow_all([list(req.checks)], ctx)[0]
        if err:
            ctx.abort(code, err)
        return res

    def AllowAllBatch(self, req, ctx):
        """many such requests: one submission, one launch; a request that
        cannot run, or that a fail-closed limiter failed, carries the error in
        its results"""
        out = self._allow_all([list(r.checks) for r in req.requests], ctx)
        return self.a.AllowAllBatchResponse(responses=[res for _, _, res in out])

    # --- RateLimiterCharge: usage recorded after the fact ---

    def _charge_result(self, lim, t, rc, n, dec, charged, rem, reset):
        """ChargeResponse, or (None, fail-closed error text, gRPC code).  A
        storage error: a fail-open limiter answers charged = 0 with no error
        (the usage is not recorded and nobody is held up)"""
        if rc == rl_amd.RL_OK and dec in (rl_amd.ALLOWED, rl_amd.DENIED):
            return self.a.ChargeResponse(charged=charged, short=n - charged, over_limit=dec == rl_amd.DENIED,
                                         remaining=rem, reset_at_unix_ns=reset), None, None
        if lim.fail_open:
            return self.a.ChargeResponse(charged=0, short=n, over_limit=False, remaining=0,
                                         reset_at_unix_ns=reset_at_ns(lim.alg, lim.limit, lim.window_ns, t)), None, None
        if rc in self._CTX_ERR:
            err, code = self._CTX_ERR[rc]
        else:
            err = f"engine status {rc}" if rc != rl_amd.RL_OK else "script error (INCRBY overflow)"
            code = grpc.StatusCode.UNAVAILABLE
        return None, f"failed to charge rate limit: {err}", code

    def Charge(self, req, ctx):
        """record n units of usage after the fact (rl_coalescer_charge): one
        submission, applied in sequence order"""
        lim = self.by_name.get(req.limiter)
        if lim is None:
            ctx.abort(grpc.StatusCode.INVALID_ARGUMENT, f"unknown limiter {req.limiter!r}")
        if req.n <= 0:
            ctx.abort(grpc.StatusCode.INVALID_ARGUMENT, ERR_INVALID_N)
        t = self.clock()
        rc, (dec, charged, rem, reset) = self.co.charge([self._key_id(lim, req.key)], [t], [req.n], [lim.cfg_id],
                                                        deadline_ns=self._deadline(ctx))
        res, err, code = self._charge_result(lim, t, rc, req.n, int(dec[0]), int(charged[0]), int(rem[0]),
                                             int(reset[0]))
        if err:
            ctx.abort(code, err)
        return res

    def ChargeBatch(self, req, ctx):
        """many charges: one Charge submission to the coalescer (one engine
        call); an unknown limiter or n <= 0 is that entry's error string"""
        rs = req.requests
        t = self.clock()
        out = [None] * len(rs)
        idx, keys, cfg, ns = [], [], [], []
        groups = {}
        for i, r in enumerate(rs):
            lim = self.by_name.get(r.limiter)
            if lim is None:
                out[i] = self.a.ChargeResponse(error=f"unknown limiter {r.limiter!r}")
            elif r.n <= 0:
                out[i] = self.a.ChargeResponse(error=ERR_INVALID_N)
            else:
                groups.setdefault(r.limiter, []).append(len(idx))
                idx.append(i)
                keys.append(r.key.encode())
                cfg.append(lim.cfg_id)
                ns.append(r.n)
        if idx:
            kid = np.empty(len(idx), np.uint64)
            for name, pos in groups.items():
                kid[pos] = self._ids(self.by_name[name], [keys[p] for p in pos], len(pos))
            rc, (dec, charged, rem, reset) = self.co.charge(kid, np.full(len(idx), t, np.int64), np.array(ns, np.int64),
                                                            np.array(cfg, np.uint32), deadline_ns=self._deadline(ctx))
            for j, i in enumerate(idx):
                res, err, _ = self._charge_result(self.by_name[rs[i].limiter], t, rc, ns[j], int(dec[j]),
                                                  int(charged[j]), int(rem[j]), int(reset[j]))
                out[i] = res if res is not None else self.a.ChargeResponse(error=err)
        return self.a.ChargeBatchResponse(results=out)

    def AllowBatch(self, req, ctx):
        """many AllowN calls: one submission to the coalescer (one GPU batch
        when it fits); per-request errors in AllowResponse.error"""
        rs = req.requests
        m = len(rs)
        t = self.clock()
        out = [None] * m
        idx, keys, cfg, ns = [], [], [], []
        groups = {}
        for i, r in enumerate(rs):
            lim = self.by_name.get(r.limiter)
            if lim is None:
                out[i] = self.a.AllowResponse(error=f"unknown limiter {r.limiter!r}")
            elif r.n <= 0:
                out[i] = self.a.AllowResponse(error=ERR_INVALID_N)
            else:
                groups.setdefault(r.limiter, []).append(len(idx))
                idx.append(i)
                keys.append(r.key.encode())
                cfg.append(lim.cfg_id)
                ns.append(r.n)
        if idx:
            kid = np.empty(len(idx), np.uint64)
            for name, pos in groups.items():
                kid[pos] = self._ids(self.by_name[name], [keys[p] for p in pos], len(pos))
            tk = self.co.submit(kid, np.full(len(idx), t, np.int64), np.array(ns, np.int64), np.array(cfg, np.uint32),
                                deadline_ns=self._deadline(ctx))
            rc, (dec, rem, retry, reset) = self.co.wait(tk, len(idx))
            for j, i in enumerate(idx):
                lim = self.by_name[rs[i].limiter]
                if rc == rl_amd.RL_OK and ((dec[j] == rl_amd.DENIED and self.tally) or int(kid[j]) in self.watch):
                    self._remember(int(kid[j]), rs[i].key)
                res, err, _ = self._result(lim, t, rc, int(dec[j]), int(rem[j]), int(retry[j]), int(reset[j]))
                out[i] = res if res is not None else self.a.AllowResponse(error=err)
        return self.a.AllowBatchResponse(results=out)

    def Check(self, req, ctx):
        S = self.h.HealthCheckResponse
        if req.service not in ("", "ratelimiter.v1.RateLimiter"):
            return S(status=3)   # SERVICE_UNKNOWN
        return S(status=1 if self.serving else 2)


def build_server(service: RateLimiterService, address: str, workers: int = 64) -> tuple[grpc.Server, int]:
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=workers),
                         options=[("grpc.so_reuseport", 0)])
    for a, sname, impl in ((service.a, "RateLimiter", service), (service.a, "RateLimiterStatus", service),
                           (service.a, "RateLimiterAdmin", service), (service.a, "RateLimiterMetrics", service),
                           (service.a, "RateLimiterTopKeys", service), (service.a, "RateLimiterRefund", service),
                           (service.a, "RateLimiterMulti", service), (service.a, "RateLimiterCharge", service),
                           (service.h, "Health", service)):
        handlers = {}
        for mname, inp, out in a.services[sname]:
            handlers[mname] = grpc.unary_unary_rpc_method_handler(
                getattr(impl, mname), request_deserializer=getattr(a, inp).FromString,
                response_serializer=getattr(a, out).SerializeToString)
        server.add_generic_rpc_handlers((grpc.method_handlers_generic_handler(a.full_service(sname), handlers),))
    port = server.add_insecure_port(address)
    return server, port


class GpuBackend:
    """engine + coalescer on one GPU (the production backend)"""

    def __init__(self, device=0, tb_capacity=1 << 22, win_capacity=1 << 22, max_batch=1 << 16):
        self.eng = rl_amd.Engine(profile=rl_amd.PROFILE_REDIS7, tb_capacity=tb_capacity, win_capacity=win_capacity,
                                 max_batch=max_batch, device=device, flags=rl_amd.OPT_PIPELINE)
        self.register = self.eng.register
        self.co = None

    def start(self, max_batch=1 << 16, gc_interval_ns=NS, gc_margin_ms=1000, tally_key_slots=0, **hot):
        """the coalescer, with the tables collected from the serving path
        (tally_key_slots != 0: with the usage tally, RateLimiterMetrics.Usage;
        hot_min != 0, with hot_width, hot_key_slots and hot_weight: with the
        top keys, RateLimiterTopKeys.TopKeys)"""
        self.co = rl_amd.Coalescer(self.eng, max_batch=max_batch, max_in_flight=3, gc_interval_ns=gc_interval_ns,
                                   gc_margin_ms=gc_margin_ms, tally_key_slots=tally_key_slots, **hot)
        return self.co

    def close(self):
        if self.co:
            self.co.close()
        self.eng.close()


def serve(service, address, workers=64, grace_s=5.0, ready=None, stop_event=None):
    """run until SIGTERM / SIGINT (or stop_event): then NOT_SERVING, stop
    accepting, finish in-flight RPCs within grace_s (graceful shutdown)"""
    server, port = build_server(service, address, workers)
    server.start()
    if ready:
        ready(port)
    stop = stop_event or threading.Event()
    if threading.current_thread() is threading.main_thread():
        for sig in (signal.SIGTERM, signal.SIGINT):
            signal.signal(sig, lambda *_: stop.set())
    stop.wait()
    service.serving = False
    server.stop(grace_s).wait()
    return port


def serve_native(co, limiters, address, io_threads=4, isolate=False, grace_s=5.0, ready=None, stop_event=None,
                 tally=False):
    """the native front end (include/rl_grpc.h) until SIGTERM / SIGINT (or
    stop_event): then health NOT_SERVING, stop accepting, answer the RPCs in
    flight within grace_s"""
    host, port = address.rsplit(":", 1)
    srv = rl_amd.GrpcServer(co, [(l.name, l.cfg_id, l.alg, l.limit, l.window_ns, l.prefix, l.fail_open)
                                 for l in limiters], host=host, port=int(port), io_threads=io_threads,
                            isolate=isolate, tally=tally)
    try:
        if ready:
            ready(srv.port)
        stop = stop_event or threading.Event()
        if threading.current_thread() is threading.main_thread():
            for sig in (signal.SIGTERM, signal.SIGINT):
                signal.signal(sig, lambda *_: stop.set())
        stop.wait()
        srv.shutdown(grace_s)
        if os.environ.get("RL_SERVER_STATS"):
            import json
            cs, gs = co.stats(), srv.stats()
            print(json.dumps({"coalescer": {k: getattr(cs, k) for k, _ in cs._fields_[2:]},
                              "grpc": {k: getattr(gs, k) for k, _ in gs._fields_[2:]}}), file=sys.stderr, flush=True)
    finally:
        srv.close()
    return srv.port


def main(argv=None):
    ap = argparse.ArgumentParser(description="rate limiter gRPC server (MI355X engine)")
    ap.add_argument("--address", default="127.0.0.1:8080", help="listen address (docs/ARCHITECTURE.md: port 8080)")
    ap.add_argument("--limiter", action="append", default=[],
                    help="name:algorithm:limit:window[:prefix[:fail_open]], repeatable")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frontend", choices=["native", "python"], default="native",
                    help="native: C++ HTTP/2 event loops (include/rl_grpc.h); python: grpcio server")
    ap.add_argument("--io-threads", type=int, default=4, help="native front end: event-loop threads")
    ap.add_argument("--workers", type=int, default=64, help="python front end: handler threads")
    ap.add_argument("--max-batch", type=int, default=1 << 16)
    ap.add_argument("--tb-capacity", type=int, default=1 << 22)
    ap.add_argument("--win-capacity", type=int, default=1 << 22)
    ap.add_argument("--gc-interval-ms", type=float, default=1000.0,
                    help="count the tables at least this often and collect expired keys (0 = never)")
    ap.add_argument("--gc-margin-ms", type=int, default=1000,
                    help="GC at the last request's clock minus this (request clocks may lag by this much)")
    ap.add_argument("--isolate-limiters", action="store_true",
                    help="one key namespace per limiter (the reference shares state between limiters with "
                         "the same prefix, as Redis keys are the formatted strings)")
    ap.add_argument("--tally-key-slots", type=int, default=0,
                    help="usage tally (RateLimiterMetrics.Usage): records of the throttled-key table, 0 = off")
    ap.add_argument("--hot-min", type=int, default=0,
                    help="top keys (RateLimiterTopKeys.TopKeys): a key whose estimated weight reaches this becomes "
                         "a candidate, 0 = off")
    ap.add_argument("--hot-width", type=int, default=0, help="top keys: counters per sketch row, 0 = 262144")
    ap.add_argument("--hot-key-slots", type=int, default=0, help="top keys: candidate records, 0 = 65536")
    ap.add_argument("--hot-units", action="store_true", help="top keys: weigh a request by n, not by 1")
    args = ap.parse_args(argv)
    specs = args.limiter or ["default:token_bucket:20:12s"]
    limiters = [Limiter.parse(s) for s in specs]
    be = GpuBackend(args.device, args.tb_capacity, args.win_capacity, args.max_batch)
    hot = dict(hot_min=args.hot_min, hot_width=args.hot_width, hot_key_slots=args.hot_key_slots,
               hot_weight=rl_amd.HOT_UNITS if args.hot_units else rl_amd.HOT_REQUESTS)
    print(f"rate limiter gRPC server on {args.address} ({args.frontend} front end): " + ", ".join(specs),
          file=sys.stderr, flush=True)
    try:
        if args.frontend == "native":
            for lim in limiters:
                lim.cfg_id = be.register(lim.alg, lim.limit, lim.window_ns)
            co = be.start(args.max_batch, int(args.gc_interval_ms * 1e6),
                          args.gc_margin_ms, args.tally_key_slots, **hot)
            serve_native(co, limiters, args.address, args.io_threads, args.isolate_limiters,
                         ready=lambda p: print(f"READY {p}", flush=True), tally=args.tally_key_slots != 0)
        else:
            svc = RateLimiterService(limiters, None, be.register, isolate=args.isolate_limiters,
                                     tally=args.tally_key_slots != 0, hot=args.hot_min != 0)
            svc.co = be.start(args.max_batch, int(args.gc_interval_ms * 1e6), args.gc_margin_ms,
                              args.tally_key_slots, **hot)
            serve(svc, args.address, args.workers, ready=lambda p: print(f"READY {p}", flush=True))
    finally:
        be.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
