/*
 * rl_route.h -- hash-sharded routing of request batches across GPUs
 * (BASELINE.json configs[3]).
 *
 * The reference's deployment is N stateless app servers sharing one Redis
 * (docs/ARCHITECTURE.md:142-164): every server may ask about any key, and the
 * store applies each key's requests in arrival order.  Here the key space is
 * split over the GPUs of a node -- GPU owner(k) = (mix64(k) >> 32) mod G keeps
 * key k's state in its HBM tables -- and every GPU accepts requests for any
 * key.  One step of G ranks, each with a batch of requests, runs with no host
 * involvement at all (nothing is read back to size anything):
 *
 *   sender   rl_route_pack      owner of every request; requests grouped by
 *                               owner (stable) into fixed-capacity buckets of
 *                               `cap` 32-byte records, send[o * cap + j]; per
 *                               owner an info row {count sent, earliest ts,
 *                               latest ts, flags: 2 * count dropped + 1 if
 *                               the batch's ts ever decrease}.  A request past
 *                               its owner's capacity is dropped: never
 *                               executed, decision RL_DROPPED, and the
 *                               router's sticky status reports RL_EOVERFLOW
 *            equal-split all-to-alls of the info rows and of the buckets
 *            (RCCL over xGMI; the caller drives the collectives, e.g.
 *            torch.distributed "nccl"): every split is `cap` records, so the
 *            collectives need no host-side sizes
 *   owner    rl_route_merge     the received buckets -- source s's `count`
 *                               records at recv[s * cap], in its order -- in
 *                               the order ONE shared store sees them: by
 *                               arrival time, ties by (source rank, source
 *                               position), where a request arrives at the
 *                               running max of its source's ts so far (each
 *                               source's own order is kept, also for a batch
 *                               out of time order).  Planned on the device:
 *                               per-source running maxima, then a tree of
 *                               merge-path merges; writes the decision order
 *                               order[p] (a receive index), each request's
 *                               store clock server_ms[p] and the number
 *                               received into *count (device memory)
 *            rl_decide_routed_device: the owner's engine reads the received
 *                               records in that order and writes 32-byte
 *                               result records at their receive index
 *            (a peek, reset, refund or charge step calls
 *                               rl_peek_routed_device / rl_reset_routed_device /
 *                               rl_refund_routed_device / rl_charge_routed_device
 *                               here instead; see there)
 *            equal-split all-to-all of the result buckets back
 *   sender   rl_route_unpack    results to the caller's order
 * (a routed AllowAll is two such steps with a settle on the sender between
 * them and rl_route_pack_sel packing the second; see rl_allow_all_settle_device)
 *
 * The store's clock (Redis TTLs) is one clock that never goes back: request
 * p of step b expires keys at server_ms = max(floor(arrival_p / 1e6), the
 * latest floor(ts / 1e6) of any request of any rank in steps before b).
 * Every owner learns each rank's latest ts through the info rows, so all
 * owners keep the same clock (in device memory), and per key the clock never
 * decreases (merge order is arrival order), which is what makes expiry exact
 * (rl_window.h).
 *
 * Every array is device memory; every call is asynchronous on `stream` (a
 * hipStream_t).  Calls on one router use its scratch: packs must run in step
 * order, merges too (the store clock), e.g. each on one stream or ordered by
 * events.
 */
#ifndef RL_ROUTE_H
#define RL_ROUTE_H

#include <stddef.h>
#include <stdint.h>

#include "rl_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RL_EOVERFLOW (-75)     /* a request exceeded its owner's bucket capacity (rl_router_sync) */
#define RL_DROPPED 4           /* decision: not executed, its owner's bucket was full (resubmit it) */
#define RL_ROUTE_INFO 4        /* int64 per info row: count sent, earliest ts, latest ts, 2 * dropped + unsorted */
#define RL_ORDER_IDENTITY 0xffffffffu   /* order[0]: the received order is the decision order (rl_route_merge) */

/* one routed request (send and receive buckets) */
typedef struct rl_route_rec {
    uint64_t key;
    int64_t ts;
    int64_t n;
    uint32_t cfg;
    uint32_t pos;      /* position in the sender's batch */
} rl_route_rec;

/* one routed result (the four Result fields of include/rl_engine.h) */
typedef struct rl_route_res {
    int64_t decision;
    int64_t remaining;
    int64_t retry_after_ns;
    int64_t reset_at_ns;
} rl_route_res;

typedef struct rl_router rl_router;

/* scratch for batches of up to max_batch requests and buckets of `cap`
 * records per peer (rounded up to a multiple of 2048; rl_router_capacity).
 * cap = max_batch can never drop a request; a hash partition of a uniform
 * key stream needs about max_batch / world plus a margin. */
int rl_router_create(int32_t device, int32_t world, uint32_t max_batch, uint32_t cap, rl_router** out);
int rl_router_destroy(rl_router* r);
/* the bucket capacity in records (every split of the collectives) */
uint32_t rl_router_capacity(const rl_router* r);
/* wait for the router's queued work on `stream`; returns and clears the
 * sticky status: RL_EOVERFLOW when a request was dropped since the last sync */
int rl_router_sync(rl_router* r, void* stream);

/* A stream on a hardware queue of its own (CU-masked with every CU, which
 * the runtime never shares): with more streams than the process's hardware
 * queues, a stream that waits on an event blocks every stream sharing its
 * queue; the routed pipeline's streams wait on the engine's, so they need
 * their own.  Returns a hipStream_t in *out. */
int rl_stream_create_dedicated(int32_t device, void** out);
int rl_stream_destroy(void* stream);

/* owner of each key id (the partition: (mix64(k) >> 32) mod world) */
int rl_route_owner(rl_router* r, size_t m, const uint64_t* key, uint32_t* owner, void* stream);

/* sender: request i for owner o is the j-th of the batch's requests for o
 * (batch order); j < cap: send[o * cap + j], slot[i] = o * cap + j; else
 * dropped, slot[i] = UINT32_MAX.  send_info[RL_ROUTE_INFO * o + k]: k = 0
 * requests sent to o (<= cap), 1 the batch's earliest ts, 2 its latest ts
 * (INT64_MAX / INT64_MIN if the batch is empty), 3 twice the requests for o
 * dropped, plus 1 when the batch's ts decrease somewhere (a source in time
 * order needs no running max of its arrival times at the owner).  Rows 1-2
 * cover the whole batch, dropped requests included: every owner must derive
 * the same store clock, and a dropped request's time is still a time the
 * shared store's clock (real time in the reference's single Redis) has
 * reached -- so a dropped request advances the store clock like a sent one
 * (tests/test_route_gpu.py::test_route_dropped_request_advances_store_clock). */
int rl_route_pack(rl_router* r, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                  const uint32_t* cfg, rl_route_rec* send, int64_t* send_info, uint32_t* slot, void* stream);

#define RL_SLOT_DROPPED 0xffffffffu   /* slot[i]: dropped, its owner's bucket was full */
#define RL_SLOT_SKIPPED 0xfffffffeu   /* slot[i]: not selected (rl_route_pack_sel) */

/* sender: rl_route_pack of the requests with sel[i] != 0 (a byte per request).
 * A request with sel[i] == 0 is not sent: it takes no bucket position, does not
 * count against cap, never raises the overflow status, and gets slot[i] =
 * RL_SLOT_SKIPPED.  The selected requests are grouped by owner, stable, exactly
 * as rl_route_pack groups a batch.  Info row 0 counts the selected requests
 * sent and row 3 the selected requests dropped; rows 1-2 and the unsorted bit
 * still cover the WHOLE batch, skipped requests included, by the argument
 * above for dropped ones: every owner must derive the same store clock, and the
 * sender's batch reached those times whether or not a request went out.  With
 * sel all ones, send, send_info and slot are byte-identical to rl_route_pack's
 * (the same kernels, a template predicate).  Real slots stay below 2^30
 * (rl_router_create), so the two codes never collide with one. */
int rl_route_pack_sel(rl_router* r, size_t m, const uint64_t* key, const int64_t* ts, const int64_t* n,
                      const uint32_t* cfg, const uint8_t* sel, rl_route_rec* send, int64_t* send_info,
                      uint32_t* slot, void* stream);

/* owner: recv[world * cap] (source s's bucket at s * cap) and recv_info (the
 * received info rows, source s's at RL_ROUTE_INFO * s) -> the decision order:
 * order[p] = receive index of the p-th request, server_ms[p] its store clock,
 * *count = requests received (p < *count are valid).  One source whose batch
 * is in time order (world 1, info flag clear) is its own decision order: the
 * merge then writes only order[0] = RL_ORDER_IDENTITY and server_ms[0] = the
 * store clock of the earlier steps, meaning order[p] = p and server_ms[p] =
 * max(server_ms[0], floor(recv[p].ts / 1e6)); rl_decide_routed_device reads
 * that form directly.  Call once per step, in step order (it advances the
 * store clock). */
int rl_route_merge(rl_router* r, const rl_route_rec* recv, const int64_t* recv_info, uint32_t* order,
                   int64_t* server_ms, uint32_t* count, void* stream);

/* owner: the engine on the merged requests -- request p is recv[order[p]]
 * with store clock server_ms[p], p < *count (device memory, at most m_max <=
 * the engine's max_batch); its result goes to res[order[p]].  The grouping
 * waits for `stream` (the merge); `stream` waits for the results.  m_max must
 * be at least world * rl_router_capacity (the most a merge can count): a
 * device count above m_max decides only the first m_max requests, and the
 * next rl_engine_sync returns RL_EOVERFLOW. */
int rl_decide_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                            const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* stream);
/* the same with the two sides on two streams: the grouping waits for
 * in_stream (the merge), out_stream waits for the results -- so in_stream
 * can go on with the next step's pack and merge while this one decides */
int rl_decide_routed_device_io(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                               const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                               void* out_stream);

/* the same with the results' completion recorded into done_event (a
 * hipEvent_t the caller owns) instead of a stream wait made at call time: a
 * pipeline that issues its result side later (after the next step's request
 * exchange) waits on the event then, so its result stream does not queue
 * behind this batch before the collectives issued in between */
int rl_decide_routed_device_ev(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                               const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                               void* done_event);

/* Peek and Reset steps.  A routed step is homogeneous: every rank runs it with
 * one kind -- decide, peek or reset.  A peek or reset step is packed,
 * exchanged and merged exactly as a decide step; the owner then calls one of
 * these instead of rl_decide_routed_device.  Request p is recv[order[p]] with
 * store clock server_ms[p], p < *count (or the RL_ORDER_IDENTITY form), and its
 * result is one rl_route_res at res[order[p]]:
 *   peek   the four Result fields rl_peek_batch gives for (key, ts, n, cfg,
 *          server_ms[p]): n == 0 is legal; n < 0, an unknown cfg and
 *          RL_KEY_RESERVED give {RL_INVALID, 0, 0, 0}; a window count whose
 *          INCRBY would overflow gives RL_ERROR with reset_at.  Nothing in the
 *          tables changes and rl_stats does not move.
 *   reset  the effect of rl_reset(cfg, key, ts) for every request, in any
 *          order (they commute); n is ignored.  {RL_RESET_DONE, 0, 0, 0}, or
 *          {RL_INVALID, 0, 0, 0} for an unknown cfg or RL_KEY_RESERVED.  A
 *          request dropped at its sender was not applied.
 * Order: the step sees the state left by every decide or reset step (and every
 * other engine call) issued before it on this engine and none issued after it:
 * one kernel on the engine's replay stream, as rl_peek_batch_device and
 * rl_reset_batch_device.
 * Store clock: a peek or reset step is a step of the shared store's timeline.
 * rl_route_merge advances the store clock from its info rows whatever the
 * owner runs afterwards, so the requests of a peek or reset step (dropped ones
 * included) move the clock of every later step like a decide step's.
 * The kernel waits for in_stream (NULL: the engine's stream), where the merge
 * ran.  With done_event (a hipEvent_t the caller owns) the results' completion
 * is recorded into it, as rl_decide_routed_device_ev (m_max == 0: recorded on
 * in_stream); without, out_stream (NULL: in_stream) waits for the results, as
 * rl_decide_routed_device_io.  m_max is bounded by `order` being 32-bit, not by
 * the engine's max_batch (no batch buffer is used); recv and res are 16-byte
 * aligned, as every device allocation is.  A device count above m_max runs
 * only the first m_max requests and the next rl_engine_sync returns
 * RL_EOVERFLOW -- the only sticky status these calls raise. */
int rl_peek_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                          const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                          void* out_stream, void* done_event);
int rl_reset_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                           const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                           void* out_stream, void* done_event);

/* Refund step: the routed form of rl_refund_batch (include/rl_engine.h).  A
 * refund step is homogeneous like the other kinds and is packed, exchanged,
 * merged and unpacked exactly as a decide step -- the router does not change
 * and the wire record carries no op code; the owner calls this instead of
 * rl_decide_routed_device.  Arguments, argument checks and the stream / event
 * behaviour are those of rl_peek_routed_device / rl_reset_routed_device.
 *   request p   recv[order[p]] at store clock server_ms[p] (or the
 *          RL_ORDER_IDENTITY form): a refund (key, ts, n, cfg, store clock) with
 *          the meaning of rl_refund_batch -- ts picks the window, the store
 *          clock decides whether the target is live.
 *   one call    the merged batch is ONE refund call: its valid requests are
 *          grouped by target across all source ranks, and each target with a
 *          live contributor gets one script run with N = the saturated sum of
 *          the contributors' n (bucket: min(capacity, tokens + N) through
 *          tostring, last_refill and the TTL untouched; window: DEL if count <=
 *          N, else DECRBY N).  Bucket refunds do not commute (%.14g), so the
 *          sum is the one answer that depends neither on the thread order nor
 *          on the merge order.
 *   result      one rl_route_res at res[order[p]]: {RL_REFUND_DONE, 0, 0, 0}
 *          when the request contributed, {RL_REFUND_NOKEY, 0, 0, 0} when it was
 *          valid but found no live target (nothing is stored for it),
 *          {RL_INVALID, 0, 0, 0} for n <= 0, an unknown cfg or RL_KEY_RESERVED.
 *          rl_stats, the tally, the top keys and the GC budgets do not move.
 *   bound       the kernels execute the first B = min(m_max, rl_refund_max(e))
 *          requests of the merged batch, as one call (the engine's refund
 *          scratch is sized for rl_refund_max).  m_max itself is limited only
 *          by the 32-bit `order`.  If *count > B, the requests B <= p <
 *          min(*count, m_max) get {RL_DROPPED, 0, 0, 0} -- not executed, to be
 *          resubmitted -- and the next rl_engine_sync returns RL_EOVERFLOW, the
 *          only sticky status the call raises.
 * Order: as a peek or reset step -- one chain op (two kernels) on the engine's
 * replay stream, after every engine call issued before it and before every
 * later one; the call parity of the refund scratch is shared with
 * rl_refund_batch_device.  Store clock: a refund step advances the router's
 * store clock like any step (rl_route_merge, before the engine runs); a request
 * dropped at its sender comes back RL_DROPPED and was not applied.  The first
 * refund of an engine, routed or not, allocates the scratch (m_max == 0
 * allocates nothing and records done_event on in_stream). */
int rl_refund_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                            const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                            void* out_stream, void* done_event);

/* Charge step: the routed form of rl_charge_batch (include/rl_engine.h,
 * DESIGN.md §10m, §10n) -- usage that is only known after the fact, recorded
 * on the key's owner GPU in order with the routed steps in flight.  A charge
 * step is homogeneous like the other kinds and is packed, exchanged, merged
 * and unpacked exactly as a decide step -- the router does not change and the
 * wire record carries no op code; the owner calls this instead of
 * rl_decide_routed_device.  Arguments, argument checks and the stream / event
 * behaviour are those of rl_refund_routed_device.
 *   request p   recv[order[p]] at store clock server_ms[p] (or the
 *          RL_ORDER_IDENTITY form): a charge (key, ts, n, cfg, store clock) with
 *          the meaning of rl_charge_batch.
 *   one call    the merged batch is ONE Charge call in merge order -- the three
 *          steps of rl_charge_batch with "array order" read as merge position p.
 *          Ask: every request is asked against the state left by every engine
 *          call issued before this step: n' = min(n, Peek(key, 0).remaining) for
 *          a token bucket, n' = n for a window, 0 for an invalid request.
 *          Decide: the unchanged routed decide runs on n' as one batch.  Result:
 *          the rule of rl_charge_batch.
 *          All ranks' charges of one bucket in a step are therefore duplicates
 *          of one call.  The verb is exact for a bucket that appears once in the
 *          merged batch and conservative otherwise: every duplicate was asked
 *          against the same state, so a later one can find less than its n',
 *          takes nothing and is RL_DENIED with charged 0 -- the caller charges
 *          again.  The bound of rl_charge_batch holds across ranks: at one time
 *          stamp, a bucket that refused any ask ends with fewer whole tokens
 *          than that ask, and never below zero.  Windows INCRBY before they
 *          compare, so every window charge is recorded in full.
 *   result      one rl_route_res at res[order[p]]: {decision, remaining,
 *          charged, reset_at_ns}.  `charged` travels in the record's retry_after
 *          field -- nothing is retried after a charge -- so rl_route_unpack
 *          delivers it into the caller's retry_after_ns array.  decision:
 *          RL_ALLOWED when charged == n; RL_DENIED when less was taken (a bucket)
 *          or the window is now over its limit (charged == n all the same);
 *          RL_ERROR / RL_INVALID as the decide's.  An empty bucket's row is
 *          {RL_DENIED, 0, 0, the ask's reset_at}.  `tokens` is not carried, as
 *          in every routed result.
 *   bound       the call executes the first B = min(m_max, rl_charge_max(e))
 *          requests of the merged batch, as one call (the scratch is sized for
 *          rl_charge_max).  m_max itself is limited only by the 32-bit `order`.
 *          If *count > B, the requests B <= p < min(*count, m_max) get
 *          {RL_DROPPED, 0, 0, 0} -- not executed, to be resubmitted -- and the
 *          next rl_engine_sync returns RL_EOVERFLOW, the only sticky status the
 *          call adds to the decide's own (a full table: RL_ENOMEM).
 *   counters    rl_stats moves as a routed decide of bound B moves it; the
 *          tally, the top keys and the GC budgets do not move.
 * Order: the ask is a chain op like a peek step's kernel, after every engine
 * call issued before the step; the decide is ordered as any routed decide; the
 * finish runs on the engine's finish stream behind the decide's.  `recv`,
 * `order`, `server_ms` and `count` are only read.  Store clock: a charge step
 * advances the router's store clock like any step; a request dropped at its
 * sender comes back RL_DROPPED and was not recorded.  The first routed charge
 * of an engine allocates its scratch before anything is enqueued (m_max == 0
 * allocates nothing and records done_event on in_stream). */
int rl_charge_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                            const uint32_t* order, const int64_t* server_ms, rl_route_res* res, void* in_stream,
                            void* out_stream, void* done_event);

/* Routed usage tally and top keys: the routed forms of rl_tally_batch_device
 * and rl_hot_batch_device (include/rl_engine.h),
 * counted on the key's OWNER GPU.  A key has one owner, so its counts are whole
 * there: the tally's "tracked completely or not at all" holds per key, hot_min
 * means what it means on one GPU, every owner's sketch holds only its share of
 * the keys, and the cluster's top-k is contained in the union of the ranks'
 * local top-k lists (shard.merge_tallies / merge_hots).
 *   request p   of a finished decide step: (key, cfg, n) of recv[order[p]] (or
 *          the RL_ORDER_IDENTITY form) and res[order[p]].decision, p <
 *          min(m_max, *count) -- the requests the engine gave results; ts, pos
 *          and the store clock are not used.  The counting rules are those of
 *          the array forms, the decision being an int64: with a registered cfg,
 *          a decision outside 0..3 (negative values included) adds one to
 *          bad_codes (tally) or skipped (top keys) and nothing else.
 *   drops       a request dropped at its sender never reaches the owner; with
 *          recv_info (the received info rows, nullable) the tally adds the sum
 *          over the `world` sources of recv_info[RL_ROUTE_INFO * s + 3] >> 1 to
 *          dropped_requests.  Only their number is known, not their units.
 *   streams     enqueued on `stream` (NULL: the engine's stream): one launch
 *          for the tally, two (the adds, then the pick) for the top keys.  The
 *          caller guarantees that the step's results are complete on `stream`
 *          and that recv / res stay unmodified until the stream has passed the
 *          call.  The calls use neither the replay stream nor the state tables,
 *          write only the feature's own memory and leave rl_stats and the sticky
 *          status alone -- except that a count above m_max re-raises
 *          RL_EOVERFLOW, which the decide of that step raised already.
 *   status      RL_EINVAL before rl_tally_enable / rl_hot_enable, for m_max
 *          above 32 bits, and for a null count, recv, order, server_ms or res
 *          with m_max > 0; m_max == 0 is RL_OK without a launch.
 *   reads       rl_tally_read / rl_hot_read return the routed and the array
 *          calls' counts together; rl_tally_info and rl_hot_info keep their
 *          meaning (batches / requests count array calls only; the sketch's
 *          total and skipped are device words, so routed calls move them).
 *          rl_tally_routed_read (synchronous) adds what is the routed form's
 *          own: steps = calls with m_max > 0 (kept on the host), requests =
 *          routed requests looked at, dropped_requests as above.  A clearing
 *          rl_tally_read zeroes all three.
 * Which steps to count is the caller's choice; shard.RoutedPipeline(observe=)
 * counts decide steps and the member decide step of a routed AllowAll, not its
 * give-backs, and no peek, reset, refund or charge step. */
int rl_tally_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                           const uint32_t* order, const int64_t* server_ms, const rl_route_res* res,
                           const int64_t* recv_info, uint32_t world, void* stream);
int rl_hot_routed_device(rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv,
                         const uint32_t* order, const int64_t* server_ms, const rl_route_res* res, void* stream);
typedef struct rl_tally_routed_info {
    uint32_t struct_size, pad_;
    uint64_t steps, requests, dropped_requests;
} rl_tally_routed_info;
int rl_tally_routed_read(rl_engine* e, rl_tally_routed_info* out);

/* Routed AllowAll: rl_allow_all_batch (include/rl_engine.h)
 * for members whose keys live on different GPUs.  It is two
 * routed steps, b and b + 1, with a settle on the sender between them and no
 * host read (shard.RoutedPipeline.allow_all):
 *   step b      a decide step of the M members, unchanged; its result side is
 *               issued at once and unpacked into the caller's arrays
 *   settle      rl_allow_all_settle_device on the unpacked decisions: verdict
 *               per member, give-back g per member, sel[i] = g[i] > 0
 *   step b + 1  a refund step of the selection: rl_route_pack_sel with n = g
 *               and the members' key, ts and cfg, then exchange, merge and
 *               rl_refund_routed_device, unchanged; unpacked into rollback
 * Effect on the shared store: a decide step of ALL ranks' members (merged by
 * arrival order) followed by ONE refund step of all ranks' give-backs (per
 * target the sum across ranks, rl_refund_routed_device).  The verb is
 * conservative across ranks as rl_allow_all_batch is within a call: a group
 * can be denied on another rank's transient take, and is never admitted on
 * quota a sequential run would not have.
 * Clock: the give-backs run at the refund step's store clock, which is at
 * least the latest ts of the decide step on any rank (rl_allow_all_batch runs
 * them at the member's own clock): a short window can have expired by then, so
 * RL_REFUND_NOKEY is more common here.
 * rollback[i]: RL_REFUND_DONE; RL_REFUND_NOKEY; RL_INVALID -- nothing was asked
 * back, the member was skipped; RL_DROPPED -- the owner's refund bound
 * (rl_refund_routed_device) was passed: the take is still in place and the
 * caller re-issues it as a refund step.  The sender cannot drop a give-back: a
 * selected member held a bucket position in step b (a member dropped there has
 * g = 0), and the selected members are a subsequence of step b's, so each has
 * at most the position it had.
 * rl_stats moves as for the decide step; the tally and the top keys do not.
 *
 * rl_allow_all_settle_device: one kernel on `stream`; it uses none of the
 * engine's streams, scratch or tables and reads only the engine's device
 * config table (for the algorithm).  Groups as rl_allow_all_batch: member i
 * starts a group when i == 0 or first[i] != 0; a run longer than
 * RL_ALLOW_ALL_MAX_GROUP is RL_INVALID.  decision[] holds the unpacked results
 * of a routed decide step, so a member may be RL_DROPPED.  verdict[i], on every
 * member of a group, is the most severe decision of the group, RL_INVALID >
 * RL_DROPPED > RL_ERROR > RL_DENIED > RL_ALLOWED (a byte of 5 or more counts as
 * RL_INVALID).  RL_DROPPED tells the caller to resubmit the whole group; it
 * ranks below RL_INVALID because an invalid group can never pass.  g[i] = n[i]
 * if the verdict is not RL_ALLOWED and the member took something (a bucket
 * when it allowed, a window counter when it allowed or denied), else 0 -- a
 * dropped member took nothing, like an error or invalid one.  sel[i] = g[i] >
 * 0.  All arrays are device memory of m elements; m is at most the engine's
 * max_batch; RL_EINVAL for a null pointer (m > 0) or a larger m. */
int rl_allow_all_settle_device(rl_engine* e, size_t m, const uint8_t* first, const uint32_t* cfg_id,
                               const int64_t* n, const uint8_t* decision, uint8_t* verdict, int64_t* g,
                               uint8_t* sel, void* stream);

/* sender: back[world * cap] (the result buckets, send layout) -> the caller's
 * order; a dropped request gets decision RL_DROPPED and zeros; a request that
 * rl_route_pack_sel skipped gets {RL_INVALID, 0, 0, 0}: nothing was asked */
int rl_route_unpack(rl_router* r, size_t m, const uint32_t* slot, const rl_route_res* back, uint8_t* decision,
                    int64_t* remaining, int64_t* retry_after_ns, int64_t* reset_at_ns, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RL_ROUTE_H */
