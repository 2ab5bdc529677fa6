/*
 * rl_snapshot.h -- export, inspect and import the engine's HBM state tables.
 *
 * The engine's tables are the Redis keyspace of the limiter (include/rl_engine.h):
 * a snapshot is what an RDB file or DUMP / RESTORE is to Redis.  It carries
 * every key live at a server clock, optionally only the keys one rank of a
 * `world`-way partition owns (owner(k) = (mix64(k) >> 32) mod world, the
 * routing rule of include/rl_route.h), so that state survives a restart, a
 * move to another card and a change of the world size ("Snapshots").
 *
 * Format (version 1): one little-endian blob.
 *
 *   offset size  field
 *        0    8  magic "RLSNAP01"
 *        8    4  version (1)
 *       12    4  header_size (128)
 *       16    4  profile (RL_PROFILE_*: expiry is judged by the exporter's profile)
 *       20    4  tb_entry_size (32)
 *       24    4  win_entry_size (64)
 *       28    4  spill_entry_size (32)
 *       32    8  tb_count
 *       40    8  win_count
 *       48    8  spill_count
 *       56    8  tb_offset     = 128
 *       64    8  win_offset    = round_up(tb_offset + 32 * tb_count, 64)
 *       72    8  spill_offset  = win_offset + 64 * win_count
 *       80    8  total_bytes   = spill_offset + 32 * spill_count
 *       88    8  now_ms        (int64: the server clock of the export)
 *       96    4  world         (partition filter; 1 = every key)
 *      100    4  rank
 *      104    8  payload_checksum
 *      112    8  header_checksum
 *      120    8  reserved (0)
 *
 * then three dense sections, each at its 64-byte-aligned offset, records in
 * any order, padding bytes zero:
 *
 *   token-bucket records, 32 B: u64 key, f64 tokens, f64 last_refill, i64 when
 *   window records, 64 B:       u64 key, i64 nspill (always 0: recounted on
 *                               import), 2 x { i64 window_start, i64 count, i64 when }
 *   spill records, 32 B:        u64 user key, i64 window_start, i64 count, i64 when
 *
 * `when` is the key's expiry in server ms (INT64_MIN: the key does not exist,
 * INT64_MAX: no TTL); window_start is Unix seconds.
 *
 * Checksums.  mix64 is the splitmix64 finalizer of the tables' hash:
 *   x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31.
 * A record's hash folds its 8-byte words w_0.. in order, h = mix64(h ^ w_j),
 * starting from its section's tag (RL_SNAPSHOT_TAG_*); payload_checksum is the
 * sum of all record hashes mod 2^64, so it does not depend on the order the
 * export kernel emitted the records in.  header_checksum folds the header's
 * sixteen words the same way from RL_SNAPSHOT_TAG_HEADER, with the
 * header_checksum word itself taken as 0.
 *
 * Not built: incremental / delta snapshots, a device-pointer variant, removal
 * of the exported keys from the source, a gRPC admin RPC, an rll_* mirror.
 */
#ifndef RL_SNAPSHOT_H
#define RL_SNAPSHOT_H

#include "rl_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RL_SNAPSHOT_MAGIC       "RLSNAP01"
#define RL_SNAPSHOT_VERSION     1u
#define RL_SNAPSHOT_HEADER_SIZE 128u
#define RL_SNAPSHOT_TAG_TB      0x524c534e41505442ull   /* per-section start values of a record's hash */
#define RL_SNAPSHOT_TAG_WIN     0x524c534e4150574eull
#define RL_SNAPSHOT_TAG_SPILL   0x524c534e41505350ull
#define RL_SNAPSHOT_TAG_HEADER  0x524c534e41504844ull

typedef struct rl_snapshot_info {
    uint32_t struct_size, version;   /* sizeof(rl_snapshot_info); format version */
    int32_t profile;
    uint32_t world, rank, pad_;
    int64_t now_ms;
    uint64_t tb_keys, win_keys, spill_keys;   /* records per section */
    uint64_t bytes, checksum;                 /* total_bytes, payload_checksum */
} rl_snapshot_info;

/* Export every key live at server clock now_ms that rank `rank` of `world`
 * owns (world == 1: every key) into the host buffer `buf` of `cap` bytes.
 * A window entry is exported while it is live or its user key owns spill
 * entries (what rl_table_gc keeps); spill entries travel with their user key.
 * Synchronous; waits for queued batches; the engine is unchanged.
 *   buf == NULL && cap == 0   size query: RL_OK, out->bytes and the counts set
 *   cap < out->bytes          RL_ENOMEM, out->bytes set, nothing written
 *   world == 0, rank >= world RL_EINVAL
 * RL_ENOMEM also when the device staging buffer (the live bytes) cannot be
 * allocated. */
int rl_snapshot_export(rl_engine* e, int64_t now_ms, uint32_t world, uint32_t rank,
                       void* buf, size_t cap, rl_snapshot_info* out);

/* Validate a blob on the host (no GPU is touched): magic, version, sizes,
 * counts and offsets against `len` (which must equal total_bytes), the header
 * checksum and the payload checksum.  RL_EINVAL on any mismatch. */
int rl_snapshot_inspect(const void* buf, size_t len, rl_snapshot_info* out);

/* rl_table_gc at now_ms plus a merge of the blob's records, in one rebuild:
 * fresh tables of the requested capacities (0 = keep; rounding and limits as
 * rl_table_gc) receive the engine's own live state, then the blob's records
 * that are live at now_ms, and replace the old tables.  The blob may come from
 * an engine of any capacity and any partition filter.  On any failure the old
 * tables stay and later decisions are unchanged:
 *   RL_EINVAL  bad header, profile different from the engine's, or the payload
 *              checksum computed on the device differs from the header's
 *   RL_EEXIST  a token-bucket key or a window user key is in the engine and in
 *              the blob
 *   RL_ENOMEM  the live keys do not fit the capacities (or allocation failed)
 * The contract on now_ms is rl_table_gc's: exact provided no later request
 * carries a server clock below now_ms.  `out` (nullable): the tables afterwards. */
int rl_snapshot_import(rl_engine* e, const void* buf, size_t len, int64_t now_ms,
                       uint64_t tb_capacity, uint64_t win_capacity, rl_table_info* out);

#ifdef __cplusplus
}
#endif
#endif
