// rl_snapshot.h -- export / import of the HBM state tables (include/rl_snapshot.h
// documents the blob; DESIGN.md "Snapshots" the design).
//
// Export: one compacting pass over the three tables.  Every wave takes a
// 64-bit ballot of its exporting lanes, its first such lane reserves the
// wave's records with one atomicAdd per section, and each lane writes its
// record at the reserved base + its rank in the mask: one atomic per wave and
// section instead of one per key (k_table_keys' key_emit), and the records of
// a wave land next to each other.  Records leave as 16-byte vector stores.
// Import: the dense sections are re-inserted into the fresh tables of a table
// rebuild (rl_table_gc's), as k_rehash / k_spill_rehash re-insert an old table.
#pragma once

#include <cstring>

#include "../../include/rl_snapshot.h"
#include "rl_table.h"

namespace rl {

// the 128-byte header (little-endian, as the device and every supported host)
struct SnapHeader {
    char magic[8];
    uint32_t version, header_size;
    int32_t profile;
    uint32_t tb_size, win_size, spill_size;
    uint64_t tb_count, win_count, spill_count;
    uint64_t tb_off, win_off, spill_off, total;
    int64_t now_ms;
    uint32_t world, rank;
    uint64_t payload_sum, header_sum, reserved;
};
static_assert(sizeof(SnapHeader) == RL_SNAPSHOT_HEADER_SIZE, "snapshot header must be 128 bytes");

// more records than any table can hold (capacities stay below 2^32 slots):
// keeps the offset arithmetic of a forged header from wrapping
constexpr uint64_t SNAP_MAX_COUNT = 1ull << 40;

// section offsets and the total size from the three counts
inline bool snap_layout(SnapHeader& h) {
    if (h.tb_count > SNAP_MAX_COUNT || h.win_count > SNAP_MAX_COUNT || h.spill_count > SNAP_MAX_COUNT) return false;
    h.tb_off = RL_SNAPSHOT_HEADER_SIZE;
    h.win_off = (h.tb_off + sizeof(TbEntry) * h.tb_count + 63) & ~63ull;
    h.spill_off = h.win_off + sizeof(WinEntry) * h.win_count;
    h.total = h.spill_off + sizeof(SpillEntry) * h.spill_count;
    return true;
}

// a record's hash: its 8-byte words folded from the section's tag
template <int W>
RL_HD inline uint64_t snap_fold(const uint64_t (&w)[W], uint64_t tag) {
    uint64_t h = tag;
    for (int j = 0; j < W; j++) h = mix64(h ^ w[j]);
    return h;
}
template <typename E>
RL_HD inline uint64_t snap_hash(const E& x, uint64_t tag) {
    uint64_t w[sizeof(E) / 8];
    __builtin_memcpy(w, &x, sizeof(E));
    return snap_fold(w, tag);
}

inline uint64_t snap_header_sum(const SnapHeader& h) {
    SnapHeader t = h;
    t.header_sum = 0;
    return snap_hash(t, RL_SNAPSHOT_TAG_HEADER);
}

inline SnapHeader snap_make_header(int32_t profile, uint64_t ntb, uint64_t nwin, uint64_t nsp, int64_t now_ms,
                                   uint32_t world, uint32_t rank, uint64_t payload_sum) {
    SnapHeader h{};
    memcpy(h.magic, RL_SNAPSHOT_MAGIC, 8);
    h.version = RL_SNAPSHOT_VERSION;
    h.header_size = RL_SNAPSHOT_HEADER_SIZE;
    h.profile = profile;
    h.tb_size = sizeof(TbEntry);
    h.win_size = sizeof(WinEntry);
    h.spill_size = sizeof(SpillEntry);
    h.tb_count = ntb;
    h.win_count = nwin;
    h.spill_count = nsp;
    (void)snap_layout(h);
    h.now_ms = now_ms;
    h.world = world;
    h.rank = rank;
    h.payload_sum = payload_sum;
    h.header_sum = snap_header_sum(h);
    return h;
}

// everything but the payload checksum: magic, version, sizes, the partition
// filter, counts and offsets against len, the header's own checksum
inline bool snap_header_ok(const void* buf, size_t len, SnapHeader* out) {
    if (!buf || len < sizeof(SnapHeader)) return false;
    SnapHeader h;
    memcpy(&h, buf, sizeof h);
    if (memcmp(h.magic, RL_SNAPSHOT_MAGIC, 8) != 0 || h.version != RL_SNAPSHOT_VERSION ||
        h.header_size != RL_SNAPSHOT_HEADER_SIZE)
        return false;
    if (h.header_sum != snap_header_sum(h) || h.reserved != 0) return false;
    if (h.profile != PROFILE_REDIS7 && h.profile != PROFILE_MINIREDIS) return false;
    if (h.tb_size != sizeof(TbEntry) || h.win_size != sizeof(WinEntry) || h.spill_size != sizeof(SpillEntry))
        return false;
    if (h.world == 0 || h.rank >= h.world) return false;
    SnapHeader want = h;
    if (!snap_layout(want)) return false;
    if (h.tb_off != want.tb_off || h.win_off != want.win_off || h.spill_off != want.spill_off ||
        h.total != want.total || h.total != len)
        return false;
    *out = h;
    return true;
}

// the payload checksum on the host (rl_snapshot_inspect); also requires the
// padding between the sections to be zero
inline bool snap_payload_ok(const void* buf, const SnapHeader& h) {
    const uint8_t* p = (const uint8_t*)buf;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < h.tb_count; i++) {
        TbEntry x;
        memcpy(&x, p + h.tb_off + i * sizeof x, sizeof x);
        sum += snap_hash(x, RL_SNAPSHOT_TAG_TB);
    }
    for (uint64_t i = 0; i < h.win_count; i++) {
        WinEntry x;
        memcpy(&x, p + h.win_off + i * sizeof x, sizeof x);
        sum += snap_hash(x, RL_SNAPSHOT_TAG_WIN);
    }
    for (uint64_t i = 0; i < h.spill_count; i++) {
        SpillEntry x;
        memcpy(&x, p + h.spill_off + i * sizeof x, sizeof x);
        sum += snap_hash(x, RL_SNAPSHOT_TAG_SPILL);
    }
    for (uint64_t o = h.tb_off + sizeof(TbEntry) * h.tb_count; o < h.win_off; o++)
        if (p[o]) return false;
    return sum == h.payload_sum;
}

constexpr int SNAP_BLOCK = 256;
constexpr int SNAP_WAVES = SNAP_BLOCK / 64;

// counter block of k_snapshot_export: records per section, payload checksum
enum : int { SNAP_TB = 0, SNAP_WIN = 1, SNAP_SPILL = 2, SNAP_SUM = 3, SNAP_WORDS = 4 };
// counters of one imported section: records live at now_ms, records that found
// no slot, keys that were already present, the section's checksum
enum : int { SNAP_LIVE = 0, SNAP_LOST = 1, SNAP_CONFLICT = 2, SNAP_CHECK = 3 };

// dst[k] += the block's sum of v[k], one atomic per block and word (called by
// every thread of the block)
template <int K>
__device__ inline void snap_block_add(const unsigned long long (&v)[K], unsigned long long* dst) {
    __shared__ unsigned long long part[K][SNAP_WAVES];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < K; k++) {
        unsigned long long x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
        if (lane == 0) part[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        unsigned long long x = 0;
        for (int w = 0; w < SNAP_WAVES; w++) x += part[threadIdx.x][w];
        if (x) atomicAdd(&dst[threadIdx.x], x);
    }
}

// what a snapshot carries, and the record as it is written
__device__ inline bool snap_take(const TbEntry& x, int64_t now_ms, int32_t profile) {
    return entry_live(x, now_ms, profile);
}
__device__ inline bool snap_take(const WinEntry& x, int64_t now_ms, int32_t profile) {
    // also while its user key has spill entries (the import sorts out which are live)
    return x.key != EMPTY_KEY && (x.nspill > 0 || entry_live(x, now_ms, profile));
}
__device__ inline bool snap_take(const SpillEntry& x, int64_t now_ms, int32_t profile) {
    return entry_live(x, now_ms, profile);
}
__device__ inline TbEntry snap_record(const TbEntry& x) { return x; }
__device__ inline WinEntry snap_record(const WinEntry& x) {
    WinEntry y = x;
    y.nspill = 0;   // recounted from the imported spill records
    return y;
}
__device__ inline SpillEntry snap_record(const SpillEntry& x) { return x; }

template <typename E>
__device__ inline void snap_store(E* dst, const E& x) {
    static_assert(sizeof(E) % 16 == 0 && alignof(E) >= 16, "records are stored as 16-byte vectors");
    ulonglong2 v[sizeof(E) / 16];
    __builtin_memcpy(v, &x, sizeof(E));
    for (size_t j = 0; j < sizeof(E) / 16; j++) reinterpret_cast<ulonglong2*>(dst)[j] = v[j];
}

// one table's pass of k_snapshot_export.  The loop's trip count is the same
// for every lane of a wave (lanes past n carry take = false), so the ballot and
// the shuffle see the whole wave.  WRITE false: count and checksum only; no
// record needs a position then, so the count stays in the thread (`cnt`) and
// the block adds it once at the end, as k_table_count does.
template <bool WRITE, typename E>
__device__ inline void snap_export_section(const E* __restrict__ t, uint64_t n, E* out, uint64_t cap,
                                           unsigned long long* count, uint64_t tag, int64_t now_ms,
                                           int32_t profile, uint32_t world, uint32_t rank,
                                           unsigned long long& cnt, unsigned long long& sum) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t base = blockIdx.x * (uint64_t)blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {
        const uint64_t i = base + lane;
        E x{};
        bool take = false;
        if (i < n) {
            x = t[i];
            take = snap_take(x, now_ms, profile) && (world == 1 || (uint32_t)((mix64(x.key) >> 32) % world) == rank);
        }
        if constexpr (!WRITE) {
            if (take) {
                cnt++;
                sum += snap_hash(snap_record(x), tag);
            }
            continue;
        }
        const unsigned long long m = __ballot(take);
        if (m == 0) continue;
        const uint32_t leader = (uint32_t)__ffsll(m) - 1;
        unsigned long long first = 0;
        if (lane == leader) first = atomicAdd(count, (unsigned long long)__popcll(m));
        first = __shfl(first, (int)leader, 64);
        if (!take) continue;
        const E y = snap_record(x);
        sum += snap_hash(y, tag);
        const uint64_t pos = first + (uint64_t)__popcll(m & ((1ull << lane) - 1));
        if (WRITE && pos < cap) snap_store(&out[pos], y);
    }
}

// rl_snapshot_export: the three tables in one launch.  The out_* sections
// hold cap_* records (the counts of a first, counting launch -- WRITE false --
// on the drained engine); a record past its section's capacity is counted and
// not written.
template <bool WRITE>
__global__ __launch_bounds__(SNAP_BLOCK) void k_snapshot_export(
    const TbEntry* __restrict__ tb, uint64_t ntb, const WinEntry* __restrict__ win, uint64_t nwin,
    const SpillEntry* __restrict__ sp, uint64_t nsp, int64_t now_ms, int32_t profile, uint32_t world, uint32_t rank,
    TbEntry* out_tb, uint64_t cap_tb, WinEntry* out_win, uint64_t cap_win, SpillEntry* out_sp, uint64_t cap_sp,
    unsigned long long* counters) {
    unsigned long long c[SNAP_WORDS] = {0, 0, 0, 0};
    snap_export_section<WRITE>(tb, ntb, out_tb, cap_tb, &counters[SNAP_TB], RL_SNAPSHOT_TAG_TB, now_ms, profile,
                               world, rank, c[SNAP_TB], c[SNAP_SUM]);
    snap_export_section<WRITE>(win, nwin, out_win, cap_win, &counters[SNAP_WIN], RL_SNAPSHOT_TAG_WIN, now_ms,
                               profile, world, rank, c[SNAP_WIN], c[SNAP_SUM]);
    snap_export_section<WRITE>(sp, nsp, out_sp, cap_sp, &counters[SNAP_SPILL], RL_SNAPSHOT_TAG_SPILL, now_ms,
                               profile, world, rank, c[SNAP_SPILL], c[SNAP_SUM]);
    // WRITE: the waves already added the counts, c[SNAP_TB..SNAP_SPILL] are 0
    snap_block_add(c, counters);
}

// rl_snapshot_import, token-bucket and window sections: k_rehash reading the
// blob's dense records.  The fresh table already holds the engine's own live
// entries, so a key this call did not insert is on both sides: a conflict.
template <typename E>
__global__ __launch_bounds__(SNAP_BLOCK) void k_snapshot_import(const E* __restrict__ rec, uint64_t n, E* nu,
                                                                uint64_t mask_new, int64_t now_ms, int32_t profile,
                                                                uint64_t tag, unsigned long long* counters) {
    unsigned long long c[4] = {0, 0, 0, 0};
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const E x = rec[i];
        c[SNAP_CHECK] += snap_hash(x, tag);
        const E y = snap_record(x);
        if (!entry_live(y, now_ms, profile)) continue;
        c[SNAP_LIVE]++;
        const uint64_t h = mix64(y.key) & mask_new;
        bool ins = false;
        const uint32_t s = probe_insert_at(nu, mask_new, y.key, h, nu[h].key, &ins);
        if (s == NO_SLOT) { c[SNAP_LOST]++; continue; }
        if (!ins) { c[SNAP_CONFLICT]++; continue; }
        gc_copy(nu[s], y);
    }
    snap_block_add(c, counters);
}

// ... spill section, after the window section: k_spill_rehash reading the
// blob's records.  A user key whose window record was expired (and skipped)
// gets an empty window entry here, so its live spill records keep their owner.
__global__ __launch_bounds__(SNAP_BLOCK) void k_snapshot_import_spill(const SpillEntry* __restrict__ rec, uint64_t n,
                                                                      SpillEntry* nu, uint64_t mask_new, WinEntry* win,
                                                                      uint64_t win_mask, int64_t now_ms,
                                                                      int32_t profile, unsigned long long* counters) {
    unsigned long long c[4] = {0, 0, 0, 0};
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const SpillEntry x = rec[i];
        c[SNAP_CHECK] += snap_hash(x, RL_SNAPSHOT_TAG_SPILL);
        if (!entry_live(x, now_ms, profile)) continue;
        c[SNAP_LIVE]++;
        const uint64_t hw = mix64(x.key) & win_mask;
        const uint32_t w = probe_insert_at(win, win_mask, x.key, hw, win[hw].key);
        uint64_t h = spill_home(x.key, mask_new);
        bool placed = false;
        for (uint64_t p = 0; w != NO_SLOT && p <= mask_new && p < MAX_PROBES; p++) {
            if (atomicCAS((unsigned long long*)&nu[h].key, (unsigned long long)EMPTY_KEY,
                          (unsigned long long)x.key) == EMPTY_KEY) {
                nu[h].ws = x.ws;
                nu[h].cnt = x.cnt;
                nu[h].when = x.when;
                atomicAdd((unsigned long long*)&win[w].nspill, 1ull);
                placed = true;
                break;
            }
            h = (h + 1) & mask_new;
        }
        if (!placed) c[SNAP_LOST]++;
    }
    snap_block_add(c, counters);
}

}  // namespace rl
