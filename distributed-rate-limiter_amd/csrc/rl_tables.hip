// rl_tables.hip -- maintenance of the HBM state tables: initialisation, counts
// (rl_table_info_get), key listing (rl_table_keys), GC / resize (rl_table_gc)
// and snapshots (include/rl_snapshot.h).  Every entry point here drains the
// engine first and runs on its stream.  A code object of its own: that of the
// decision kernels (rl_engine.hip) does not change with it.
#include <hip/hip_runtime.h>

#include "../../include/rl_engine.h"
#include "../../include/rl_snapshot.h"
#include "rl_engine_impl.h"
#include "rl_snapshot.h"
#include "rl_table.h"

using namespace rl;

__global__ void k_init_tb(TbEntry* t, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        t[i].key = EMPTY_KEY;
        t[i].tok = 0.0;
        t[i].last = 0.0;
        t[i].when = ABSENT;
    }
}

__global__ void k_init_win(WinEntry* t, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        t[i].key = EMPTY_KEY;
        t[i].nspill = 0;
        for (int k = 0; k < 2; k++) { t[i].s[k].ws = 0; t[i].s[k].cnt = 0; t[i].s[k].when = ABSENT; }
    }
}

__global__ void k_init_spill(SpillEntry* t, uint64_t n) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        t[i] = SpillEntry{EMPTY_KEY, 0, 0, ABSENT};
}

// Table GC of the spill table, after the window table's k_rehash: every live
// spill entry moves to the fresh spill table (strict CAS: two entries of one
// user key may be moved at once) and is counted in its user key's new window
// entry, which is inserted here (empty) if k_rehash dropped the old one as
// expired.  counters as k_rehash.
__global__ void k_spill_rehash(const SpillEntry* __restrict__ old, uint64_t n_old, SpillEntry* nu, uint64_t mask_new,
                               WinEntry* win, uint64_t win_mask, int64_t now_ms, int32_t profile,
                               unsigned long long* counters) {
    unsigned long long live = 0, lost = 0;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n_old;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const SpillEntry x = old[i];
        if (!entry_live(x, now_ms, profile)) continue;
        live++;
        const uint32_t w = probe_insert(win, win_mask, x.key);
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
        if (!placed) lost++;
    }
    if (live) atomicAdd(&counters[0], live);
    if (lost) atomicAdd(&counters[1], lost);
}

// Redis KEYS (rl_table_keys): every live key of the three tables
__device__ inline void key_emit(rl_key_rec* out, uint64_t cap, unsigned long long* cnt, uint64_t k, int64_t ws,
                                uint32_t kind) {
    const unsigned long long i = atomicAdd(cnt, 1ull);
    if (i < cap) out[i] = rl_key_rec{k, ws, kind, 0};
}
__global__ void k_table_keys(const TbEntry* tb, uint64_t ntb, const WinEntry* win, uint64_t nwin,
                             const SpillEntry* sp, uint64_t nsp, int64_t now_ms, int32_t profile, rl_key_rec* out,
                             uint64_t cap, unsigned long long* cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < ntb + nwin + nsp; i += stride) {
        if (i < ntb) {
            if (entry_live(tb[i], now_ms, profile)) key_emit(out, cap, cnt, tb[i].key, 0, RL_KIND_HASH);
        } else if (i < ntb + nwin) {
            const WinEntry& x = win[i - ntb];
            if (x.key == EMPTY_KEY) continue;
            for (int k = 0; k < 2; k++)
                if (x.s[k].when != ABSENT && key_alive(x.s[k].when, now_ms, profile))
                    key_emit(out, cap, cnt, x.key, x.s[k].ws, RL_KIND_WINDOW);
        } else {
            const SpillEntry& x = sp[i - ntb - nwin];
            if (entry_live(x, now_ms, profile)) key_emit(out, cap, cnt, x.key, x.ws, RL_KIND_WINDOW);
        }
    }
}

void rl::tables_init(TbEntry* tb, uint64_t tb_cap, WinEntry* win, uint64_t win_cap, SpillEntry* sp,
                     uint64_t spill_cap, hipStream_t s) {
    k_init_tb<<<2048, 256, 0, s>>>(tb, tb_cap);
    k_init_win<<<2048, 256, 0, s>>>(win, win_cap);
    k_init_spill<<<2048, 256, 0, s>>>(sp, spill_cap);
}

// the table count and GC kernels, on empty ranges: a server's first periodic
// count must not wait for their lazy load
int rl::tables_warm_up(rl_engine* e) {
    hipStream_t s = e->stream;
    k_table_count<<<1, 256, 0, s>>>(e->d_tb, 0, 0, e->profile, e->d_count);
    k_table_count<<<1, 256, 0, s>>>(e->d_win, 0, 0, e->profile, e->d_count);
    k_table_count<<<1, 256, 0, s>>>(e->d_spill, 0, 0, e->profile, e->d_count);
    k_rehash<<<1, 256, 0, s>>>(e->d_tb, 0, e->d_tb, e->tb_cap - 1, 0, e->profile, e->d_count);
    k_rehash<<<1, 256, 0, s>>>(e->d_win, 0, e->d_win, e->win_cap - 1, 0, e->profile, e->d_count);
    k_spill_rehash<<<1, 256, 0, s>>>(e->d_spill, 0, e->d_spill, e->spill_cap - 1, e->d_win, e->win_cap - 1, 0,
                                     e->profile, e->d_count);
    HIPCHK(e, hipGetLastError());
    return RL_OK;
}

extern "C" int rl_table_info_get(rl_engine* e, int64_t now_ms, rl_table_info* out) {
    if (!e || !out || out->struct_size < 8) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    int r = drain(e);
    if (r != RL_OK) return r;
    // preallocated counters (no hipMalloc / hipFree, which synchronize the
    // device, on a server's periodic count)
    unsigned long long* d = e->d_count;
    unsigned long long* h = e->h_count;
    hipStream_t s = e->stream;
    bool ok = hipMemsetAsync(d, 0, 6 * sizeof(unsigned long long), s) == hipSuccess;
    k_table_count<<<1024, 256, 0, s>>>(e->d_tb, e->tb_cap, now_ms, e->profile, d);
    k_table_count<<<1024, 256, 0, s>>>(e->d_win, e->win_cap, now_ms, e->profile, d + 2);
    k_table_count<<<1024, 256, 0, s>>>(e->d_spill, e->spill_cap, now_ms, e->profile, d + 4);
    ok = ok && hipMemcpyAsync(h, d, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return fail(e, RL_EDEVICE, "table count failed");
    return copy_out(out, rl_table_info{sizeof(rl_table_info), 0, e->tb_cap, h[0], h[1], e->win_cap, h[2], h[3],
                                       e->spill_cap, h[4], h[5]});
}

extern "C" int rl_table_keys(rl_engine* e, int64_t now_ms, rl_key_rec* out, size_t cap, uint64_t* count) {
    if (!e || !count || (cap && !out)) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    int r = drain(e);
    if (r != RL_OK) return r;
    unsigned long long* d = nullptr;
    rl_key_rec* dout = nullptr;
    HIPCHK(e, hipMalloc(&d, sizeof(unsigned long long)));
    if (cap && hipMalloc(&dout, sizeof(rl_key_rec) * cap) != hipSuccess) {
        (void)hipFree(d);
        return fail(e, RL_ENOMEM, "table keys: allocation failed");
    }
    hipStream_t s = e->stream;
    unsigned long long n = 0;
    bool ok = hipMemsetAsync(d, 0, sizeof n, s) == hipSuccess;
    k_table_keys<<<1024, 256, 0, s>>>(e->d_tb, e->tb_cap, e->d_win, e->win_cap, e->d_spill, e->spill_cap, now_ms,
                                       e->profile, dout, cap, d);
    ok = ok && hipMemcpyAsync(&n, d, sizeof n, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (ok && cap && n)
        ok = hipMemcpy(out, dout, sizeof(rl_key_rec) * std::min<uint64_t>(n, cap), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    (void)hipFree(dout);
    if (!ok) return fail(e, RL_EDEVICE, "table keys failed");
    *count = n;
    return RL_OK;
}

// A table rebuild: fresh tables that receive the live state and then replace
// the engine's.  rl_table_gc and rl_snapshot_import share every step, so what
// follows the capacities (slot ids, sort bits) cannot drift between them.
struct Rebuild {
    TbEntry* tb = nullptr;
    WinEntry* win = nullptr;
    SpillEntry* sp = nullptr;
    uint64_t tb_cap = 0, win_cap = 0, spill_cap = 0;
    // [0..5] the engine's own tables (live, lost per table); from REBUILD_IMPORT
    // on, four words per imported section (rl_snapshot.h SNAP_LIVE..)
    unsigned long long* d = nullptr;
};
constexpr int REBUILD_IMPORT = 6;
constexpr int REBUILD_WORDS = REBUILD_IMPORT + 3 * 4;

static void rebuild_abort(Rebuild& R) {
    (void)hipFree(R.tb);
    (void)hipFree(R.win);
    (void)hipFree(R.sp);
    (void)hipFree(R.d);
    R = Rebuild{};
}

// capacities (0 = keep; rounding and limits), drain, allocate and initialise
// the fresh tables, and enqueue the rehash of the engine's live state at
// now_ms on the engine's stream (not waited for)
static int rebuild_begin(rl_engine* e, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity, Rebuild& R,
                         const char* what) {
    R.tb_cap = tb_capacity ? pow2_at_least(std::max<uint64_t>(tb_capacity, 1024)) : e->tb_cap;
    R.win_cap = win_capacity ? pow2_at_least(std::max<uint64_t>(win_capacity, 1024)) : e->win_cap;
    R.spill_cap = e->spill_follows ? pow2_at_least(std::max<uint64_t>(2 * R.win_cap, 1024)) : e->spill_cap;
    if (!caps_fit(R.tb_cap, R.win_cap)) return fail(e, RL_EINVAL, "table capacities too large");
    int r = drain(e);
    if (r != RL_OK) return r;
    bool ok = hipMalloc(&R.tb, sizeof(TbEntry) * R.tb_cap) == hipSuccess;
    ok = ok && hipMalloc(&R.win, sizeof(WinEntry) * R.win_cap) == hipSuccess;
    ok = ok && hipMalloc(&R.sp, sizeof(SpillEntry) * R.spill_cap) == hipSuccess;
    ok = ok && hipMalloc(&R.d, REBUILD_WORDS * sizeof(unsigned long long)) == hipSuccess;
    if (!ok) {
        rebuild_abort(R);
        return fail(e, RL_ENOMEM, std::string(what) + ": allocation failed");
    }
    hipStream_t s = e->stream;
    tables_init(R.tb, R.tb_cap, R.win, R.win_cap, R.sp, R.spill_cap, s);
    if (hipMemsetAsync(R.d, 0, REBUILD_WORDS * sizeof(unsigned long long), s) != hipSuccess) {
        (void)hipStreamSynchronize(s);
        rebuild_abort(R);
        return fail(e, RL_EDEVICE, std::string(what) + " failed");
    }
    k_rehash<<<2048, 256, 0, s>>>(e->d_tb, e->tb_cap, R.tb, R.tb_cap - 1, now_ms, e->profile, R.d);
    k_rehash<<<2048, 256, 0, s>>>(e->d_win, e->win_cap, R.win, R.win_cap - 1, now_ms, e->profile, R.d + 2);
    // after the window entries: each live spill entry is counted in its new entry
    k_spill_rehash<<<2048, 256, 0, s>>>(e->d_spill, e->spill_cap, R.sp, R.spill_cap - 1, R.win, R.win_cap - 1, now_ms,
                                        e->profile, R.d + 4);
    return RL_OK;
}

// wait for the rebuild's kernels and read its counters
static bool rebuild_finish(rl_engine* e, Rebuild& R, unsigned long long (&h)[REBUILD_WORDS]) {
    hipStream_t s = e->stream;
    bool ok = hipMemcpyAsync(h, R.d, sizeof h, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = hipStreamSynchronize(s) == hipSuccess && ok;
    return ok;
}

// the fresh tables become the engine's
static void rebuild_commit(rl_engine* e, Rebuild& R) {
    (void)hipFree(e->d_tb);
    (void)hipFree(e->d_win);
    (void)hipFree(e->d_spill);
    (void)hipFree(R.d);
    e->d_tb = R.tb;
    e->d_win = R.win;
    e->d_spill = R.sp;
    set_geometry(e, R.tb_cap, R.win_cap, R.spill_cap);
    R = Rebuild{};
}

extern "C" int rl_table_gc(rl_engine* e, int64_t now_ms, uint64_t tb_capacity, uint64_t win_capacity,
                           rl_table_info* out) {
    if (!e || (out && out->struct_size < 8)) return RL_EINVAL;
    (void)hipSetDevice(e->device);
    Rebuild R;
    int r = rebuild_begin(e, now_ms, tb_capacity, win_capacity, R, "table gc");
    if (r != RL_OK) return r;
    unsigned long long h[REBUILD_WORDS];
    const bool ok = rebuild_finish(e, R, h);
    if (!ok || h[1] || h[3] || h[5]) {
        rebuild_abort(R);
        return ok ? fail(e, RL_ENOMEM, "table gc: live keys do not fit the requested capacity")
                  : fail(e, RL_EDEVICE, "table gc failed");
    }
    rebuild_commit(e, R);
    return out ? rl_table_info_get(e, now_ms, out) : RL_OK;
}

// ---------------------------------------------------------------------------
// snapshots (include/rl_snapshot.h)
// ---------------------------------------------------------------------------

static rl_snapshot_info snapshot_info_of(const SnapHeader& h) {
    return rl_snapshot_info{sizeof(rl_snapshot_info), h.version, h.profile, h.world, h.rank, 0, h.now_ms,
                            h.tb_count, h.win_count, h.spill_count, h.total, h.payload_sum};
}

extern "C" int rl_snapshot_inspect(const void* buf, size_t len, rl_snapshot_info* out) {
    if (!out || out->struct_size < 8) return RL_EINVAL;
    SnapHeader h;
    if (!snap_header_ok(buf, len, &h) || !snap_payload_ok(buf, h)) return RL_EINVAL;
    return copy_out(out, snapshot_info_of(h));
}

extern "C" int rl_snapshot_export(rl_engine* e, int64_t now_ms, uint32_t world, uint32_t rank, void* buf, size_t cap,
                                  rl_snapshot_info* out) {
    if (!e || !out || out->struct_size < 8 || (!buf && cap)) return RL_EINVAL;
    if (world == 0 || rank >= world) return fail(e, RL_EINVAL, "snapshot export: rank outside the world");
    (void)hipSetDevice(e->device);
    int r = drain(e);
    if (r != RL_OK) return r;
    hipStream_t s = e->stream;
    unsigned long long* d = e->d_count;
    unsigned long long* h = e->h_count;
    // the live size first (count and checksum, no writes): nothing runs on
    // the drained engine, so the writing launch finds the same records
    bool ok = hipMemsetAsync(d, 0, SNAP_WORDS * sizeof(unsigned long long), s) == hipSuccess;
    k_snapshot_export<false><<<2048, SNAP_BLOCK, 0, s>>>(e->d_tb, e->tb_cap, e->d_win, e->win_cap, e->d_spill,
                                                         e->spill_cap, now_ms, e->profile, world, rank, nullptr, 0,
                                                         nullptr, 0, nullptr, 0, d);
    ok = ok && hipMemcpyAsync(h, d, SNAP_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) == hipSuccess;
    ok = ok && hipStreamSynchronize(s) == hipSuccess;
    if (!ok) return fail(e, RL_EDEVICE, "snapshot export: count failed");
    const SnapHeader hd = snap_make_header(e->profile, h[SNAP_TB], h[SNAP_WIN], h[SNAP_SPILL], now_ms, world, rank,
                                           h[SNAP_SUM]);
    r = copy_out(out, snapshot_info_of(hd));
    if (r != RL_OK || !buf) return r;
    if (cap < hd.total) return fail(e, RL_ENOMEM, "snapshot export: buffer too small");
    const size_t payload = hd.total - sizeof hd;
    if (payload) {
        uint8_t* stage = nullptr;
        if (hipMalloc(&stage, payload) != hipSuccess) return fail(e, RL_ENOMEM, "snapshot export: allocation failed");
        const size_t tb_end = hd.tb_off + sizeof(TbEntry) * hd.tb_count;
        ok = hipMemsetAsync(d, 0, SNAP_WORDS * sizeof(unsigned long long), s) == hipSuccess;
        if (hd.win_off > tb_end)   // the padding in front of the window section
            ok = ok && hipMemsetAsync(stage + (tb_end - sizeof hd), 0, hd.win_off - tb_end, s) == hipSuccess;
        k_snapshot_export<true><<<2048, SNAP_BLOCK, 0, s>>>(
            e->d_tb, e->tb_cap, e->d_win, e->win_cap, e->d_spill, e->spill_cap, now_ms, e->profile, world, rank,
            (TbEntry*)(stage + (hd.tb_off - sizeof hd)), hd.tb_count, (WinEntry*)(stage + (hd.win_off - sizeof hd)),
            hd.win_count, (SpillEntry*)(stage + (hd.spill_off - sizeof hd)), hd.spill_count, d);
        ok = ok && hipMemcpyAsync(h, d, SNAP_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s) == hipSuccess;
        ok = ok && hipStreamSynchronize(s) == hipSuccess;
        ok = ok && h[SNAP_TB] == hd.tb_count && h[SNAP_WIN] == hd.win_count && h[SNAP_SPILL] == hd.spill_count &&
             h[SNAP_SUM] == hd.payload_sum;
        ok = ok && hipMemcpy((uint8_t*)buf + sizeof hd, stage, payload, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(stage);
        if (!ok) return fail(e, RL_EDEVICE, "snapshot export failed");
    }
    memcpy(buf, &hd, sizeof hd);
    return RL_OK;
}

extern "C" int rl_snapshot_import(rl_engine* e, const void* buf, size_t len, int64_t now_ms, uint64_t tb_capacity,
                                  uint64_t win_capacity, rl_table_info* out) {
    if (!e || (out && out->struct_size < 8)) return RL_EINVAL;
    SnapHeader hd;
    if (!snap_header_ok(buf, len, &hd)) return fail(e, RL_EINVAL, "snapshot import: bad header");
    if (hd.profile != e->profile) return fail(e, RL_EINVAL, "snapshot import: taken under the other profile");
    (void)hipSetDevice(e->device);
    const size_t payload = hd.total - sizeof hd;
    uint8_t* stage = nullptr;
    if (payload && hipMalloc(&stage, payload) != hipSuccess)
        return fail(e, RL_ENOMEM, "snapshot import: allocation failed");
    Rebuild R;
    int r = rebuild_begin(e, now_ms, tb_capacity, win_capacity, R, "snapshot import");
    if (r != RL_OK) {
        (void)hipFree(stage);
        return r;
    }
    hipStream_t s = e->stream;
    bool ok = !payload || hipMemcpyAsync(stage, (const uint8_t*)buf + sizeof hd, payload, hipMemcpyHostToDevice, s) ==
                              hipSuccess;
    if (ok) {
        unsigned long long* c = R.d + REBUILD_IMPORT;
        k_snapshot_import<<<2048, SNAP_BLOCK, 0, s>>>((const TbEntry*)(stage + (hd.tb_off - sizeof hd)), hd.tb_count,
                                                      R.tb, R.tb_cap - 1, now_ms, e->profile,
                                                      (uint64_t)RL_SNAPSHOT_TAG_TB, c);
        k_snapshot_import<<<2048, SNAP_BLOCK, 0, s>>>((const WinEntry*)(stage + (hd.win_off - sizeof hd)),
                                                      hd.win_count, R.win, R.win_cap - 1, now_ms, e->profile,
                                                      (uint64_t)RL_SNAPSHOT_TAG_WIN, c + 4);
        // after the window section: a spill record is counted in its user key's new entry
        k_snapshot_import_spill<<<2048, SNAP_BLOCK, 0, s>>>((const SpillEntry*)(stage + (hd.spill_off - sizeof hd)),
                                                            hd.spill_count, R.sp, R.spill_cap - 1, R.win,
                                                            R.win_cap - 1, now_ms, e->profile, c + 8);
    }
    unsigned long long h[REBUILD_WORDS];
    ok = rebuild_finish(e, R, h) && ok;
    (void)hipFree(stage);
    const unsigned long long* c = h + REBUILD_IMPORT;
    int code = RL_OK;
    const char* msg = "";
    if (!ok) {
        code = RL_EDEVICE, msg = "snapshot import failed";
    } else if (c[SNAP_CHECK] + c[4 + SNAP_CHECK] + c[8 + SNAP_CHECK] != hd.payload_sum) {
        code = RL_EINVAL, msg = "snapshot import: payload checksum mismatch";
    } else if (c[SNAP_CONFLICT] || c[4 + SNAP_CONFLICT]) {
        code = RL_EEXIST, msg = "snapshot import: a key is in the engine and in the snapshot";
    } else if (h[1] || h[3] || h[5] || c[SNAP_LOST] || c[4 + SNAP_LOST] || c[8 + SNAP_LOST]) {
        code = RL_ENOMEM, msg = "snapshot import: live keys do not fit the requested capacity";
    }
    if (code != RL_OK) {
        rebuild_abort(R);
        return fail(e, code, msg);
    }
    rebuild_commit(e, R);
    return out ? rl_table_info_get(e, now_ms, out) : RL_OK;
}
