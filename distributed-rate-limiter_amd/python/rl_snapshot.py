"""The engine's state-snapshot format (include/rl_snapshot.h) in pure numpy.

No GPU and no native library: a blob written by rl_snapshot_export can be
parsed, checked, listed and rebuilt anywhere, and the tests build blobs here
that rl_snapshot_inspect / rl_snapshot_import must accept.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"RLSNAP01"
VERSION = 1
HEADER_SIZE = 128
TAG_TB = 0x524c534e41505442
TAG_WIN = 0x524c534e4150574e
TAG_SPILL = 0x524c534e41505350
TAG_HEADER = 0x524c534e41504844

ABSENT = -(1 << 63)          # `when` of a key that does not exist
NO_EXPIRY = (1 << 63) - 1    # `when` of a key without TTL
EMPTY_KEY = (1 << 64) - 1
PROFILE_REDIS7, PROFILE_MINIREDIS = 0, 1
KIND_HASH, KIND_WINDOW = 0, 1

TB_DTYPE = np.dtype([("key", "<u8"), ("tok", "<f8"), ("last", "<f8"), ("when", "<i8")])
WIN_SLOT_DTYPE = np.dtype([("ws", "<i8"), ("cnt", "<i8"), ("when", "<i8")])
WIN_DTYPE = np.dtype([("key", "<u8"), ("nspill", "<i8"), ("s", WIN_SLOT_DTYPE, (2,))])
SPILL_DTYPE = np.dtype([("key", "<u8"), ("ws", "<i8"), ("cnt", "<i8"), ("when", "<i8")])
HEADER_DTYPE = np.dtype([
    ("magic", "S8"), ("version", "<u4"), ("header_size", "<u4"), ("profile", "<i4"),
    ("tb_size", "<u4"), ("win_size", "<u4"), ("spill_size", "<u4"),
    ("tb_count", "<u8"), ("win_count", "<u8"), ("spill_count", "<u8"),
    ("tb_off", "<u8"), ("win_off", "<u8"), ("spill_off", "<u8"), ("total", "<u8"),
    ("now_ms", "<i8"), ("world", "<u4"), ("rank", "<u4"),
    ("payload_sum", "<u8"), ("header_sum", "<u8"), ("reserved", "<u8"),
])
assert TB_DTYPE.itemsize == 32 and WIN_DTYPE.itemsize == 64 and SPILL_DTYPE.itemsize == 32
assert HEADER_DTYPE.itemsize == HEADER_SIZE

_M1 = np.uint64(0xbf58476d1ce4e5b9)
_M2 = np.uint64(0x94d049bb133111eb)


class FormatError(ValueError):
    pass


def mix64(x: np.ndarray) -> np.ndarray:
    """splitmix64 finalizer (rl_table.h mix64)"""
    x = np.array(x, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= _M1
        x ^= x >> np.uint64(27)
        x *= _M2
        x ^= x >> np.uint64(31)
    return x


def _fold(words: np.ndarray, tag: int) -> np.ndarray:
    """per row of 8-byte words: h = mix64(h ^ w_j), from the tag"""
    h = np.full(words.shape[0], tag, dtype=np.uint64)
    for j in range(words.shape[1]):
        h = mix64(h ^ words[:, j])
    return h


def _words(rec: np.ndarray) -> np.ndarray:
    rec = np.ascontiguousarray(rec)
    return rec.view(np.uint8).reshape(rec.size, rec.dtype.itemsize).view("<u8")


def records(x, dtype) -> np.ndarray:
    """x (a structured array, a list of tuples, or nothing) as a 1-d array of dtype"""
    return np.asarray(x, dtype=dtype).reshape(-1) if len(x) else np.zeros(0, dtype)


def checksum(tb, win, spill) -> int:
    """the payload checksum: the sum of every record's hash, mod 2^64"""
    tb, win, spill = records(tb, TB_DTYPE), records(win, WIN_DTYPE), records(spill, SPILL_DTYPE)
    total = np.uint64(0)
    with np.errstate(over="ignore"):
        for rec, tag in ((tb, TAG_TB), (win, TAG_WIN), (spill, TAG_SPILL)):
            if len(rec):
                total = total + np.add.reduce(_fold(_words(rec), tag), dtype=np.uint64)
    return int(total)


def header_checksum(header: np.ndarray) -> int:
    h = np.array(header, dtype=HEADER_DTYPE).reshape(1).copy()
    h["header_sum"] = 0
    return int(_fold(_words(h), TAG_HEADER)[0])


def layout(tb_count: int, win_count: int, spill_count: int):
    """(tb_off, win_off, spill_off, total) of a blob with these counts"""
    tb_off = HEADER_SIZE
    win_off = (tb_off + 32 * tb_count + 63) & ~63
    spill_off = win_off + 64 * win_count
    return tb_off, win_off, spill_off, spill_off + 32 * spill_count


def build(tb=(), win=(), spill=(), *, profile=PROFILE_REDIS7, now_ms=0, world=1, rank=0) -> np.ndarray:
    """a blob (uint8 array) from the header fields and the three record arrays"""
    tb, win, spill = records(tb, TB_DTYPE), records(win, WIN_DTYPE), records(spill, SPILL_DTYPE)
    tb_off, win_off, spill_off, total = layout(tb.size, win.size, spill.size)
    h = np.zeros(1, HEADER_DTYPE)
    h["magic"], h["version"], h["header_size"], h["profile"] = MAGIC, VERSION, HEADER_SIZE, profile
    h["tb_size"], h["win_size"], h["spill_size"] = 32, 64, 32
    h["tb_count"], h["win_count"], h["spill_count"] = tb.size, win.size, spill.size
    h["tb_off"], h["win_off"], h["spill_off"], h["total"] = tb_off, win_off, spill_off, total
    h["now_ms"], h["world"], h["rank"] = now_ms, world, rank
    h["payload_sum"] = checksum(tb, win, spill)
    h["header_sum"] = header_checksum(h)
    blob = np.zeros(total, np.uint8)
    blob[:HEADER_SIZE] = h.view(np.uint8)
    blob[tb_off:tb_off + 32 * tb.size] = tb.view(np.uint8)
    blob[win_off:spill_off] = win.view(np.uint8)
    blob[spill_off:total] = spill.view(np.uint8)
    return blob


def parse(blob, check=True) -> dict:
    """{'header', 'tb', 'win', 'spill'}: the header (a HEADER_DTYPE scalar) and
    the three sections as structured arrays (copies).  check: validate as
    rl_snapshot_inspect does, raising FormatError."""
    blob = np.frombuffer(bytes(blob), dtype=np.uint8) if not isinstance(blob, np.ndarray) else blob
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    if blob.size < HEADER_SIZE:
        raise FormatError("shorter than a header")
    h = blob[:HEADER_SIZE].view(HEADER_DTYPE)[0]
    if bytes(h["magic"]) != MAGIC or h["version"] != VERSION or h["header_size"] != HEADER_SIZE:
        raise FormatError("not a version-1 snapshot")
    counts = [int(h[k]) for k in ("tb_count", "win_count", "spill_count")]
    if max(counts) > 1 << 40:
        raise FormatError("record count out of range")
    want = layout(*counts)
    got = tuple(int(h[k]) for k in ("tb_off", "win_off", "spill_off", "total"))
    if got != want or want[3] != blob.size:
        raise FormatError("offsets do not match the counts and the length")
    if (h["tb_size"], h["win_size"], h["spill_size"]) != (32, 64, 32):
        raise FormatError("record sizes")
    tb_off, win_off, spill_off, total = want
    tb = blob[tb_off:tb_off + 32 * counts[0]].view(TB_DTYPE).copy()
    win = blob[win_off:spill_off].view(WIN_DTYPE).copy()
    spill = blob[spill_off:total].view(SPILL_DTYPE).copy()
    if check:
        if int(h["header_sum"]) != header_checksum(h) or h["reserved"] != 0:
            raise FormatError("header checksum")
        if h["profile"] not in (PROFILE_REDIS7, PROFILE_MINIREDIS) or h["world"] == 0 or h["rank"] >= h["world"]:
            raise FormatError("profile or partition filter")
        if blob[tb_off + 32 * counts[0]:win_off].any():
            raise FormatError("padding is not zero")
        if int(h["payload_sum"]) != checksum(tb, win, spill):
            raise FormatError("payload checksum")
    return {"header": h.copy(), "tb": tb, "win": win, "spill": spill}


def alive(when: np.ndarray, now_ms: int, profile: int) -> np.ndarray:
    """key_alive (rl_semantics.h): Redis 7 expires a key once now > when,
    miniredis once now >= when"""
    when = np.asarray(when, dtype=np.int64)
    live = (now_ms <= when) if profile == PROFILE_REDIS7 else (now_ms < when)
    return (when != ABSENT) & ((when == NO_EXPIRY) | live)


def logical_keys(parsed: dict, now_ms: int, profile: int):
    """yield (key_id, kind, window_start) of every key live at now_ms, as
    rl_table_keys defines them: a token-bucket record is one hash key; each live
    slot of a window record and each live spill record is one window key"""
    tb = parsed["tb"]
    for k in tb["key"][alive(tb["when"], now_ms, profile) & (tb["key"] != EMPTY_KEY)]:
        yield int(k), KIND_HASH, 0
    win = parsed["win"]
    if len(win):
        ok = alive(win["s"]["when"], now_ms, profile) & (win["key"] != EMPTY_KEY)[:, None]
        for k, ws in zip(np.repeat(win["key"], 2)[ok.reshape(-1)], win["s"]["ws"][ok]):
            yield int(k), KIND_WINDOW, int(ws)
    sp = parsed["spill"]
    ok = alive(sp["when"], now_ms, profile) & (sp["key"] != EMPTY_KEY)
    for k, ws in zip(sp["key"][ok], sp["ws"][ok]):
        yield int(k), KIND_WINDOW, int(ws)
