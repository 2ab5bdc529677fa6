"""The snapshot format (include/rl_snapshot.h) on a CPU-only host: blobs built
by python/rl_snapshot.py from hand-made records must pass the library's
rl_snapshot_inspect with the same counts and checksum, every kind of damage
must be refused, and parse / build / logical_keys must agree with the format."""
import numpy as np
import pytest

import rl_snapshot as snap

NOW = 1_760_000_000_000      # server ms
A = snap.ABSENT


def tb_recs(n, when=NOW + 5000):
    r = np.zeros(n, snap.TB_DTYPE)
    r["key"] = np.arange(n, dtype=np.uint64) * 7919 + 3
    r["tok"] = 1.5 + np.arange(n)
    r["last"] = 1.76e9 + np.arange(n) / 8
    r["when"] = when
    return r


def win_rec(key, slots):
    r = np.zeros(1, snap.WIN_DTYPE)
    r["key"] = key
    for k, (ws, cnt, when) in enumerate(slots):
        r["s"][0, k] = (ws, cnt, when)
    return r


def spill_recs(rows):
    return np.array(rows, dtype=snap.SPILL_DTYPE)


def window_case():
    win = win_rec(42, [(1_760_000_000, 3, NOW + 1000), (1_759_999_940, 7, NOW + 61_000)])
    sp = spill_recs([(42, 1_759_999_880, 2, NOW + 10), (42, 1_759_999_820, 9, NOW + 20)])
    return dict(win=win, spill=sp)


CASES = {
    "empty": dict(),
    "one_tb": dict(tb=tb_recs(1)),
    "window_and_spill": window_case(),
    "tb65": dict(tb=tb_recs(65)),
    "all": dict(tb=tb_recs(3), **window_case()),
}


def blob_of(case, **kw):
    return snap.build(case.get("tb", ()), case.get("win", ()), case.get("spill", ()), now_ms=NOW, **kw)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("profile", [0, 1])
def test_inspect_accepts_built_blobs(rl, name, profile):
    case = CASES[name]
    blob = blob_of(case, profile=profile, world=3, rank=2)
    rc, info = rl.snapshot_inspect(blob)
    assert rc == rl.RL_OK
    counts = [len(case.get(k, ())) for k in ("tb", "win", "spill")]
    assert [info.tb_keys, info.win_keys, info.spill_keys] == counts
    p = snap.parse(blob)
    assert info.checksum == snap.checksum(p["tb"], p["win"], p["spill"]) == int(p["header"]["payload_sum"])
    assert info.bytes == blob.size == snap.layout(*counts)[3]
    assert (info.version, info.profile, info.world, info.rank, info.now_ms) == (1, profile, 3, 2, NOW)
    # sections start on 64-byte boundaries, the header is 128 bytes
    h = p["header"]
    assert h["tb_off"] == 128 and h["win_off"] % 64 == 0 and h["spill_off"] % 64 == 0


def test_checksum_is_order_independent_and_tagged():
    tb = tb_recs(65)
    w = window_case()
    assert snap.checksum(tb, w["win"], w["spill"]) == snap.checksum(tb[::-1], w["win"], w["spill"][::-1])
    assert snap.checksum(tb, (), ()) != snap.checksum(tb[:64], (), ())
    # the same 32 bytes hash differently as a token-bucket and as a spill record
    assert snap.checksum(tb[:1], (), ()) != snap.checksum((), (), tb[:1].view(snap.SPILL_DTYPE))
    # one record by hand: h = mix64(h ^ w_j) from the section's tag
    h = np.uint64(snap.TAG_TB)
    for word in tb[:1].view("<u8"):
        h = snap.mix64(h ^ word)
    assert snap.checksum(tb[:1], (), ()) == int(h)


def with_header(blob, **fields):
    """the blob with header fields replaced and the header checksum redone"""
    b = blob.copy()
    h = b[:128].view(snap.HEADER_DTYPE)
    for k, v in fields.items():
        h[k] = v
    h["header_sum"] = snap.header_checksum(h[0])
    return b


@pytest.mark.parametrize("name", ["one_tb", "window_and_spill", "tb65", "all"])
def test_inspect_refuses_damage(rl, name):
    blob = blob_of(CASES[name])
    assert rl.snapshot_inspect(blob)[0] == rl.RL_OK

    def refused(b, what):
        assert rl.snapshot_inspect(b)[0] == rl.RL_EINVAL, what
        with pytest.raises(snap.FormatError):
            snap.parse(b)

    for off in (128, blob.size - 1, (128 + blob.size) // 2):    # payload bytes
        b = blob.copy()
        b[off] ^= 0x10
        refused(b, f"payload byte {off}")
    for off in (0, 9, 16, 33, 57, 81, 88, 97, 104, 112, 127):     # header bytes
        b = blob.copy()
        b[off] ^= 0x01
        refused(b, f"header byte {off}")
    refused(blob[:-1], "truncated")
    refused(np.concatenate([blob, np.zeros(1, np.uint8)]), "one byte more")
    refused(blob[:127], "shorter than the header")
    refused(with_header(blob, magic=b"RLSNAP02"), "magic")
    refused(with_header(blob, version=2), "version")
    # counts that overrun len, with a valid header checksum (and offsets redone)
    for field in ("tb_count", "win_count", "spill_count"):
        h = blob[:128].view(snap.HEADER_DTYPE)[0]
        counts = {k: int(h[k]) for k in ("tb_count", "win_count", "spill_count")}
        for bump in (1, 1 << 30, (1 << 64) - 1 - counts[field]):
            c = dict(counts)
            c[field] += bump
            fields = dict(c)
            if max(c.values()) < 1 << 50:
                o = snap.layout(c["tb_count"], c["win_count"], c["spill_count"])
                fields.update(tb_off=o[0], win_off=o[1], spill_off=o[2], total=o[3])
            refused(with_header(blob, **fields), f"{field} + {bump}")
    refused(with_header(blob, world=0), "world 0")
    refused(with_header(blob, world=2, rank=2), "rank outside the world")
    refused(with_header(blob, tb_size=64), "entry size")


def test_inspect_refuses_nonzero_padding(rl):
    blob = blob_of(CASES["all"])          # 3 token-bucket records: 32 bytes of padding follow
    pad = 128 + 3 * 32
    assert not blob[pad:pad + 32].any()
    blob[pad + 5] = 1
    assert rl.snapshot_inspect(blob)[0] == rl.RL_EINVAL


@pytest.mark.parametrize("name", sorted(CASES))
def test_parse_build_round_trip(name):
    case = CASES[name]
    blob = blob_of(case, profile=1, world=4, rank=1)
    p = snap.parse(blob)
    for k in ("tb", "win", "spill"):
        want = snap.records(case.get(k, ()), p[k].dtype)
        assert p[k].tobytes() == want.tobytes()
    h = p["header"]
    again = snap.build(p["tb"], p["win"], p["spill"], profile=int(h["profile"]), now_ms=int(h["now_ms"]),
                       world=int(h["world"]), rank=int(h["rank"]))
    assert again.tobytes() == blob.tobytes()


def test_logical_keys_expiry_edges():
    """a key whose expiry equals now_ms is alive on Redis 7 (expired once
    now > when) and gone on miniredis (now >= when)"""
    tb = tb_recs(4)
    tb["when"] = [NOW - 1, NOW, NOW + 1, A]
    win = np.concatenate([win_rec(100, [(50, 1, NOW), (40, 1, NOW - 1)]),
                          win_rec(101, [(50, 1, A), (40, 1, snap.NO_EXPIRY)])])
    sp = spill_recs([(100, 30, 1, NOW), (100, 20, 1, NOW + 1), (101, 30, 1, NOW - 1), (101, 20, 1, A)])
    p = snap.parse(snap.build(tb, win, sp, now_ms=NOW))
    k = [int(x) for x in tb["key"]]
    redis7 = {(k[1], 0, 0), (k[2], 0, 0), (100, 1, 50), (101, 1, 40), (100, 1, 30), (100, 1, 20)}
    mini = {(k[2], 0, 0), (101, 1, 40), (100, 1, 20)}
    got7 = list(snap.logical_keys(p, NOW, snap.PROFILE_REDIS7))
    gotm = list(snap.logical_keys(p, NOW, snap.PROFILE_MINIREDIS))
    assert len(got7) == len(set(got7)) and set(got7) == redis7
    assert len(gotm) == len(set(gotm)) and set(gotm) == mini
    # one ms earlier the `when == NOW` keys are alive on both, and the
    # `when == NOW - 1` keys sit on the edge
    assert set(snap.logical_keys(p, NOW - 1, snap.PROFILE_MINIREDIS)) == redis7
    assert set(snap.logical_keys(p, NOW - 1, snap.PROFILE_REDIS7)) == \
        redis7 | {(k[0], 0, 0), (100, 1, 40), (101, 1, 30)}
    # far in the future only the key without a TTL is left
    assert set(snap.logical_keys(p, NOW + 10 ** 9, snap.PROFILE_REDIS7)) == {(101, 1, 40)}


def test_host_backend_coalescer_has_no_snapshot(rl):
    """snapshots work on the engine-backed coalescer only: over function
    pointers both operations return RL_EINVAL, in sequence order like a GC"""
    def backend(user, m, *ptrs):
        return 0
    co = rl.Coalescer(backend, max_batch=8)
    with pytest.raises(rl.EngineError) as ei:
        co.snapshot(NOW)
    assert ei.value.code == rl.RL_EINVAL
    assert co.restore(blob_of(CASES["all"]), NOW)[0] == rl.RL_EINVAL
    st = co.stats()
    assert (st.gc_runs, st.gc_failures) == (1, 1)      # the restore counts as a (failed) GC run
    co.close()
