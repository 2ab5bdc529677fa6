"""Charge's C ABI (include/rl_engine.h, include/rl_coalescer.h,
include/rl_limiter.h): the symbols, the struct sizes and the argument checks
that need no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["rl_charge_batch", "rl_charge_batch_device", "rl_charge_max", "rl_charge_grid_cap", "rl_coalescer_charge",
           "rl_coalescer_get_stats_charge", "rll_charge_n", "rll_charge_many"]


def header_of(name):
    return "rl_coalescer.h" if "coalescer" in name else "rl_limiter.h" if name.startswith("rll_") else "rl_engine.h"


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol(rl, name):
    assert hasattr(rl.lib, name)
    src = open(os.path.join(ROOT, "include", header_of(name))).read()
    assert re.search(r"^(int|uint32_t)\s+%s\s*\(" % name, src, flags=re.M), f"{name} not declared"


def test_constants_and_struct_sizes(rl):
    assert rl.lib.rl_charge_grid_cap() == 1024 * 256 == rl.CHARGE_GRID_CAP
    assert rl.RLL_ERR_CHARGE == 7
    src = open(os.path.join(ROOT, "include", "rl_limiter.h")).read()
    assert re.search(r"#define\s+RLL_ERR_CHARGE\s+7\b", src)
    # the Charge members trail the structs a caller compiled before them passes
    old, new = rl.rl_coalescer_stats, rl.rl_coalescer_stats_charge
    assert new._fields_[:-1] == old._fields_ and new._fields_[-1][0] == "charge_launches"
    assert all(getattr(new, n).offset == getattr(old, n).offset for n, _ in old._fields_)
    assert (new.charge_launches.offset, C.sizeof(new)) == (C.sizeof(old), C.sizeof(old) + 8)
    old, new = rl.rl_coalescer_backend, rl.rl_coalescer_backend_charge
    assert new._fields_[:-1] == old._fields_ and new._fields_[-1][0] == "charge"
    assert (new.charge.offset, C.sizeof(new)) == (C.sizeof(old), C.sizeof(old) + 8)
    hdr = open(os.path.join(ROOT, "include", "rl_coalescer.h")).read()
    for outer, inner, last in (("rl_coalescer_stats_charge", "rl_coalescer_stats s;", "charge_launches"),
                               ("rl_coalescer_backend_charge", "rl_coalescer_backend b;", "charge")):
        body = hdr[hdr.index("typedef struct %s {" % outer):hdr.index("} %s;" % outer)]
        names = re.findall(r"^\s*\w+\s+(\w+);", body, flags=re.M)
        assert inner in body and names[0] in ("s", "b") and names[-1] == last and len(names) == 2
    assert C.sizeof(rl.rll_charge) == 40
    assert [n for n, _ in rl.rll_charge._fields_] == ["charged", "short_by", "remaining", "reset_at_unix_ns",
                                                     "over_limit", "pad_"]
    body = src[src.index("typedef struct rll_charge {"):src.index("} rll_charge;")]
    assert re.findall(r"^\s*\w+\s+(\w+)(?:\[7\])?;", body, flags=re.M) == [n for n, _ in rl.rll_charge._fields_]


def test_no_engine_is_einval(rl):
    assert rl.lib.rl_charge_batch(None, 0, *[None] * 10) == rl.RL_EINVAL
    assert rl.lib.rl_charge_batch_device(None, 0, *[None] * 11) == rl.RL_EINVAL
    assert rl.lib.rl_charge_max(None) == 0
    assert rl.lib.rl_coalescer_charge(None, 0, None, None, None, None, 0, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_get_stats_charge(None, None) == rl.RL_EINVAL
    assert rl.lib.rll_charge_n(None, b"k", 1, 1, 0, 0, None, None, 0) == rl.RLL_ERR_ARG
    assert rl.lib.rll_charge_many(None, 1, None, None, None, 0, 0, None, None, 0) == rl.RLL_ERR_ARG


def test_the_older_structs_keep_their_size(rl):
    """rl_coalescer_get_stats never writes past rl_coalescer_stats, whatever
    size the caller passes; rl_coalescer_get_stats_charge fills in the rest"""
    co = rl.Coalescer(lambda *a: 0)
    big = (C.c_uint8 * (C.sizeof(rl.rl_coalescer_stats_charge) + 16))()
    C.memset(big, 0xAB, C.sizeof(big))
    C.cast(big, C.POINTER(C.c_uint32))[0] = C.sizeof(big)
    assert rl.lib.rl_coalescer_get_stats(co.h, C.cast(big, C.POINTER(rl.rl_coalescer_stats))) == 0
    assert C.cast(big, C.POINTER(C.c_uint32))[0] == C.sizeof(rl.rl_coalescer_stats)
    assert bytes(big[C.sizeof(rl.rl_coalescer_stats):]) == b"\xab" * 24
    C.cast(big, C.POINTER(C.c_uint32))[0] = C.sizeof(big)
    assert rl.lib.rl_coalescer_get_stats_charge(co.h, C.cast(big, C.POINTER(rl.rl_coalescer_stats_charge))) == 0
    assert C.cast(big, C.POINTER(C.c_uint32))[0] == C.sizeof(rl.rl_coalescer_stats_charge)
    assert bytes(big[C.sizeof(rl.rl_coalescer_stats):]) == b"\x00" * 8 + b"\xab" * 16
    st = co.stats_charge()
    assert (st.struct_size, st.charge_launches, st.batches) == (C.sizeof(rl.rl_coalescer_stats_charge), 0, 0)
    st.struct_size = 4
    assert rl.lib.rl_coalescer_get_stats_charge(co.h, C.byref(st)) == rl.RL_EINVAL
    co.close()
