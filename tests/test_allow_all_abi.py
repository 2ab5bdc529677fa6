"""AllowAll's C ABI (include/rl_engine.h, include/rl_coalescer.h): the symbols,
the trailing struct fields and the argument checks that need no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["rl_allow_all_batch", "rl_allow_all_batch_device", "rl_allow_all_max", "rl_allow_all_grid_cap",
           "rl_coalescer_allow_all"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol(rl, name):
    assert hasattr(rl.lib, name)
    hdr = "rl_coalescer.h" if "coalescer" in name else "rl_engine.h"
    src = open(os.path.join(ROOT, "include", hdr)).read()
    assert re.search(r"^(int|uint32_t)\s+%s\s*\(" % name, src, flags=re.M), f"{name} not declared in {hdr}"


def test_constants_and_trailing_fields(rl):
    src = open(os.path.join(ROOT, "include", "rl_engine.h")).read()
    assert re.search(r"#define\s+RL_ALLOW_ALL_MAX_GROUP\s+16\b", src) and rl.ALLOW_ALL_MAX_GROUP == 16
    assert rl.lib.rl_allow_all_grid_cap() == 1024 * 256 == rl.ALLOW_ALL_GRID_CAP
    # the new fields trail the structs a caller compiled before them passes
    assert [n for n, _ in rl.rl_coalescer_stats._fields_[-4:]] == ["refunds", "refund_launches", "allow_all_groups",
                                                                  "allow_all_launches"]
    assert [n for n, _ in rl.rl_coalescer_backend._fields_[-2:]] == ["refund", "allow_all"]
    hdr = open(os.path.join(ROOT, "include", "rl_coalescer.h")).read()
    body = hdr[hdr.index("typedef struct rl_coalescer_stats"):hdr.index("} rl_coalescer_stats;")]
    assert re.findall(r"^\s*uint64_t\s+(\w+);", body, flags=re.M)[-2:] == ["allow_all_groups", "allow_all_launches"]
    body = hdr[hdr.index("typedef struct rl_coalescer_backend"):hdr.index("} rl_coalescer_backend;")]
    assert re.findall(r"^\s*\w+\s+(\w+);", body, flags=re.M)[-2:] == ["refund", "allow_all"]
    assert C.sizeof(rl.rl_coalescer_stats) == 8 + 8 * 17


def test_no_engine_is_einval(rl):
    assert rl.lib.rl_allow_all_batch(None, 0, *[None] * 13) == rl.RL_EINVAL
    assert rl.lib.rl_allow_all_batch_device(None, 0, *[None] * 14) == rl.RL_EINVAL
    assert rl.lib.rl_allow_all_max(None) == 0
    assert rl.lib.rl_coalescer_allow_all(None, 0, None, None, None, None, None, 0, None, None, None, None, None) \
        == rl.RL_EINVAL


def test_limiter_mirror_symbol(rl):
    assert hasattr(rl.lib, "rll_allow_all")
    src = open(os.path.join(ROOT, "include", "rl_limiter.h")).read()
    assert re.search(r"^int\s+rll_allow_all\s*\(", src, flags=re.M)
    assert rl.lib.rll_allow_all(None, 1, None, None, None, 0, 0, None, None, None, None, 0) == rl.RLL_ERR_ARG
