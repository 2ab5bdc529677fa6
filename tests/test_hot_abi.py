"""The top keys' C ABI (include/rl_engine.h, include/rl_coalescer.h): the
symbols, the struct sizes the header fixes, and the argument checks that need
no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["rl_hot_enable", "rl_hot_batch_device", "rl_hot_batch", "rl_hot_read", "rl_hot_grid_cap",
           "rl_coalescer_hot"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol(rl, name):
    assert hasattr(rl.lib, name)
    hdr = "rl_coalescer.h" if "coalescer" in name else "rl_engine.h"
    src = open(os.path.join(ROOT, "include", hdr)).read()
    assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), f"{name} not declared in {hdr}"


def test_struct_sizes(rl):
    # rl_hot_opts {u32 x 4, u64}; rl_hot_key {u64 x 2, u32 x 2}; rl_hot_info {u32, u32, u64 x 11}
    assert C.sizeof(rl.rl_hot_opts) == 24
    assert rl.HOT_KEY.itemsize == 24
    assert C.sizeof(rl.rl_hot_info) == 96
    assert [n for n, _ in rl.rl_hot_opts._fields_] == ["struct_size", "width", "key_slots", "weight", "hot_min"]
    assert [n for n, _ in rl.rl_hot_info._fields_] == [
        "struct_size", "pad_", "width", "depth", "key_slots", "hot_min", "weight", "keys_tracked", "dropped", "total",
        "skipped", "batches", "requests"]
    assert rl.HOT_KEY.names == ("key_id", "estimate", "cfg_id", "pad_")
    assert rl.rl_hot_info().struct_size == 96 and rl.rl_hot_opts().struct_size == 24
    assert (rl.HOT_REQUESTS, rl.HOT_UNITS, rl.HOT_DEPTH) == (0, 1, 4)
    src = open(os.path.join(ROOT, "include", "rl_engine.h")).read()
    assert re.search(r"#define\s+RL_HOT_DEPTH\s+4\b", src)
    # the coalescer's trailing options, behind the struct a caller compiled before them passes
    full, old = rl.rl_coalescer_opts_hot, rl.rl_coalescer_opts
    assert [n for n, _ in full._fields_[-4:]] == ["hot_width", "hot_key_slots", "hot_weight", "hot_min"]
    assert full._fields_[:-4] == old._fields_ and all(getattr(full, n).offset == getattr(old, n).offset
                                                      for n, _ in old._fields_)
    assert (full.hot_width.offset, full.hot_key_slots.offset, full.hot_weight.offset, full.hot_min.offset,
            C.sizeof(full)) == (68, 72, 76, 80, 88)
    hdr = open(os.path.join(ROOT, "include", "rl_coalescer.h")).read()
    body = hdr[hdr.index("typedef struct rl_coalescer_opts"):hdr.index("} rl_coalescer_opts;")]
    assert re.findall(r"^\s*uint\d+_t\s+(\w+);", body, flags=re.M)[-5:] == ["tally_key_slots", "hot_width", "hot_key_slots", "hot_weight", "hot_min"]


def test_no_engine_is_einval(rl):
    o = rl.rl_hot_opts(hot_min=1)
    assert rl.lib.rl_hot_enable(None, C.byref(o)) == rl.RL_EINVAL
    assert rl.lib.rl_hot_batch_device(None, 0, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_hot_batch(None, 0, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_hot_read(None, None, 0, None, None, 0) == rl.RL_EINVAL
    assert rl.lib.rl_coalescer_hot(None, None, 0, None, None, 0) == rl.RL_EINVAL
    assert rl.lib.rl_hot_grid_cap() == 1024 * 256 == rl.HOT_GRID_CAP
