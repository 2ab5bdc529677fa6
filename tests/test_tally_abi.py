"""The usage tally's C ABI (include/rl_engine.h, include/rl_coalescer.h): the
symbols, the struct sizes the header fixes, and the argument checks that need
no GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["rl_tally_enable", "rl_tally_batch_device", "rl_tally_batch", "rl_tally_read", "rl_tally_grid_cap",
           "rl_coalescer_tally"]


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol(rl, name):
    assert hasattr(rl.lib, name)
    hdr = "rl_coalescer.h" if "coalescer" in name else "rl_engine.h"
    src = open(os.path.join(ROOT, "include", hdr)).read()
    assert re.search(r"^int\s+%s\s*\(" % name, src, flags=re.M), f"{name} not declared in {hdr}"


def test_struct_sizes(rl):
    # rl_tally_opts {u32, u32}; rl_tally_cfg {u64[4], u64[2]}; rl_tally_key
    # {u64 x 3, u32 x 2}; rl_tally_info {u32, u32, u64 x 8}
    assert C.sizeof(rl.rl_tally_opts) == 8
    assert rl.TALLY_CFG.itemsize == 48
    assert rl.TALLY_KEY.itemsize == 32
    assert C.sizeof(rl.rl_tally_info) == 72
    assert [n for n, _ in rl.rl_tally_info._fields_] == [
        "struct_size", "pad_", "key_slots", "keys_tracked", "untracked_requests", "untracked_units", "unknown_cfg",
        "bad_codes", "batches", "requests"]
    assert rl.TALLY_KEY.names == ("key_id", "denied", "units_denied", "cfg_id", "pad_")
    assert rl.rl_tally_info().struct_size == 72 and rl.rl_tally_opts().struct_size == 8
    # the coalescer's trailing option
    assert rl.rl_coalescer_opts._fields_[-1][0] == "tally_key_slots"
    # and the native gRPC server's
    assert [n for n, _ in rl.rl_grpc_opts._fields_[-2:]] == ["tally", "names_cap"]


def test_no_engine_is_einval(rl):
    o = rl.rl_tally_opts()
    assert rl.lib.rl_tally_enable(None, C.byref(o)) == rl.RL_EINVAL
    assert rl.lib.rl_tally_batch_device(None, 0, None, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_batch(None, 0, None, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_read(None, None, 0, None, None, 0, None, None, 0) == rl.RL_EINVAL
    assert rl.lib.rl_tally_grid_cap() == 1024 * 256 == rl.TALLY_GRID_CAP
