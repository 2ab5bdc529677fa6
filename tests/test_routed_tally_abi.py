"""The routed tally's and top keys' C ABI (include/rl_route.h): the symbols,
their declarations, the Python binding and the argument checks that need no
GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decl(name):
    src = open(os.path.join(ROOT, "include", "rl_route.h")).read()
    d = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", src, flags=re.M)
    assert d, f"{name} not declared"
    return " ".join(d.group(1).split())


def test_symbols(rl):
    vp = C.c_void_p
    fn = rl.lib.rl_tally_routed_device
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, C.c_size_t] + [vp] * 6 + [C.c_uint32, vp]
    fn = rl.lib.rl_hot_routed_device
    assert fn.restype is C.c_int and list(fn.argtypes) == [vp, C.c_size_t] + [vp] * 6
    assert rl.lib.rl_tally_routed_read.restype is C.c_int
    # the leading arguments of the routed decide, the results only read
    lead = ("rl_engine* e, size_t m_max, const uint32_t* count, const rl_route_rec* recv, const uint32_t* order, "
            "const int64_t* server_ms, const rl_route_res* res, ")
    assert _decl("rl_tally_routed_device") == lead + "const int64_t* recv_info, uint32_t world, void* stream"
    assert _decl("rl_hot_routed_device") == lead + "void* stream"
    assert _decl("rl_decide_routed_device") == lead.replace("const rl_route_res* res", "rl_route_res* res") + \
        "void* stream"
    assert _decl("rl_tally_routed_read") == "rl_engine* e, rl_tally_routed_info* out"


def test_info_struct(rl):
    """rl_tally_routed_info: a sized struct of three counters; the existing
    info structs keep their sizes"""
    info = rl.rl_tally_routed_info()
    assert C.sizeof(info) == 32 and info.struct_size == 32
    assert [k for k, _ in info._fields_] == ["struct_size", "pad_", "steps", "requests", "dropped_requests"]
    assert C.sizeof(rl.rl_tally_info) == 8 + 8 * 8 and C.sizeof(rl.rl_hot_info) == 8 + 11 * 8
    src = open(os.path.join(ROOT, "include", "rl_route.h")).read()
    body = re.search(r"typedef struct rl_tally_routed_info \{([^}]*)\} rl_tally_routed_info;", src)
    assert body and " ".join(body.group(1).split()) == \
        "uint32_t struct_size, pad_; uint64_t steps, requests, dropped_requests;"


def test_binding(rl):
    import inspect

    import routed_tally_cases as tc
    import shard
    for name in ("tally_routed", "hot_routed", "tally_routed_read"):
        assert callable(getattr(rl.Engine, name))
    # both counting methods are observe= callables as they stand
    want = ["self", "m_max", "count_p", "recv_p", "order_p", "sms_p", "res_p", "rcnt_p", "world", "stream"]
    assert list(inspect.signature(rl.Engine.tally_routed).parameters) == want
    assert list(inspect.signature(rl.Engine.hot_routed).parameters) == want
    assert "routed" in rl.Tally.__dataclass_fields__
    assert (tc.TALLY_CFG, tc.TALLY_KEY, tc.HOT_KEY) == (rl.TALLY_CFG, rl.TALLY_KEY, rl.HOT_KEY)
    assert "observe" in inspect.signature(shard.RoutedPipeline).parameters


def test_no_engine_is_einval(rl):
    """without an engine every call is RL_EINVAL before a device is touched:
    m_max zero or not, pointers null or not"""
    word = (C.c_uint64 * 8)()
    p = C.cast(word, C.c_void_p)
    t, h = rl.lib.rl_tally_routed_device, rl.lib.rl_hot_routed_device
    assert t(None, 0, None, None, None, None, None, None, 0, None) == rl.RL_EINVAL
    assert t(None, 4, p, p, p, p, p, p, 1, None) == rl.RL_EINVAL
    assert t(None, 1 << 32, p, p, p, p, p, None, 0, None) == rl.RL_EINVAL
    assert h(None, 0, None, None, None, None, None, None) == rl.RL_EINVAL
    assert h(None, 4, p, p, p, p, p, None) == rl.RL_EINVAL
    assert rl.lib.rl_tally_routed_read(None, None) == rl.RL_EINVAL
    info = rl.rl_tally_routed_info()
    assert rl.lib.rl_tally_routed_read(None, C.byref(info)) == rl.RL_EINVAL
