"""The routed Charge's C ABI (include/rl_route.h): the symbol, its declaration,
the Python binding and the argument checks that need no GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol(rl):
    assert hasattr(rl.lib, "rl_charge_routed_device")
    fn = rl.lib.rl_charge_routed_device
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    # the arguments of the other routed steps
    assert list(fn.argtypes) == list(rl.lib.rl_refund_routed_device.argtypes)
    src = open(os.path.join(ROOT, "include", "rl_route.h")).read()
    decl = re.search(r"^int\s+rl_charge_routed_device\s*\(([^;]*)\);", src, flags=re.M)
    assert decl, "rl_charge_routed_device not declared"
    ref = re.search(r"^int\s+rl_refund_routed_device\s*\(([^;]*)\);", src, flags=re.M)
    assert " ".join(decl.group(1).split()) == " ".join(ref.group(1).split())


def test_binding(rl):
    import shard
    for name in ("charge_routed", "charge_routed_ev"):
        assert callable(getattr(rl.Engine, name))
    assert shard.OP_CHARGE == 4
    assert len({shard.OP_DECIDE, shard.OP_PEEK, shard.OP_RESET, shard.OP_REFUND, shard.OP_CHARGE}) == 5


def test_no_engine_is_einval(rl):
    """without an engine every call is RL_EINVAL before a device is touched,
    as for rl_refund_routed_device: m_max zero or not, pointers null or not"""
    fn = rl.lib.rl_charge_routed_device
    word = (C.c_uint32 * 8)()
    p = C.cast(word, C.c_void_p)
    assert fn(None, 0, None, None, None, None, None, None, None, None) == rl.RL_EINVAL
    assert fn(None, 0, p, None, None, None, None, None, None, None) == rl.RL_EINVAL
    assert fn(None, 4, p, p, p, p, p, None, None, None) == rl.RL_EINVAL
    assert fn(None, 1 << 32, p, p, p, p, p, None, None, None) == rl.RL_EINVAL
    assert rl.lib.rl_refund_routed_device(None, 4, p, p, p, p, p, None, None, None) == rl.RL_EINVAL
