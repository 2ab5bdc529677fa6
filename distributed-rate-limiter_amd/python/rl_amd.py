"""ctypes binding of the MI355X rate-limit engine (include/rl_engine.h) and of
its host mirror of the reference Go API (include/rl_limiter.h).

This is plumbing for tests and bench.py: the product is the HIP library
lib/librl_amd.so.  There is no CPU fallback: if the library is missing,
importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RL_AMD_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librl_amd.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"HIP engine library not built: {LIB_PATH} (run `make -C distributed-rate-limiter_amd` "
        "or __graft_entry__.build())"
    )
lib = C.CDLL(LIB_PATH)

# --- constants (include/rl_engine.h) -----------------------------------------
RL_OK, RL_EINVAL, RL_ENOMEM, RL_EDEVICE, RL_ETIMEOUT, RL_EORDER = 0, -22, -12, -5, -110, -34
RL_EEXIST = -17
TOKEN_BUCKET, SLIDING_WINDOW, FIXED_WINDOW = 1, 2, 3
ALG_BY_NAME = {"token_bucket": TOKEN_BUCKET, "sliding_window": SLIDING_WINDOW, "fixed_window": FIXED_WINDOW}
PROFILE_REDIS7, PROFILE_MINIREDIS = 0, 1
DENIED, ALLOWED, ERROR, INVALID = 0, 1, 2, 3
RESET_DONE = 1   # per-request status of a reset batch (RL_RESET_DONE; RL_INVALID otherwise)
REFUND_NOKEY, REFUND_DONE = 0, 1   # per-request status of a refund call (RL_REFUND_*; RL_INVALID otherwise)
KEY_RESERVED = (1 << 64) - 1

RLL_OK, RLL_ERR_INVALID_N, RLL_ERR_FAILED, RLL_ERR_CONFIG, RLL_ERR_RESET, RLL_ERR_ARG = 0, 1, 2, 3, 4, 5
RLL_ERR_REFUND = 6
RLL_ERR_CHARGE = 7
NOW_WALL = -(1 << 63)
SMS_DEFAULT = -(1 << 63)


class _Sized(C.Structure):
    """an ABI struct whose first field is struct_size (include/rl_engine.h)"""

    def __init__(self, *args, **kw):
        super().__init__(C.sizeof(self), *args, **kw)


class rll_charge(C.Structure):
    """rll_charge (include/rl_limiter.h): what became of one charge"""
    _fields_ = [
        ("charged", C.c_int64),
        ("short_by", C.c_int64),
        ("remaining", C.c_int64),
        ("reset_at_unix_ns", C.c_int64),
        ("over_limit", C.c_uint8),
        ("pad_", C.c_uint8 * 7),
    ]


class rl_opts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device", C.c_int32),
        ("profile", C.c_int32),
        ("tb_capacity", C.c_uint64),
        ("win_capacity", C.c_uint64),
        ("max_batch", C.c_uint32),
        ("flags", C.c_uint32),
        ("spill_capacity", C.c_uint64),
    ]


class rl_stats(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("pad_", C.c_uint32),
        ("batches", C.c_uint64),
        ("decisions", C.c_uint64),
        ("last_segments", C.c_uint64),
        ("last_heavy", C.c_uint64),
        ("last_coop_rounds", C.c_uint64),
        ("last_coop_iters", C.c_uint64),
        ("sort_bits", C.c_uint32),
        ("sort_passes", C.c_uint32),
        ("stamp_cycles", C.c_uint64 * 7),
        ("coop_ends", C.c_uint64 * 4),
        ("sort_predicted", C.c_uint64),
        ("light_batches", C.c_uint64),
        ("plain_finish_batches", C.c_uint64),
    ]


class rll_result(C.Structure):
    _fields_ = [
        ("allowed", C.c_uint8),
        ("limit", C.c_int64),
        ("remaining", C.c_int64),
        ("retry_after_ns", C.c_int64),
        ("reset_at_ns", C.c_int64),
    ]


class rl_table_info(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32)] + [(k, C.c_uint64) for k in ("tb_capacity", "tb_used", "tb_live", "win_capacity", "win_used",
                                          "win_live", "spill_capacity", "spill_used", "spill_live")]


class rl_tally_opts(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("key_slots", C.c_uint32)]


class rl_tally_info(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32)] + [
        (k, C.c_uint64) for k in ("key_slots", "keys_tracked", "untracked_requests", "untracked_units",
                                  "unknown_cfg", "bad_codes", "batches", "requests")]


class rl_tally_routed_info(_Sized):
    """include/rl_route.h"""
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32)] + [
        (k, C.c_uint64) for k in ("steps", "requests", "dropped_requests")]


# rl_tally_cfg / rl_tally_key as numpy records
TALLY_CFG = np.dtype([("count", np.uint64, 4), ("units", np.uint64, 2)])
TALLY_KEY = np.dtype([("key_id", np.uint64), ("denied", np.uint64), ("units_denied", np.uint64),
                      ("cfg_id", np.uint32), ("pad_", np.uint32)])


class rl_hot_opts(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_uint32), ("key_slots", C.c_uint32),
                ("weight", C.c_uint32), ("hot_min", C.c_uint64)]


class rl_hot_info(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32)] + [
        (k, C.c_uint64) for k in ("width", "depth", "key_slots", "hot_min", "weight", "keys_tracked", "dropped",
                                  "total", "skipped", "batches", "requests")]


# rl_hot_key as a numpy record
HOT_KEY = np.dtype([("key_id", np.uint64), ("estimate", np.uint64), ("cfg_id", np.uint32), ("pad_", np.uint32)])
HOT_REQUESTS, HOT_UNITS = 0, 1
HOT_DEPTH = 4


class rl_snapshot_info(_Sized):
    """include/rl_snapshot.h"""
    _fields_ = [("struct_size", C.c_uint32), ("version", C.c_uint32), ("profile", C.c_int32), ("world", C.c_uint32),
                ("rank", C.c_uint32), ("pad_", C.c_uint32), ("now_ms", C.c_int64)] + [
        (k, C.c_uint64) for k in ("tb_keys", "win_keys", "spill_keys", "bytes", "checksum")]


class rl_coalescer_opts(_Sized):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("max_batch", C.c_uint32),
        ("max_in_flight", C.c_uint32),
        ("gc_high_pct", C.c_uint32),
        ("linger_ns", C.c_int64),
        ("queue_cap", C.c_uint64),
        ("gc_interval_ns", C.c_int64),
        ("gc_margin_ms", C.c_int64),
        ("gc_max_tb_capacity", C.c_uint64),
        ("gc_max_win_capacity", C.c_uint64),
        ("tally_key_slots", C.c_uint32),
    ]


class rl_coalescer_opts_hot(_Sized):
    """rl_coalescer_opts with the top keys' trailing options: the whole struct
    of include/rl_coalescer.h.  rl_coalescer_opts above is the struct up to
    tally_key_slots, as a caller compiled before them passes it (its shorter
    struct_size: top keys off)."""
    _fields_ = rl_coalescer_opts._fields_ + [
        ("hot_width", C.c_uint32),
        ("hot_key_slots", C.c_uint32),
        ("hot_weight", C.c_uint32),
        ("hot_min", C.c_uint64),
    ]


class rl_coalescer_stats(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32)] + [
        (k, C.c_uint64) for k in ("submitted", "decided", "batches", "max_batch_seen", "pending", "expired",
                                  "cancelled", "gc_runs", "gc_checks", "gc_failures", "peeked", "resets",
                                  "reset_launches", "refunds", "refund_launches", "allow_all_groups",
                                  "allow_all_launches")]


class rl_coalescer_stats_charge(_Sized):
    """rl_coalescer_stats_charge (include/rl_coalescer.h): rl_coalescer_stats
    with Charge's trailing counter.  rl_coalescer_stats above is the struct up
    to allow_all_launches, as a caller compiled before Charge passes it."""
    _fields_ = rl_coalescer_stats._fields_ + [("charge_launches", C.c_uint64)]


vp = C.c_void_p
# rl_batch_fn (include/rl_coalescer.h)
BATCH_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp)
RESET_FN = C.CFUNCTYPE(C.c_int, vp, C.c_uint32, C.c_uint64, C.c_int64)
RESET_BATCH_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp)
REFUND_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp)
ALLOW_ALL_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp)
CHARGE_FN = C.CFUNCTYPE(C.c_int, vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, vp)
INFO_FN = C.CFUNCTYPE(C.c_int, vp, C.c_int64, C.POINTER(rl_table_info))
GC_FN = C.CFUNCTYPE(C.c_int, vp, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(rl_table_info))


class rl_coalescer_backend(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("batch", BATCH_FN), ("reset", RESET_FN), ("table_info", INFO_FN),
                ("gc", GC_FN), ("user", vp), ("peek", BATCH_FN), ("reset_batch", RESET_BATCH_FN),
                ("refund", REFUND_FN), ("allow_all", ALLOW_ALL_FN)]



class rl_coalescer_backend_charge(_Sized):
    """rl_coalescer_backend_charge: rl_coalescer_backend with Charge's trailing
    function"""
    _fields_ = rl_coalescer_backend._fields_ + [("charge", CHARGE_FN)]


_sig = {
    "rl_engine_create": (C.c_int, [C.POINTER(rl_opts), C.POINTER(vp)]),
    "rl_engine_destroy": (C.c_int, [vp]),
    "rl_config_register": (C.c_int, [vp, C.c_uint8, C.c_int64, C.c_int64, C.POINTER(C.c_uint32)]),
    "rl_decide_batch": (C.c_int, [vp, C.c_size_t] + [vp] * 10),
    "rl_decide_batch_device": (C.c_int, [vp, C.c_size_t] + [vp] * 11),
    "rl_peek_batch": (C.c_int, [vp, C.c_size_t] + [vp] * 10),
    "rl_peek_batch_device": (C.c_int, [vp, C.c_size_t] + [vp] * 11),
    "rl_peek_grid_cap": (C.c_int, []),
    "rl_coalescer_peek": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rll_peek_n": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int,
                             C.POINTER(rll_result), C.c_char_p, C.c_size_t]),
    "rl_reset_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp]),
    "rl_reset_batch_device": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
    "rl_reset_grid_cap": (C.c_int, []),
    "rl_refund_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp, vp]),
    "rl_refund_batch_device": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp, vp, vp]),
    "rl_refund_max": (C.c_uint32, [vp]),
    "rl_refund_grid_cap": (C.c_int, []),
    "rl_allow_all_batch": (C.c_int, [vp, C.c_size_t] + [vp] * 13),
    "rl_allow_all_batch_device": (C.c_int, [vp, C.c_size_t] + [vp] * 14),
    "rl_allow_all_max": (C.c_uint32, [vp]),
    "rl_allow_all_grid_cap": (C.c_int, []),
    "rl_charge_batch": (C.c_int, [vp, C.c_size_t] + [vp] * 10),
    "rl_charge_batch_device": (C.c_int, [vp, C.c_size_t] + [vp] * 11),
    "rl_charge_max": (C.c_uint32, [vp]),
    "rl_charge_grid_cap": (C.c_int, []),
    "rl_tally_enable": (C.c_int, [vp, C.POINTER(rl_tally_opts)]),
    "rl_tally_batch_device": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
    "rl_tally_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp]),
    "rl_tally_read": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_uint32), vp, C.c_size_t, C.POINTER(C.c_uint64),
                                C.POINTER(rl_tally_info), C.c_int]),
    "rl_tally_grid_cap": (C.c_int, []),
    "rl_coalescer_tally": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_uint32), vp, C.c_size_t,
                                     C.POINTER(C.c_uint64), C.POINTER(rl_tally_info), C.c_int]),
    "rl_hot_enable": (C.c_int, [vp, C.POINTER(rl_hot_opts)]),
    "rl_hot_batch_device": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
    "rl_hot_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp]),
    "rl_hot_read": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(rl_hot_info), C.c_int]),
    "rl_hot_grid_cap": (C.c_int, []),
    "rl_coalescer_hot": (C.c_int, [vp, vp, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(rl_hot_info), C.c_int]),
    "rl_engine_sync": (C.c_int, [vp]),
    "rl_reset": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_int64]),
    "rl_reset_device": (C.c_int, [vp, C.c_uint32, C.c_uint64, C.c_int64, vp]),
    "rl_engine_stats": (C.c_int, [vp, C.POINTER(rl_stats)]),
    "rl_engine_set_timing": (C.c_int, [vp, C.c_int]),
    "rl_table_info_get": (C.c_int, [vp, C.c_int64, C.POINTER(rl_table_info)]),
    "rl_table_gc": (C.c_int, [vp, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(rl_table_info)]),
    "rl_snapshot_export": (C.c_int, [vp, C.c_int64, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                     C.POINTER(rl_snapshot_info)]),
    "rl_snapshot_inspect": (C.c_int, [vp, C.c_size_t, C.POINTER(rl_snapshot_info)]),
    "rl_snapshot_import": (C.c_int, [vp, vp, C.c_size_t, C.c_int64, C.c_uint64, C.c_uint64,
                                     C.POINTER(rl_table_info)]),
    "rl_coalescer_snapshot": (C.c_int, [vp, C.c_int64, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                        C.POINTER(rl_snapshot_info)]),
    "rl_coalescer_restore": (C.c_int, [vp, vp, C.c_size_t, C.c_int64, C.c_uint64, C.c_uint64,
                                       C.POINTER(rl_table_info)]),
    "rl_engine_stage_times": (C.c_int, [vp, vp, C.c_int, C.POINTER(C.c_uint64)]),
    "rl_last_error": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "rl_engine_debug_words": (C.c_int, [vp, vp, C.c_size_t]),
    "rl_engine_debug_stamps": (C.c_int, [vp, vp, C.c_size_t]),
    "rl_selftest_q14_host": (C.c_int, [vp, vp, C.c_size_t]),
    "rl_selftest_q14_device": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "rll_engine_new": (C.c_int, [C.POINTER(rl_opts), C.POINTER(vp), C.c_char_p, C.c_size_t]),
    "rll_engine_free": (C.c_int, [vp]),
    "rll_engine_raw": (vp, [vp]),
    "rll_engine_set_server_ms": (C.c_int, [vp, C.c_int64]),
    "rll_keys": (C.c_int, [vp, C.c_int64, C.c_char_p, C.c_size_t]),
    "rl_table_keys": (C.c_int, [vp, C.c_int64, vp, C.c_size_t, C.POINTER(C.c_uint64)]),
    "rll_config_validate": (C.c_int, [C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_size_t]),
    "rll_format_key": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t]),
    "rll_duration_string": (C.c_int, [C.c_int64, C.c_char_p, C.c_size_t]),
    "rll_new": (C.c_int, [vp, C.c_char_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int, C.c_int,
                          C.POINTER(vp), C.c_char_p, C.c_size_t]),
    "rll_allow_n": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int,
                              C.POINTER(rll_result), C.c_char_p, C.c_size_t]),
    "rll_allow_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp, vp]),
    "rll_reset": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_int64, C.c_char_p, C.c_size_t]),
    "rll_reset_many": (C.c_int, [vp, C.c_size_t, vp, vp, C.c_int64, C.c_char_p, C.c_size_t]),
    "rll_refund_n": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int64, vp, C.c_char_p,
                               C.c_size_t]),
    "rll_charge_n": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.c_int64, C.c_int64, C.c_int, vp, C.c_char_p, C.c_size_t]),
    "rll_charge_many": (C.c_int, [vp, C.c_size_t, vp, vp, vp, C.c_int64, C.c_int, vp, C.c_char_p, C.c_size_t]),
    "rll_allow_all": (C.c_int, [vp, C.c_size_t, vp, vp, vp, C.c_int64, C.c_int, vp, vp, vp, C.c_char_p, C.c_size_t]),
    "rll_refund_many": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, C.c_int64, vp, C.c_char_p, C.c_size_t]),
    "rll_close": (C.c_int, [vp]),
    "rll_free": (C.c_int, [vp]),
    "rll_new_allowed_result": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(rll_result)]),
    "rll_new_denied_result": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(rll_result)]),
    "rll_new_fail_open_result": (C.c_int, [C.POINTER(rll_result)]),
    "rll_add_metrics": (C.c_int, [vp]),
    "rll_metrics_expose": (C.c_int, [vp, C.c_char_p, C.c_size_t]),
    "rll_add_logging": (C.c_int, [vp, C.c_size_t]),
    "rll_log_drain": (C.c_int, [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64)]),
    "rll_new_fail_closed_result": (C.c_int, [C.POINTER(rll_result)]),
    # the options by address: rl_coalescer_opts or rl_coalescer_opts_hot, told apart by struct_size
    "rl_coalescer_create": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "rl_coalescer_create_with_backend": (C.c_int, [BATCH_FN, vp, vp, C.POINTER(vp)]),
    "rl_coalescer_create_with_backends": (C.c_int, [BATCH_FN, RESET_FN, vp, vp, C.POINTER(vp)]),
    # the backend by address: rl_coalescer_backend or rl_coalescer_backend_charge, told apart by struct_size
    "rl_coalescer_create_with_host_backend": (C.c_int, [vp, vp, C.POINTER(vp)]),
    "rl_coalescer_reset": (C.c_int, [vp, C.c_uint64, C.c_int64, C.c_uint32]),
    "rl_coalescer_reset_batch": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp]),
    "rl_coalescer_refund": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp]),
    "rl_coalescer_allow_all": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp]),
    "rl_coalescer_now_ns": (C.c_int64, []),
    "rl_coalescer_submit_deadline": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, C.c_int64, C.POINTER(C.c_uint64)]),
    "rl_coalescer_cancel": (C.c_int, [vp, C.c_uint64]),
    "rl_coalescer_decide_deadline": (C.c_int, [vp, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_int64,
                                               vp, vp, vp, vp]),
    "rl_coalescer_table_info": (C.c_int, [vp, C.c_int64, C.POINTER(rl_table_info)]),
    "rl_coalescer_gc": (C.c_int, [vp, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(rl_table_info)]),
    "rl_hash_keys_host": (C.c_int, [C.c_size_t, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_char_p, C.c_size_t, vp]),
    "rl_coalescer_destroy": (C.c_int, [vp]),
    "rl_coalescer_submit": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, C.POINTER(C.c_uint64)]),
    "rl_coalescer_wait": (C.c_int, [vp, C.c_uint64, C.c_int64, vp, vp, vp, vp]),
    "rl_coalescer_decide": (C.c_int, [vp, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, vp, vp, vp, vp]),
    "rl_coalescer_get_stats": (C.c_int, [vp, C.POINTER(rl_coalescer_stats)]),
    "rl_coalescer_get_stats_charge": (C.c_int, [vp, C.POINTER(rl_coalescer_stats_charge)]),
    "rl_coalescer_charge": (C.c_int, [vp, C.c_size_t, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp]),
    "rl_hash_keys_device": (C.c_int, [C.c_size_t, vp, C.c_uint64, vp, C.c_uint64, C.c_char_p, C.c_size_t, vp, vp]),
    "rl_decide_batch_keys_device": (C.c_int, [vp, C.c_size_t, vp, C.c_uint64, vp, C.c_uint64, C.c_char_p,
                                              C.c_size_t] + [vp] * 10),
    "rl_hash_keys": (C.c_int, [C.c_int32, C.c_size_t, vp, C.c_uint64, vp, C.c_uint64, C.c_char_p, C.c_size_t, vp]),
    "rl_router_create": (C.c_int, [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "rl_router_destroy": (C.c_int, [vp]),
    "rl_router_sync": (C.c_int, [vp, vp]),
    "rl_route_owner": (C.c_int, [vp, C.c_size_t, vp, vp, vp]),
    "rl_stream_create_dedicated": (C.c_int, [C.c_int32, C.POINTER(vp)]),
    "rl_stream_destroy": (C.c_int, [vp]),
    "rl_router_capacity": (C.c_uint32, [vp]),
    "rl_route_pack": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_route_pack_sel": (C.c_int, [vp, C.c_size_t] + [vp] * 9),
    "rl_allow_all_settle_device": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_route_merge": (C.c_int, [vp] + [vp] * 6),
    "rl_route_unpack": (C.c_int, [vp, C.c_size_t] + [vp] * 7),
    "rl_decide_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 6),
    "rl_decide_routed_device_io": (C.c_int, [vp, C.c_size_t] + [vp] * 7),
    "rl_decide_routed_device_ev": (C.c_int, [vp, C.c_size_t] + [vp] * 7),
    "rl_peek_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_reset_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_refund_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_charge_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 8),
    "rl_tally_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 6 + [C.c_uint32, vp]),
    "rl_hot_routed_device": (C.c_int, [vp, C.c_size_t] + [vp] * 6),
    "rl_tally_routed_read": (C.c_int, [vp, C.POINTER(rl_tally_routed_info)]),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def _ptr(a):
    return None if a is None else a.ctypes.data_as(vp)


class EngineError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{msg} (status {code})")
        self.code = code


def q14_host(x: np.ndarray) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    lib.rl_selftest_q14_host(_ptr(x), _ptr(out), x.size)
    return out


@dataclass
class Decisions:
    decision: np.ndarray
    remaining: np.ndarray
    retry_after_ns: np.ndarray
    reset_at_ns: np.ndarray
    tokens: np.ndarray | None


@dataclass
class Charges:
    """rl_charge_batch: one row per request (no retry-after: nothing is retried)"""
    decision: np.ndarray
    charged: np.ndarray
    remaining: np.ndarray
    reset_at_ns: np.ndarray
    tokens: np.ndarray | None


# rl_opts.flags (include/rl_engine.h)
OPT_PIPELINE = 1
# requests one k_peek launch covers at one request per thread (grid cap x block size)
PEEK_GRID_CAP = lib.rl_peek_grid_cap()
# the same of k_reset_batch
RESET_GRID_CAP = lib.rl_reset_grid_cap()
# the same of k_refund_add / k_refund_apply
REFUND_GRID_CAP = lib.rl_refund_grid_cap()
# the same of k_allow_all_settle
ALLOW_ALL_GRID_CAP = lib.rl_allow_all_grid_cap()
# the same of k_charge_ask / k_charge_finish
CHARGE_GRID_CAP = lib.rl_charge_grid_cap()
# the largest group of an AllowAll call (RL_ALLOW_ALL_MAX_GROUP)
ALLOW_ALL_MAX_GROUP = 16
# the same of k_tally
TALLY_GRID_CAP = lib.rl_tally_grid_cap()
# the same of k_hot_add / k_hot_pick
HOT_GRID_CAP = lib.rl_hot_grid_cap()


@dataclass
class Hot:
    """rl_hot_read: keys the top candidates (HOT_KEY, largest estimate first),
    info the rl_hot_info"""
    keys: np.ndarray
    keys_tracked: int
    info: rl_hot_info


@dataclass
class Tally:
    """rl_tally_read: cfg[c] the counters of config c (TALLY_CFG), keys the
    top throttled keys (TALLY_KEY, most denied first), info the rl_tally_info,
    routed the rl_tally_routed_info of an Engine's read (as it was before a
    clearing read cleared it)"""
    cfg: np.ndarray
    keys: np.ndarray
    keys_tracked: int
    info: rl_tally_info
    routed: rl_tally_routed_info | None = None


class Engine:
    """rl_engine: the batched decision engine on one GPU."""

    def __init__(self, profile=PROFILE_REDIS7, tb_capacity=1 << 16, win_capacity=1 << 16,
                 max_batch=1 << 20, device=0, flags=0, spill_capacity=0):
        o = rl_opts(device=device, profile=profile, tb_capacity=tb_capacity, win_capacity=win_capacity,
                    max_batch=max_batch, flags=flags, spill_capacity=spill_capacity)
        h = vp()
        rc = lib.rl_engine_create(C.byref(o), C.byref(h))
        if rc != RL_OK:
            raise EngineError(rc, "rl_engine_create failed")
        self.h = h
        self.profile = profile

    def close(self):
        if self.h:
            lib.rl_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        buf = C.create_string_buffer(512)
        lib.rl_last_error(self.h, buf, 512)
        return buf.value.decode()

    def register(self, alg: int, limit: int, window_ns: int) -> int:
        cid = C.c_uint32()
        rc = lib.rl_config_register(self.h, alg, limit, window_ns, C.byref(cid))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return cid.value

    def decide(self, key, ts, n, cfg, server_ms=None, want_tokens=True, check=True) -> Decisions:
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        sms = None if server_ms is None else np.ascontiguousarray(server_ms, dtype=np.int64)
        m = key.size
        out = Decisions(np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64),
                        np.empty(m, np.int64), np.empty(m, np.float64) if want_tokens else None)
        rc = lib.rl_decide_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(sms),
                                 _ptr(out.decision), _ptr(out.remaining), _ptr(out.retry_after_ns),
                                 _ptr(out.reset_at_ns), _ptr(out.tokens))
        if check and rc != RL_OK:
            raise EngineError(rc, self.last_error())
        out.status = rc
        return out

    def decide_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream=None, out_stream=None):
        """rl_decide_routed_device(_io) (include/rl_route.h): the merged
        routed batch (its size in device memory at count_p, at most m_max);
        the grouping waits for `stream`, `out_stream` (default: `stream`)
        waits for the results"""
        if out_stream is None:
            rc = lib.rl_decide_routed_device(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, stream)
        else:
            rc = lib.rl_decide_routed_device_io(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, stream,
                                                out_stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def decide_routed_ev(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p):
        """rl_decide_routed_device_ev: the grouping waits for `stream`; the
        results' completion is recorded into the hipEvent_t at event_p"""
        rc = lib.rl_decide_routed_device_ev(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def _routed_op(self, fn, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, out_stream, event_p):
        rc = fn(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, out_stream, event_p)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def peek_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream=None, out_stream=None):
        """rl_peek_routed_device (include/rl_route.h): the peek step of the
        routed path on the merged batch -- what decide_routed would write,
        with nothing changed; the kernel waits for `stream`, `out_stream`
        (default: `stream`) waits for the results"""
        self._routed_op(lib.rl_peek_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream,
                        out_stream, None)

    def peek_routed_ev(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p):
        """the same with the results' completion recorded into the hipEvent_t
        at event_p"""
        if not event_p:
            raise ValueError("peek_routed_ev needs an event")
        self._routed_op(lib.rl_peek_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, None,
                        event_p)

    def reset_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream=None, out_stream=None):
        """rl_reset_routed_device: the reset step of the routed path -- every
        request of the merged batch deletes its key (as reset()); result
        records {RESET_DONE or INVALID, 0, 0, 0}"""
        self._routed_op(lib.rl_reset_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream,
                        out_stream, None)

    def reset_routed_ev(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p):
        """the same with the results' completion recorded into the hipEvent_t
        at event_p"""
        if not event_p:
            raise ValueError("reset_routed_ev needs an event")
        self._routed_op(lib.rl_reset_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, None,
                        event_p)

    def refund_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream=None, out_stream=None):
        """rl_refund_routed_device: the refund step of the routed path -- the
        merged batch as ONE refund call (refund()): all ranks' refunds of one
        target are summed and applied once; result records {REFUND_DONE,
        REFUND_NOKEY or INVALID, 0, 0, 0}, and {RL_DROPPED, 0, 0, 0} for the
        requests past min(m_max, refund_max())"""
        self._routed_op(lib.rl_refund_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream,
                        out_stream, None)

    def refund_routed_ev(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p):
        """the same with the results' completion recorded into the hipEvent_t
        at event_p"""
        if not event_p:
            raise ValueError("refund_routed_ev needs an event")
        self._routed_op(lib.rl_refund_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, None,
                        event_p)

    def charge_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream=None, out_stream=None):
        """rl_charge_routed_device: the charge step of the routed path -- the
        merged batch as ONE Charge call (charge()) in merge order; result
        records {decision, remaining, charged, reset_at} (`charged` in the
        retry_after field), and {RL_DROPPED, 0, 0, 0} for the requests past
        min(m_max, charge_max())"""
        self._routed_op(lib.rl_charge_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream,
                        out_stream, None)

    def charge_routed_ev(self, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, event_p):
        """the same with the results' completion recorded into the hipEvent_t
        at event_p"""
        if not event_p:
            raise ValueError("charge_routed_ev needs an event")
        self._routed_op(lib.rl_charge_routed_device, m_max, count_p, recv_p, order_p, sms_p, res_p, stream, None,
                        event_p)

    def tally_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, rcnt_p=None, world=0, stream=None):
        """rl_tally_routed_device: the usage tally of a finished routed decide
        step, counted on the keys' owner -- the merged batch and its result
        records, enqueued on `stream` behind the results; rcnt_p (the received
        info rows of `world` sources, or None) counts the requests dropped at
        their senders.  The signature of RoutedPipeline's observe= callables"""
        rc = lib.rl_tally_routed_device(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, rcnt_p, world, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def hot_routed(self, m_max, count_p, recv_p, order_p, sms_p, res_p, rcnt_p=None, world=0, stream=None):
        """rl_hot_routed_device: the top keys of a finished routed decide step,
        counted on the keys' owner (the adds, then the pick, on `stream`).
        rcnt_p and world are taken and ignored -- dropped requests have no key
        here -- so that the method is an observe= callable as it stands"""
        rc = lib.rl_hot_routed_device(self.h, m_max, count_p, recv_p, order_p, sms_p, res_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def tally_routed_read(self) -> rl_tally_routed_info:
        """rl_tally_routed_read: the routed tally's own counters -- steps,
        requests looked at, requests dropped at their senders (zeroed by a
        clearing tally_read)"""
        info = rl_tally_routed_info()
        rc = lib.rl_tally_routed_read(self.h, C.byref(info))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return info

    def decide_device(self, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, rem_p, retry_p, reset_p, tok_p,
                      stream=None):
        rc = lib.rl_decide_batch_device(self.h, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, rem_p,
                                        retry_p, reset_p, tok_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def peek(self, key, ts, n, cfg, server_ms=None, want_tokens=True) -> Decisions:
        """rl_peek_batch: what decide() would return for each request, with
        nothing changed; n == 0 asks how much is left"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        sms = None if server_ms is None else np.ascontiguousarray(server_ms, dtype=np.int64)
        m = key.size
        out = Decisions(np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64),
                        np.empty(m, np.int64), np.empty(m, np.float64) if want_tokens else None)
        rc = lib.rl_peek_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(sms),
                               _ptr(out.decision), _ptr(out.remaining), _ptr(out.retry_after_ns),
                               _ptr(out.reset_at_ns), _ptr(out.tokens))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return out

    def peek_device(self, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, rem_p, retry_p, reset_p, tok_p,
                    stream=None):
        rc = lib.rl_peek_batch_device(self.h, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, rem_p,
                                      retry_p, reset_p, tok_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def sync(self) -> int:
        return lib.rl_engine_sync(self.h)

    def reset(self, cfg: int, key: int, ts: int):
        rc = lib.rl_reset(self.h, cfg, key, ts)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def reset_batch(self, key, ts, cfg, want_status=True):
        """rl_reset_batch: m resets in one launch (chunks of max_batch), with
        the effect of m reset() calls in any order -> the per-request status
        (RESET_DONE, or INVALID for an unknown config / the reserved key)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        m = key.size
        assert ts.size == m and cfg.size == m
        status = np.empty(m, np.uint8) if want_status else None
        rc = lib.rl_reset_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(cfg), _ptr(status))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return status

    def reset_batch_device(self, m, key_p, ts_p, cfg_p, status_p=None, stream=None):
        rc = lib.rl_reset_batch_device(self.h, m, key_p, ts_p, cfg_p, status_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def refund(self, key, ts, n, cfg, server_ms=None, want_status=True):
        """rl_refund_batch: one refund call -- per target (a bucket, or the
        window counter key of ts) one script run with the sum of the n of the
        requests that found it live -> the per-request status (REFUND_DONE,
        REFUND_NOKEY, INVALID)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        sms = None if server_ms is None else np.ascontiguousarray(server_ms, dtype=np.int64)
        m = key.size
        assert ts.size == m and n.size == m and cfg.size == m and (sms is None or sms.size == m)
        status = np.empty(m, np.uint8) if want_status else None
        rc = lib.rl_refund_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(sms), _ptr(status))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return status

    def refund_device(self, m, key_p, ts_p, n_p, cfg_p, sms_p=None, status_p=None, stream=None):
        rc = lib.rl_refund_batch_device(self.h, m, key_p, ts_p, n_p, cfg_p, sms_p, status_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def refund_max(self) -> int:
        return lib.rl_refund_max(self.h)

    def allow_all(self, key, ts, n, cfg, first, server_ms=None, want_tokens=True, want_rollback=True,
                  check=True) -> Decisions:
        """rl_allow_all_batch: all-or-nothing checks across several limiters.
        Member i starts a group when i == 0 or first[i] != 0.  -> the members'
        Decisions as decide() gives them, plus `.verdict` (the group's verdict
        on every member) and `.rollback` (REFUND_DONE, REFUND_NOKEY, INVALID:
        what became of the member's give-back)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        first = np.ascontiguousarray(first, dtype=np.uint8)
        sms = None if server_ms is None else np.ascontiguousarray(server_ms, dtype=np.int64)
        m = key.size
        assert ts.size == m and n.size == m and cfg.size == m and first.size == m and (sms is None or sms.size == m)
        out = Decisions(np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64),
                        np.empty(m, np.int64), np.empty(m, np.float64) if want_tokens else None)
        out.verdict = np.empty(m, np.uint8)
        out.rollback = np.empty(m, np.uint8) if want_rollback else None
        rc = lib.rl_allow_all_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(sms), _ptr(first),
                                    _ptr(out.decision), _ptr(out.remaining), _ptr(out.retry_after_ns),
                                    _ptr(out.reset_at_ns), _ptr(out.tokens), _ptr(out.verdict), _ptr(out.rollback))
        if check and rc != RL_OK:
            raise EngineError(rc, self.last_error())
        out.status = rc
        return out

    def allow_all_device(self, m, key_p, ts_p, n_p, cfg_p, sms_p, first_p, dec_p, rem_p, retry_p, reset_p, tok_p,
                         verdict_p, rollback_p=None, stream=None):
        rc = lib.rl_allow_all_batch_device(self.h, m, key_p, ts_p, n_p, cfg_p, sms_p, first_p, dec_p, rem_p, retry_p,
                                           reset_p, tok_p, verdict_p, rollback_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def allow_all_max(self) -> int:
        return lib.rl_allow_all_max(self.h)

    def charge(self, key, ts, n, cfg, server_ms=None, want_tokens=True, check=True) -> "Charges":
        """rl_charge_batch: record usage after the fact.  A token bucket gives
        up min(n, what it holds); a window counter records the whole n.  ->
        Charges: `decision` (ALLOWED: all of n was charged; DENIED: a bucket
        charged less than n, or a window is now over its limit), `charged`,
        `remaining`, `reset_at_ns`, `tokens`"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        sms = None if server_ms is None else np.ascontiguousarray(server_ms, dtype=np.int64)
        m = key.size
        assert ts.size == m and n.size == m and cfg.size == m and (sms is None or sms.size == m)
        out = Charges(np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64),
                      np.empty(m, np.float64) if want_tokens else None)
        rc = lib.rl_charge_batch(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(sms), _ptr(out.decision),
                                 _ptr(out.charged), _ptr(out.remaining), _ptr(out.reset_at_ns), _ptr(out.tokens))
        if check and rc != RL_OK:
            raise EngineError(rc, self.last_error())
        out.status = rc
        return out

    def charge_device(self, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, charged_p, rem_p, reset_p, tok_p=None,
                      stream=None):
        rc = lib.rl_charge_batch_device(self.h, m, key_p, ts_p, n_p, cfg_p, sms_p, dec_p, charged_p, rem_p, reset_p,
                                        tok_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def charge_max(self) -> int:
        return lib.rl_charge_max(self.h)

    def allow_all_settle(self, m, first_p, cfg_p, n_p, dec_p, verdict_p, g_p, sel_p, stream=None):
        """rl_allow_all_settle_device (include/rl_route.h): the sender's settle
        of a routed AllowAll on the unpacked decisions (RL_DROPPED included) ->
        verdict, give-back g and selection sel; device pointers, one kernel on
        `stream`"""
        rc = lib.rl_allow_all_settle_device(self.h, m, first_p, cfg_p, n_p, dec_p, verdict_p, g_p, sel_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def tally_enable(self, key_slots=0):
        """rl_tally_enable: allocate the usage tally (key_slots: records of
        the throttled-key table, 0 = 65536)"""
        o = rl_tally_opts(key_slots=key_slots)
        rc = lib.rl_tally_enable(self.h, C.byref(o))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def tally(self, key, cfg, n, decision):
        """rl_tally_batch: count one finished batch (host arrays, synchronous)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.int64)
        decision = np.ascontiguousarray(decision, dtype=np.uint8)
        m = key.size
        assert cfg.size == m and n.size == m and decision.size == m
        rc = lib.rl_tally_batch(self.h, m, _ptr(key), _ptr(cfg), _ptr(n), _ptr(decision))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def tally_device(self, m, key_p, cfg_p, n_p, dec_p, stream=None):
        """rl_tally_batch_device: the same with device pointers, enqueued on `stream`"""
        rc = lib.rl_tally_batch_device(self.h, m, key_p, cfg_p, n_p, dec_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def tally_read(self, top=0, clear=False) -> Tally:
        """rl_tally_read: every config's counters and the `top` most denied
        tracked keys; clear: zero everything afterwards"""
        ncfg, tracked, info = C.c_uint32(), C.c_uint64(), rl_tally_info()
        rc = lib.rl_tally_read(self.h, None, 0, C.byref(ncfg), None, 0, None, None, 0)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        cfg = np.zeros(ncfg.value, TALLY_CFG)
        keys = np.zeros(top, TALLY_KEY)
        routed = self.tally_routed_read()
        rc = lib.rl_tally_read(self.h, _ptr(cfg), cfg.size, C.byref(ncfg), _ptr(keys), top, C.byref(tracked),
                               C.byref(info), 1 if clear else 0)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return Tally(cfg, keys[:min(top, tracked.value)], tracked.value, info, routed)

    def hot_enable(self, hot_min, width=0, key_slots=0, weight=HOT_REQUESTS):
        """rl_hot_enable: allocate the top-keys sketch (width counters per row,
        0 = 1 << 18) and candidate table (key_slots records, 0 = 65536); a key
        whose estimate reaches hot_min becomes a candidate"""
        o = rl_hot_opts(width=width, key_slots=key_slots, weight=weight, hot_min=hot_min)
        rc = lib.rl_hot_enable(self.h, C.byref(o))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def hot_batch(self, key, cfg, n, decision):
        """rl_hot_batch: count one finished batch (host arrays, synchronous)"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        n = np.ascontiguousarray(n, dtype=np.int64)
        decision = np.ascontiguousarray(decision, dtype=np.uint8)
        m = key.size
        assert cfg.size == m and n.size == m and decision.size == m
        rc = lib.rl_hot_batch(self.h, m, _ptr(key), _ptr(cfg), _ptr(n), _ptr(decision))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def hot_batch_device(self, m, key_p, cfg_p, n_p, dec_p, stream=None):
        """rl_hot_batch_device: the same with device pointers, enqueued on `stream`"""
        rc = lib.rl_hot_batch_device(self.h, m, key_p, cfg_p, n_p, dec_p, stream)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())

    def hot_read(self, top=0, clear=False) -> Hot:
        """rl_hot_read: the `top` candidates with the largest estimates, read
        from the sketch as it is now; clear: zero everything afterwards"""
        tracked, info = C.c_uint64(), rl_hot_info()
        keys = np.zeros(top, HOT_KEY)
        rc = lib.rl_hot_read(self.h, _ptr(keys) if top else None, top, C.byref(tracked), C.byref(info),
                             1 if clear else 0)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return Hot(keys[:min(top, tracked.value)], tracked.value, info)

    def stats(self) -> rl_stats:
        s = rl_stats()
        lib.rl_engine_stats(self.h, C.byref(s))
        return s

    def debug_stamps(self) -> np.ndarray | None:
        """RL_STAMP_KERNELS=1 diagnostics: [256, 6] realtime (10 ns) stamps per
        batch slot (front start/end, replay start/end, finish start/end)"""
        out = np.zeros(6 * 256, np.uint32)
        if lib.rl_engine_debug_stamps(self.h, _ptr(out), out.size) != 0:
            return None
        return out.reshape(256, 6)

    def debug_words(self, n=88) -> np.ndarray:
        out = np.zeros(n, np.uint32)
        lib.rl_engine_debug_words(self.h, _ptr(out), n)
        return out

    def table_info(self, now_ms: int) -> rl_table_info:
        out = rl_table_info()
        rc = lib.rl_table_info_get(self.h, now_ms, C.byref(out))
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return out

    def table_gc(self, now_ms: int, tb_capacity=0, win_capacity=0, check=True):
        out = rl_table_info()
        rc = lib.rl_table_gc(self.h, now_ms, tb_capacity, win_capacity, C.byref(out))
        if check and rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return rc, out

    def snapshot(self, now_ms: int, world=1, rank=0) -> np.ndarray:
        """rl_snapshot_export (include/rl_snapshot.h): the keys live at now_ms
        that `rank` of `world` owns, as a uint8 blob (a size query, then the
        export into a buffer of that size)"""
        return _snapshot(lambda buf, cap, out: lib.rl_snapshot_export(self.h, now_ms, world, rank, buf, cap, out),
                         self.last_error)

    def restore(self, blob, now_ms: int, tb_capacity=0, win_capacity=0, check=True):
        """rl_snapshot_import: GC at now_ms plus a merge of the blob's keys"""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        out = rl_table_info()
        rc = lib.rl_snapshot_import(self.h, _ptr(blob), blob.size, now_ms, tb_capacity, win_capacity, C.byref(out))
        if check and rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return rc, out

    def set_timing(self, level):
        """0 off, 1 replay events only, 2 every stage (True == 2), -k replay
        events on every k-th batch only (timed runs: each event pair costs the
        replay stream ~10 us)"""
        lib.rl_engine_set_timing(self.h, 2 if level is True else int(level))

    def stage_times(self):
        ms = np.zeros(5, np.float64)
        nb = C.c_uint64()
        lib.rl_engine_stage_times(self.h, _ptr(ms), 5, C.byref(nb))
        return ms, nb.value

    def q14_device(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        rc = lib.rl_selftest_q14_device(self.h, _ptr(x), _ptr(out), x.size)
        if rc != RL_OK:
            raise EngineError(rc, self.last_error())
        return out


def _snapshot(export, last_error) -> np.ndarray:
    """size query, then the export; `export(buf, cap, out)` is rl_snapshot_export
    or rl_coalescer_snapshot with the leading arguments bound"""
    info = rl_snapshot_info()
    rc = export(None, 0, C.byref(info))
    if rc != RL_OK:
        raise EngineError(rc, last_error())
    blob = np.zeros(info.bytes, np.uint8)
    rc = export(_ptr(blob), blob.size, C.byref(info))
    if rc != RL_OK:
        raise EngineError(rc, last_error())
    return blob[:info.bytes]


def snapshot_inspect(blob):
    """rl_snapshot_inspect: (rc, rl_snapshot_info) of a blob, checked on the
    host (no GPU)"""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    info = rl_snapshot_info()
    rc = lib.rl_snapshot_inspect(_ptr(blob), blob.size, C.byref(info))
    return rc, info


_DEDICATED_STREAMS = []   # rl_stream_create_dedicated handles (release_dedicated_streams)


def release_dedicated_streams():
    """destroy every Router.dedicated_stream: call once nothing uses them any
    more (pipelines and their tensors dropped); synchronizes the device and
    empties torch's allocator cache first, whose blocks may carry events on
    those streams"""
    import gc

    import torch
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    while _DEDICATED_STREAMS:
        lib.rl_stream_destroy(_DEDICATED_STREAMS.pop())


# rl_route.h
RL_EOVERFLOW = -75
DROPPED = 4
SLOT_DROPPED = 0xffffffff
SLOT_SKIPPED = 0xfffffffe


class Router:
    """rl_router (include/rl_route.h): the routing kernels of one rank.  All
    arguments are device pointers (ints) and a hipStream_t; asynchronous.
    `cap`: records per peer bucket (rounded up: self.capacity)."""

    def __init__(self, device, world, max_batch, cap):
        h = vp()
        rc = lib.rl_router_create(device, world, max_batch, cap, C.byref(h))
        if rc != RL_OK:
            raise EngineError(rc, "rl_router_create failed")
        self.h = h
        self.world = world
        self.device = device
        self.capacity = lib.rl_router_capacity(h)

    def _chk(self, rc, what):
        if rc != RL_OK:
            raise EngineError(rc, what)

    def dedicated_stream(self):
        """a torch stream on a hardware queue of its own
        (rl_stream_create_dedicated)"""
        import torch
        h = vp()
        self._chk(lib.rl_stream_create_dedicated(self.device, C.byref(h)), "rl_stream_create_dedicated")
        # kept for the life of the process: torch's allocator and process
        # groups may still hold events on them after the router is closed
        _DEDICATED_STREAMS.append(h)
        return torch.cuda.ExternalStream(h.value, device=torch.device("cuda", self.device))

    def owner(self, m, key, owner, stream):
        self._chk(lib.rl_route_owner(self.h, m, key, owner, stream), "rl_route_owner")

    def pack(self, m, key, ts, n, cfg, send, send_info, slot, stream):
        self._chk(lib.rl_route_pack(self.h, m, key, ts, n, cfg, send, send_info, slot, stream), "rl_route_pack")

    def pack_sel(self, m, key, ts, n, cfg, sel, send, send_info, slot, stream):
        """rl_route_pack_sel: pack() of the requests with sel[i] != 0; the
        others get slot RL_SLOT_SKIPPED"""
        self._chk(lib.rl_route_pack_sel(self.h, m, key, ts, n, cfg, sel, send, send_info, slot, stream),
                  "rl_route_pack_sel")

    def merge(self, recv, recv_info, order, sms, count, stream):
        self._chk(lib.rl_route_merge(self.h, recv, recv_info, order, sms, count, stream), "rl_route_merge")

    def unpack(self, m, slot, back, dec, rem, retry, reset, stream):
        self._chk(lib.rl_route_unpack(self.h, m, slot, back, dec, rem, retry, reset, stream), "rl_route_unpack")

    def sync(self, stream=None) -> int:
        return lib.rl_router_sync(self.h, stream)

    def close(self):
        if self.h:
            lib.rl_router_destroy(self.h)
            self.h = None


    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --- host mirror of the Go API (include/rl_limiter.h) ------------------------

def pack_keys(keys) -> tuple[np.ndarray, np.ndarray]:
    """Concatenate raw keys (bytes / str) into (bytes u8, offsets u64[m+1])."""
    bs = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return np.frombuffer(b"".join(bs), dtype=np.uint8).copy(), off


def hash_keys(keys_or_packed, seed: int, prefix: bytes | str = b"", device=0, check=True) -> np.ndarray:
    """On-GPU FormatKey + XXH64 (include/rl_keyhash.h): key ids for rl_decide_batch."""
    data, off = keys_or_packed if isinstance(keys_or_packed, tuple) else pack_keys(keys_or_packed)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    pre = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
    m = len(off) - 1
    out = np.zeros(max(m, 0), dtype=np.uint64)
    rc = lib.rl_hash_keys(device, m, _ptr(data), data.size, _ptr(off), seed, pre, len(pre), _ptr(out))
    if check and rc != RL_OK:
        raise EngineError(rc, "rl_hash_keys failed")
    return out if check else (rc, out)


def hash_keys_host(keys_or_packed, seed: int, prefix: bytes | str = b"", cfg=None) -> np.ndarray:
    """rl_hash_keys_host: the raw-key ids on the CPU (cfg: per-key config ids
    mixed into the seed, as rl_decide_batch_keys_device does)."""
    data, off = keys_or_packed if isinstance(keys_or_packed, tuple) else pack_keys(keys_or_packed)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    pre = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
    m = len(off) - 1
    c = None if cfg is None else np.ascontiguousarray(cfg, dtype=np.uint32)
    out = np.zeros(max(m, 0), dtype=np.uint64)
    rc = lib.rl_hash_keys_host(m, _ptr(data), data.size, _ptr(off), seed, _ptr(c), pre, len(pre), _ptr(out))
    if rc != RL_OK:
        raise EngineError(rc, "rl_hash_keys_host failed")
    return out


def config_validate(algorithm, limit, window_ns):
    """Config.Validate(); algorithm None == nil *Config.  Returns '' or the message."""
    buf = C.create_string_buffer(512)
    a = None if algorithm is None else algorithm.encode()
    rc = lib.rll_config_validate(a, limit, window_ns, buf, 512)
    return "" if rc == RLL_OK else buf.value.decode()


def format_key(prefix, key):
    buf = C.create_string_buffer(4096)
    lib.rll_format_key(None if prefix is None else prefix.encode(), key.encode(), buf, 4096)
    return buf.value.decode()


def duration_string(d):
    buf = C.create_string_buffer(64)
    lib.rll_duration_string(d, buf, 64)
    return buf.raw.split(b"\0", 1)[0].decode("utf-8")


@dataclass
class Result:
    Allowed: bool
    Limit: int
    Remaining: int
    RetryAfter: int
    ResetAt: int


@dataclass
class Charge:
    """rll_charge: `charged` of the n units were recorded, `short` were not;
    over_limit: a bucket charged less than n, or a window is over its limit"""
    charged: int
    short: int
    over_limit: bool
    remaining: int
    reset_at_ns: int


class GoError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code
        self.msg = msg


class LimiterEngine:
    """rll_engine: one GPU engine + key interner shared by limiters."""

    def __init__(self, profile=PROFILE_REDIS7, tb_capacity=1 << 16, win_capacity=1 << 16,
                 max_batch=1 << 16, device=0):
        o = rl_opts(device=device, profile=profile, tb_capacity=tb_capacity, win_capacity=win_capacity,
                    max_batch=max_batch)
        h = vp()
        buf = C.create_string_buffer(512)
        rc = lib.rll_engine_new(C.byref(o), C.byref(h), buf, 512)
        if rc != RLL_OK:
            raise GoError(rc, buf.value.decode())
        self.h = h

    def set_server_ms(self, ms):
        lib.rll_engine_set_server_ms(self.h, SMS_DEFAULT if ms is None else ms)

    def keys(self, server_ms):
        """Redis KEYS: the live keys' formatted names, sorted (rll_keys)"""
        n = lib.rll_keys(self.h, server_ms, None, 0)
        if n < 0:
            raise GoError(-n, "rll_keys failed")
        buf = C.create_string_buffer(n + 1)
        lib.rll_keys(self.h, server_ms, buf, n + 1)
        return buf.value.decode().splitlines()

    def close(self):
        if self.h:
            lib.rll_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RateLimiter:
    """Mirror of the reference RateLimiter (interface.go:76-145)."""

    def __init__(self, h):
        self.h = h

    def allow(self, key, now_ns=NOW_WALL, cancelled=False):
        return self.allow_n(key, 1, now_ns, cancelled)

    def allow_n(self, key, n, now_ns=NOW_WALL, cancelled=False):
        """Returns (Result | None, error message | None, code)."""
        r = rll_result()
        buf = C.create_string_buffer(512)
        kb = key.encode()
        rc = lib.rll_allow_n(self.h, kb, len(kb), n, now_ns, 1 if cancelled else 0, C.byref(r), buf, 512)
        if rc == RLL_OK:
            return Result(bool(r.allowed), r.limit, r.remaining, r.retry_after_ns, r.reset_at_ns), None, rc
        return None, buf.value.decode(), rc

    def peek_n(self, key, n=0, now_ns=NOW_WALL, cancelled=False):
        """rll_peek_n: (Result | None, error message | None, code); n == 0 asks
        how much is left, nothing changes"""
        r = rll_result()
        buf = C.create_string_buffer(512)
        kb = key.encode()
        rc = lib.rll_peek_n(self.h, kb, len(kb), n, now_ns, 1 if cancelled else 0, C.byref(r), buf, 512)
        if rc == RLL_OK:
            return Result(bool(r.allowed), r.limit, r.remaining, r.retry_after_ns, r.reset_at_ns), None, rc
        return None, buf.value.decode(), rc

    def batch_allow(self, keys, n, now_ns=None):
        m = len(keys)
        kbs = [k.encode() for k in keys]
        arr = (C.c_char_p * m)(*kbs)
        lens = np.array([len(k) for k in kbs], np.uint64)
        nn = np.ascontiguousarray(n, np.int64)
        now = None if now_ns is None else np.ascontiguousarray(now_ns, np.int64)
        out = (rll_result * m)()
        codes = np.empty(m, np.int32)
        lib.rll_allow_batch(self.h, m, C.cast(arr, vp), _ptr(lens), _ptr(nn), _ptr(now), C.cast(out, vp),
                            _ptr(codes))
        res = [Result(bool(o.allowed), o.limit, o.remaining, o.retry_after_ns, o.reset_at_ns) for o in out]
        return res, codes

    def add_metrics(self):
        """MetricsDecorator (ADR-003) around this limiter, in place."""
        if lib.rll_add_metrics(self.h) != RLL_OK:
            raise GoError(RLL_ERR_ARG, "rll_add_metrics failed")

    def metrics_text(self) -> str:
        n = lib.rll_metrics_expose(self.h, None, 0)
        if n < 0:
            raise GoError(RLL_ERR_ARG, "no metrics decorator")
        buf = C.create_string_buffer(n + 1)
        lib.rll_metrics_expose(self.h, buf, n + 1)
        return buf.value.decode()

    def add_logging(self, capacity=4096):
        """LoggingDecorator (ADR-003): records queue in the library until drained."""
        if lib.rll_add_logging(self.h, capacity) != RLL_OK:
            raise GoError(RLL_ERR_ARG, "rll_add_logging failed")

    def drain_logs(self):
        """-> ([(level, msg, fields)], dropped)"""
        out = []
        dropped = C.c_uint64()
        while True:
            buf = C.create_string_buffer(1 << 16)
            n = lib.rll_log_drain(self.h, buf, 1 << 16, C.byref(dropped))
            if n < 0:
                raise GoError(RLL_ERR_ARG, "no logging decorator")
            for line in buf.value.decode().splitlines():
                lv, msg, fields = line.split("\t", 2)
                out.append((int(lv), msg, fields))
            if n == 0:
                return out, dropped.value

    def reset(self, key, now_ns=NOW_WALL):
        buf = C.create_string_buffer(512)
        kb = key.encode()
        rc = lib.rll_reset(self.h, kb, len(kb), now_ns, buf, 512)
        return None if rc == RLL_OK else buf.value.decode()

    def reset_many(self, keys, now_ns=NOW_WALL):
        """rll_reset_many: Reset of every key, one engine launch -> error
        message | None"""
        m = len(keys)
        kbs = [k.encode() for k in keys]
        arr = (C.c_char_p * m)(*kbs)
        lens = np.array([len(k) for k in kbs], np.uint64)
        buf = C.create_string_buffer(512)
        rc = lib.rll_reset_many(self.h, m, C.cast(arr, vp), _ptr(lens), now_ns, buf, 512)
        return None if rc == RLL_OK else buf.value.decode()

    def refund_n(self, key, n=1, now_ns=NOW_WALL, at_ns=0):
        """rll_refund_n: give n units back to `key`; at_ns picks the window (0
        = now) -> (applied | None, error message | None, code)"""
        buf = C.create_string_buffer(512)
        kb = key.encode()
        applied = C.c_uint8(0)
        rc = lib.rll_refund_n(self.h, kb, len(kb), n, now_ns, at_ns, C.byref(applied), buf, 512)
        if rc == RLL_OK:
            return bool(applied.value), None, rc
        return None, buf.value.decode(), rc

    def refund_many(self, keys, n, at_ns=None, now_ns=NOW_WALL):
        """rll_refund_many: m refunds as one engine call (refunds of one key
        and window are summed) -> (applied [bool] | None, error message |
        None, code)"""
        m = len(keys)
        kbs = [k.encode() for k in keys]
        arr = (C.c_char_p * m)(*kbs)
        lens = np.array([len(k) for k in kbs], np.uint64)
        nn = np.ascontiguousarray(n, np.int64)
        at = None if at_ns is None else np.ascontiguousarray(at_ns, np.int64)
        assert nn.size == m and (at is None or at.size == m)
        applied = np.zeros(m, np.uint8)
        buf = C.create_string_buffer(512)
        rc = lib.rll_refund_many(self.h, m, C.cast(arr, vp), _ptr(lens), _ptr(nn), _ptr(at), now_ns, _ptr(applied),
                                 buf, 512)
        if rc == RLL_OK:
            return applied.astype(bool), None, rc
        return None, buf.value.decode(), rc

    def charge_n(self, key, n=1, now_ns=NOW_WALL, cancelled=False):
        """rll_charge_n: record n units of usage after the fact -> (Charge |
        None, error message | None, code)"""
        got, err, rc = self.charge_many([key], [n], now_ns, cancelled)
        return (got[0] if got else None), err, rc

    def charge_many(self, keys, n, now_ns=NOW_WALL, cancelled=False):
        """rll_charge_many: m charges in ONE engine call, all at now_ns ->
        ([Charge] | None, error message | None, code)"""
        m = len(keys)
        kbs = [k.encode() for k in keys]
        arr = (C.c_char_p * m)(*kbs)
        lens = np.array([len(k) for k in kbs], np.uint64)
        nn = np.ascontiguousarray(n, np.int64)
        assert nn.size == m
        out = (rll_charge * max(m, 1))()
        buf = C.create_string_buffer(512)
        rc = lib.rll_charge_many(self.h, m, C.cast(arr, vp), _ptr(lens), _ptr(nn), now_ns, 1 if cancelled else 0,
                                 C.cast(out, vp), buf, 512)
        if rc != RLL_OK:
            return None, buf.value.decode(), rc
        return [Charge(o.charged, o.short_by, bool(o.over_limit), o.remaining, o.reset_at_unix_ns)
                for o in out[:m]], None, rc

    @staticmethod
    def allow_all(checks, now_ns=NOW_WALL, cancelled=False):
        """rll_allow_all: one request against several limiters of one
        LimiterEngine, all or nothing.  checks: [(limiter, key, n)], 1 to 16.
        -> (allowed, [Result], denied_by, None, RLL_OK), or (None, None, None,
        error message, code)"""
        k = len(checks)
        hs = (vp * max(k, 1))(*[c[0].h for c in checks])
        kbs = [c[1].encode() for c in checks]
        arr = (C.c_char_p * max(k, 1))(*kbs)
        lens = np.array([len(b) for b in kbs], np.uint64)
        nn = np.array([c[2] for c in checks], np.int64)
        res = (rll_result * max(k, 1))()
        ok, by = C.c_uint8(), C.c_int32(-1)
        buf = C.create_string_buffer(512)
        rc = lib.rll_allow_all(C.cast(hs, vp), k, C.cast(arr, vp), _ptr(lens), _ptr(nn), now_ns, 1 if cancelled else 0,
                               C.cast(res, vp), C.byref(ok), C.byref(by), buf, 512)
        if rc != RLL_OK:
            return None, None, None, buf.value.decode(), rc
        out = [Result(bool(r.allowed), r.limit, r.remaining, r.retry_after_ns, r.reset_at_ns) for r in res[:k]]
        return bool(ok.value), out, by.value, None, rc

    def close(self):
        lib.rll_close(self.h)

    def __del__(self):
        try:
            lib.rll_free(self.h)
        except Exception:
            pass


def new_limiter(engine: LimiterEngine | None, algorithm, limit, window_ns, prefix="", fail_open=False,
                config_nil=False):
    """NewTokenBucket/NewSlidingWindow/NewFixedWindow by name; raises GoError like the constructor."""
    h = vp()
    buf = C.create_string_buffer(512)
    rc = lib.rll_new(None if engine is None else engine.h, algorithm.encode(), limit, window_ns,
                     prefix.encode(), 1 if fail_open else 0, 1 if config_nil else 0, C.byref(h), buf, 512)
    if rc != RLL_OK:
        raise GoError(rc, buf.value.decode())
    return RateLimiter(h)


RL_EAGAIN, RL_ECLOSED, RL_EDEADLINE, RL_ECANCELED = -11, -32, -62, -125


def now_ns() -> int:
    """the coalescer's deadline clock (rl_coalescer_now_ns: CLOCK_MONOTONIC)"""
    return lib.rl_coalescer_now_ns()


class Coalescer:
    """rl_coalescer (include/rl_coalescer.h): concurrent submissions gathered
    into engine batches.  `engine` is an Engine (GPU) or, for the CPU tests of
    the batching logic, a Python function with rl_decide_batch's host-array
    signature (the test seam rl_coalescer_create_with_host_backend; `reset`,
    `table_info`, `gc`, `peek`, `reset_batch`, `refund`, `allow_all`, `charge`: the
    other backend functions, optional).

    gc_interval_ns > 0 turns on the automatic table GC (rl_coalescer_opts);
    tally_key_slots the usage tally; hot_min (with hot_width, hot_key_slots,
    hot_weight) the top keys."""

    def __init__(self, engine, max_batch=65536, max_in_flight=3, linger_ns=0, queue_cap=0, reset=None,
                 table_info=None, gc=None, peek=None, gc_interval_ns=0, gc_high_pct=0, gc_margin_ms=0,
                 gc_max_tb_capacity=0, gc_max_win_capacity=0, reset_batch=None, tally_key_slots=0, hot_min=0,
                 hot_width=0, hot_key_slots=0, hot_weight=HOT_REQUESTS, refund=None, allow_all=None, charge=None):
        o = rl_coalescer_opts_hot(hot_min=hot_min, hot_width=hot_width, hot_key_slots=hot_key_slots, hot_weight=hot_weight,
                              max_batch=max_batch, max_in_flight=max_in_flight, gc_high_pct=gc_high_pct,
                              linger_ns=linger_ns, queue_cap=queue_cap, gc_interval_ns=gc_interval_ns,
                              gc_margin_ms=gc_margin_ms, gc_max_tb_capacity=gc_max_tb_capacity,
                              gc_max_win_capacity=gc_max_win_capacity, tally_key_slots=tally_key_slots)
        h = vp()
        if isinstance(engine, Engine):
            rc = lib.rl_coalescer_create(engine.h, C.byref(o), C.byref(h))
            self._be = None
        else:
            # the callbacks live as long as the coalescer
            self._be = (rl_coalescer_backend_charge if charge else rl_coalescer_backend)(
                **({"charge": CHARGE_FN(charge)} if charge else {}),
                batch=BATCH_FN(engine), reset=RESET_FN(reset) if reset else C.cast(None, RESET_FN),
                table_info=INFO_FN(table_info) if table_info else C.cast(None, INFO_FN),
                gc=GC_FN(gc) if gc else C.cast(None, GC_FN), user=None,
                peek=BATCH_FN(peek) if peek else C.cast(None, BATCH_FN),
                reset_batch=RESET_BATCH_FN(reset_batch) if reset_batch else C.cast(None, RESET_BATCH_FN),
                refund=REFUND_FN(refund) if refund else C.cast(None, REFUND_FN),
                allow_all=ALLOW_ALL_FN(allow_all) if allow_all else C.cast(None, ALLOW_ALL_FN))
            rc = lib.rl_coalescer_create_with_host_backend(C.byref(self._be), C.byref(o), C.byref(h))
        if rc != RL_OK:
            raise EngineError(rc, "rl_coalescer_create failed")
        self.h = h

    def submit(self, key, ts, n, cfg, deadline_ns=0) -> int:
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        t = C.c_uint64()
        rc = lib.rl_coalescer_submit_deadline(self.h, key.size, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg),
                                              deadline_ns, C.byref(t))
        if rc != RL_OK:
            raise EngineError(rc, "rl_coalescer_submit failed")
        return t.value

    def wait(self, ticket: int, m: int, timeout_ns=-1, out=None):
        if out is None:
            out = (np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64))
        rc = lib.rl_coalescer_wait(self.h, ticket, timeout_ns, *[_ptr(x) for x in out])
        return rc, out

    def cancel(self, ticket: int) -> int:
        return lib.rl_coalescer_cancel(self.h, ticket)

    def decide(self, key, ts, n, cfg, deadline_ns=0):
        d, rem, retry, reset = C.c_uint8(), C.c_int64(), C.c_int64(), C.c_int64()
        rc = lib.rl_coalescer_decide_deadline(self.h, key, ts, n, cfg, deadline_ns, C.byref(d), C.byref(rem),
                                              C.byref(retry), C.byref(reset))
        return rc, (d.value, rem.value, retry.value, reset.value)

    def reset(self, key, ts, cfg) -> int:
        return lib.rl_coalescer_reset(self.h, key, ts, cfg)

    def reset_batch(self, key, ts, cfg):
        """rl_coalescer_reset_batch: m resets as one submission in sequence
        order; blocks until applied.  -> (rc, status): RESET_DONE or INVALID
        per request"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        assert ts.size == key.size and cfg.size == key.size
        status = np.empty(key.size, np.uint8)
        rc = lib.rl_coalescer_reset_batch(self.h, key.size, _ptr(key), _ptr(ts), _ptr(cfg), _ptr(status))
        return rc, status

    def refund(self, key, ts, n, cfg):
        """rl_coalescer_refund: one refund call as one submission in sequence
        order, one launch, never merged or split; blocks until applied.
        -> (rc, status): REFUND_DONE, REFUND_NOKEY or INVALID per request"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        assert ts.size == key.size and n.size == key.size and cfg.size == key.size
        status = np.empty(key.size, np.uint8)
        rc = lib.rl_coalescer_refund(self.h, key.size, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(status))
        return rc, status

    def allow_all(self, key, ts, n, cfg, first, deadline_ns=0):
        """rl_coalescer_allow_all: one AllowAll call (member i starts a group
        when i == 0 or first[i] != 0) as one submission in sequence order, one
        launch, never merged or split; blocks until applied.  -> (rc,
        (decision, remaining, retry_after_ns, reset_at_ns, verdict))"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        first = np.ascontiguousarray(first, dtype=np.uint8)
        m = key.size
        assert ts.size == m and n.size == m and cfg.size == m and first.size == m
        out = (np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64),
               np.empty(m, np.uint8))
        rc = lib.rl_coalescer_allow_all(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), _ptr(first), deadline_ns,
                                        *[_ptr(x) for x in out])
        return rc, out

    def charge(self, key, ts, n, cfg, deadline_ns=0):
        """rl_coalescer_charge: one Charge call as one submission in sequence
        order, one launch, never merged or split; blocks until applied.
        -> (rc, (decision, charged, remaining, reset_at_ns))"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        m = key.size
        assert ts.size == m and n.size == m and cfg.size == m
        out = (np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64))
        rc = lib.rl_coalescer_charge(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), deadline_ns,
                                     *[_ptr(x) for x in out])
        return rc, out

    def peek(self, key, ts, n, cfg):
        """rl_coalescer_peek: read-only queries in sequence order; blocks.
        -> (rc, (decision, remaining, retry_after_ns, reset_at_ns))"""
        key = np.ascontiguousarray(key, dtype=np.uint64)
        ts = np.ascontiguousarray(ts, dtype=np.int64)
        n = np.ascontiguousarray(n, dtype=np.int64)
        cfg = np.ascontiguousarray(cfg, dtype=np.uint32)
        m = key.size
        out = (np.empty(m, np.uint8), np.empty(m, np.int64), np.empty(m, np.int64), np.empty(m, np.int64))
        rc = lib.rl_coalescer_peek(self.h, m, _ptr(key), _ptr(ts), _ptr(n), _ptr(cfg), *[_ptr(x) for x in out])
        return rc, out

    def table_info(self, now_ms):
        out = rl_table_info()
        rc = lib.rl_coalescer_table_info(self.h, now_ms, C.byref(out))
        return rc, out

    def gc(self, now_ms, tb_capacity=0, win_capacity=0):
        out = rl_table_info()
        rc = lib.rl_coalescer_gc(self.h, now_ms, tb_capacity, win_capacity, C.byref(out))
        return rc, out

    def snapshot(self, now_ms, world=1, rank=0) -> np.ndarray:
        """rl_coalescer_snapshot: a size query, then the export, each in
        sequence order (requests submitted in between can outgrow the buffer:
        RL_ENOMEM)"""
        return _snapshot(lambda buf, cap, out: lib.rl_coalescer_snapshot(self.h, now_ms, world, rank, buf, cap, out),
                         lambda: "rl_coalescer_snapshot failed")

    def restore(self, blob, now_ms, tb_capacity=0, win_capacity=0):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        out = rl_table_info()
        rc = lib.rl_coalescer_restore(self.h, _ptr(blob), blob.size, now_ms, tb_capacity, win_capacity, C.byref(out))
        return rc, out

    def tally(self, top=0, clear=False, max_configs=1024):
        """rl_coalescer_tally: the usage tally in sequence order -- every
        request submitted before the call is counted, none submitted after.
        -> (rc, Tally); tally_key_slots=0 at creation: RL_EINVAL"""
        ncfg, tracked, info = C.c_uint32(), C.c_uint64(), rl_tally_info()
        # one call, one point of the sequence: room for max_configs rows
        cfg = np.zeros(max_configs, TALLY_CFG)
        keys = np.zeros(top, TALLY_KEY)
        rc = lib.rl_coalescer_tally(self.h, _ptr(cfg), cfg.size, C.byref(ncfg), _ptr(keys), top, C.byref(tracked),
                                    C.byref(info), 1 if clear else 0)
        if rc != RL_OK:
            return rc, None
        # rows of config ids >= max_configs are not returned (as rl_tally_read's cfg_cap)
        return rc, Tally(cfg[:min(ncfg.value, cfg.size)], keys[:min(top, tracked.value)], tracked.value, info)

    def hot(self, top=0, clear=False):
        """rl_coalescer_hot: the top keys in sequence order -- every request
        submitted before the call is counted, none submitted after.
        -> (rc, Hot); hot_min=0 at creation: RL_EINVAL"""
        tracked, info = C.c_uint64(), rl_hot_info()
        keys = np.zeros(top, HOT_KEY)
        rc = lib.rl_coalescer_hot(self.h, _ptr(keys) if top else None, top, C.byref(tracked), C.byref(info),
                                  1 if clear else 0)
        if rc != RL_OK:
            return rc, None
        return rc, Hot(keys[:min(top, tracked.value)], tracked.value, info)

    def stats(self) -> rl_coalescer_stats:
        st = rl_coalescer_stats()
        lib.rl_coalescer_get_stats(self.h, C.byref(st))
        return st

    def stats_charge(self) -> rl_coalescer_stats_charge:
        """rl_coalescer_get_stats_charge: the same counters and charge_launches"""
        st = rl_coalescer_stats_charge()
        lib.rl_coalescer_get_stats_charge(self.h, C.byref(st))
        return st

    def close(self):
        if self.h:
            lib.rl_coalescer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --- the native gRPC front end (include/rl_grpc.h, lib/librl_grpc.so) ----------
GRPC_LIB_PATH = os.environ.get("RL_GRPC_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "librl_grpc.so")
_grpc_lib = None


def grpc_lib():
    global _grpc_lib
    if _grpc_lib is None:
        if not os.path.exists(GRPC_LIB_PATH):
            raise ImportError(f"native gRPC server not built: {GRPC_LIB_PATH} (make -C distributed-rate-limiter_amd)")
        _grpc_lib = C.CDLL(GRPC_LIB_PATH)
        _grpc_lib.rl_grpc_server_start.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(vp)]
        _grpc_lib.rl_grpc_server_shutdown.argtypes = [vp, C.c_int64]
        _grpc_lib.rl_grpc_server_destroy.argtypes = [vp]
        _grpc_lib.rl_grpc_server_port.argtypes = [vp]
        _grpc_lib.rl_grpc_server_get_stats.argtypes = [vp, C.c_void_p]
    return _grpc_lib


class rl_grpc_limiter(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("cfg_id", C.c_uint32), ("name", C.c_char_p), ("algorithm", C.c_int32),
                ("fail_open", C.c_int32), ("limit", C.c_int64), ("window_ns", C.c_int64), ("prefix", C.c_char_p)]


class rl_grpc_opts(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("io_threads", C.c_uint32), ("host", C.c_char_p), ("port", C.c_int32),
                ("isolate", C.c_int32), ("clock_start_ns", C.c_int64), ("clock_step_ns", C.c_int64),
                ("tally", C.c_int32), ("names_cap", C.c_uint32)]


class rl_grpc_stats(_Sized):
    _fields_ = [("struct_size", C.c_uint32), ("pad_", C.c_uint32), ("connections", C.c_uint64), ("rpcs", C.c_uint64),
                ("decisions", C.c_uint64), ("errors", C.c_uint64), ("cancelled", C.c_uint64)]


class GrpcServer:
    """rl_grpc_server (include/rl_grpc.h): the rate limiter service served by
    native event loops over `coalescer`.  limiters: (name, cfg_id, algorithm,
    limit, window_ns, prefix, fail_open) tuples, already registered.  tally:
    serve RateLimiterMetrics.Usage (the coalescer was created with
    tally_key_slots) and remember the names of the last names_cap (0 = 4096)
    keys a denied response went out for.  With
    clock_step_ns != 0 the server's time.Now() is the test clock
    clock_start_ns + k * clock_step_ns on its k-th read."""

    def __init__(self, coalescer, limiters, host="127.0.0.1", port=0, io_threads=4, isolate=False,
                 clock_start_ns=0, clock_step_ns=0, tally=False, names_cap=0):
        L = grpc_lib()
        self._lims = (rl_grpc_limiter * max(1, len(limiters)))()
        for i, (name, cfg, alg, limit, window, prefix, fail_open) in enumerate(limiters):
            self._lims[i] = rl_grpc_limiter(cfg_id=cfg, name=name.encode(), algorithm=alg, fail_open=int(fail_open),
                                            limit=limit, window_ns=window,
                                            prefix=prefix if isinstance(prefix, bytes) else prefix.encode())
        self._opts = rl_grpc_opts(io_threads=io_threads, host=host.encode(), port=port, isolate=int(isolate),
                                  clock_start_ns=clock_start_ns, clock_step_ns=clock_step_ns, tally=int(tally),
                                  names_cap=names_cap)
        self.co = coalescer
        h = vp()
        rc = L.rl_grpc_server_start(coalescer.h, C.cast(self._lims, C.c_void_p), len(limiters),
                                    C.cast(C.pointer(self._opts), C.c_void_p), C.byref(h))
        if rc != RL_OK:
            raise EngineError(rc, "rl_grpc_server_start failed")
        self.h = h
        self.port = L.rl_grpc_server_port(h)

    def stats(self) -> rl_grpc_stats:
        st = rl_grpc_stats()
        grpc_lib().rl_grpc_server_get_stats(self.h, C.byref(st))
        return st

    def shutdown(self, grace_s=5.0):
        if self.h:
            grpc_lib().rl_grpc_server_shutdown(self.h, int(grace_s * 1e9))

    def close(self):
        if self.h:
            grpc_lib().rl_grpc_server_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
