"""ctypes binding of the C ABI (include/dint_abi.h) exported by dint_amd/libdint.so.

There is deliberately no fallback: if the HIP extension is missing or fails to load,
importing the engine raises -- the product path never runs on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DINT_LIB_PATH") or os.path.join(HERE, "libdint.so")  # (DINT_LIB_PATH: same-box A/B runs of two builds, tools/)

ABI_VERSION = 5
#: dint_config.flags (include/dint_abi.h)
FLAG_KV_ROUNDS, FLAG_COPY_STREAMS, FLAG_LOCK_SAME_KEY, FLAG_KV_NO_HOT, FLAG_INPUTS_READY = 1, 2, 4, 8, 16
#: a shard of a replica set: takes routed records in state_repair / state_diff / log_apply_device / log_apply_folded
FLAG_SHARD_REPLICA = 32
#: records per workgroup of dint_records_route's kernels (csrc/state_route.h RR_TILE; dint_records_route_tile() says the same)
ROUTE_TILE = 512
#: shards dint_records_route takes at most
ROUTE_MAX_SHARDS = 255
MICRO_BATCH = 65536

#: every symbol include/dint_abi.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "dint_engine_create", "dint_engine_destroy", "dint_msg_size", "dint_last_error", "dint_submit",
    "dint_submit_device", "dint_sync", "dint_load_rows", "dint_populate", "dint_hash_size", "dint_dump_rows",
    "dint_read_locks", "dint_read_log", "dint_get_stats", "dint_reset", "dint_snapshot", "dint_restore",
    "dint_home_shard", "dint_bench_rand64", "dint_timing_enable", "dint_timing_read", "dint_kv_trace_read",
    "dint_submit_async", "dint_wait", "dint_alloc_pinned", "dint_free_pinned", "dint_engine_stream", "dint_max_pass",
    "dint_stream_wait", "dint_stream_signal", "dint_route_pack", "dint_route_unpack", "dint_submit_segments",
    "dint_log_drain", "dint_refuse", "dint_route_pack_multi", "dint_route_unpack_multi", "dint_bench_access", "dint_selftest",
    "dint_submit_segments_multi", "dint_submit_device_ahead", "dint_submit_segments_multi_ahead",
    "dint_log_drain_device", "dint_log_apply_device", "dint_log_apply_folded_device", "dint_state_digest", "dint_state_diff", "dint_state_repair",
    "dint_state_export", "dint_state_import", "dint_state_rehash", "dint_state_stats",
    "dint_load_rows_device", "dint_populate_device",
    "dint_state_verify", "dint_state_compact",
    "dint_state_block_digest", "dint_state_block_select", "dint_state_block_rows", "dint_state_block_diff",
    "dint_records_route", "dint_traffic_report",
    "dint_state_locks", "dint_state_unlock",
]
#: dint_traffic_report: requests / list entries a call takes at most
TRAFFIC_MAX_N = 1 << 24
TRAFFIC_MAX_TOP = 4096
#: dint_log_apply_folded_device flags
FOLD_DRY_RUN = 1
#: dint_state_rehash flags
REHASH_DROP_LOCKS = 1
#: dint_state_verify flags
VERIFY_RECLAIM = 1
#: dint_state_compact flags
COMPACT_DRY_RUN = 1
#: dint_state_unlock flags
UNLOCK_ALL = 1
UNLOCK_DRY_RUN = 2
#: dint_lock_record.flags
LOCK_KEY_OWNER = 1
LOCK_KEY_ROW = 2
LOCK_WALK_CUT = 4
#: bytes of a table's control block in a TablesView (include/dint_driver.h DINT_VIEW_CTL_BYTES)
VIEW_CTL_BYTES = 1600


class RouteItem(C.Structure):
    """dint_route_item (include/dint_abi.h)"""
    _fields_ = [("engine", C.c_void_p), ("d_reqs", C.c_void_p), ("n", C.c_uint32), ("seg_cap", C.c_uint32),
                ("d_slots", C.c_void_p), ("d_cnt", C.c_void_p), ("d_slot", C.c_void_p), ("d_replies", C.c_void_p),
                ("d_n", C.c_void_p)]


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("workload", C.c_uint32), ("device", C.c_int32), ("flags", C.c_uint32),
        ("n_slots", C.c_uint64), ("n_rows", C.c_uint64), ("log_entries", C.c_uint32),
        ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("max_pass", C.c_uint32),
        ("pool_entries", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("batches", C.c_uint64), ("requests", C.c_uint64), ("bad_requests", C.c_uint64),
        ("missing_keys", C.c_uint64), ("foreign_requests", C.c_uint64), ("pool_exhausted", C.c_uint64),
        ("route_overflow", C.c_uint64), ("big_bin_requests", C.c_uint64), ("late_requests", C.c_uint64),
        ("reserved", C.c_uint64 * 3),
    ]


class ApplyStats(C.Structure):
    """dint_apply_stats (include/dint_abi.h)"""
    _fields_ = [("applied", C.c_uint64), ("commits", C.c_uint64), ("inserts", C.c_uint64), ("deletes", C.c_uint64),
                ("chunks", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class FoldStats(C.Structure):
    """dint_fold_stats (include/dint_abi.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "applied", "commits", "inserts", "deletes", "chunks", "rows", "folded_records", "deferred_records", "deferred_buckets",
        "repair_records", "updated", "inserted", "deleted", "refused")] + [("ns", C.c_uint64 * 4), ("reserved", C.c_uint64 * 5)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k not in ("ns", "reserved")}
        d["stage_ns"] = dict(zip(("sort", "fold", "repair", "deferred"), list(self.ns)))
        return d


class TableDigest(C.Structure):
    """dint_table_digest (include/dint_abi.h)"""
    _fields_ = [("rows", C.c_uint64), ("sum", C.c_uint64), ("xr", C.c_uint64), ("reserved", C.c_uint64)]


class DiffStats(C.Structure):
    """dint_diff_stats (include/dint_abi.h)"""
    _fields_ = [("total", C.c_uint64), ("only_a", C.c_uint64), ("only_b", C.c_uint64), ("val_differs", C.c_uint64),
                ("ver_only", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class BlockDigest(C.Structure):
    """dint_block_digest (include/dint_abi.h)"""
    _fields_ = [("rows", C.c_uint64), ("sum", C.c_uint64), ("xr", C.c_uint64), ("reserved", C.c_uint64)]


class BlockStats(C.Structure):
    """dint_block_stats (include/dint_abi.h)"""
    _fields_ = [("total", C.c_uint64), ("n_blocks", C.c_uint32), ("n_tables", C.c_uint32), ("blocks", C.c_uint32 * 5),
                ("block_buckets", C.c_uint32), ("reserved", C.c_uint64 * 3)]

    def as_dict(self) -> dict:
        return {"total": self.total, "n_blocks": self.n_blocks, "block_buckets": self.block_buckets,
                "blocks": list(self.blocks)[:self.n_tables]}


class RepairStats(C.Structure):
    """dint_repair_stats (include/dint_abi.h)"""
    _fields_ = [("applied", C.c_uint64), ("updated", C.c_uint64), ("inserted", C.c_uint64), ("deleted", C.c_uint64),
                ("refused", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class ImageStats(C.Structure):
    """dint_image_stats (include/dint_abi.h)"""
    _fields_ = [("bytes", C.c_uint64), ("buckets", C.c_uint64), ("overflow_entries", C.c_uint64), ("rows", C.c_uint64),
                ("reserved", C.c_uint64 * 4)]


class RehashTableStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("overflow_entries", C.c_uint64), ("longest_chain", C.c_uint64), ("reserved", C.c_uint64)]


class LoadTableStats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("overflow_entries", C.c_uint64), ("longest_chain_entries", C.c_uint64), ("direct", C.c_uint64)]


class LoadStats(C.Structure):
    """dint_load_stats (include/dint_abi.h)"""
    _fields_ = [("rows_loaded", C.c_uint64), ("foreign_rows", C.c_uint64), ("table", LoadTableStats * 5), ("direct", C.c_uint64),
                ("temp_bytes", C.c_uint64), ("stage_ns", C.c_uint64 * 6), ("reserved", C.c_uint64 * 4)]


class RehashStats(C.Structure):
    """dint_rehash_stats (include/dint_abi.h)"""
    _fields_ = [("rows_seen", C.c_uint64), ("rows_placed", C.c_uint64), ("rows_foreign", C.c_uint64), ("locks_held", C.c_uint64),
                ("table", RehashTableStats * 5), ("stage_ns", C.c_uint64 * 5), ("reserved", C.c_uint64 * 3)]


class TableStats(C.Structure):
    """dint_table_stats (include/dint_abi.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "buckets", "buckets_empty", "rows", "entries", "overflow_entries", "holes", "inline_first", "inline_unlinked", "hit_entries",
        "shadowed_rows", "buckets_unchecked", "longest_chain", "longest_chain_bucket", "most_rows", "locks_held", "pool_cap",
        "pool_top")] + [("chain_hist", C.c_uint64 * 17), ("rows_hist", C.c_uint64 * 33), ("reserved", C.c_uint64 * 13)]

    def as_dict(self) -> dict:
        return {k: (list(getattr(self, k)) if k.endswith("_hist") else int(getattr(self, k))) for k, _ in self._fields_ if k != "reserved"}


class TrafficKey(C.Structure):
    """dint_traffic_key (include/dint_abi.h)"""
    _fields_ = [("key", C.c_uint64)] + [(k, C.c_uint32) for k in (
        "table", "requests", "reads", "locks", "unlocks", "writes", "rejects", "misses", "first_index", "reserved")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class TrafficReport(C.Structure):
    """struct dint_traffic_report (include/dint_abi.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "n", "keyed", "bad_table", "log_requests", "reads", "locks", "unlocks", "writes", "others", "rejects", "misses",
        "distinct_keys", "distinct_units", "distinct_lock_slots", "max_key_requests", "max_unit_requests", "max_unit", "max_unit_table",
        "shared_units", "shared_unit_requests", "shared_unit_rejects", "shared_slots", "shared_slot_requests", "shared_slot_rejects",
        "n_by_requests", "n_by_rejects", "temp_bytes")] + [
        ("reserved", C.c_uint64 * 5), ("key_hist", C.c_uint64 * 25), ("unit_hist", C.c_uint64 * 25),
        ("req_types", (C.c_uint64 * 32) * 5), ("rep_types", (C.c_uint64 * 32) * 5)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k not in ("reserved", "key_hist", "unit_hist", "req_types", "rep_types")}
        d["key_hist"], d["unit_hist"] = list(self.key_hist), list(self.unit_hist)
        d["req_types"] = [list(r) for r in self.req_types]
        d["rep_types"] = [list(r) for r in self.rep_types]
        return d


class TableVerify(C.Structure):
    """dint_table_verify (include/dint_abi.h)"""
    _fields_ = [(k, C.c_uint64) for k in (
        "pool_cap", "pool_top", "rows", "linked", "free_entries", "pending_entries", "unaccounted", "longest_list", "bad_chains",
        "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries", "stray_rows", "misplaced_rows", "odd_valid_bytes",
        "reclaimed", "stray_rows_cleared")] + [("reserved", C.c_uint64 * 14)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class TableCompact(C.Structure):
    """dint_table_compact (include/dint_abi.h)"""
    _fields_ = [("verify", TableVerify)] + [(k, C.c_uint64) for k in (
        "rows", "entries_before", "entries_after", "overflow_before", "overflow_after", "pool_top_before", "pool_top_after",
        "holes_before", "holes_after", "buckets_rewritten", "unaccounted_dropped", "staging_bytes")] + [("reserved", C.c_uint64 * 20)]

    def as_dict(self) -> dict:
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k not in ("reserved", "verify")}
        d["verify"] = self.verify.as_dict()
        return d


class LockStats(C.Structure):
    """dint_lock_stats (include/dint_abi.h)"""
    _fields_ = [("total", C.c_uint64), ("held", C.c_uint64 * 5), ("sum_a", C.c_uint64), ("sum_b", C.c_uint64), ("no_row", C.c_uint64),
                ("walk_cut", C.c_uint64), ("reserved", C.c_uint64 * 6)]

    def as_dict(self) -> dict:
        return {"total": int(self.total), "held": list(self.held), "sum_a": int(self.sum_a), "sum_b": int(self.sum_b),
                "no_row": int(self.no_row), "walk_cut": int(self.walk_cut)}


class UnlockStats(C.Structure):
    """dint_unlock_stats (include/dint_abi.h)"""
    _fields_ = [("released", C.c_uint64), ("stale", C.c_uint64), ("released_a", C.c_uint64), ("released_b", C.c_uint64),
                ("per_table", C.c_uint64 * 5), ("reserved", C.c_uint64 * 7)]

    def as_dict(self) -> dict:
        return {"released": int(self.released), "stale": int(self.stale), "released_a": int(self.released_a),
                "released_b": int(self.released_b), "per_table": list(self.per_table)}


class LockGeometry(C.Structure):
    """struct dint_lock_geometry (include/dint_driver.h)"""
    _fields_ = [("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("n_tables", C.c_uint32), ("reserved", C.c_uint32),
                ("size", C.c_uint64 * 5)]


class TableView(C.Structure):
    """dint_table_view (include/dint_driver.h)"""
    _fields_ = [("entries", C.c_void_p), ("n_local", C.c_uint64), ("hash_size", C.c_uint64), ("pool_cap", C.c_uint32),
                ("stride", C.c_uint32), ("val_size", C.c_uint32), ("reserved", C.c_uint32), ("pool_next", C.c_void_p), ("ctl", C.c_void_p)]


class TablesView(C.Structure):
    """dint_tables_view (include/dint_driver.h)"""
    _fields_ = [("workload", C.c_uint32), ("n_tables", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("table", TableView * 5)]


class DintError(RuntimeError):
    pass


_lib = None


class SegmentsItem(C.Structure):
    """dint_segments_item (include/dint_abi.h)"""
    _fields_ = [("engine", C.c_void_p), ("d_base", C.c_void_p), ("n_seg", C.c_uint32), ("seg_cap", C.c_uint32),
                ("seg_stride", C.c_uint64), ("d_cnt", C.c_void_p), ("cnt_stride", C.c_uint64)]


def load() -> C.CDLL:
    """Load libdint.so (built in-tree by dint_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # libdint.so is linked against libamdhip64; torch ships its own copy.  Loading torch first makes the two share
        # ONE HIP runtime (the same SONAME resolves to the copy already mapped) -- with two runtimes in the process the
        # one initialised second finds no device.  Only the ordering matters; no torch symbol is used here.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise DintError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -m dint_amd.build`); there is no CPU fallback"
        )
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64, C.c_int32
    sig = {
        "dint_engine_create": (C.c_int, [C.POINTER(Config), C.POINTER(vp)]),
        "dint_engine_destroy": (None, [vp]),
        "dint_msg_size": (C.c_int, [u32]),
        "dint_last_error": (C.c_char_p, []),
        "dint_submit": (C.c_int, [vp, vp, u32, vp]),
        "dint_submit_device": (C.c_int, [vp, vp, u32, vp, vp]),
        "dint_submit_device_ahead": (C.c_int, [vp, vp, u32, vp, vp, u32, vp, vp]),
        "dint_sync": (C.c_int, [vp]),
        "dint_load_rows": (C.c_int, [vp, u32, vp, vp, vp, u64]),
        "dint_populate": (C.c_int, [vp, u64]),
        "dint_hash_size": (i64, [vp, u32]),
        "dint_dump_rows": (i64, [vp, u32, vp, vp, vp, u64]),
        "dint_read_locks": (i64, [vp, u32, vp, vp, u64]),
        "dint_read_log": (i64, [vp, vp, u64]),
        "dint_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "dint_reset": (C.c_int, [vp]),
        "dint_snapshot": (C.c_int, [vp]),
        "dint_restore": (C.c_int, [vp]),
        "dint_home_shard": (C.c_int, [vp, vp, u32, vp, vp]),
        "dint_bench_rand64": (C.c_int, [i32, u64, u64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dint_selftest": (C.c_int, [i32]),
        "dint_bench_access": (C.c_int, [i32, u64, u64, u32, u32, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "dint_kv_trace_read": (C.c_int, [vp, vp, u64]),
        "dint_timing_enable": (C.c_int, [vp, C.c_int]),
        "dint_timing_read": (C.c_int, [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(u64), C.c_int]),
        "dint_submit_async": (C.c_int, [vp, vp, u32, vp, C.POINTER(u64)]),
        "dint_wait": (C.c_int, [vp, u64]),
        "dint_alloc_pinned": (C.c_int, [C.c_size_t, C.POINTER(vp)]),
        "dint_free_pinned": (None, [vp]),
        "dint_engine_stream": (vp, [vp]),
        "dint_max_pass": (u32, [vp]),
        "dint_stream_wait": (C.c_int, [vp, vp]),
        "dint_stream_signal": (C.c_int, [vp, vp]),
        "dint_route_pack": (C.c_int, [vp, vp, u32, vp, u32, u64, vp, u64, vp, vp]),
        "dint_route_unpack": (C.c_int, [vp, vp, u32, u64, vp, vp, u32, vp, vp]),
        "dint_route_pack_multi": (C.c_int, [C.POINTER(RouteItem), u32, u64, u64, vp]),
        "dint_route_unpack_multi": (C.c_int, [C.POINTER(RouteItem), u32, u64, vp]),
        "dint_submit_segments": (C.c_int, [vp, vp, u32, u32, u64, vp, u64, vp]),
        "dint_submit_segments_multi": (C.c_int, [C.POINTER(SegmentsItem), u32, vp]),
        "dint_submit_segments_multi_ahead": (C.c_int, [C.POINTER(SegmentsItem), u32, C.POINTER(SegmentsItem), vp]),
        "dint_log_drain": (i64, [vp, vp, u64, C.POINTER(u64)]),
        "dint_refuse": (C.c_int, [u32, vp, u32, vp]),
        "dint_log_drain_device": (i64, [vp, vp, u64, C.POINTER(u64), vp]),
        "dint_log_apply_device": (C.c_int, [vp, vp, u64, u32, C.POINTER(ApplyStats)]),
        "dint_log_apply_folded_device": (C.c_int, [vp, vp, u64, u32, u32, C.POINTER(FoldStats)]),
        "dint_state_digest": (C.c_int, [vp, C.POINTER(TableDigest), u32, vp]),
        "dint_state_diff": (i64, [vp, vp, vp, u64, C.POINTER(DiffStats), vp]),
        "dint_state_repair": (C.c_int, [vp, vp, u64, C.POINTER(RepairStats), vp]),
        "dint_state_block_digest": (i64, [vp, u64, vp, u64, C.POINTER(BlockStats), vp]),
        "dint_state_block_select": (i64, [vp, vp, u32, vp, u64, vp]),
        "dint_state_block_rows": (i64, [vp, u64, vp, u32, vp, u64, C.POINTER(BlockStats), vp]),
        "dint_state_block_diff": (i64, [vp, u64, vp, u32, vp, u64, vp, u64, C.POINTER(DiffStats), vp]),
        "dint_records_route": (i64, [vp, u32, vp, u64, vp, u64, vp, vp]),
        "dint_state_export": (C.c_int, [vp, u32, u32, vp, u64, C.POINTER(ImageStats), vp]),
        "dint_state_import": (C.c_int, [vp, vp, u64, C.POINTER(ImageStats), vp]),
        "dint_state_rehash": (C.c_int, [vp, C.POINTER(vp), u32, u32, C.POINTER(RehashStats), vp]),
        "dint_state_stats": (C.c_int, [vp, C.POINTER(TableStats), u32, vp]),
        "dint_state_verify": (C.c_int, [vp, C.POINTER(TableVerify), u32, u32, vp]),
        "dint_state_compact": (C.c_int, [vp, C.POINTER(TableCompact), u32, u32, vp]),
        "dint_state_locks": (i64, [vp, vp, u64, C.POINTER(LockStats), vp]),
        "dint_state_unlock": (C.c_int, [vp, vp, u64, u32, C.POINTER(UnlockStats), vp]),
        # include/dint_driver.h: the held locks' rule (csrc/state_locks.h) over an image / a record list in host memory
        "dint_state_locks_image_host": (i64, [vp, u64, vp, u64, C.POINTER(LockStats)]),
        "dint_state_unlock_check_host": (u64, [u32, C.POINTER(LockGeometry), vp, u64]),
        # include/dint_driver.h: the replay's classification rule on the host (no device call)
        "dint_log_classify_host": (C.c_int, [vp, u64, vp, vp]),
        # ... and the log ring's words under announcements, cancels and drains (csrc/log_ring.h)
        "dint_log_ring_host": (i64, [u32, vp, u32, vp, u64]),
        "dint_log_fold_host": (i64, [u32, u32, vp, vp, vp, vp, vp, u64, vp, vp, u64, C.POINTER(FoldStats)]),
        # ... and the state sync's rules (csrc/state_sync.h) over dumped rows
        "dint_state_row_hash_host": (u64, [u64, u32, u32, vp, u32]),
        "dint_state_digest_host": (C.c_int, [u32, vp, vp, vp, u32, u64, C.POINTER(TableDigest)]),
        "dint_state_diff_host": (i64, [u32, u64, u32, vp, vp, vp, u64, vp, vp, vp, u64, vp, u64, C.POINTER(DiffStats)]),
        # ... and the state image's check (csrc/state_image.h) over an image in host memory
        "dint_state_image_check_host": (C.c_int, [vp, u64]),
        # ... and the table report's rule (csrc/state_stats.h) over an image in host memory
        "dint_state_stats_image_host": (C.c_int, [vp, u64, C.POINTER(TableStats), u32]),
        # ... and the table verify's rule (csrc/state_verify.h) over tables the caller describes, in host / in device memory
        "dint_state_verify_view_host": (C.c_int, [C.POINTER(TablesView), C.POINTER(TableVerify), u32, u32]),
        "dint_state_verify_view": (C.c_int, [i32, C.POINTER(TablesView), C.POINTER(TableVerify), u32, u32, vp]),
        # ... and the compaction's rule (csrc/state_compact.h) over the same views
        "dint_state_compact_view_host": (C.c_int, [C.POINTER(TablesView), C.POINTER(TableCompact), u32, u32]),
        "dint_state_compact_view": (C.c_int, [i32, C.POINTER(TablesView), C.POINTER(TableCompact), u32, u32, vp]),
        # ... and the block sync's rule (csrc/state_block.h) over the same views in host memory
        "dint_state_block_digest_host": (i64, [C.POINTER(TablesView), u64, vp, u64, C.POINTER(BlockStats)]),
        "dint_state_block_rows_host": (i64, [C.POINTER(TablesView), u64, vp, u32, vp, u64, C.POINTER(BlockStats)]),
        "dint_state_block_diff_host": (i64, [C.POINTER(TablesView), u64, vp, u32, vp, u64, vp, u64, C.POINTER(DiffStats)]),
        # ... and the record routing's rule (csrc/state_route.h) over a list in host memory
        "dint_records_route_host": (i64, [u32, u64, u32, vp, u64, vp, vp]),
        "dint_records_route_tile": (u32, []),
        # the traffic report (csrc/traffic_report.h): a batch in device memory / the same rule over a batch in host memory
        "dint_traffic_report": (C.c_int, [vp, vp, vp, u64, u32, C.POINTER(TrafficReport), vp, vp, vp]),
        "dint_traffic_report_host": (C.c_int, [u32, u64, u64, u32, vp, vp, u64, u32, C.POINTER(TrafficReport), vp, vp]),
        # ... and the rehash's layout rule (csrc/state_rehash.h) over keys in source order
        "dint_state_rehash_place_host": (i64, [vp, u64, u64, u32, u32, vp, vp, vp]),
        # ... and the bulk load's rule (csrc/state_load.h): placement over a host view, the population's rows, its tile tables
        "dint_load_rows_device": (C.c_int, [vp, u32, vp, vp, vp, u64, C.POINTER(LoadStats), vp]),
        "dint_populate_device": (C.c_int, [vp, u64, C.POINTER(LoadStats), vp]),
        "dint_state_load_place_host": (C.c_int, [vp, u32, vp, vp, vp, u64, C.POINTER(LoadStats)]),
        "dint_populate_rows_host": (i64, [u32, u32, u64, u64, vp, vp, u64]),
        "dint_populate_tile": (u32, []),
        "dint_populate_tile_states_host": (i64, [u32, u32, u64, vp, vp, u64]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)  # AttributeError here = the .so does not export the ABI
        f.restype, f.argtypes = res, args
    _lib = L
    return L


def check(rc: int) -> int:
    if rc < 0:
        raise DintError(f"dint error {rc}: {load().dint_last_error().decode(errors='replace')}")
    return rc
