"""Host-side mirror of the reference servers over the C ABI.

One :class:`Engine` plays the role of one reference server process
(``lock_fasst/udp/server``, ``tatp/udp/server_shard`` ...): it owns the tables and
answers batches of wire messages.  ``submit`` takes/returns numpy arrays of the packed
wire structs (:mod:`dint_amd.wire`); ``submit_device`` works on HBM-resident buffers
(torch uint8 tensors or raw device pointers) without any host copy.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from .wire import LOG_REC, MSG_DTYPE, Workload

#: dint_lock_record (include/dint_abi.h): one held lock unit
LOCK_REC = np.dtype([("slot", "<u8"), ("a", "<u4"), ("b", "<u4"), ("key", "<u8"), ("cand_rows", "<u4"), ("table", "u1"), ("flags", "u1"),
                     ("zero", "<u2")])


def lock_records(t, n: int) -> np.ndarray:
    """the first n records of a state_locks tensor as a numpy array of LOCK_REC (a copy in host memory)"""
    return t.reshape(-1)[:32 * n].cpu().numpy().view(LOCK_REC).copy()


_N_TABLES = {Workload.STORE: 1, Workload.TATP: 5, Workload.SMALLBANK: 2}


def _ptr(x):
    """Device pointer of a torch tensor / int."""
    if isinstance(x, int):
        return x
    return x.data_ptr()


def _hptr(x):
    """Host pointer of a numpy array / pinned torch tensor / int."""
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    return x.data_ptr()


class Pinned:
    """A page-locked host buffer from dint_alloc_pinned, viewed as a numpy uint8 array."""

    def __init__(self, nbytes: int):
        self._L = _lib.load()
        p = C.c_void_p()
        _lib.check(self._L.dint_alloc_pinned(nbytes, C.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.frombuffer((C.c_uint8 * nbytes).from_address(self.ptr), np.uint8)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._L.dint_free_pinned(self.ptr)
            self.ptr = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()


class Engine:
    def __init__(self, workload: Workload, *, n_slots: int = 0, n_rows: int = 0, log_entries: int = 0,
                 device: int = -1, shard_index: int = 0, shard_count: int = 1, flags: int = 0, max_pass: int = 0,
                 pool_entries: int = 0):
        self._L = _lib.load()
        self.workload = Workload(workload)
        self.msg_dtype = MSG_DTYPE[self.workload]
        self.msg_size = self.msg_dtype.itemsize
        cfg = _lib.Config(abi_version=_lib.ABI_VERSION, workload=int(workload), device=device, flags=flags, n_slots=n_slots,
                          n_rows=n_rows, log_entries=log_entries, shard_index=shard_index, shard_count=shard_count,
                          max_pass=max_pass, pool_entries=pool_entries)
        h = C.c_void_p()
        _lib.check(self._L.dint_engine_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self.shard_index, self.shard_count = shard_index, max(1, shard_count)
        self.device_index = device
        self.flags = flags
        self.val_size = 8 if self.workload == Workload.SMALLBANK else 40
        self.pass_max = int(self._L.dint_max_pass(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()

    # ---- hot path ---------------------------------------------------------
    def submit(self, reqs: np.ndarray) -> np.ndarray:
        """Process a batch held in host memory; returns the reply array (same dtype)."""
        reqs = np.ascontiguousarray(reqs)
        assert reqs.dtype.itemsize in (1, self.msg_size)
        n = reqs.nbytes // self.msg_size
        out = np.empty_like(reqs)
        _lib.check(self._L.dint_submit(self._h, reqs.ctypes.data, n, out.ctypes.data))
        return out

    def submit_device(self, d_reqs, n: int, d_replies=None, stream: int = 0, ahead=None) -> None:
        """Enqueue a batch that already lives in HBM (asynchronous).  `ahead` = (d_reqs, n, d_replies) of the engine's NEXT
        submit_device call, complete in HBM already (dint_submit_device_ahead: its partition stage runs beside this batch's
        hot keys; that call must follow, with exactly these buffers)."""
        d_replies = d_reqs if d_replies is None else d_replies
        if ahead is None or not ahead[1]:
            _lib.check(self._L.dint_submit_device(self._h, _ptr(d_reqs), n, _ptr(d_replies), stream))
        else:
            nq, nn, nr = ahead
            _lib.check(self._L.dint_submit_device_ahead(self._h, _ptr(d_reqs), n, _ptr(d_replies), _ptr(nq), nn,
                                                        _ptr(nq if nr is None else nr), stream))

    def submit_async(self, reqs, n: int, replies) -> int:
        """Pipelined host submit on raw host pointers (page-locked for real overlap); returns the ticket."""
        t = C.c_uint64()
        _lib.check(self._L.dint_submit_async(self._h, _hptr(reqs), n, _hptr(replies), C.byref(t)))
        return t.value

    def wait(self, ticket: int):
        _lib.check(self._L.dint_wait(self._h, ticket))

    def sync(self):
        _lib.check(self._L.dint_sync(self._h))

    # ---- streams / multi-GPU routing (dint_amd.sharded.Router) ------------------------------------------
    @property
    def stream(self) -> int:
        return self._L.dint_engine_stream(self._h) or 0

    def stream_wait(self, other_stream: int):
        _lib.check(self._L.dint_stream_wait(self._h, other_stream))

    def stream_signal(self, other_stream: int):
        _lib.check(self._L.dint_stream_signal(self._h, other_stream))

    def route_pack(self, d_reqs, n: int, d_send, seg_cap: int, seg_stride: int, d_cnt, cnt_stride: int, d_slot,
                   stream: int = 0):
        _lib.check(self._L.dint_route_pack(self._h, _ptr(d_reqs), n, _ptr(d_send), seg_cap, seg_stride, _ptr(d_cnt),
                                           cnt_stride, _ptr(d_slot), stream))

    def route_unpack(self, d_back, seg_cap: int, seg_stride: int, d_slot, d_reqs, n: int, d_replies, stream: int = 0):
        _lib.check(self._L.dint_route_unpack(self._h, _ptr(d_back), seg_cap, seg_stride, _ptr(d_slot), _ptr(d_reqs), n,
                                             _ptr(d_replies), stream))

    def submit_segments(self, d_base, n_seg: int, seg_cap: int, seg_stride: int, d_cnt, cnt_stride: int, stream: int = 0):
        _lib.check(self._L.dint_submit_segments(self._h, _ptr(d_base), n_seg, seg_cap, seg_stride, _ptr(d_cnt),
                                                cnt_stride, stream))

    def home_shard(self, d_reqs, n: int, d_home, stream: int = 0) -> None:
        _lib.check(self._L.dint_home_shard(self._h, _ptr(d_reqs), n, _ptr(d_home), stream))

    # ---- population / state ---------------------------------------------------
    def populate(self, populate_n: int):
        _lib.check(self._L.dint_populate(self._h, populate_n))

    def load_rows(self, table: int, keys, vers, vals):
        keys = np.ascontiguousarray(keys, "<u8")
        vals = np.ascontiguousarray(vals, "u1").reshape(len(keys), self.val_size)
        vp = None
        if vers is not None:
            vers = np.ascontiguousarray(vers, "<u4")
            vp = vers.ctypes.data
        _lib.check(self._L.dint_load_rows(self._h, table, keys.ctypes.data, vp, vals.ctypes.data, len(keys)))

    # ---- bulk load on the device (dint_load_rows_device / dint_populate_device) --------------------------------
    def _load_result(self, s, rc) -> dict:
        d = {k: getattr(s, k) for k in ("rows_loaded", "foreign_rows", "direct", "temp_bytes")}
        d["tables"] = [{k: getattr(s.table[t], k) for k in ("rows", "overflow_entries", "longest_chain_entries", "direct")}
                       for t in range(_N_TABLES.get(self.workload, 0))]
        d["stage_ns"] = dict(zip(("generate", "keys", "sort", "plan", "build", "prepass"), s.stage_ns))
        self.last_load = d
        _lib.check(rc)
        return d

    def load_rows_device(self, table: int, keys, vers, vals, stream: int = 0, n=None) -> dict:
        """dint_load_rows_device: load_rows for torch DEVICE tensors -- keys (int64 / uint64 view, n), vers (int32, n, or None:
        version 0), vals (uint8, n x val_size) -- in insertion order.  A table that has taken nothing since creation / reset is
        built directly (csrc/state_load.h: what n kvs_insert calls leave, newest entry first); any other takes the rows as
        load-mode passes formed on the device.  Returns {rows_loaded, foreign_rows, direct, temp_bytes, tables: [{rows,
        overflow_entries, longest_chain_entries, direct}], stage_ns}, also kept in `last_load` -- as far as the call got when it
        raises (the need per table after DINT_ENOMEM: nothing was written then).  With `n` given, keys / vers / vals may be
        raw device addresses."""
        if n is None:
            n = int(keys.numel())
            assert keys.is_contiguous() and vals.is_contiguous() and keys.element_size() == 8 and vals.numel() == n * self.val_size
            assert vers is None or (vers.is_contiguous() and vers.element_size() == 4 and vers.numel() == n)
        s = _lib.LoadStats()
        rc = self._L.dint_load_rows_device(self._h, table, _ptr(keys), None if vers is None else _ptr(vers), _ptr(vals), n, C.byref(s), stream)
        return self._load_result(s, rc)

    def populate_device(self, populate_n: int, stream: int = 0) -> dict:
        """dint_populate_device: populate() without the host -- the reference's rows of the first populate_n subscribers /
        accounts generated on the device table by table and loaded directly.  The engine must be blank.  Result as
        load_rows_device's, summed over the tables."""
        s = _lib.LoadStats()
        rc = self._L.dint_populate_device(self._h, populate_n, C.byref(s), stream)
        return self._load_result(s, rc)

    def hash_size(self, table: int) -> int:
        return _lib.check(self._L.dint_hash_size(self._h, table))

    def dump_rows(self, table: int):
        n = _lib.check(self._L.dint_dump_rows(self._h, table, None, None, None, 0))
        keys = np.zeros(n, "<u8"); vers = np.zeros(n, "<u4"); vals = np.zeros((n, self.val_size), "u1")
        got = _lib.check(self._L.dint_dump_rows(self._h, table, keys.ctypes.data, vers.ctypes.data, vals.ctypes.data, n))
        assert got == n
        return keys, vers, vals

    def read_locks(self, table: int = 0):
        n = _lib.check(self._L.dint_read_locks(self._h, table, None, None, 0))
        a = np.zeros(n, "<u4"); b = np.zeros(n, "<u4")
        _lib.check(self._L.dint_read_locks(self._h, table, a.ctypes.data, b.ctypes.data, n))
        return a, b

    def read_log(self, cap: int):
        rec = np.zeros(cap, LOG_REC)
        tail = _lib.check(self._L.dint_read_log(self._h, rec.ctypes.data, cap))
        return rec, tail

    def log_drain(self, cap: int = 1 << 20):
        """records appended since the previous drain (oldest first) and how many were lost to ring overwrite"""
        rec = np.zeros(cap, LOG_REC)
        lost = C.c_uint64()
        n = _lib.check(self._L.dint_log_drain(self._h, rec.ctypes.data, cap, C.byref(lost)))
        return rec[:n], lost.value

    def log_drain_device(self, d_buf, cap: int, stream: int = 0):
        """dint_log_drain_device: the records appended since the previous drain into the HBM buffer d_buf (cap 64-byte
        records; a torch uint8 tensor or a device pointer); returns (n, lost).  Shares log_drain's cursor."""
        lost = C.c_uint64()
        n = _lib.check(self._L.dint_log_drain_device(self._h, _ptr(d_buf), cap, C.byref(lost), stream))
        return n, lost.value

    def log_apply_device(self, d_records, n: int, chunk: int = 0, stats: bool = True) -> dict:
        """dint_log_apply_device: replay n drained records held in HBM (log order) into this engine, `chunk` records per
        pass (0 = pass_max).  stats=True waits for the replay and returns the acks by kind, the number of chunks and --
        with timing_enable on -- the nanoseconds per stage; stats=False returns {} once the work is queued."""
        if not stats:
            _lib.check(self._L.dint_log_apply_device(self._h, _ptr(d_records), n, chunk, None))
            return {}
        s = _lib.ApplyStats()
        _lib.check(self._L.dint_log_apply_device(self._h, _ptr(d_records), n, chunk, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}
        d["stage_ns"] = dict(zip(("group", "probe", "apply"), s.reserved))
        return d

    def log_apply_folded(self, d_records, n: int, chunk: int = 0, dry_run: bool = False) -> dict:
        """dint_log_apply_folded_device: log_apply_device with every chunk folded first -- the records of a row collapse to its
        last value and the version their count gives (csrc/log_fold.h), written by the state repair's kernel; only the records of
        buckets that hold a touched key twice go through the serial replay.  Leaves the rows log_apply_device leaves.  Returns
        the counts (as log_apply_device's, then rows / folded_records / deferred_records / deferred_buckets / repair_records /
        updated / inserted / deleted / refused) and stage_ns (with timing_enable on).  dry_run=True writes no table byte.
        Raises DintError (DINT_ENOMEM) after applying the rest when inserts found the overflow pool full; `last_fold` holds
        the counts also then."""
        s = _lib.FoldStats()
        rc = self._L.dint_log_apply_folded_device(self._h, _ptr(d_records), n, chunk, _lib.FOLD_DRY_RUN if dry_run else 0, C.byref(s))
        self.last_fold = s.as_dict()
        _lib.check(rc)
        return self.last_fold

    # ---- state sync (dint_state_digest / dint_state_diff / dint_state_repair) ----------------------------
    def state_digest(self, stream: int = 0) -> list:
        """dint_state_digest: per table {rows, sum, xr} over the valid rows -- the row count, and the sum mod 2^64 and the
        xor of the row hashes (fasthash64 over key | ver | table | val).  Independent of chain layout and bucket order;
        64 bytes per table reach the host.  A sharded engine digests its local rows."""
        d = (_lib.TableDigest * 5)()
        n = _lib.check(self._L.dint_state_digest(self._h, d, 5, stream))
        return [{"rows": d[t].rows, "sum": d[t].sum, "xr": d[t].xr} for t in range(n)]

    def state_diff(self, other, d_buf=None, cap: int = 0, stream: int = 0):
        """dint_state_diff: what must be done to `other` to make its visible rows equal this engine's, as 64-byte log
        records in the HBM buffer d_buf (room for cap records; a torch uint8 tensor or a device pointer; None with cap = 0
        only counts).  Order: table, bucket, this engine's rows in chain order, then the rows only `other` has.  Returns
        (records written, stats); stats["total"] is the number the full diff has.  Neither engine is modified."""
        s = _lib.DiffStats()
        n = _lib.check(self._L.dint_state_diff(self._h, other._h, None if d_buf is None else _ptr(d_buf), cap, C.byref(s), stream))
        return n, {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}

    def state_repair(self, d_records, n: int, stream: int = 0) -> dict:
        """dint_state_repair: apply n records of state_diff's form and order to this engine with the versions they carry.
        Raises DintError (DINT_ENOMEM) after applying the rest when inserts found the overflow pool full; `last_repair`
        holds the counts also then."""
        s = _lib.RepairStats()
        rc = self._L.dint_state_repair(self._h, _ptr(d_records), n, C.byref(s), stream)
        self.last_repair = {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}
        _lib.check(rc)
        return self.last_repair

    # ---- block sync (dint_state_block_digest / _select / _rows / _diff) ------------------------------------
    def state_block_digest(self, block_buckets: int, d_out=None, stream: int = 0):
        """dint_state_block_digest: {rows, sum, xr, 0} (32 bytes) per block of `block_buckets` consecutive local buckets -- a
        power of two, 64 .. 2^20 -- of every table, in block-id order (table 0's blocks, then table 1's ...; csrc/state_block.h),
        into the HBM buffer d_out (a torch tensor of 32 bytes per block; None allocates one of int64 [blocks, 4] on this
        engine's device).  Returns (tensor, blocks, stats); stats["blocks"] = the blocks per table.  A sharded engine is taken."""
        import torch

        s = _lib.BlockStats()
        if d_out is None:
            n = _lib.check(self._L.dint_state_block_digest(self._h, block_buckets, None, 0, C.byref(s), stream))  # (counts only)
            d_out = torch.empty((max(n, 1), 4), dtype=torch.int64, device=self._torch_device())
        n = _lib.check(self._L.dint_state_block_digest(self._h, block_buckets, _ptr(d_out), d_out.numel() * d_out.element_size() // 32, C.byref(s), stream))
        return d_out, n, s.as_dict()

    def state_block_select(self, d_a, d_b, n_blocks: int, d_ids=None, cap=None, stream: int = 0):
        """dint_state_block_select: the ascending ids (int32 tensor, on d_a's device) of the blocks whose 32 bytes differ between
        the two digest arrays.  Returns (ids tensor, how many differ in all); the first `cap` (default: all) are written."""
        import torch

        cap = n_blocks if cap is None else cap
        if d_ids is None:
            d_ids = torch.empty(max(cap, 1), dtype=torch.int32, device=d_a.device)
        n = _lib.check(self._L.dint_state_block_select(_ptr(d_a), _ptr(d_b), n_blocks, _ptr(d_ids), cap, stream))
        return d_ids, n

    def state_block_rows(self, block_buckets: int, d_ids, n_ids: int, d_records=None, cap: int = 0, stream: int = 0):
        """dint_state_block_rows: the visible rows of the listed blocks (d_ids: int32 tensor in HBM, strictly ascending) as 64-byte
        records in the HBM buffer d_records (room for cap; None with cap = 0 only counts): ascending id, ascending bucket, chain
        order.  Returns (records written, total the blocks hold)."""
        s = _lib.BlockStats()
        n = _lib.check(self._L.dint_state_block_rows(self._h, block_buckets, _ptr(d_ids) if n_ids else None, n_ids,
                                                     None if d_records is None else _ptr(d_records), cap, C.byref(s), stream))
        return n, int(s.total)

    def state_block_diff(self, block_buckets: int, d_ids, n_ids: int, d_rows, n_rows: int, d_records=None, cap: int = 0, stream: int = 0):
        """dint_state_block_diff: what must be done to THIS engine inside the listed blocks to make its visible rows those of the
        row list d_rows (state_block_rows' records of the other side, carried to this engine's device), in state_diff's record
        form, order and stats; the output goes to state_repair unchanged.  Returns (records written, stats).  A list that is
        out of order, names a table the workload has not or holds a row of an unlisted block raises DintError (DINT_EINVAL) with
        nothing written."""
        s = _lib.DiffStats()
        n = _lib.check(self._L.dint_state_block_diff(self._h, block_buckets, _ptr(d_ids) if n_ids else None, n_ids, _ptr(d_rows) if n_rows else None,
                                                     n_rows, None if d_records is None else _ptr(d_records), cap, C.byref(s), stream))
        return n, {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}

    # ---- record routing (dint_records_route) ------------------------------------------------------------------
    def records_route(self, dst_count: int, d_records, n: int, d_out=None, stream: int = 0, wait: bool = True):
        """dint_records_route: the n 64-byte records at d_records (HBM: a torch uint8 tensor or a device pointer, 16-byte aligned)
        partitioned, stably, by their home among `dst_count` shards -- (fasthash64(key) % the table's bucket count) % dst_count,
        csrc/state_route.h -- into d_out (None allocates a uint8 tensor of n records on this engine's device).  Returns (d_out,
        offsets): shard h's records are d_out[64 * offsets[h] : 64 * offsets[h + 1]], in their input order.  This engine only
        lends its workload and n_rows (and its stream and scratch): its shard layout is ignored and its tables are not touched.
        A record whose table the workload has not raises DintError (DINT_EINVAL) with nothing written.  The call returns with
        the offsets known and the records' write enqueued on `stream` (0 = this engine's own); wait=True then waits for it, so that
        any other engine or stream may read d_out; wait=False leaves that to the caller (stream_signal, or work on `stream`)."""
        import torch

        if d_out is None:
            d_out = torch.empty(max(n, 1) * 64, dtype=torch.uint8, device=self._torch_device())
        cap = d_out.numel() * d_out.element_size() // 64 if hasattr(d_out, "numel") else n
        off = (C.c_uint64 * (dst_count + 1))()
        _lib.check(self._L.dint_records_route(self._h, dst_count, _ptr(d_records) if n else None, n, _ptr(d_out), cap, off, stream))
        if wait and n:
            if stream:
                torch.cuda.synchronize(self._torch_device())
            else:
                self.sync()
        return d_out, list(off)

    def _torch_device(self):
        import torch

        return torch.device("cuda", self.device_index) if getattr(self, "device_index", -1) >= 0 else torch.device("cuda")

    # ---- state image (dint_state_export / dint_state_import) ---------------------------------------------
    def state_export(self, dst_index: int = 0, dst_count: int = 1, d_buf=None, stream: int = 0):
        """dint_state_export: the image of everything this engine holds that belongs to shard dst_index of dst_count
        (csrc/state_image.h: inline entries and chains verbatim, lock words included, links image-relative; lock tables: the
        slots).  d_buf = an HBM buffer (torch uint8 tensor, 16-byte aligned); None sizes one by a count-only call.  Returns
        (tensor, nbytes, stats); the engine is left untouched.  Raises DintError (DINT_ENOMEM) when d_buf is too small;
        `last_image["bytes"]` then says what it takes."""
        import torch

        s = _lib.ImageStats()
        if d_buf is None:
            _lib.check(self._L.dint_state_export(self._h, dst_index, dst_count, None, 0, C.byref(s), stream))
            d_buf = torch.empty(int(s.bytes), dtype=torch.uint8, device="cuda")
        rc = self._L.dint_state_export(self._h, dst_index, dst_count, _ptr(d_buf), d_buf.numel(), C.byref(s), stream)
        self.last_image = {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}
        _lib.check(rc)
        return d_buf, int(s.bytes), self.last_image

    def state_import(self, d_buf, nbytes: int, stream: int = 0) -> dict:
        """dint_state_import: place an image addressed to this engine's (shard_index, shard_count) into its tables.  The
        engine must be blank (created or reset, and since then nothing but imports); the image is checked on the device
        before any table byte changes.  The log ring, the drain cursor and stats() stay as they were."""
        s = _lib.ImageStats()
        _lib.check(self._L.dint_state_import(self._h, _ptr(d_buf), nbytes, C.byref(s), stream))
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}

    # ---- rehash (dint_state_rehash) ------------------------------------------------------------------------
    def state_rehash(self, sources, drop_locks: bool = False, stream: int = 0) -> dict:
        """dint_state_rehash: fill this BLANK engine with every row of `sources` (engines of the same workload, flags and
        device, in the order given) whose key is home to it under ITS n_rows and shard (csrc/state_rehash.h: the rows of a
        bucket in source order, inline entry first, no holes; lock words are not moved).  Returns {rows_seen, rows_placed,
        rows_foreign, locks_held, tables: [{rows, overflow_entries, longest_chain}], stage_ns}.  Raises DintError on a refusal
        -- the engine is then untouched and still blank; `last_rehash` holds the stats as far as the call got (locks_held
        after DINT_ESTATE, the need per table after DINT_ENOMEM)."""
        sources = list(sources)
        arr = (C.c_void_p * max(1, len(sources)))(*[e._h for e in sources])
        s = _lib.RehashStats()
        rc = self._L.dint_state_rehash(self._h, arr, len(sources), _lib.REHASH_DROP_LOCKS if drop_locks else 0, C.byref(s), stream)
        d = {k: getattr(s, k) for k in ("rows_seen", "rows_placed", "rows_foreign", "locks_held")}
        d["tables"] = [{k: getattr(s.table[t], k) for k in ("rows", "overflow_entries", "longest_chain")} for t in range(_N_TABLES.get(self.workload, 0))]
        d["stage_ns"] = dict(zip(("count", "keys", "sort", "plan", "build"), s.stage_ns))
        self.last_rehash = d
        _lib.check(rc)
        return d

    # ---- table report (dint_state_stats) -------------------------------------------------------------------
    def state_stats(self, stream: int = 0) -> list:
        """dint_state_stats: per table a dict of the fields of dint_table_stats (include/dint_abi.h; csrc/state_stats.h is
        the rule) -- buckets, rows, entries, holes, hit_entries, shadowed_rows, longest_chain, locks_held, the pool words ...,
        chain_hist and rows_hist as lists.  Every chain is walked once on the device; nothing is modified, and a blank engine
        stays blank."""
        s = (_lib.TableStats * 5)()
        n = _lib.check(self._L.dint_state_stats(self._h, s, 5, stream))
        return [s[t].as_dict() for t in range(n)]

    # ---- table verify (dint_state_verify) ------------------------------------------------------------------
    def state_verify(self, stream: int = 0, reclaim: bool = False) -> list:
        """dint_state_verify: per table a dict of the fields of dint_table_verify (include/dint_abi.h; csrc/state_verify.h is
        the rule) -- the exact census of chains, free lists, pend lists and pool (rows, linked, free_entries, pending_entries,
        unaccounted, longest_list) and the violations counted (bad_chains, cross_linked, linked_beyond_top, list_bad_links,
        stray_valid_entries, stray_rows, misplaced_rows, odd_valid_bytes).  Violations are the report, not an error.  Nothing
        is modified, and a blank engine stays blank."""
        s = (_lib.TableVerify * 5)()
        rc = self._L.dint_state_verify(self._h, s, 5, _lib.VERIFY_RECLAIM if reclaim else 0, stream)
        self.last_verify = [s[t].as_dict() for t in range(_N_TABLES.get(self.workload, 0))]
        self.last_verify_stage_ns = dict(zip(("chains", "lists", "pool"), list(s[0].reserved)[11:14]))  # with timing_enable on
        n = _lib.check(rc)
        return self.last_verify[:n]

    def state_reclaim(self, stream: int = 0) -> list:
        """dint_state_verify with DINT_VERIFY_RECLAIM: the census, then every table's unaccounted (leaked) pool entries back on
        its free lists; `reclaimed` says how many.  Raises DintError (DINT_ESTATE) with not a byte written when a table has a
        bad chain, a cross-linked entry, an entry linked beyond the pool's top or a bad list link; `last_verify` holds the
        reports also then."""
        return self.state_verify(stream, reclaim=True)

    # ---- table compaction (dint_state_compact) ---------------------------------------------------------------
    def state_compact(self, stream: int = 0, dry_run: bool = False) -> list:
        """dint_state_compact: every bucket's valid rows packed, in chain order, into its inline entry and as few overflow
        entries as they need, the overflow entries laid end to end from pool entry 0, pool_top lowered to them and the free
        and pend lists emptied -- in place, lock words untouched (include/dint_abi.h; csrc/state_compact.h is the rule).  Per
        table a dict: the census before the move under "verify", then rows, entries_before / _after, overflow_before /
        _after, pool_top_before / _after, holes_before / _after, buckets_rewritten, unaccounted_dropped, staging_bytes.
        dry_run=True fills the same report and writes nothing.  Raises DintError (DINT_ESTATE) with not a byte written when
        the census finds a violation; `last_compact` holds the reports also then."""
        s = (_lib.TableCompact * 5)()
        rc = self._L.dint_state_compact(self._h, s, 5, _lib.COMPACT_DRY_RUN if dry_run else 0, stream)
        self.last_compact = [s[t].as_dict() for t in range(_N_TABLES.get(self.workload, 0))]
        self.last_compact_stage_ns = dict(zip(("census", "count", "move", "commit"), list(s[0].reserved)[:4]))  # with timing_enable on
        n = _lib.check(rc)
        return self.last_compact[:n]

    # ---- held locks (dint_state_locks / dint_state_unlock) ----------------------------------------------------
    def state_locks(self, d_buf=None, cap: int = 0, stream: int = 0):
        """dint_state_locks: the lock units this engine holds as 32-byte records (LOCK_REC; include/dint_abi.h
        dint_lock_record, csrc/state_locks.h is the rule) in the HBM buffer d_buf (room for cap records, 8-byte aligned; a
        torch tensor or a device pointer), in the order table, local bucket, q (lock tables: local slot).  d_buf=None counts
        first and allocates a uint8 tensor [records, 32] on this engine's device.  Returns (records tensor, records written,
        stats); stats["total"] is the number there are, "held" per table.  Nothing is modified.  `lock_records(t, n)` turns
        the tensor into a numpy array of LOCK_REC."""
        import torch

        s = _lib.LockStats()
        if d_buf is None:
            _lib.check(self._L.dint_state_locks(self._h, None, 0, C.byref(s), stream))  # (counts only)
            cap = int(s.total)
            d_buf = torch.empty((max(cap, 1), 32), dtype=torch.uint8, device=self._torch_device())
        n = _lib.check(self._L.dint_state_locks(self._h, _ptr(d_buf), cap, C.byref(s), stream))
        return d_buf, n, s.as_dict()

    def state_unlock(self, d_records=None, n: int = 0, all: bool = False, dry_run: bool = False, stream: int = 0) -> dict:
        """dint_state_unlock: compare and release.  The n records of state_locks' form and order in the HBM buffer d_records
        (its output or any sub-sequence) are checked as a whole, then each unit is released only if it still holds what its
        record says -- the others are counted "stale"; all=True releases every held unit instead; dry_run=True gives the same
        check and counts and writes nothing.  Returns released, stale, released_a, released_b, per_table.  Raises DintError
        (DINT_EINVAL) with nothing released for a list that is not one; the message names the first bad record."""
        s = _lib.UnlockStats()
        flags = (_lib.UNLOCK_ALL if all else 0) | (_lib.UNLOCK_DRY_RUN if dry_run else 0)
        _lib.check(self._L.dint_state_unlock(self._h, None if d_records is None else _ptr(d_records), n, flags, C.byref(s), stream))
        return s.as_dict()

    # ---- traffic report (dint_traffic_report) ----------------------------------------------------------------
    def traffic_report(self, d_reqs, n: int, d_replies=None, top: int = 16, stream: int = 0) -> dict:
        """dint_traffic_report: one batch of n wire messages in HBM (and, d_replies given, the replies it got -- a buffer of
        its own: an in-place reply has lost the request types) as a dict of the fields of struct dint_traffic_report
        (include/dint_abi.h; csrc/traffic_report.h is the rule): counts by class and reply flag, distinct keys / units / lock
        slots, key_hist, unit_hist, req_types and rep_types as lists, the shared_* numbers, and "by_requests" / "by_rejects":
        lists of at most `top` dicts of dint_traffic_key.  Read-only; leaves a batch announced with submit_device(ahead=)
        pending.  dint_amd.traffic formats and merges these dicts."""
        from .traffic import unpack

        out = _lib.TrafficReport()
        a, b = (_lib.TrafficKey * max(top, 1))(), (_lib.TrafficKey * max(top, 1))()
        _lib.check(self._L.dint_traffic_report(self._h, _ptr(d_reqs) if d_reqs is not None else None, None if d_replies is None else _ptr(d_replies),
                                               n, top, C.byref(out), a, b, stream))
        return unpack(out, a, b)

    def stats(self) -> dict:
        s = _lib.Stats()
        _lib.check(self._L.dint_get_stats(self._h, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}
        d["late_items"] = list(s.reserved)  # diagnostic: late work items by kind (a sub as listed / a solo item / pieces)
        return d

    def reset(self): _lib.check(self._L.dint_reset(self._h))
    def snapshot(self): _lib.check(self._L.dint_snapshot(self._h))
    def restore(self): _lib.check(self._L.dint_restore(self._h))

    # ---- measurement -----------------------------------------------------------
    def timing_enable(self, on: bool = True):
        _lib.check(self._L.dint_timing_enable(self._h, int(on)))

    def kv_trace(self, workgroups: bool = False):
        """DINT_KV_TRACE=1: [32768, 16] u64 per-bin timeline of the resolve launches since the last read; with
        workgroups=True also [8192, 16] per workgroup: {first wave in, last wave out, phase stamps of its first big bin}
        (10 ns ticks)."""
        out = np.zeros(32768 * 16 + 16 * 8192, "<u8")
        _lib.check(self._L.dint_kv_trace_read(self._h, out.ctypes.data, out.size))
        if self.workload in (Workload.STORE, Workload.TATP, Workload.SMALLBANK):
            # kv engines (r04): 32 words per resolve workgroup -- [0] in, [1] descriptors / count / first records there,
            # [2] records counted per sub, [3] laid out, [4] placed, [5] first chunk sorted, [6..10] that chunk's kv_chunk
            # stamps (run / segment masks, rows located, replies, write-backs, rounds), [11] chunks done, [12] big subs
            # done, [13] coarse bin, [14] records, [15] records in big subs, [16] chunks
            wg = out[:2048 * 32].reshape(2048, 32)
            # ... and 32 words per k_kv_big workgroup: {in, out, records, sub} of the first big sub it resolved, then the
            # phase stamps of one of its stretches ([4] in .. [13] out, [16] .. [22] its dominant-key path: kv_big_bin)
            return (wg, out[2048 * 32:2048 * 32 + 4 * 512 * 32].reshape(2048, 32)) if workgroups else wg
        bins = out[:32768 * 16].reshape(32768, 16)
        return (bins, out[32768 * 16:].reshape(8192, 16)) if workgroups else bins

    def timing_read(self) -> dict:
        names = (C.c_char_p * 8)(); us = (C.c_double * 8)(); cnt = (C.c_uint64 * 8)()
        k = _lib.check(self._L.dint_timing_read(self._h, names, us, cnt, 8))
        return {names[i].decode(): {"avg_us": us[i], "launches": cnt[i]} for i in range(k)}


def submit_segments_multi(engines, d_bases, n_seg: int, seg_caps, seg_stride: int, d_cnts, cnt_stride: int, stream: int = 0, ahead=None):
    """dint_submit_segments_multi: engine k answers its n_seg segments at d_bases[k] in place; the engines' kernels run
    side by side in ONE set of launches on ONE stream (no fork / join across the engines' streams).
    `ahead` = (d_bases, d_cnts) of the NEXT call (same engines, same geometry; dint_submit_segments_multi_ahead)."""
    items = (_lib.SegmentsItem * len(engines))()
    for k, e in enumerate(engines):
        items[k] = _lib.SegmentsItem(e._h, _ptr(d_bases[k]), n_seg, seg_caps[k], seg_stride, _ptr(d_cnts[k]), cnt_stride)
    if ahead is None:
        _lib.check(engines[0]._L.dint_submit_segments_multi(items, len(engines), stream))
        return
    nxt = (_lib.SegmentsItem * len(engines))()
    for k, e in enumerate(engines):
        nxt[k] = _lib.SegmentsItem(e._h, _ptr(ahead[0][k]), n_seg, seg_caps[k], seg_stride, _ptr(ahead[1][k]), cnt_stride)
    _lib.check(engines[0]._L.dint_submit_segments_multi_ahead(items, len(engines), nxt, stream))


def route_pack_multi(engines, d_reqs, counts, d_slots, seg_caps, seg_stride: int, d_cnts, cnt_stride: int, d_slot,
                     stream: int = 0, d_n=None) -> None:
    """dint_route_pack_multi: batch k (engine k's hash / modulus) into its slot d_slots[k] of every peer chunk, one set
    of kernel launches for all of them.  d_n[k]: device pointer to batch k's live request count (counts[k] is then
    its upper bound)."""
    items = (_lib.RouteItem * len(engines))()
    for k, e in enumerate(engines):
        items[k] = _lib.RouteItem(e._h, _ptr(d_reqs[k]), counts[k], seg_caps[k], _ptr(d_slots[k]), _ptr(d_cnts[k]),
                                  _ptr(d_slot[k]), None, d_n[k] if d_n else None)
    _lib.check(engines[0]._L.dint_route_pack_multi(items, len(engines), seg_stride, cnt_stride, stream))


def route_unpack_multi(engines, d_backs, seg_caps, seg_stride: int, d_slot, d_reqs, counts, d_replies, stream: int = 0,
                       d_n=None) -> None:
    items = (_lib.RouteItem * len(engines))()
    for k, e in enumerate(engines):
        items[k] = _lib.RouteItem(e._h, _ptr(d_reqs[k]), counts[k], seg_caps[k], _ptr(d_backs[k]), None, _ptr(d_slot[k]),
                                  _ptr(d_replies[k]), d_n[k] if d_n else None)
    _lib.check(engines[0]._L.dint_route_unpack_multi(items, len(engines), seg_stride, stream))


def bench_rand64(bytes_: int, n_access: int, write_back: bool = False, device: int = -1):
    """Random 64-byte gather microbenchmark (roofline denominator); returns (accesses/s, seconds)."""
    L = _lib.load()
    aps = C.c_double(); sec = C.c_double()
    _lib.check(L.dint_bench_rand64(device, bytes_, n_access, int(write_back), C.byref(aps), C.byref(sec)))
    return aps.value, sec.value


BENCH_MODES = {"gather": 0, "rmw": 1, "scatter": 2, "atomic": 3, "atomic_ret": 4, "stream_rd": 5, "stream_wr": 6}


def bench_access(bytes_: int, n_access: int, mode: str, width: int = 64, blocks_per_cu: int = 8, device: int = -1):
    """One access pattern of csrc/k_bench.hip over `bytes_` of HBM; returns (accesses/s, seconds) -- for the two
    streaming modes 16-byte vectors/s."""
    L = _lib.load()
    aps = C.c_double(); sec = C.c_double()
    _lib.check(L.dint_bench_access(device, bytes_, n_access, BENCH_MODES[mode], width, blocks_per_cu,
                                   C.byref(aps), C.byref(sec)))
    return aps.value, sec.value


def refuse(workload, reqs: np.ndarray) -> np.ndarray:
    """the back-pressure replies of the eBPF-flavour servers (REJECT_* / RETRY) for a batch that is not taken"""
    L = _lib.load()
    reqs = np.ascontiguousarray(reqs)
    out = np.empty_like(reqs)
    _lib.check(L.dint_refuse(int(workload), reqs.ctypes.data, len(reqs), out.ctypes.data))
    return out
