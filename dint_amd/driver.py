"""ctypes binding of the closed-loop transaction drivers (include/dint_driver.h, csrc/txn_driver.cc).

A :class:`Driver` plays W reference clients in lock step: ``next()`` returns the three per-shard
request batches of one epoch (numpy arrays of packed wire structs), ``consume(replies)`` feeds the
servers' replies back.  :func:`run_epochs` wires a driver to three servers (GPU engines, or any
object with ``submit``).
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib
from .wire import MSG_DTYPE, Workload

N_SHARDS = 3


class DriverConfig(C.Structure):
    _fields_ = [("workload", C.c_uint32), ("n_clients", C.c_uint32), ("n_rows", C.c_uint64),
                ("first_client", C.c_uint32), ("key_dist", C.c_uint32), ("zipf_theta", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 7)]


#: dint_driver_config.flags (include/dint_driver.h)
DRIVER_LATENCY = 1
#: histogram sizes of dint_driver_latency
LAT_RT_BINS, LAT_TICK_BINS = 32, 240


class DriverStats(C.Structure):
    _fields_ = [("txns", C.c_uint64), ("committed", C.c_uint64), ("messages", C.c_uint64),
                ("by_type", C.c_uint64 * 8), ("committed_by_type", C.c_uint64 * 8), ("epochs", C.c_uint64)]


class DriverLatency(C.Structure):
    """dint_driver_latency (include/dint_driver.h)"""
    _fields_ = [("round_trips", (C.c_uint64 * LAT_RT_BINS) * 8), ("aborted_round_trips", (C.c_uint64 * LAT_RT_BINS) * 8),
                ("rt_sum", C.c_uint64 * 8), ("rt_max", C.c_uint64 * 8), ("ticks", (C.c_uint64 * LAT_TICK_BINS) * 8),
                ("tick_sum", C.c_uint64 * 8), ("tick_max", C.c_uint64 * 8), ("tick_khz", C.c_uint64), ("epochs", C.c_uint64)]

    def as_dict(self) -> dict:
        """histograms as uint64 arrays [type, bin], sums and maxima as [type]"""
        d = {k: np.array(getattr(self, k), dtype=np.uint64) for k in
             ("round_trips", "aborted_round_trips", "rt_sum", "rt_max", "ticks", "tick_sum", "tick_max")}
        d["tick_khz"], d["epochs"] = int(self.tick_khz), int(self.epochs)
        return d


def tick_bin(ticks: int) -> int:
    """the tick histogram's bin of a value (csrc/txn_latency.h lat_tick_bin)"""
    return int(_bind().dint_latency_tick_bin_host(ticks))


def tick_bin_lo(b: int) -> int:
    """the smallest value of a tick bin (LAT_TICK_BINS: where the last bin would end if it did not saturate)"""
    return int(_bind().dint_latency_tick_lo_host(b))


def merge_latency(lats) -> dict:
    """the latency of several client groups as one (:meth:`Driver.latency` / :meth:`GpuDriver.latency` dicts): histograms and
    sums add, maxima take the maximum; tick_khz is the groups' common rate (0 from host drivers), epochs the largest count"""
    lats = list(lats)
    khz = {l["tick_khz"] for l in lats if l["tick_khz"]}
    if len(khz) > 1:
        raise ValueError(f"the groups' clocks differ: {sorted(khz)} kHz")
    out = {k: np.sum([l[k] for l in lats], axis=0, dtype=np.uint64) for k in ("round_trips", "aborted_round_trips", "rt_sum", "ticks", "tick_sum")}
    for k in ("rt_max", "tick_max"):
        out[k] = np.max([l[k] for l in lats], axis=0).astype(np.uint64)
    out["tick_khz"], out["epochs"] = (khz.pop() if khz else 0), max(l["epochs"] for l in lats)
    return out


def latency_percentiles(lat: dict, kind: str = "ticks", ps=(50, 99, 99.9), types=None) -> dict:
    """Average and percentiles of COMMITTED transactions from a latency dict, by the reference's rule (Percentile(),
    tatp/caladan/stat.h:12-17): the element at index floor(p * n / 100) of the sorted samples -- in a histogram the first bin
    whose cumulative count exceeds that index (the last sample for an index of n: p = 100).  kind = "round_trips": values
    in round trips (the last bin stands for 31 and more).  kind = "ticks": a bin is reported by its lower bound, converted
    to microseconds with tick_khz; the average comes from the exact tick sum.  `types` = the transaction types to pool
    (default: all).  Returns {"n", "avg", "max", "p": {p: value}}; with n = 0 every value is None."""
    if kind not in ("ticks", "round_trips"):
        raise ValueError(kind)
    if kind == "ticks" and not lat["tick_khz"]:
        raise ValueError("no tick rate: ticks are kept by the GPU-resident driver only")
    ts = list(range(8)) if types is None else list(types)
    hist = np.asarray(lat[kind], dtype=np.uint64)[ts].sum(axis=0, dtype=np.uint64)
    n = int(hist.sum())
    if n == 0:
        return {"n": 0, "avg": None, "max": None, "p": {p: None for p in ps}}
    if kind == "ticks":
        unit = 1000.0 / lat["tick_khz"]  # microseconds per tick
        value = lambda b: tick_bin_lo(b) * unit  # noqa: E731
        total, top = int(np.asarray(lat["tick_sum"])[ts].sum(dtype=np.uint64)) * unit, int(np.asarray(lat["tick_max"])[ts].max()) * unit
    else:
        value = lambda b: b  # noqa: E731
        total, top = int(np.asarray(lat["rt_sum"])[ts].sum(dtype=np.uint64)), int(np.asarray(lat["rt_max"])[ts].max())
    cum = np.cumsum(hist, dtype=np.uint64)
    out = {}
    for p in ps:
        idx = min(int(float(p) * n / 100), n - 1)  # in double arithmetic, as the reference computes it
        out[p] = value(int(np.searchsorted(cum, idx, side="right")))
    return {"n": n, "avg": total / n, "max": top, "p": out}


def _bind():
    L = _lib.load()
    if getattr(L, "_driver_bound", False):
        return L
    vp, u32 = C.c_void_p, C.c_uint32
    L.dint_driver_create.restype, L.dint_driver_create.argtypes = C.c_int, [C.POINTER(DriverConfig), C.POINTER(vp)]
    L.dint_driver_destroy.restype, L.dint_driver_destroy.argtypes = None, [vp]
    L.dint_driver_msg_size.restype, L.dint_driver_msg_size.argtypes = C.c_int, [vp]
    L.dint_driver_next.restype, L.dint_driver_next.argtypes = C.c_int, [vp, C.POINTER(u32 * N_SHARDS)]
    L.dint_driver_batch.restype, L.dint_driver_batch.argtypes = vp, [vp, u32]
    L.dint_driver_consume.restype, L.dint_driver_consume.argtypes = C.c_int, [vp, C.POINTER(vp * N_SHARDS)]
    L.dint_driver_get_stats.restype, L.dint_driver_get_stats.argtypes = C.c_int, [vp, C.POINTER(DriverStats)]
    L.dint_driver_get_latency.restype, L.dint_driver_get_latency.argtypes = C.c_int, [vp, C.POINTER(DriverLatency)]
    L.dint_latency_tick_bin_host.restype, L.dint_latency_tick_bin_host.argtypes = u32, [C.c_uint64]
    L.dint_latency_tick_lo_host.restype, L.dint_latency_tick_lo_host.argtypes = C.c_uint64, [u32]
    L._driver_bound = True
    return L


class Driver:
    def __init__(self, workload: Workload, n_clients: int, n_rows: int, *, first_client: int = 0,
                 zipf_theta: float | None = None):
        self._L = _bind()
        self.workload = Workload(workload)
        self.dtype = MSG_DTYPE[self.workload]
        cfg = DriverConfig(workload=int(workload), n_clients=n_clients, n_rows=n_rows, first_client=first_client,
                           key_dist=0 if zipf_theta is None else 1, zipf_theta=zipf_theta or 0.0)
        h = C.c_void_p()
        rc = self._L.dint_driver_create(C.byref(cfg), C.byref(h))
        if rc:
            raise _lib.DintError(f"dint_driver_create failed: {rc}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_driver_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()

    def next(self):
        """Requests of the next epoch: list of 3 numpy arrays (copies) of packed wire structs."""
        cnt = (C.c_uint32 * N_SHARDS)()
        _lib.check(self._L.dint_driver_next(self._h, C.byref(cnt)))
        out = []
        for s in range(N_SHARDS):
            n = cnt[s]
            if n == 0:
                out.append(np.zeros(0, self.dtype))
                continue
            p = self._L.dint_driver_batch(self._h, s)
            buf = (C.c_uint8 * (n * self.dtype.itemsize)).from_address(p)
            out.append(np.frombuffer(buf, self.dtype, n).copy())
        return out

    def consume(self, replies):
        keep = [np.ascontiguousarray(r) for r in replies]
        ptrs = (C.c_void_p * N_SHARDS)(*[r.ctypes.data if len(r) else None for r in keep])
        _lib.check(self._L.dint_driver_consume(self._h, C.byref(ptrs)))

    def stats(self) -> dict:
        s = DriverStats()
        _lib.check(self._L.dint_driver_get_stats(self._h, C.byref(s)))
        return {"txns": s.txns, "committed": s.committed, "messages": s.messages, "epochs": s.epochs,
                "by_type": list(s.by_type), "committed_by_type": list(s.committed_by_type)}

    def latency(self) -> dict:
        """round trips of the finished transactions per type (DriverLatency.as_dict; the tick fields are 0 on the host)"""
        l = DriverLatency()
        _lib.check(self._L.dint_driver_get_latency(self._h, C.byref(l)))
        return l.as_dict()


class GpuDriver:
    """The same closed-loop clients resident on the GPU (csrc/k_txn.hip, include/dint_driver.h dint_gdriver_*):
    ``next(stream)`` emits the epoch's three request batches into device arrays (``batch_ptr[s]``, refreshed by every
    ``next``; live sizes at ``counts_ptr``), the shard servers answer in place, ``consume(stream)`` feeds the replies
    back (on the stream of ``next``: fused into the next emit kernel).  The request stream is bit-identical to
    :class:`Driver`'s.  ``latency=True`` (DINT_DRIVER_LATENCY) keeps the committed transactions' latency in round trips
    and in ticks of the device clock: ``latency()``, ``latency_reset(stream)``; the request stream is the same bytes."""

    def __init__(self, workload: Workload, n_clients: int, n_rows: int, cap: int, *, first_client: int = 0,
                 zipf_theta: float | None = None, device: int = -1, latency: bool = False, flags: int = 0):
        L = self._L = _bind()
        vp, u32 = C.c_void_p, C.c_uint32
        L.dint_gdriver_create.restype, L.dint_gdriver_create.argtypes = C.c_int, [C.POINTER(DriverConfig), C.c_int32, u32, C.POINTER(vp)]
        L.dint_gdriver_destroy.restype, L.dint_gdriver_destroy.argtypes = None, [vp]
        L.dint_gdriver_next.restype, L.dint_gdriver_next.argtypes = C.c_int, [vp, vp]
        L.dint_gdriver_consume.restype, L.dint_gdriver_consume.argtypes = C.c_int, [vp, vp]
        L.dint_gdriver_batch.restype, L.dint_gdriver_batch.argtypes = vp, [vp, u32]
        L.dint_gdriver_counts.restype, L.dint_gdriver_counts.argtypes = vp, [vp]
        L.dint_gdriver_get_stats.restype, L.dint_gdriver_get_stats.argtypes = C.c_int, [vp, C.POINTER(DriverStats), C.POINTER(C.c_uint64)]
        L.dint_gdriver_read_batch.restype, L.dint_gdriver_read_batch.argtypes = C.c_int64, [vp, u32, vp, C.c_uint64]
        L.dint_gdriver_get_latency.restype, L.dint_gdriver_get_latency.argtypes = C.c_int, [vp, C.POINTER(DriverLatency)]
        L.dint_gdriver_latency_reset.restype, L.dint_gdriver_latency_reset.argtypes = C.c_int, [vp, vp]
        L.dint_gdriver_read_stamps.restype, L.dint_gdriver_read_stamps.argtypes = C.c_int, [vp, C.POINTER(C.c_uint64 * 256), C.POINTER(C.c_uint64)]
        self.workload = Workload(workload)
        self.dtype = MSG_DTYPE[self.workload]
        self.cap = cap
        cfg = DriverConfig(workload=int(workload), n_clients=n_clients, n_rows=n_rows, first_client=first_client,
                           key_dist=0 if zipf_theta is None else 1, zipf_theta=zipf_theta or 0.0,
                           flags=flags | (DRIVER_LATENCY if latency else 0))
        h = vp()
        rc = L.dint_gdriver_create(C.byref(cfg), device, cap, C.byref(h))
        if rc:
            raise _lib.DintError(f"dint_gdriver_create failed: {rc}")
        self._h = h
        self.batch_ptr = [L.dint_gdriver_batch(h, s) for s in range(N_SHARDS)]
        self.counts_ptr = L.dint_gdriver_counts(h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_gdriver_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()

    def next(self, stream: int = 0):
        rc = self._L.dint_gdriver_next(self._h, stream)
        if rc:
            raise _lib.DintError(f"dint_gdriver_next failed: {rc}")
        # the epoch's batches alternate between two buffer sets (replies of epoch k are read while epoch k+1 is written)
        self.batch_ptr = [self._L.dint_gdriver_batch(self._h, s) for s in range(N_SHARDS)]

    def consume(self, stream: int = 0):
        rc = self._L.dint_gdriver_consume(self._h, stream)
        if rc:
            raise _lib.DintError(f"dint_gdriver_consume failed: {rc}")

    def stats(self) -> dict:
        s, ov = DriverStats(), C.c_uint64()
        rc = self._L.dint_gdriver_get_stats(self._h, C.byref(s), C.byref(ov))
        if rc:
            raise _lib.DintError(f"dint_gdriver_get_stats failed: {rc}")
        return {"txns": s.txns, "committed": s.committed, "messages": s.messages, "epochs": s.epochs,
                "by_type": list(s.by_type), "committed_by_type": list(s.committed_by_type), "overflow": ov.value}

    def latency(self) -> dict:
        """latency of the finished transactions (DriverLatency.as_dict); synchronises.  Needs latency=True."""
        l = DriverLatency()
        rc = self._L.dint_gdriver_get_latency(self._h, C.byref(l))
        if rc:
            raise _lib.DintError(f"dint_gdriver_get_latency failed: {rc}")
        return l.as_dict()

    def latency_reset(self, stream: int = 0):
        """zero the histograms in stream order (the reference's stat_started window); transactions under way keep their latency"""
        rc = self._L.dint_gdriver_latency_reset(self._h, stream)
        if rc:
            raise _lib.DintError(f"dint_gdriver_latency_reset failed: {rc}")

    def read_stamps(self):
        """(uint64[256] epoch stamps: slot e & 255 = the clock at the start of epoch e's emit kernel, epochs emitted);
        synchronises (tests and debugging)"""
        out, ep = (C.c_uint64 * 256)(), C.c_uint64()
        rc = self._L.dint_gdriver_read_stamps(self._h, C.byref(out), C.byref(ep))
        if rc:
            raise _lib.DintError(f"dint_gdriver_read_stamps failed: {rc}")
        return np.array(out, dtype=np.uint64), ep.value

    def read_batches(self):
        """host copies of the current epoch's three batches (synchronises; tests and debugging)"""
        out = []
        for s in range(N_SHARDS):
            buf = np.zeros(self.cap, self.dtype)
            n = self._L.dint_gdriver_read_batch(self._h, s, buf.ctypes.data, self.cap)
            if n < 0:
                raise _lib.DintError(f"dint_gdriver_read_batch failed: {n}")
            out.append(buf[:n].copy())
        return out


class FasstClientConfig(C.Structure):
    _fields_ = [("n_workers", C.c_uint32), ("first_worker", C.c_uint32), ("key_space", C.c_uint32),
                ("read_pct", C.c_uint32), ("key_dist", C.c_uint32), ("reserved0", C.c_uint32),
                ("zipf_theta", C.c_double), ("reserved", C.c_uint32 * 8)]


class FasstClientStats(C.Structure):
    _fields_ = [("requests", C.c_uint64), ("epochs", C.c_uint64), ("committed", C.c_uint64), ("rejects", C.c_uint64),
                ("rollbacks", C.c_uint64), ("protocol_errors", C.c_uint64), ("reserved", C.c_uint64 * 2)]


class FasstClient:
    """The lock_fasst load generator (lock_fasst/caladan/client.cc:183-280 restated, csrc/fasst_client.cc): W
    workers in lock step, ``next()`` = one 9-byte request per worker, ``consume(replies)`` advances them."""

    def __init__(self, n_workers: int = 4096, key_space: int = 24_000_000, *, read_pct: int = 80,
                 zipf_theta: float | None = 0.8, first_worker: int = 0):
        from .wire import FASST_MSG

        L = self._L = _lib.load()
        vp = C.c_void_p
        L.dint_fasst_client_create.restype, L.dint_fasst_client_create.argtypes = C.c_int, [C.POINTER(FasstClientConfig), C.POINTER(vp)]
        L.dint_fasst_client_destroy.restype, L.dint_fasst_client_destroy.argtypes = None, [vp]
        L.dint_fasst_client_next.restype, L.dint_fasst_client_next.argtypes = vp, [vp]
        L.dint_fasst_client_consume.restype, L.dint_fasst_client_consume.argtypes = C.c_int, [vp, vp]
        L.dint_fasst_client_get_stats.restype, L.dint_fasst_client_get_stats.argtypes = C.c_int, [vp, C.POINTER(FasstClientStats)]
        self.dtype, self.n = FASST_MSG, n_workers
        cfg = FasstClientConfig(n_workers=n_workers, first_worker=first_worker, key_space=key_space, read_pct=read_pct,
                                key_dist=0 if zipf_theta is None else 1, zipf_theta=zipf_theta or 0.0)
        h = vp()
        rc = L.dint_fasst_client_create(C.byref(cfg), C.byref(h))
        if rc:
            raise _lib.DintError(f"dint_fasst_client_create failed: {rc}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_fasst_client_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()

    def next(self) -> np.ndarray:
        p = self._L.dint_fasst_client_next(self._h)
        if not p:
            raise _lib.DintError("dint_fasst_client_next: replies of the previous epoch are still outstanding")
        return np.frombuffer((C.c_uint8 * (self.n * 9)).from_address(p), self.dtype).copy()

    def consume(self, replies: np.ndarray):
        replies = np.ascontiguousarray(replies)
        _lib.check(self._L.dint_fasst_client_consume(self._h, replies.ctypes.data))

    def peek(self, worker: int = 0):
        """(read set, write set) of the transaction `worker` is running"""
        k, w = (C.c_uint32 * 10)(), (C.c_uint32 * 10)()
        nk, nw = C.c_uint32(), C.c_uint32()
        self._L.dint_fasst_client_peek.restype = C.c_int
        self._L.dint_fasst_client_peek.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.check(self._L.dint_fasst_client_peek(self._h, worker, k, C.byref(nk), w, C.byref(nw)))
        return list(k[:nk.value]), list(w[:nw.value])

    def stats(self) -> dict:
        s = FasstClientStats()
        _lib.check(self._L.dint_fasst_client_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}


class TplClientStats(C.Structure):
    _fields_ = [("requests", C.c_uint64), ("epochs", C.c_uint64), ("committed", C.c_uint64), ("rejects", C.c_uint64),
                ("protocol_errors", C.c_uint64), ("reserved", C.c_uint64 * 3)]


class LcgTplClient:
    """The lock_2pl load generator in C (lock_2pl/caladan/client.cc:167-240 restated, csrc/tpl_client.cc): W workers in
    lock step that draw their transactions exactly as :class:`FasstClient` does (the reference's LCG seeded 0xdeadbeef +
    worker), with :class:`TplClient`'s state machine -- so the GPU-resident client (:class:`GpuLockClient`) can reproduce
    its stream.  ``next()`` = one 6-byte request per worker, ``consume(replies)`` advances them."""

    def __init__(self, n_workers: int = 4096, key_space: int = 24_000_000, *, read_pct: int = 80,
                 zipf_theta: float | None = 0.8, first_worker: int = 0):
        from .wire import TPL_MSG

        L = self._L = _lib.load()
        vp = C.c_void_p
        L.dint_tpl_client_create.restype, L.dint_tpl_client_create.argtypes = C.c_int, [C.POINTER(FasstClientConfig), C.POINTER(vp)]
        L.dint_tpl_client_destroy.restype, L.dint_tpl_client_destroy.argtypes = None, [vp]
        L.dint_tpl_client_next.restype, L.dint_tpl_client_next.argtypes = vp, [vp]
        L.dint_tpl_client_consume.restype, L.dint_tpl_client_consume.argtypes = C.c_int, [vp, vp]
        L.dint_tpl_client_get_stats.restype, L.dint_tpl_client_get_stats.argtypes = C.c_int, [vp, C.POINTER(TplClientStats)]
        L.dint_tpl_client_peek.restype, L.dint_tpl_client_peek.argtypes = C.c_int, [vp, C.c_uint32, vp, vp, vp]
        self.dtype, self.n = TPL_MSG, n_workers
        cfg = FasstClientConfig(n_workers=n_workers, first_worker=first_worker, key_space=key_space, read_pct=read_pct,
                                key_dist=0 if zipf_theta is None else 1, zipf_theta=zipf_theta or 0.0)
        h = vp()
        _lib.check(L.dint_tpl_client_create(C.byref(cfg), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_tpl_client_destroy(self._h)
            self._h = None

    def __del__(self):
        if not sys.is_finalizing():
            self.close()

    def next(self) -> np.ndarray:
        p = self._L.dint_tpl_client_next(self._h)
        if not p:
            raise _lib.DintError("dint_tpl_client_next: replies of the previous epoch are still outstanding")
        return np.frombuffer((C.c_uint8 * (self.n * 6)).from_address(p), self.dtype).copy()

    def consume(self, replies: np.ndarray):
        replies = np.ascontiguousarray(replies)
        _lib.check(self._L.dint_tpl_client_consume(self._h, replies.ctypes.data))

    def peek(self, worker: int = 0):
        """(lids in ascending order, their types: 1 = exclusive) of the transaction `worker` is running"""
        lid, typ, n = (C.c_uint32 * 10)(), (C.c_uint8 * 10)(), C.c_uint32()
        _lib.check(self._L.dint_tpl_client_peek(self._h, worker, lid, typ, C.byref(n)))
        return list(lid[:n.value]), list(typ[:n.value])

    def stats(self) -> dict:
        s = TplClientStats()
        _lib.check(self._L.dint_tpl_client_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}


class LockClientConfig(C.Structure):
    """dint_lock_client_config (include/dint_driver.h): FasstClientConfig with the workload where it has reserved0"""
    _fields_ = [("n_workers", C.c_uint32), ("first_worker", C.c_uint32), ("key_space", C.c_uint32),
                ("read_pct", C.c_uint32), ("key_dist", C.c_uint32), ("workload", C.c_uint32),
                ("zipf_theta", C.c_double), ("reserved", C.c_uint32 * 8)]


class GpuLockClient:
    """The lock_fasst / lock_2pl load generator resident on the GPU (csrc/k_lock_client.hip, include/dint_driver.h
    dint_lock_gclient_*): the workers of :class:`FasstClient` / :class:`LcgTplClient`, one lane each.  ``next(stream)``
    emits the epoch's ``n`` requests (request i = worker i) into a device buffer (``batch_ptr``, refreshed by every
    ``next``: two buffers alternate), the lock server answers in place, ``consume(stream)`` feeds the replies back (on the
    stream of ``next``: fused into the next emit kernel).  The request stream is bit-identical to the host client's."""

    def __init__(self, workload: Workload, n_workers: int = 4096, key_space: int = 24_000_000, *, read_pct: int = 80,
                 zipf_theta: float | None = 0.8, first_worker: int = 0, device: int = -1):
        L = self._L = _lib.load()
        vp = C.c_void_p
        L.dint_lock_gclient_create.restype, L.dint_lock_gclient_create.argtypes = C.c_int, [C.POINTER(LockClientConfig), C.c_int32, C.POINTER(vp)]
        L.dint_lock_gclient_destroy.restype, L.dint_lock_gclient_destroy.argtypes = None, [vp]
        L.dint_lock_gclient_next.restype, L.dint_lock_gclient_next.argtypes = C.c_int, [vp, vp]
        L.dint_lock_gclient_consume.restype, L.dint_lock_gclient_consume.argtypes = C.c_int, [vp, vp]
        L.dint_lock_gclient_batch.restype, L.dint_lock_gclient_batch.argtypes = vp, [vp]
        L.dint_lock_gclient_read_batch.restype, L.dint_lock_gclient_read_batch.argtypes = C.c_int, [vp, vp]
        L.dint_lock_gclient_get_stats.restype, L.dint_lock_gclient_get_stats.argtypes = C.c_int, [vp, C.POINTER(FasstClientStats)]
        from .wire import MSG_DTYPE

        self.workload = Workload(workload)
        self.dtype, self.n = MSG_DTYPE[self.workload], n_workers
        cfg = LockClientConfig(n_workers=n_workers, first_worker=first_worker, key_space=key_space, read_pct=read_pct,
                               key_dist=0 if zipf_theta is None else 1, workload=int(workload), zipf_theta=zipf_theta or 0.0)
        h = vp()
        _lib.check(L.dint_lock_gclient_create(C.byref(cfg), device, C.byref(h)))
        self._h = h
        self.batch_ptr = L.dint_lock_gclient_batch(h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dint_lock_gclient_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter exit the HIP runtime may already be gone (module teardown order): the process is ending anyway
        if not sys.is_finalizing():
            self.close()

    def next(self, stream: int = 0):
        _lib.check(self._L.dint_lock_gclient_next(self._h, stream))
        self.batch_ptr = self._L.dint_lock_gclient_batch(self._h)  # the two buffers alternate

    def consume(self, stream: int = 0):
        _lib.check(self._L.dint_lock_gclient_consume(self._h, stream))

    def read_batch(self) -> np.ndarray:
        """host copy of the current batch (synchronises; tests and debugging)"""
        out = np.zeros(self.n, self.dtype)
        _lib.check(self._L.dint_lock_gclient_read_batch(self._h, out.ctypes.data))
        return out

    def stats(self) -> dict:
        """synchronises; lock_2pl has no rollbacks (the key is left out)"""
        s = FasstClientStats()
        _lib.check(self._L.dint_lock_gclient_get_stats(self._h, C.byref(s)))
        d = {k: getattr(s, k) for k, _ in s._fields_ if k != "reserved"}
        if self.workload == Workload.TPL:
            del d["rollbacks"]
        return d


def fasst_trace(server, n_requests: int = 24_000_000, **kw):
    """The lock_fasst request trace: closed loop of a FasstClient against `server` (an object with
    submit(ndarray) -> ndarray) until n_requests requests were issued.  Returns (requests, replies, client stats);
    the trace is a function of the client parameters alone as long as the server is correct."""
    c = FasstClient(**kw)
    reqs, reps, n = [], [], 0
    while n < n_requests:
        r = c.next()[:n_requests - n]  # the last epoch is cut: the server sees exactly n_requests requests
        p = server.submit(r)
        if len(r) == c.n:
            c.consume(p)
        reqs.append(r)
        reps.append(p)
        n += len(r)
    st = c.stats()
    return np.concatenate(reqs), np.concatenate(reps), st


class TplClient:
    """The lock_2pl load generator, W workers in lock step (numpy over the workers): lock_2pl/caladan/client.cc:167-240
    over transactions shaped by lock_2pl/caladan/trace_init.sh:6-27 -- 5..10 distinct locks in ascending order, each
    exclusive with probability 1 - read_prop -- acquire them one by one; a REJECT releases what the transaction holds
    (in acquisition order) and starts it again; once all are held, release them in reverse order.  ``next()`` = one
    6-byte request per worker, ``consume(replies)`` advances them.  Only granted locks are ever released, as in the
    reference."""

    ACQ, ROLL, REL = 0, 1, 2

    def __init__(self, n_workers: int = 4096, key_space: int = 24_000_000, *, read_prop: float = 0.8,
                 zipf_theta: float | None = 0.8, seed: int = 0xDEADBEEF):
        from .wire import TPL_MSG
        from .workloads import Zipf

        self.dtype, self.n, self.key_space, self.read_prop = TPL_MSG, n_workers, key_space, read_prop
        self.rng = np.random.default_rng(seed)
        self.z = Zipf(key_space, zipf_theta or 0.0, seed + 1)
        W = n_workers
        self.lid = np.zeros((W, 10), np.uint32)
        self.typ = np.zeros((W, 10), np.uint8)
        self.nlock = np.zeros(W, np.int64)
        self.mode = np.zeros(W, np.int64)
        self.pos = np.zeros(W, np.int64)   # ACQ: lock being acquired; ROLL: lock being released; REL: lock being released
        self.held = np.zeros(W, np.int64)  # locks the transaction holds (ROLL releases 0 .. held-1)
        self.stats_ = {"requests": 0, "committed": 0, "rejects": 0, "protocol_errors": 0}
        self._new_txn(np.arange(W))
        self._out = False

    def _new_txn(self, w):
        if len(w) == 0:
            return
        n = self.rng.integers(5, 11, len(w))
        k = self.z.sample((len(w), 10)).astype(np.uint32)
        k[np.arange(10)[None, :] >= n[:, None]] = 0xFFFFFFFF  # unused tail sorts last
        for _ in range(64):  # distinct lids per transaction (random.sample in trace_init.sh)
            k.sort(axis=1)
            dup = (k[:, 1:] == k[:, :-1]) & (k[:, 1:] != 0xFFFFFFFF)
            if not dup.any():
                break
            r, c = np.nonzero(dup)
            k[r, c + 1] = self.rng.integers(0, self.key_space, len(r))
        self.lid[w] = k
        self.typ[w] = (self.rng.random((len(w), 10)) >= self.read_prop).astype(np.uint8)
        self.nlock[w], self.mode[w], self.pos[w], self.held[w] = n, self.ACQ, 0, 0

    def next(self) -> np.ndarray:
        assert not self._out, "replies of the previous epoch are still outstanding"
        m = np.zeros(self.n, self.dtype)
        r = np.arange(self.n)
        m["action"] = (self.mode != self.ACQ).astype(np.uint8)  # 0 ACQUIRE, 1 RELEASE (lock_2pl/udp/net.h:11-16)
        m["lid"] = self.lid[r, self.pos]
        m["type"] = self.typ[r, self.pos]
        self._out = True
        self.stats_["requests"] += self.n
        return m

    def consume(self, rep: np.ndarray):
        a = rep["action"]
        acq, roll, rel = self.mode == self.ACQ, self.mode == self.ROLL, self.mode == self.REL
        self.stats_["protocol_errors"] += int((acq & ~np.isin(a, (2, 3))).sum() + ((roll | rel) & (a != 5)).sum())
        grant, rej = acq & (a == 2), acq & (a == 3)
        self.stats_["rejects"] += int(rej.sum())
        self.pos[grant] += 1
        self.held[grant] += 1
        full = grant & (self.pos == self.nlock)
        self.mode[full], self.pos[full] = self.REL, self.nlock[full] - 1
        rb = rej & (self.held > 0)          # release what is held, then start the transaction again
        self.mode[rb], self.pos[rb] = self.ROLL, 0
        # (a reject with nothing held: the same ACQUIRE goes out again)
        self.pos[roll] += 1
        done_roll = roll & (self.pos == self.held)
        self.mode[done_roll], self.pos[done_roll], self.held[done_roll] = self.ACQ, 0, 0
        self.pos[rel] -= 1
        fin = rel & (self.pos < 0)
        self.stats_["committed"] += int(fin.sum())
        self._new_txn(np.nonzero(fin)[0])
        self._out = False

    def stats(self) -> dict:
        return dict(self.stats_)


def tpl_trace(server, n_requests: int, **kw):
    """closed loop of a TplClient against `server` (submit(ndarray) -> ndarray) for n_requests requests"""
    c = TplClient(**kw)
    reqs, reps, n = [], [], 0
    while n < n_requests:
        r = c.next()[:n_requests - n]
        p = server.submit(r)
        if len(r) == c.n:
            c.consume(p)
        reqs.append(r)
        reps.append(p)
        n += len(r)
    return np.concatenate(reqs), np.concatenate(reps), c.stats()


def run_epochs(driver: Driver, servers, n_epochs: int, record: bool = False):
    """Closed loop: `servers` = 3 objects with submit(ndarray) -> ndarray (one per shard).
    Returns the recorded [(requests[3], replies[3])] per epoch when record=True."""
    trace = []
    for _ in range(n_epochs):
        req = driver.next()
        rep = [servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(N_SHARDS)]
        driver.consume(rep)
        if record:
            trace.append((req, rep))
    return trace
