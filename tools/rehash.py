#!/usr/bin/env python3
"""Rehash a server's tables to another bucket count on the device (dint_state_rehash through Engine.state_rehash) next to the
host way (dump_rows of the source + load_rows into blank engines of the new size).

    tools/rehash.py [--workload tatp|smallbank] [--rows N] [--case x2|half|shards|all] [--repeats R] [--epochs E] [--timeout S]

The source is one server populated with N subscribers / accounts that has answered E closed-loop epochs of the transaction
driver (rows inserted and deleted, lock words held: they are dropped); all engines live on the one GPU.  Cases: x2 = a blank
engine of 2 N rows, half = of N / 2 rows, shards = 8 blank shards of 2 N rows.  One JSON object per case:
  device       milliseconds of the whole rehash (every destination takes the source; HIP events on the stream the kernels run
               on; min / median / max of R runs after a warm one, the destinations reset before each -- the host round trips of
               each call are inside), and the medians of the stages between events of their own: count, keys, sort, plan, build
  entry_bytes  what the source's linked entries hold, and GB/s of it over the median
  stream_rd    bench_access("stream_rd") over as many bytes -- the yardstick of a stream
  host         dump_rows of the source, the numpy selection, load_rows into fresh destinations (wall clock, one run)
  ok           the destinations' digests add up to the source's after every run

All GPU work happens in ONE child process under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"x2": (2.0, 1), "half": (0.5, 1), "shards": (2.0, 8)}


def spread(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "runs": len(ms)}


def child(a):
    import ctypes as C

    import numpy as np
    import torch

    from dint_amd import _lib, recovery, wire
    from dint_amd.driver import Driver
    from dint_amd.engine import Engine, bench_access

    tatp = a.workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    tables, stride = (5, 256) if tatp else (2, 128)
    stream = torch.cuda.Stream()  # (torch's default stream has handle 0, which the ABI reads as "the engine's own")
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    assert st != 0

    def bucket_of(keys, hash_size):
        def mix(h):
            h = h ^ (h >> np.uint64(23))
            h = h * np.uint64(0x2127599BF4325C37)
            return h ^ (h >> np.uint64(47))

        m = np.uint64(0x880355F21E6D1965)
        with np.errstate(over="ignore"):
            h = (np.uint64(0xDEADBEEF) ^ (np.uint64(8) * m) ^ mix(np.asarray(keys, np.uint64))) * m
            return mix(h) % np.uint64(hash_size)

    servers = [Engine(wl, n_rows=a.rows, log_entries=1 << 20) for _ in range(3)]
    for e in servers:
        e.populate(a.rows)
    d = Driver(wl, a.clients, a.rows, zipf_theta=0.8)
    for _ in range(a.epochs):
        req = d.next()
        d.consume([servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(3)])
    src = servers[0]
    del servers[1:]
    want = src.state_digest()
    s = _lib.ImageStats()
    _lib.check(src._L.dint_state_export(src._h, 0, 1, None, 0, C.byref(s), st))  # (a count: the entries the chains hold)
    entry_bytes = int(s.buckets + s.overflow_entries) * stride
    bench_access(entry_bytes, entry_bytes // 16, "stream_rd", 16, 16)
    rd = bench_access(entry_bytes, entry_bytes // 16, "stream_rd", 16, 16)[0] * 16 / 1e9

    def timed(fn, before=None):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        return r, e0.elapsed_time(e1)

    all_ok = True
    for case in (CASES if a.case == "all" else [a.case]):
        factor, H = CASES[case]
        n_new = max(1, int(a.rows * factor))

        def layout():
            # (a pool that takes every row: what a caller sizes from a refused call's need)
            return [Engine(wl, n_rows=n_new, shard_index=j, shard_count=H, log_entries=1 << 12, max_pass=65536,
                           pool_entries=max(4096, int(s.rows) // (3 * H))) for j in range(H)]

        dst = layout()
        for e in dst:
            e.timing_enable(True)

        def reset():
            for e in dst:
                e.reset()

        def move():
            return [e.state_rehash([src], drop_locks=True, stream=st) for e in dst]

        per, _ = timed(move, reset)  # warm: kernel load, scratch allocation
        ok = recovery.digest_sum(dst) == want
        ms, stages = [], []
        for _ in range(a.repeats):
            per, t = timed(move, reset)
            ms.append(t)
            stages.append({k: sum(p["stage_ns"][k] for p in per) / 1e6 for k in per[0]["stage_ns"]})
        ok = ok and recovery.digest_sum(dst) == want
        med = statistics.median(ms)
        out = {"workload": a.workload, "rows": a.rows, "case": case, "n_rows_new": n_new, "dst_shards": H, "runs": "same box, one process",
               "rows_moved": per[0]["rows_seen"], "locks_dropped": per[0]["locks_held"],
               "overflow_entries": sum(t["overflow_entries"] for p in per for t in p["tables"]),
               "longest_chain": max(t["longest_chain"] for p in per for t in p["tables"]),
               "device": {"ms": spread(ms), "stage_ms_median": {k: round(statistics.median(x[k] for x in stages), 4) for k in stages[0]},
                          "Mrows_per_s": round(per[0]["rows_seen"] * H / 1e3 / med, 1)},
               "entry_bytes": entry_bytes, "entry_GBps": round(entry_bytes * H / 1e6 / med, 1), "stream_rd_GBps": round(rd, 1)}
        if not a.no_host:
            del dst
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dumps = [src.dump_rows(t) for t in range(tables)]
            t1 = time.perf_counter()
            fresh = layout()
            t2 = time.perf_counter()
            for t in range(tables):
                keys, vers, vals = dumps[t]
                home = (bucket_of(keys, fresh[0].hash_size(t)) % np.uint64(H)).astype(np.int64)
                for j in range(H):
                    m = home == j
                    if m.any():
                        fresh[j].load_rows(t, keys[m], vers[m], vals[m])
            for e in fresh:
                e.sync()
            t3 = time.perf_counter()
            rows_ok = recovery.digest_sum(fresh) == want
            out["host"] = {"dump_rows_s": round(t1 - t0, 3), "select_and_load_rows_s": round(t3 - t2, 3), "total_s": round(t1 - t0 + t3 - t2, 3),
                           "rows_equal": rows_ok, "speedup_of_device": round((t1 - t0 + t3 - t2) * 1e3 / med, 1)}
            ok = ok and rows_ok
            del fresh
        out["ok"] = bool(ok)
        all_ok = all_ok and ok
        print(json.dumps(out), flush=True)
    return 0 if all_ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank"), default="tatp")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--case", choices=tuple(CASES) + ("all",), default="all")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="closed-loop epochs the source answers before the rehash")
    ap.add_argument("--clients", type=int, default=20_000)
    ap.add_argument("--no-host", action="store_true", help="skip the dump_rows + load_rows comparison")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--rows", str(a.rows), "--case", a.case, "--repeats", str(a.repeats), "--epochs", str(a.epochs),
           "--clients", str(a.clients)] + (["--no-host"] if a.no_host else [])
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
