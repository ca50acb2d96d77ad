#!/usr/bin/env python3
"""Move a server's tables from G shards to H shards on the device (dint_state_export / dint_state_import through
recovery.reshard) next to the host way (dump_rows of the sources + load_rows into fresh destinations: rows only).

    tools/reshard.py [--workload tatp|smallbank] [--rows N] [--src G] [--dst H] [--repeats R] [--epochs E] [--timeout S]

The source set is populated with N subscribers / accounts and answers E closed-loop epochs of the transaction driver (lock
words held, rows inserted and deleted); all engines live on the one GPU.  Printed as one JSON object:
  device       milliseconds of the whole move (every compatible piece exported into one HBM buffer and imported from it; HIP
               events on the stream the kernels run on; min / median / max of R runs after a warm one, the destinations reset
               before each), the image bytes moved, GB/s of image and of memory traffic (every entry is read and written
               once by the export and once by the import: 4 x the image), and where the time goes: the count pass alone and the
               exports (medians of R runs each), the imports by difference.  Every call synchronises on the host, so
               the time between the events includes the host round trips of each piece
  stream_rd    bench_access("stream_rd") over the image's bytes -- the yardstick of a stream
  host         dump_rows of the sources, the numpy selection, load_rows into fresh destinations (wall clock, one run)
  ok           the destinations' digests add up to the sources' after every move

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


def spread(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "runs": len(ms)}


def digest_sum(engines):
    out = None
    for e in engines:
        d = e.state_digest()
        if out is None:
            out = [dict(x) for x in d]
        else:
            for x, y in zip(out, d):
                x["rows"] += y["rows"]; x["sum"] = (x["sum"] + y["sum"]) % (1 << 64); x["xr"] ^= y["xr"]
    return out


def child(a):
    import numpy as np
    import torch

    from dint_amd import recovery, wire
    from dint_amd.driver import Driver
    from dint_amd.engine import Engine, bench_access

    tatp = a.workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    tables = 5 if tatp else 2
    stream = torch.cuda.Stream()  # (torch's default stream has handle 0, which the ABI reads as "the engine's own")
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    assert st != 0
    G, H = a.src, a.dst

    def layout(n, **kw):
        return [Engine(wl, n_rows=a.rows, shard_index=s, shard_count=n, log_entries=1 << 20, **kw) for s in range(n)]

    def bucket_of(keys, hash_size):
        def mix(h):
            h = h ^ (h >> np.uint64(23))
            h = h * np.uint64(0x2127599BF4325C37)
            return h ^ (h >> np.uint64(47))

        m = np.uint64(0x880355F21E6D1965)
        with np.errstate(over="ignore"):
            h = (np.uint64(0xDEADBEEF) ^ (np.uint64(8) * m) ^ mix(np.asarray(keys, np.uint64))) * m
            return mix(h) % np.uint64(hash_size)

    # the source: one unsharded server of the three the driver talks to, after a short closed loop -- then, for G > 1, moved
    # into G shards by the call under test (checked by digest like every move)
    servers = [Engine(wl, n_rows=a.rows, log_entries=1 << 20) for _ in range(3)]
    for e in servers:
        e.populate(a.rows)
    d = Driver(wl, a.clients, a.rows, zipf_theta=0.8)
    for _ in range(a.epochs):
        req = d.next()
        d.consume([servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(3)])
    one = servers[0]
    del servers[1:]
    want = one.state_digest()
    src = [one]
    if G > 1:
        src = layout(G, max_pass=65536)
        recovery.reshard([one], src)
        assert digest_sum(src) == want
    dst = layout(H, max_pass=65536)
    pieces = recovery.image_pieces(G, H)
    import ctypes as C

    from dint_amd import _lib
    s = _lib.ImageStats()

    def count(i, j):  # the count pass alone: the piece's size
        _lib.check(src[i]._L.dint_state_export(src[i]._h, j, H, None, 0, C.byref(s), st))
        return int(s.bytes)

    buf = torch.empty(max(count(i, j) for i, j in pieces), dtype=torch.uint8, device="cuda")  # one buffer for every piece

    def reset():
        for e in dst:
            e.reset()

    def move():
        tot = {"bytes": 0, "pieces": 0}
        for i, j in pieces:
            _, n, _ = src[i].state_export(j, H, buf, stream=st)
            dst[j].state_import(buf, n, stream=st)
            tot["bytes"] += n
            tot["pieces"] += 1
        return tot

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

    ok = True
    tot, _ = timed(move, reset)  # warm: kernel load, scratch allocation
    ok = ok and digest_sum(dst) == want
    ms = []
    for _ in range(a.repeats):
        ms.append(timed(move, reset)[1])
    ok = ok and digest_sum(dst) == want
    nbytes = tot["bytes"]
    med = statistics.median(ms)
    # where the time goes (medians of as many runs): the count pass alone, all exports; the imports by difference
    count_ms = statistics.median(timed(lambda: [count(i, j) for i, j in pieces])[1] for _ in range(a.repeats))
    export_ms = statistics.median(timed(lambda: [src[i].state_export(j, H, buf, stream=st) for i, j in pieces])[1] for _ in range(a.repeats))
    import_ms = max(0.0, med - export_ms)
    bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)
    rd = bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)[0] * 16 / 1e9
    out = {"workload": a.workload, "rows": a.rows, "src": G, "dst": H, "pieces": tot["pieces"], "image_bytes": nbytes,
           "runs": "same box, one process",
           "device": {"ms": spread(ms), "image_GBps": round(nbytes / 1e6 / med, 1), "traffic_GBps": round(4 * nbytes / 1e6 / med, 1),
                      "count_only_ms": round(count_ms, 4), "export_ms": round(export_ms, 4), "import_ms_by_difference": round(import_ms, 4)},
           "stream_rd_GBps": round(rd, 1), "traffic_fraction_of_stream_rd": round(4 * nbytes / 1e6 / med / rd, 3)}

    # the host way: rows only
    if not a.no_host:
        del dst
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dumps = [[e.dump_rows(t) for e in src] for t in range(tables)]
        t1 = time.perf_counter()
        fresh = layout(H, max_pass=65536)
        t2 = time.perf_counter()
        for t in range(tables):
            hs = src[0].hash_size(t)
            for keys, vers, vals in dumps[t]:
                home = (bucket_of(keys, hs) % np.uint64(H)).astype(np.int64)
                for j in range(H):
                    m = home == j
                    if m.any():
                        fresh[j].load_rows(t, keys[m], vers[m], vals[m])
        for e in fresh:
            e.sync()
        t3 = time.perf_counter()
        rows_ok = digest_sum(fresh) == want
        out["host"] = {"dump_rows_s": round(t1 - t0, 3), "select_and_load_rows_s": round(t3 - t2, 3), "total_s": round(t1 - t0 + t3 - t2, 3),
                       "rows_equal": rows_ok, "speedup_of_device": round((t1 - t0 + t3 - t2) * 1e3 / med, 1)}
        ok = ok and rows_ok
    out["ok"] = bool(ok)
    print(json.dumps(out), flush=True)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank"), default="tatp")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--src", type=int, default=1, help="shards of the source layout (G)")
    ap.add_argument("--dst", type=int, default=8, help="shards of the destination layout (H)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="closed-loop epochs the source answers before the move")
    ap.add_argument("--clients", type=int, default=20_000)
    ap.add_argument("--no-host", action="store_true", help="skip the dump_rows + load_rows comparison")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--rows", str(a.rows), "--src", str(a.src), "--dst", str(a.dst), "--repeats", str(a.repeats), "--epochs", str(a.epochs),
           "--clients", str(a.clients)] + (["--no-host"] if a.no_host else [])
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
