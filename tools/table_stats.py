#!/usr/bin/env python3
"""A server's table report from the device (dint_state_stats through Engine.state_stats) with the advice built on it, and what
the report costs next to the digest and to a plain stream over the same bytes.

    tools/table_stats.py [--workload tatp|smallbank|both] [--rows N] [--repeats R] [--epochs E] [--timeout S]

The server is populated with N subscribers / accounts and has answered E closed-loop epochs of the transaction driver (rows
inserted and deleted, lock words held).  One JSON object per workload:
  tables       Engine.state_stats per table, the histograms cut after their last used bin; sectors_per_hit = hit_entries / rows
  check        recovery.check_tables: the chain walk's row count beside the digest's flat one
  advice       recovery.rehash_advice (needed, n_rows, load per table, pool_fill, locks_held)
  stats_ms     milliseconds of one state_stats call for ALL tables between HIP events on the stream the kernels run on (min /
               median / max of R runs after a warm one; the call's one host round trip is inside)
  digest_ms    the same for state_digest
  header_bytes 64 B x (buckets + linked overflow entries): the header sectors the walk needs;  stream_rd_header_ms: what
               bench_access("stream_rd") takes over as many bytes;  entry_bytes / stream_rd_entries_ms: the same over all
               entry bytes (buckets + pool_top entries, whole stride -- what the digest streams)

All GPU work happens in ONE child process under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "runs": len(ms)}


def cut(hist):
    last = max((i for i, v in enumerate(hist) if v), default=0)
    return hist[:last + 1]


def child(a):
    import torch

    from dint_amd import recovery, wire
    from dint_amd.driver import Driver
    from dint_amd.engine import Engine, bench_access

    stream = torch.cuda.Stream()  # (torch's default stream has handle 0, which the ABI reads as "the engine's own")
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    assert st != 0

    def timed(fn, repeats):
        fn()  # warm: kernel load, scratch allocation
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return spread(ms)

    def stream_rd_ms(nbytes):
        nbytes = max(nbytes // 16 * 16, 1 << 20)
        bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)
        return round(bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)[1] * 1e3, 4)

    ok = True
    for name in (("tatp", "smallbank") if a.workload == "both" else (a.workload,)):
        tatp = name == "tatp"
        wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
        stride = 256 if tatp else 128
        servers = [Engine(wl, n_rows=a.rows, log_entries=1 << 20) for _ in range(3)]
        for e in servers:
            e.populate(a.rows)
        d = Driver(wl, a.clients, a.rows, zipf_theta=0.8)
        for _ in range(a.epochs):
            req = d.next()
            d.consume([servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(3)])
        src = servers[0]
        del servers[1:]
        tables = src.state_stats(stream=st)
        check = recovery.check_tables(src)
        adv = recovery.rehash_advice([src])
        header_bytes = 64 * sum(t["buckets"] + t["overflow_entries"] for t in tables)
        entry_bytes = stride * sum(t["buckets"] + t["pool_top"] for t in tables)
        out = {"workload": name, "rows": a.rows, "epochs": a.epochs, "runs": "same box, one process",
               "tables": [dict({k: v for k, v in t.items() if not k.endswith("_hist")}, chain_hist=cut(t["chain_hist"]), rows_hist=cut(t["rows_hist"]),
                               sectors_per_hit=round(t["hit_entries"] / max(1, t["rows"]), 4)) for t in tables],
               "check": {"ok": check["ok"], "rows": [t["rows"] for t in check["tables"]], "digest_rows": [t["digest_rows"] for t in check["tables"]]},
               "advice": {k: adv[k] for k in ("needed", "n_rows", "load", "pool_fill", "locks_held")},
               "stats_ms": timed(lambda: src.state_stats(stream=st), a.repeats),
               "digest_ms": timed(lambda: src.state_digest(stream=st), a.repeats),
               "header_bytes": header_bytes, "stream_rd_header_ms": stream_rd_ms(header_bytes),
               "entry_bytes": entry_bytes, "stream_rd_entries_ms": stream_rd_ms(entry_bytes)}
        out["header_GBps"] = round(header_bytes / 1e6 / out["stats_ms"]["median"], 1)
        ok = ok and check["ok"]
        print(json.dumps(out), flush=True)
        src.close()
        del src, servers
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank", "both"), default="both")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="closed-loop epochs the server answers before the report")
    ap.add_argument("--clients", type=int, default=20_000)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--rows", str(a.rows), "--repeats", str(a.repeats), "--epochs", str(a.epochs), "--clients", str(a.clients)]
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
