#!/usr/bin/env python3
"""A server's tables and overflow pool verified on the device (dint_state_verify through Engine.state_verify), the verdict, and
what the census costs next to the table report, the digest and a plain stream over the header bytes its chain stage needs.

    tools/table_verify.py [--workload tatp|smallbank|both] [--rows N] [--repeats R] [--epochs E] [--timeout S]

The server is populated with N subscribers / accounts and has answered E closed-loop epochs of the transaction driver (rows
inserted and deleted, overflow entries freed and recycled).  One JSON object per workload:
  verdict      recovery.verify_tables: ok (no violation), clean (ok and nothing unaccounted)
  tables       Engine.state_verify per table
  verify_ms    milliseconds of one state_verify call for ALL tables between HIP events on the stream the kernels run on (min /
               median / max of R runs after a warm one; the call's one host round trip is inside)
  stats_ms, digest_ms   the same for state_stats and state_digest
  stage_ms     one more call with timing_enable on: the chain stage, the list stage, the pool stage and sum, between events
  longest_list the longest free or pend list: the list stage is one chain of dependent loads per list
  header_bytes 64 B x (buckets + linked overflow entries): the header sectors the chain stage needs;  stream_rd_header_ms:
               what bench_access("stream_rd") takes over as many bytes

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
        servers = [Engine(wl, n_rows=a.rows, log_entries=1 << 20) for _ in range(3)]
        for e in servers:
            e.populate(a.rows)
        d = Driver(wl, a.clients, a.rows, zipf_theta=0.8)
        for _ in range(a.epochs):
            req = d.next()
            d.consume([servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(3)])
        src = servers[0]
        del servers[1:]
        verdict = recovery.verify_tables([src])
        tables = verdict["tables"]
        buckets = [src.hash_size(t) for t in range(len(tables))]
        header_bytes = 64 * sum(b + t["linked"] for b, t in zip(buckets, tables))
        out = {"workload": name, "rows": a.rows, "epochs": a.epochs, "runs": "same box, one process",
               "verdict": {"ok": verdict["ok"], "clean": verdict["clean"]}, "tables": tables,
               "longest_list": max(t["longest_list"] for t in tables),
               "verify_ms": timed(lambda: src.state_verify(stream=st), a.repeats),
               "stats_ms": timed(lambda: src.state_stats(stream=st), a.repeats),
               "digest_ms": timed(lambda: src.state_digest(stream=st), a.repeats),
               "header_bytes": header_bytes, "stream_rd_header_ms": stream_rd_ms(header_bytes)}
        src.timing_enable(True)
        src.state_verify(stream=st)
        out["stage_ms"] = {k: round(v / 1e6, 4) for k, v in src.last_verify_stage_ns.items()}
        src.timing_enable(False)
        out["header_GBps"] = round(header_bytes / 1e6 / out["verify_ms"]["median"], 1)
        ok = ok and verdict["ok"]
        print(json.dumps(out), flush=True)
        src.close()
        del src, servers
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank", "both"), default="both")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="closed-loop epochs the server answers before the census")
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
