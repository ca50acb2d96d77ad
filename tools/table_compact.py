#!/usr/bin/env python3
"""A churned server's tables compacted in place on the device (dint_state_compact through Engine.state_compact): the table
report before and after, and what the call costs next to state_verify and to a state_rehash into a blank engine of the same shape.

    tools/table_compact.py [--workload tatp|smallbank|both] [--rows N] [--repeats R] [--epochs E] [--timeout S]

The server is populated with N subscribers / accounts and has answered E closed-loop epochs of the transaction driver (rows
inserted and deleted, overflow entries freed and recycled), as in tools/table_verify.py.  One JSON object per workload:
  advice       recovery.compact_advice before the compaction (action, hole_share, pool_top_fill, load)
  before, after   per table what Engine.state_stats says: rows, entries, overflow_entries, holes, inline_first, pool_top, and
               hit_entries / rows -- header sectors per lookup of a stored row
  compact      Engine.state_compact's report per table (without the census)
  compact_ms   milliseconds of one state_compact call for ALL tables between HIP events on the stream the kernels run on (min /
               median / max of R runs after a warm one; every run starts from the same churned state, put back by
               Engine.restore outside the timed span; the call's host round trip is inside)
  verify_ms    the same for state_verify on the churned state
  rehash_ms    the same for state_rehash(drop_locks=True) of the churned server into a blank engine of the same n_rows (reset
               outside the timed span)
  stage_ms     one more compaction with timing_enable on: census, count and scans, move, commit, between events
  staging_bytes / engine_bytes   the staging buffers against the table memory a second engine of this shape needs
  same_rows    state_digest and every table's dump_rows are the same before and after; verify afterwards is clean

All GPU work happens in ONE child process under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEYS = ("rows", "entries", "overflow_entries", "holes", "inline_first", "inline_unlinked", "pool_top", "pool_cap")


def spread(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "runs": len(ms)}


def brief(stats):
    return [dict({k: t[k] for k in KEYS}, sectors_per_hit=round(t["hit_entries"] / t["rows"], 4) if t["rows"] else 0.0) for t in stats]


def child(a):
    import torch

    from dint_amd import recovery, wire
    from dint_amd.driver import Driver
    from dint_amd.engine import Engine

    stream = torch.cuda.Stream()  # (torch's default stream has handle 0, which the ABI reads as "the engine's own")
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    assert st != 0

    def timed(fn, repeats, before=lambda: None):
        before()
        fn()  # warm: kernel load, scratch allocation
        ms = []
        for _ in range(repeats):
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return spread(ms)

    ok = True
    for name in (("tatp", "smallbank") if a.workload == "both" else (a.workload,)):
        wl = wire.Workload.TATP if name == "tatp" else wire.Workload.SMALLBANK
        servers = [Engine(wl, n_rows=a.rows, log_entries=1 << 20) for _ in range(3)]
        for e in servers:
            e.populate(a.rows)
        d = Driver(wl, a.clients, a.rows, zipf_theta=0.8)
        for _ in range(a.epochs):
            req = d.next()
            d.consume([servers[s].submit(req[s]) if len(req[s]) else req[s] for s in range(3)])
        src = servers[0]
        for e in servers[1:]:
            e.close()
        del servers[1:]
        n_tab = len(src.state_stats())
        advice = recovery.compact_advice([src])
        before = src.state_stats()
        digest = src.state_digest()
        rows = [[x.tobytes() for x in src.dump_rows(t)] for t in range(n_tab)]
        src.snapshot()
        out = {"workload": name, "rows": a.rows, "epochs": a.epochs, "runs": "same box, one process",
               "advice": {k: advice[k] for k in ("action", "hole_share", "pool_top_fill", "pool_top_fill_after", "load", "locks_held")},
               "before": brief(before)}
        out["verify_ms"] = timed(lambda: src.state_verify(stream=st), a.repeats)
        out["compact_ms"] = timed(lambda: src.state_compact(stream=st), a.repeats, before=src.restore)
        rep = src.last_compact
        out["compact"] = [{k: v for k, v in r.items() if k != "verify"} for r in rep]
        after = src.state_stats()
        out["after"] = brief(after)
        clean = recovery.verify_tables([src])
        same = src.state_digest() == digest and all([x.tobytes() for x in src.dump_rows(t)] == rows[t] for t in range(n_tab))
        out["same_rows"] = bool(same and clean["clean"])
        out["staging_bytes"] = sum(r["staging_bytes"] for r in rep)
        stride = 256 if name == "tatp" else 128
        out["engine_bytes"] = sum((t["buckets"] + t["pool_cap"]) * stride for t in before)
        src.restore()
        src.timing_enable(True)
        src.state_compact(stream=st)
        out["stage_ms"] = {k: round(v / 1e6, 4) for k, v in src.last_compact_stage_ns.items()}
        src.timing_enable(False)
        src.restore()
        dst = Engine(wl, n_rows=a.rows, log_entries=1 << 12)
        out["rehash_ms"] = timed(lambda: dst.state_rehash([src], drop_locks=True, stream=st), a.repeats, before=dst.reset)
        ok = ok and out["same_rows"]
        print(json.dumps(out), flush=True)
        src.close(); dst.close()
        del src, dst, servers
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank", "both"), default="both")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--epochs", type=int, default=10, help="closed-loop epochs the server answers before the compaction")
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
