#!/usr/bin/env python3
"""Populate a server on the device (dint_populate_device through Engine.populate_device) next to the host way (dint_populate).

    tools/populate.py [--workload store|tatp|smallbank] [--rows N ...] [--shards H] [--repeats R] [--timeout S]

Per size N (0 = the reference's: store 2M, tatp 7M, smallbank 24M) one engine of n_rows = N is populated with N subscribers /
accounts by both ways in turn, `reset` between them, R times after a warm run of each.  One JSON object per size:
  host      milliseconds of Engine.populate (wall clock: the generator runs on one core and every pass is synchronous)
  device    milliseconds of Engine.populate_device (wall clock, the host round trips of every table inside), and the medians of the
            stages between HIP events on the stream the kernels run on: generate, keys, sort, plan, build
  prepass   milliseconds of the host pre-pass over the two data-dependent tatp tables, paid once per process (the warm run)
  temp_mb   peak temporary device memory of the device way
  ok        the digests after the two ways are equal, every run
With --shards H an H-shard set on the one GPU is populated as well (recovery.populate_set against populate on every shard).

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

REF_ROWS = {"store": 2_000_000, "tatp": 7_000_000, "smallbank": 24_000_000}


def spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3), "runs": len(ms)}


def child(a):
    import torch

    from dint_amd import recovery, wire
    from dint_amd.engine import Engine

    wl = {"store": wire.Workload.STORE, "tatp": wire.Workload.TATP, "smallbank": wire.Workload.SMALLBANK}[a.workload]

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    for rows in a.rows:
        n = rows or REF_ROWS[a.workload]
        out = {"workload": a.workload, "rows": n}
        sets = [[Engine(wl, n_rows=n)]]
        if a.shards > 1:
            sets.append([Engine(wl, n_rows=n, shard_index=i, shard_count=a.shards) for i in range(a.shards)])
        for engines in sets:
            host, devc, stages, ok, prepass, temp = [], [], [], True, None, 0
            for run in range(a.repeats + 1):
                for e in engines:
                    e.timing_enable(False)  # (the host way's passes are timed by the clock alone)
                ms_h, _ = wall(lambda: [e.populate(n) for e in engines])
                want = recovery.digest_sum(engines)
                for e in engines:
                    e.reset()
                    e.timing_enable(True)
                ms_d, r = wall(lambda: recovery.populate_set(engines, n))
                ok = ok and recovery.digest_sum(engines) == want and all(p["direct"] == 1 for p in r["per_engine"])
                for e in engines:
                    e.reset()
                if run == 0:  # the warm run: it pays the pre-pass
                    prepass = r["per_engine"][0]["stage_ns"]["prepass"] / 1e6
                    continue
                host.append(ms_h)
                devc.append(ms_d)
                temp = max(temp, r["temp_bytes"])
                stages.append({k: sum(p["stage_ns"][k] for p in r["per_engine"]) / 1e6 for k in ("generate", "keys", "sort", "plan", "build")})
            rep = {"host_ms": spread(host), "device_ms": spread(devc), "prepass_ms": round(prepass, 3), "temp_mb": round(temp / 2**20, 1), "ok": ok,
                   "stage_ms": {k: round(statistics.median(s[k] for s in stages), 3) for k in stages[0]}}
            out["set_of_%d" % len(engines) if len(engines) > 1 else "one"] = rep
            for e in engines:
                e.close()
        print(json.dumps(out), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workload", choices=sorted(REF_ROWS), default="tatp")
    p.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 0])
    p.add_argument("--shards", type=int, default=1)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--timeout", type=int, default=900)
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "time limit of %d s" % a.timeout}))
        return 124


if __name__ == "__main__":
    sys.exit(main())
