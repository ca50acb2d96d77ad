#!/usr/bin/env python3
"""What it costs to find the locks a server holds and to release them: on the device (dint_state_locks / dint_state_unlock through
Engine.state_locks / Engine.state_unlock) beside the only way there was before -- dint_read_locks, numpy, and forged wire
releases -- and beside a plain stream over the bytes the listing must read.

    tools/lock_sweep.py [--workload fasst|tpl|tatp|smallbank|all] [--slots N] [--rows N] [--held K] [--repeats R] [--timeout S]

The server is populated (kv) and K locks are left held through ordinary ACQUIRE requests on known keys, so that the old way has
a key to forge its releases with.  One JSON object per workload, every time the wall-clock milliseconds of the synchronous call
(min / median / max of R runs after a warm one):
  held                 units held when the listing runs (requests on one unit grant one lock)
  state_locks_ms       Engine.state_locks into a buffer that fits: count, scan, write, one host synchronisation
  count_only_ms        ... without a buffer
  state_unlock_ms      Engine.state_unlock of the full list (the locks are taken again before every run)
  unlock_all_ms        Engine.state_unlock(all=True)
  read_locks_numpy_ms  Engine.read_locks of every table and the search for the held units in numpy
  wire_release_ms      the matching release requests through Engine.submit
  listed_bytes         the bytes the listing must read: 8 B a slot, or one 64-byte sector a bucket;  stream_rd_ms: what
                       bench_access("stream_rd") takes over as many bytes
  images_equal         a twin released by wire requests and this server released by state_unlock export equal images

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


def child(a):
    import numpy as np
    import torch

    from dint_amd import wire
    from dint_amd.engine import Engine, bench_access, lock_records

    W = wire.Workload
    names = {"fasst": W.FASST, "tpl": W.TPL, "tatp": W.TATP, "smallbank": W.SMALLBANK}

    def timed(fn, repeats, setup=None):
        ms = []
        for k in range(repeats + 1):  # (the first run is warm-up: kernel load, scratch allocation)
            if setup:
                setup()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return spread(ms[1:])

    def stream_rd_ms(nbytes):
        nbytes = max(nbytes // 16 * 16, 1 << 20)
        bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)
        return round(bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)[1] * 1e3, 4)

    def server(wl):
        if wl in (W.FASST, W.TPL):
            return Engine(wl, n_slots=a.slots)
        e = Engine(wl, n_rows=a.rows, log_entries=1 << 16)
        e.populate(a.rows)
        return e

    def acquire(wl, keys):
        m = np.zeros(len(keys), wire.MSG_DTYPE[wl])
        if wl == W.FASST:
            m["type"], m["lid"] = wire.Fasst.ACQUIRE_LOCK, keys
        elif wl == W.TPL:
            m["action"], m["type"], m["lid"] = wire.Tpl.ACQUIRE_LOCK, wire.Tpl.EXCLUSIVE, keys
        elif wl == W.TATP:
            m["type"], m["key"] = wire.Tatp.ACQUIRE_LOCK, keys
        else:
            m["type"], m["key"] = wire.Sb.ACQUIRE_EXCLUSIVE, keys
        return m

    def release(wl, keys):
        m = acquire(wl, keys)
        if wl == W.FASST:
            m["type"] = wire.Fasst.ABORT
        elif wl == W.TPL:
            m["action"] = wire.Tpl.RELEASE_LOCK
        elif wl == W.TATP:
            m["type"] = wire.Tatp.ABORT
        else:
            m["type"] = wire.Sb.RELEASE_EXCLUSIVE
        return m

    def image(e):
        buf, n, _ = e.state_export(0, 1)
        return buf[:n].cpu().numpy().tobytes()

    ok = True
    for name in (tuple(names) if a.workload == "all" else (a.workload,)):
        wl = names[name]
        kv = wl in (W.TATP, W.SMALLBANK)
        src, twin = server(wl), server(wl)
        keys = np.arange(a.held, dtype=np.uint64) * np.uint64(7919) % np.uint64(a.rows if kv else 1 << 31)  # (table 0's keys are 0 .. rows - 1)
        acq = acquire(wl, keys)
        grant = {W.FASST: wire.Fasst.GRANT_LOCK, W.TPL: wire.Tpl.GRANT_LOCK, W.TATP: wire.Tatp.GRANT_LOCK, W.SMALLBANK: wire.Sb.GRANT_EXCLUSIVE}[wl]
        rep = src.submit(acq)
        got = keys[(rep["action"] if wl == W.TPL else rep["type"]) == grant]  # the keys that hold a unit each
        twin.submit(acq)
        rel = release(wl, got)
        again = acquire(wl, got)
        _, _, st = src.state_locks()
        held = st["total"]
        buf = torch.empty((held + 1, 32), dtype=torch.uint8, device="cuda")
        n_tab = {W.FASST: 1, W.TPL: 1, W.TATP: 5, W.SMALLBANK: 2}[wl]

        def old_way():
            found = 0
            for t in range(n_tab):
                x, y = src.read_locks(t)
                found += len(np.flatnonzero(x if wl == W.FASST else (x | y)))
            return found

        listed_bytes = 8 * a.slots if not kv else 64 * sum(src.hash_size(t) for t in range(n_tab))
        out = {"workload": name, "slots": a.slots if not kv else None, "rows": a.rows if kv else None, "held": held, "runs": "same box, one process",
               "state_locks_ms": timed(lambda: src.state_locks(buf, held), a.repeats),
               "count_only_ms": timed(lambda: src._L.dint_state_locks(src._h, None, 0, None, None), a.repeats),
               "read_locks_numpy_ms": timed(old_way, a.repeats),
               "listed_bytes": listed_bytes, "stream_rd_ms": stream_rd_ms(listed_bytes)}
        ok = ok and old_way() == held == len(got)
        _, n, _ = src.state_locks(buf, held)
        out["state_unlock_ms"] = timed(lambda: src.state_unlock(buf, n), a.repeats, setup=lambda: src.submit(again))
        out["unlock_all_ms"] = timed(lambda: src.state_unlock(all=True), a.repeats, setup=lambda: src.submit(again))
        out["wire_release_ms"] = timed(lambda: twin.submit(rel), a.repeats, setup=lambda: twin.submit(again))
        out["first_records"] = [{k: int(r[k]) for k in r.dtype.names if k != "zero"} for r in lock_records(buf, min(n, 2))]
        out["images_equal"] = image(src) == image(twin)
        out["listed_GBps"] = round(listed_bytes / 1e6 / out["state_locks_ms"]["median"], 1)
        ok = ok and out["images_equal"] and src.state_locks()[2]["total"] == 0
        print(json.dumps(out), flush=True)
        src.close(); twin.close()
        del src, twin, buf
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("fasst", "tpl", "tatp", "smallbank", "all"), default="all")
    ap.add_argument("--slots", type=int, default=36_000_000, help="lock tables: n_slots")
    ap.add_argument("--rows", type=int, default=1_000_000, help="tatp / smallbank: subscribers / accounts")
    ap.add_argument("--held", type=int, default=10_000, help="ACQUIRE requests that leave their lock held")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--slots", str(a.slots), "--rows", str(a.rows), "--held", str(a.held), "--repeats", str(a.repeats)]
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
