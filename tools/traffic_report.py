#!/usr/bin/env python3
"""A batch's traffic report from the device (dint_traffic_report through Engine.traffic_report), and what the report costs next to
the pass that answers the batch and to a plain stream over the same bytes.

    tools/traffic_report.py --workload fasst|2pl|store|tatp|smallbank [--rows N] [--requests n] [--zipf THETA] [--top K]

The server is created for N rows (lock tables: N slots) and populated.  The batch: lock_fasst / lock_2pl / store -- n requests on
Zipf(THETA) keys (dint_amd.workloads.Zipf), a mix of the workload's request types; tatp / smallbank -- the messages one epoch of
the closed-loop driver (dint_amd.driver.Driver, Zipf(THETA) keys) sends to shard 0, as many clients as give about n messages.
The batch is submitted once with a reply buffer of its own, the report of (requests, replies) is printed as a table, then one
JSON object:
  report_ms     milliseconds of one traffic_report call between HIP events on the stream its kernels run on (min / median /
                max of 7 runs after a warm one; the call's three host round trips are inside)
  bytes, stream_rd_ms   the bytes of the two arrays, and what bench_access("stream_rd") takes over as many
  pass_kernel_us        the pass's own kernel time for the same batch (dint_timing_read: avg_us x launches over its kernels)
  report_over_pass      report_ms / pass kernel time
  temp_bytes            the call's temporary device memory

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


def make_batch(a, wl):
    import numpy as np

    from dint_amd import wire
    from dint_amd.driver import Driver
    from dint_amd.workloads import Zipf

    W = wire.Workload
    if wl in (W.TATP, W.SMALLBANK):
        clients = max(64, a.requests * 3 // (2 if wl == W.TATP else 1))
        req = Driver(wl, clients, a.rows, zipf_theta=a.zipf).next()[0]
        return req[:a.requests]
    rng = np.random.default_rng(1)
    keys = Zipf(a.rows, a.zipf, seed=2).sample(a.requests)
    m = np.zeros(a.requests, wire.MSG_DTYPE[wl])
    if wl == W.STORE:  # the population's keys: s_id | sf_type 1..4 << 32 | start_time 0 / 8 / 16 << 40 (store/udp/tatp.h:44-66)
        sf, st = rng.integers(1, 5, a.requests, dtype=np.uint64), rng.integers(0, 3, a.requests, dtype=np.uint64) * np.uint64(8)
        m["key"], m["type"] = keys | (sf << np.uint64(32)) | (st << np.uint64(40)), rng.choice([0, 0, 0, 1], a.requests)
    elif wl == W.FASST:
        m["lid"], m["type"] = keys, rng.choice([0, 0, 0, 1, 2, 3], a.requests)
    else:
        m["lid"], m["action"], m["type"] = keys, rng.choice([0, 0, 1], a.requests), rng.integers(0, 2, a.requests)
    return m


def child(a):
    import numpy as np
    import torch

    from dint_amd import traffic, wire
    from dint_amd.engine import Engine, bench_access

    W = wire.Workload
    wl = {"fasst": W.FASST, "2pl": W.TPL, "store": W.STORE, "tatp": W.TATP, "smallbank": W.SMALLBANK}[a.workload]
    stream = torch.cuda.Stream()  # (torch's default stream has handle 0, which the ABI reads as "the engine's own")
    torch.cuda.set_stream(stream)
    st = stream.cuda_stream
    eng = Engine(wl, n_slots=a.rows, n_rows=a.rows, log_entries=1 << 20)
    if wl in (W.STORE, W.TATP, W.SMALLBANK):
        eng.populate_device(a.rows)
    req = make_batch(a, wl)
    n = len(req)
    d_req = torch.from_numpy(np.frombuffer(req.tobytes(), np.uint8).copy()).cuda()
    d_rep = torch.zeros_like(d_req)
    eng.submit_device(d_req, n, d_rep, st)  # warm
    eng.sync()
    eng.timing_enable(True)
    eng.submit_device(d_req, n, d_rep, st)
    torch.cuda.synchronize()
    pass_us = sum(v["avg_us"] * v["launches"] for v in eng.timing_read().values())
    eng.timing_enable(False)

    rep = eng.traffic_report(d_req, n, d_rep, top=a.top, stream=st)  # warm: kernel load, scratch allocation
    print(traffic.format_report(rep), flush=True)
    ms = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        eng.traffic_report(d_req, n, d_rep, top=a.top, stream=st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    nbytes = 2 * d_req.numel()
    sb = max(nbytes // 16 * 16, 1 << 20)
    bench_access(sb, sb // 16, "stream_rd", 16, 16)
    out = {"workload": a.workload, "rows": a.rows, "requests": n, "zipf": a.zipf, "top": a.top, "report_ms": spread(ms), "bytes": nbytes,
           "stream_rd_bytes": sb, "stream_rd_ms": round(bench_access(sb, sb // 16, "stream_rd", 16, 16)[1] * 1e3, 4),
           "pass_kernel_us": round(pass_us, 1), "temp_bytes": rep["temp_bytes"], "runs": "same box, one process"}
    out["report_over_pass"] = round(out["report_ms"]["median"] * 1e3 / pass_us, 2) if pass_us else None
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("fasst", "2pl", "store", "tatp", "smallbank"), required=True)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--zipf", type=float, default=0.8)
    ap.add_argument("--top", type=int, default=16)
    ap.add_argument("--timeout", type=int, default=300, help="seconds the GPU child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload, "--rows", str(a.rows),
           "--requests", str(a.requests), "--zipf", str(a.zipf), "--top", str(a.top)]
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
