#!/usr/bin/env python3
"""The lock micro-benchmarks' closed loop on one GPU: GPU-resident workers (driver.GpuLockClient) and one lock engine,
no host round trip (replay.LockLoop).  Prints one JSON line: requests/s and committed transactions/s of the loop, the
reject and rollback rates per request, and the time per epoch split into client kernels and engine kernels.

    python tools/lock_loop.py --workload fasst --workers 65536 --theta 0.8 --slots 36000000 --epochs 2000

Client-kernel time: the same client alone (emit + fused consume, replies = its own requests: timing only).  Engine-kernel
time: dint_timing_read over a second run of the loop with the engine's kernel timing on.  Both are per epoch."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from dint_amd import wire  # noqa: E402
from dint_amd.driver import GpuLockClient  # noqa: E402
from dint_amd.engine import Engine  # noqa: E402
from dint_amd.replay import LockLoop  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["fasst", "2pl"], default="fasst")
    ap.add_argument("--workers", type=int, default=65536)
    ap.add_argument("--keys", type=int, default=24_000_000, help="key space the workers draw from")
    ap.add_argument("--theta", type=float, default=0.8, help="Zipf theta; 0 = uniform keys")
    ap.add_argument("--slots", type=int, default=36_000_000, help="lock table slots")
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    wl = wire.Workload.FASST if a.workload == "fasst" else wire.Workload.TPL
    theta = a.theta or None

    gc = GpuLockClient(wl, a.workers, a.keys, zipf_theta=theta, device=0)
    eng = Engine(wl, n_slots=a.slots, device=0)
    loop = LockLoop(eng, gc)
    loop.epochs(a.warmup)
    loop.sync()
    s0 = gc.stats()
    t0 = time.perf_counter()
    loop.epochs(a.epochs)
    loop.sync()
    dt = time.perf_counter() - t0
    s1 = gc.stats()
    req = s1["requests"] - s0["requests"]
    com = s1["committed"] - s0["committed"]
    out = {"workload": f"lock_{a.workload}", "workers": a.workers, "keys": a.keys, "theta": theta, "slots": a.slots,
           "epochs": a.epochs, "requests_per_s": req / dt, "committed_txn_per_s": com / dt,
           "reject_rate": (s1["rejects"] - s0["rejects"]) / req, "epoch_us": dt / a.epochs * 1e6,
           "protocol_errors": s1["protocol_errors"]}
    if wl == wire.Workload.FASST:
        out["rollback_rate"] = (s1["rollbacks"] - s0["rollbacks"]) / req

    # engine kernels: the same loop with the engine's kernel timing on (events around its launches)
    n_t = min(a.epochs, 500)
    eng.timing_enable(True)
    loop.epochs(n_t)
    loop.sync()
    tim = eng.timing_read()
    eng.timing_enable(False)
    out["engine_kernel_us_per_epoch"] = sum(v["avg_us"] * v["launches"] for v in tim.values()) / n_t
    out["engine_kernels"] = {k: round(v["avg_us"], 2) for k, v in tim.items()}

    # client kernels alone: a second client, its requests handed back as its replies
    gc2 = GpuLockClient(wl, a.workers, a.keys, zipf_theta=theta, device=0)
    st = torch.cuda.Stream()
    xs = st.cuda_stream
    for _ in range(a.warmup):
        gc2.next(xs)
        gc2.consume(xs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(n_t):
        gc2.next(xs)
        gc2.consume(xs)
    e1.record(st)
    e1.synchronize()
    out["client_kernel_us_per_epoch"] = e0.elapsed_time(e1) * 1e3 / n_t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
