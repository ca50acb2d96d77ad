#!/usr/bin/env python3
"""Replay one primary's log into two fresh replicas -- once over the host (dint_log_drain + recovery.apply_log), once
without leaving the GPU (dint_log_drain_device + dint_log_apply_device) -- and say what each costs.

    tools/log_ship.py [--workload tatp|smallbank] [--rows N] [--records M] [--chunk C] [--timeout S] [--fold] [--shards G:H]

A primary takes M committed writes (the log record, then the primary operation, as tests/test_ebpf_surface.py
_committed_writes sends them; rows drawn Zipf-0.8: updates, and for tatp one delete in four and inserts of rows that are
gone).  Its log is then replayed twice from the same cursor (snapshot / restore put the cursor back).  Printed: records/s
of both paths (drain + replay, wall clock, replies complete), the device path split by stage (HIP events on the replica's
stream, in a run of its own: dint_timing_enable drains the stream chunk by chunk), and whether both replicas' rows equal
the primary's.  The device path is run once before it is timed (kernel load, scratch allocation).

--fold measures the folded replay (dint_log_apply_folded_device) against the unfolded one instead: the same drained log into ONE
replica, put back by restore before every run, the two paths alternating; printed are the median and range of 7 runs of each between
HIP events after a warm one, the fold's stage times (one more run with dint_timing_enable: sort, fold, repair, deferred), its
deferred_records, and whether the digests of the two paths' end states are equal.  Both calls are synchronous, and the events are
recorded on torch's current stream, not the engine's own: a figure is the time between two synchronised points around the call
(queueing, the kernels, the per-chunk wait), not device time on the stream that did the work; the stage times are the engine's own
events on its stream.

--shards G:H measures the step between two shard SETS on the one device: a primary set of G shards (G = 1: one unsharded engine)
takes the writes, each shard its home requests; every shard's log is drained and routed to a replica set of H shards
(dint_records_route; replicas created with DINT_FLAG_SHARD_REPLICA), and the pieces are applied destination by destination.
Printed: the route's time over all G drains -- median and range of 7 runs between HIP events on the stream the route runs on, after
a warm run; the figure includes the call's one host synchronisation -- beside a plain device-to-device copy of the same bytes
measured the same way in the same process, their ratio, the per-shard apply times unfolded and folded (wall clock around the
synchronous calls, one run after a warm one, the replicas put back by restore), and whether the replica set's digests add up to
the primary set's after each.

All GPU work happens in ONE child process under a time limit; the parent never opens the GPU."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_ranks(rng, n_rows, n, theta=0.8):
    import numpy as np

    cdf = np.cumsum(1.0 / np.arange(1, n_rows + 1) ** theta)
    return np.minimum(np.searchsorted(cdf, rng.random(n) * cdf[-1]), n_rows - 1)


def writes(rng, rows, live, n, tatp):
    """n committed writes on rows[rank] (table, key): for a row that exists a delete with probability 1/4 (tatp) or an
    update, for one that does not an insert -- the per-record rule of _committed_writes, solved for a whole batch: along
    the records of one row a 'delete if it exists' coin flips the row's state, any other record leaves the row existing."""
    import numpy as np

    from dint_amd import wire

    T, S = wire.Tatp, wire.Sb
    pick = zipf_ranks(rng, len(rows[0]), n)
    coin = (rng.random(n) < 0.25) if tatp else np.zeros(n, bool)
    order = np.argsort(pick, kind="stable")
    r, c, pos = pick[order], coin[order], np.arange(n)
    gstart = np.maximum.accumulate(np.where(np.concatenate([[True], r[1:] != r[:-1]]), pos, 0))
    last_plain = np.maximum.accumulate(np.where(~c, pos, -1))
    prev_plain = np.concatenate([[-1], last_plain[:-1]])  # the last record before p that leaves its row existing
    anchored = prev_plain >= gstart
    cs = np.concatenate([[0], np.cumsum(c)])
    flips = np.where(anchored, cs[pos] - cs[np.maximum(prev_plain, 0) + 1], cs[pos] - cs[gstart])
    before = np.where(anchored, True, live[r]) ^ ((flips & 1) == 1)
    after = ~(before & c)
    last = np.concatenate([r[1:] != r[:-1], [True]])
    live[r[last]] = after[last]
    exists, dele = np.empty(n, bool), np.empty(n, bool)
    exists[order], dele[order] = before, before & c
    m = np.zeros(2 * n, wire.TATP_MSG if tatp else wire.SB_MSG)
    val = rng.integers(0, 256, (n, 40 if tatp else 8), dtype=np.uint8)
    for j in (0, 1):
        m["table"][j::2], m["key"][j::2], m["val"][j::2], m["ver"][j::2] = rows[0][pick], rows[1][pick], val, np.arange(n)
    if tatp:
        m["type"][0::2] = np.where(dele, T.DELETE_LOG, T.COMMIT_LOG)
        m["type"][1::2] = np.where(dele, T.DELETE_PRIM, np.where(exists, T.COMMIT_PRIM, T.INSERT_PRIM))
    else:
        m["type"][0::2], m["type"][1::2] = S.COMMIT_LOG, S.COMMIT_PRIM
    return m


def primary_with_log(a, G=1):
    """a primary that has taken a.records committed writes and been snapshotted: (prim, fresh, same, tatp).  G > 1: a primary SET of
    G shards, each of which took its home requests in order; `prim` is then the list."""
    import numpy as np

    from dint_amd import wire
    from dint_amd.engine import Engine

    tatp = a.workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    tables = 5 if tatp else 2

    def fresh():
        e = Engine(wl, n_rows=a.rows, log_entries=max(a.records, 1024))
        e.populate(a.rows)
        return e

    def same(x, y):
        for t in range(tables):
            p, q = x.dump_rows(t), y.dump_rows(t)
            i, j = np.argsort(p[0], kind="stable"), np.argsort(q[0], kind="stable")
            if len(p[0]) != len(q[0]) or not all((u[i] == v[j]).all() for u, v in zip(p, q)):
                return False
        return True

    rng = np.random.default_rng(1)
    prim = fresh()
    tk = [prim.dump_rows(t)[0] for t in range(tables)]
    prims = [prim]
    if G > 1:
        import torch

        prims = [Engine(wl, n_rows=a.rows, log_entries=max(a.records, 1024), shard_index=i, shard_count=G) for i in range(G)]
        for e in prims:
            e.populate(a.rows)
    if tatp:  # + rows that do not exist yet, as _committed_writes
        new = [k[:max(1, len(k) // 20)] + np.uint64(1 << 44) for k in tk]
        new = [x[~np.isin(x, k)] for x, k in zip(new, tk)]
    else:
        new = [k[:0] for k in tk]
    keys = np.concatenate([np.concatenate([k, x]) for k, x in zip(tk, new)])
    tabs = np.concatenate([np.full(len(k) + len(x), t, np.uint8) for t, (k, x) in enumerate(zip(tk, new))])
    live = np.concatenate([np.concatenate([np.ones(len(k), bool), np.zeros(len(x), bool)]) for k, x in zip(tk, new)])
    perm = rng.permutation(len(keys))  # rank 0 (the hottest) is any row
    rows, live = (tabs[perm], keys[perm]), live[perm]
    left = a.records
    while left:
        n = min(left, prim.pass_max // 2)
        m = writes(rng, rows, live, n, tatp)
        if G == 1:
            prim.submit(m)
        else:  # the home of every request from the engines' own rule (dint_home_shard), then every shard its part
            d_m = torch.from_numpy(np.frombuffer(m.tobytes(), np.uint8).copy()).cuda()
            d_home = torch.empty(len(m), dtype=torch.uint8, device="cuda")
            prims[0].home_shard(d_m, len(m), d_home)
            prims[0].sync()
            home = d_home.cpu().numpy()
            for i, e in enumerate(prims):
                e.submit(m[home == i])
        left -= n
    for e in prims:
        assert e.stats()["missing_keys"] == 0, "the generator sent a write to a row that is not there"
        e.snapshot()
    return (prim if G == 1 else prims), fresh, same, tatp


def child_fold(a):
    import statistics

    import torch

    prim, fresh, _, _ = primary_with_log(a)
    buf = torch.empty(a.records * 64, dtype=torch.uint8, device="cuda")
    assert prim.log_drain_device(buf, a.records) == (a.records, 0)
    rep = fresh()
    rep.snapshot()
    paths = {"folded": lambda: rep.log_apply_folded(buf, a.records, a.chunk), "unfolded": lambda: rep.log_apply_device(buf, a.records, a.chunk)}
    ms, last, digest = {k: [] for k in paths}, {}, {}
    for run in range(8):  # a warm run of each, then 7 timed, the two paths alternating
        for name, call in paths.items():
            rep.restore()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            last[name] = call()
            ev[1].record()
            torch.cuda.synchronize()
            if run:
                ms[name].append(ev[0].elapsed_time(ev[1]))
            digest[name] = rep.state_digest()
    rep.restore()
    rep.timing_enable(True)
    staged = rep.log_apply_folded(buf, a.records, a.chunk)
    rep.timing_enable(False)
    out = {"workload": a.workload, "rows": a.rows, "records": a.records, "chunk": a.chunk, "runs": 7}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "records_per_s": a.records / (statistics.median(v) / 1e3)}
    out["ratio"] = out["unfolded"]["median_ms"] / out["folded"]["median_ms"]
    out["stage_ms"] = {k: v / 1e6 for k, v in staged["stage_ns"].items()}
    out["fold"] = {k: v for k, v in last["folded"].items() if k != "stage_ns"}
    shared = ("applied", "commits", "inserts", "deletes", "chunks")
    out["counts_equal"] = all(last["folded"][k] == last["unfolded"][k] for k in shared)
    out["digests_equal"] = digest["folded"] == digest["unfolded"]
    print(json.dumps(out))
    return 0 if out["counts_equal"] and out["digests_equal"] else 1


def child_shards(a):
    import statistics

    import torch

    from dint_amd import _lib, recovery, wire
    from dint_amd.engine import Engine

    G, H = a.shards
    prims, _, _, tatp = primary_with_log(a, G)
    prims = prims if G > 1 else [prims]
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    bufs, ns = [], []
    for p in prims:
        buf = torch.empty(a.records * 64, dtype=torch.uint8, device="cuda")
        n, lost = p.log_drain_device(buf, a.records)
        assert lost == 0
        bufs.append(buf)
        ns.append(n)
    assert sum(ns) == a.records
    outs = [torch.empty(max(n, 1) * 64, dtype=torch.uint8, device="cuda") for n in ns]
    st = torch.cuda.Stream()  # (a stream of this tool's: the route, the copy and the events around them all run on it)

    def route_all():
        return [prims[i].records_route(H, bufs[i], ns[i], outs[i], stream=st.cuda_stream, wait=False)[1] for i in range(G)]

    def copy_all():
        with torch.cuda.stream(st):
            for i in range(G):
                outs[i][:ns[i] * 64].copy_(bufs[i][:ns[i] * 64], non_blocking=True)

    ms = {"route": [], "copy": []}
    for run in range(8):  # a warm run of each, then 7 timed, alternating
        for name, call in (("copy", copy_all), ("route", route_all)):  # (the route last: outs hold the pieces afterwards)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record(st)
            res = call()
            ev[1].record(st)
            torch.cuda.synchronize()
            if run:
                ms[name].append(ev[0].elapsed_time(ev[1]))
    offs = res
    out = {"workload": a.workload, "rows": a.rows, "records": a.records, "chunk": a.chunk, "shards": [G, H], "runs": 7,
           "bytes": a.records * 64, "records_per_source": ns}
    for name, v in ms.items():
        out[name] = {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                     "gb_per_s_moved": a.records * 64 / (statistics.median(v) / 1e3) / 1e9}
    out["route_over_copy"] = out["route"]["median_ms"] / out["copy"]["median_ms"]
    # ---- the apply, destination by destination
    # (log_entries bounds a pass, as for `fresh`: a small ring would cut the replay into passes of its size)
    reps = [Engine(wl, n_rows=a.rows, log_entries=max(a.records, 1024), shard_index=j, shard_count=H, flags=_lib.FLAG_SHARD_REPLICA if H > 1 else 0)
            for j in range(H)]
    for e in reps:
        e.populate(a.rows)
        e.snapshot()
    want = recovery.digest_sum(prims)
    out["apply"], ok = {}, True
    for name in ("unfolded", "folded"):
        for run in ("warm", "timed"):
            for e in reps:
                e.restore()
            torch.cuda.synchronize()
            per, deferred = [0.0] * H, 0
            for i in range(G):
                for j in range(H):
                    m = offs[i][j + 1] - offs[i][j]
                    if not m:
                        continue
                    view = outs[i][64 * offs[i][j]:64 * offs[i][j + 1]]
                    t0 = time.perf_counter()
                    r = reps[j].log_apply_folded(view, m, a.chunk) if name == "folded" else reps[j].log_apply_device(view, m, a.chunk)
                    per[j] += (time.perf_counter() - t0) * 1e3
                    deferred += r.get("deferred_records", 0)
        eq = recovery.digest_sum(reps) == want
        ok = ok and eq
        out["apply"][name] = {"per_shard_ms": per, "total_ms": sum(per), "records_per_s": a.records / (sum(per) / 1e3), "digests_equal": eq}
        if name == "folded":
            out["apply"][name]["deferred_records"] = deferred
    print(json.dumps(out))
    return 0 if ok else 1


def child(a):
    import numpy as np  # noqa: F401
    import torch

    from dint_amd import recovery

    prim, fresh, same, tatp = primary_with_log(a)
    out = {"workload": a.workload, "rows": a.rows, "records": a.records, "chunk": a.chunk, "runs": "one run"}

    # ---- the host path
    host = fresh()
    t0 = time.perf_counter()
    rec, lost = prim.log_drain(a.records)
    t1 = time.perf_counter()
    st_h = recovery.apply_log(host, rec)
    t2 = time.perf_counter()
    assert lost == 0 and len(rec) == a.records
    out["host"] = {"records_per_s": a.records / (t2 - t0), "drain_s": t1 - t0, "apply_s": t2 - t1}
    del rec

    # ---- the device path: warm-up, timed (wall clock), staged (events)
    buf = torch.empty(a.records * 64, dtype=torch.uint8, device="cuda")
    dev = fresh()
    for run in ("warmup", "timed", "staged"):
        if run != "warmup":
            dev.reset()
            dev.populate(a.rows)
        prim.restore()  # the drain cursor back to where the snapshot found it
        dev.timing_enable(run == "staged")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n, lost = prim.log_drain_device(buf, a.records)
        t1 = time.perf_counter()
        raw = dev.log_apply_device(buf, n, a.chunk)
        t2 = time.perf_counter()
        assert (n, lost) == (a.records, 0)
        if run == "timed":
            out["device"] = {"records_per_s": n / (t2 - t0), "drain_s": t1 - t0, "apply_s": t2 - t1, "chunks": raw["chunks"]}
        if run == "staged":
            tot = sum(raw["stage_ns"].values()) or 1
            out["device"]["stage_ms"] = {k: v / 1e6 for k, v in raw["stage_ns"].items()}
            out["device"]["stage_share"] = {k: round(v / tot, 3) for k, v in raw["stage_ns"].items()}
            out["device"]["passes"] = dev.timing_read()
    dev.timing_enable(False)
    st_d = {k: raw[k] for k in ("commits", "inserts", "deletes")}
    out["counts"] = st_d
    out["counts_equal"] = all(st_h.get(k, st_h.get("acks")) == v for k, v in st_d.items() if tatp or k == "commits")
    out["host_equals_primary"], out["device_equals_primary"] = same(prim, host), same(prim, dev)
    out["missing_keys"] = dev.stats()["missing_keys"]
    out["speedup"] = out["device"]["records_per_s"] / out["host"]["records_per_s"]
    print(json.dumps(out))
    ok = out["counts_equal"] and out["host_equals_primary"] and out["device_equals_primary"] and out["missing_keys"] == 0
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank"), default="tatp")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--records", type=int, default=4_000_000)
    ap.add_argument("--chunk", type=int, default=0, help="records per replay pass (0 = the replica's max_pass)")
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--fold", action="store_true", help="measure the folded replay against the unfolded one")
    ap.add_argument("--shards", default="", help="G:H -- route G primary shards' logs to H replica shards and apply them")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.shards:
        a.shards = tuple(int(x) for x in a.shards.split(":"))
        assert len(a.shards) == 2 and 1 <= a.shards[0] <= 255 and 1 <= a.shards[1] <= 255, "--shards G:H, 1 .. 255 each"
    if a.child:
        return child_shards(a) if a.shards else child_fold(a) if a.fold else child(a)
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--rows", str(a.rows), "--records", str(a.records), "--chunk", str(a.chunk)] + (["--fold"] if a.fold else []) + \
          (["--shards", "%d:%d" % a.shards] if a.shards else [])
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
