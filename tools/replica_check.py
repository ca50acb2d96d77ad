#!/usr/bin/env python3
"""Is a replica equal to its primary, what differs, and what does the repair cost -- on the device (dint_state_digest /
dint_state_diff / dint_state_repair) next to the host way (dump_rows of both engines + a numpy compare).

    tools/replica_check.py [--workload tatp|smallbank|both] [--rows N] [--repeats R] [--timeout S] [--blocks B] [--shards G]

Per workload, two engines of N subscribers / accounts populated alike.  Printed as one JSON object:
  digest      milliseconds of one engine's digest (HIP events on the stream the kernels run on; min / median / max of R
              runs after a warm one), the entry bytes it read, GB/s, and bench_access("stream_rd") over the same number
              of bytes -- the roofline of a read-only stream
  equal       "is the replica equal?": digest of both engines (wall clock) against dump_rows of both + the numpy compare
  diff        dint_state_diff with 0 / 1 % / all rows different (events), and the repair's records/s (wall clock)
  behind_1pct the replica that fell 1 % behind: diff + repair, against building a new replica from populate + the host
              replay (recovery.apply_log) of the primary's log
Every device result is checked: the digests are equal again after each repair.

--blocks B: the replica on ANOTHER device instead (dint_state_block_digest / _select / _rows / _diff, recovery.resync_blocks), here
two engines on one device with a `carry` that clones and counts: the block digest beside dint_state_digest and stream_rd, a replica
1 % and 0.01 % behind -- blocks differing, bytes carried each way beside the image's bytes, the time beside the same-device diff +
repair of an equal fall-behind -- and the 0.01 % case at B = 256, 4096 and 65536.

--shards G: the pairwise resync of two shard SETS of G shards (recovery.resync_set; every engine created with
DINT_FLAG_SHARD_REPLICA): the primaries take writes on 1 % of their rows, each shard its home rows; printed are the records and
the wall-clock time per pair (with --blocks B: through the block path), and whether the two sets' digests add up equal afterwards.

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


def bucket_of(keys, hash_size):
    """fasthash64(&key, 8, 0xdeadbeef) % hash_size (lock_fasst/udp/utils.h:16-53), vectorised"""
    import numpy as np

    def mix(h):
        h = h ^ (h >> np.uint64(23))
        h = h * np.uint64(0x2127599BF4325C37)
        return h ^ (h >> np.uint64(47))

    m = np.uint64(0x880355F21E6D1965)
    with np.errstate(over="ignore"):
        h = np.uint64(0xDEADBEEF) ^ (np.uint64(8) * m)
        h = (h ^ mix(np.asarray(keys, np.uint64))) * m
        return mix(h) % np.uint64(hash_size)


def spread(ms):
    return {"min": round(min(ms), 4), "median": round(statistics.median(ms), 4), "max": round(max(ms), 4), "runs": len(ms)}


def child_blocks(a, workload):
    import numpy as np
    import torch

    from dint_amd import recovery, wire
    from dint_amd.engine import Engine, bench_access

    tatp = workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    tables, stride = (5, 256) if tatp else (2, 128)
    T, S = wire.Tatp, wire.Sb
    msg = wire.TATP_MSG if tatp else wire.SB_MSG
    st = torch.cuda.current_stream().cuda_stream
    B = a.blocks

    def fresh():
        e = Engine(wl, n_rows=a.rows, log_entries=1 << 20)
        e.populate(a.rows)
        return e

    def events(fn, reps):
        fn()  # warm: kernel load, scratch allocation
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    class Carry:
        def __init__(self):
            self.bytes = 0

        def __call__(self, t):
            self.bytes += t.numel() * t.element_size()
            return t.clone()

    prim, rep = fresh(), fresh()
    dumps = [prim.dump_rows(t) for t in range(tables)]
    n_rows = sum(len(d[0]) for d in dumps)
    entries = 0
    for t, d in enumerate(dumps):
        hs = prim.hash_size(t)
        per = np.bincount(bucket_of(d[0], hs).astype(np.int64), minlength=hs)
        entries += hs + int(((np.maximum(per, 1) + 3) // 4 - 1).sum())
    nbytes = entries * stride
    keys = np.concatenate([d[0] for d in dumps])
    tabs = np.concatenate([np.full(len(d[0]), t, np.uint8) for t, d in enumerate(dumps)])
    del dumps
    try:  # the image's size: a buffer that is too small makes the call say what it takes, and nothing is written
        prim.state_export(0, 1, torch.empty(16, dtype=torch.uint8, device="cuda"))
    except recovery.DintError:
        pass
    image_bytes = prim.last_image["bytes"]
    out = {"workload": workload, "rows": a.rows, "block_buckets": B, "image_bytes": image_bytes, "entry_bytes": nbytes,
           "conditions": "two engines on ONE device, carry = clone; events: median of %d after a warm run; wall: one run each" % a.repeats}

    # the block digest beside the table digest and a read-only stream over the same bytes
    ms_t = events(lambda: prim.state_digest(stream=st), a.repeats)
    bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)
    rd = bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)[0] * 16 / 1e9
    out["digest"] = {"state_digest_ms": spread(ms_t), "stream_rd_GBps": round(rd, 1), "stream_rd_ms": round(nbytes / 1e6 / rd, 4)}
    for b in sorted({64, 256, 4096, 65536, B}):
        d_out, n, _ = prim.state_block_digest(b)
        ms = events(lambda: prim.state_block_digest(b, d_out, stream=st), a.repeats)
        out["digest"]["block_%d" % b] = {"ms": spread(ms), "blocks": n, "digest_bytes": 32 * n,
                                         "GBps": round(nbytes / 1e6 / statistics.median(ms), 1),
                                         "times_state_digest": round(statistics.median(ms) / statistics.median(ms_t), 2)}

    def writes(e, pick):
        """an update of rows `pick` of engine e: the log record and the primary operation"""
        rng = np.random.default_rng(len(pick))
        for off in range(0, len(pick), e.pass_max // 2):
            p = pick[off:off + e.pass_max // 2]
            m = np.zeros(2 * len(p), msg)
            val = rng.integers(0, 256, (len(p), 40 if tatp else 8), dtype=np.uint8)
            for j in range(2):
                m["table"][j::2], m["key"][j::2], m["val"][j::2] = tabs[p], keys[p], val
            m["type"][0::2], m["type"][1::2] = (T.COMMIT_LOG, T.COMMIT_PRIM) if tatp else (S.COMMIT_LOG, S.COMMIT_PRIM)
            e.submit(m)

    buf = torch.empty((n_rows + 4096) * 64, dtype=torch.uint8, device="cuda")  # (at 1 % every block of 4,096 buckets differs)
    cap = buf.numel() // 64
    seed = [100]

    def fall_behind(frac):
        seed[0] += 1
        pick = np.random.default_rng(seed[0]).permutation(n_rows)[:max(1, int(n_rows * frac))]
        writes(prim, pick)
        return len(pick)

    def by_blocks(frac, b):
        n = fall_behind(frac)
        c = Carry()
        r, t = wall(lambda: recovery.resync_blocks(prim, rep, block_buckets=b, cap=cap, carry=c))
        assert r["digests_equal"] and r["records"] == n, r
        return {"records": n, "blocks_differing": r["blocks_differing"], "rounds": r["rounds"], "to_replica_bytes": r["digest_bytes"] + r["row_bytes"],
                "to_primary_bytes": r["id_bytes"], "digest_bytes": r["digest_bytes"], "row_bytes": r["row_bytes"],
                "fraction_of_image": round(c.bytes / image_bytes, 5), "total_s": round(t, 5)}

    def same_device(frac):
        n = fall_behind(frac)

        def go():
            m, _ = prim.state_diff(rep, buf, cap)
            return rep.state_repair(buf, m)["applied"]

        got, t = wall(go)
        assert got == n and recovery.digests_equal(prim, rep)
        return {"records": n, "total_s": round(t, 5)}

    by_blocks(1e-5, B); same_device(1e-5)  # warm: scratch, buffers, kernel load
    for name, frac in (("behind_1pct", 0.01), ("behind_0.01pct", 0.0001)):
        out[name] = {"blocks": by_blocks(frac, B), "same_device_diff_repair": same_device(frac)}
    out["sweep_0.01pct"] = {}
    for b in (256, 4096, 65536):
        by_blocks(1e-5, b)  # warm at this size
        out["sweep_0.01pct"][str(b)] = by_blocks(0.0001, b)
    out["ok"] = recovery.digests_equal(prim, rep)
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


def child_shards(a, workload):
    import numpy as np

    from dint_amd import _lib, recovery, wire
    from dint_amd.engine import Engine

    tatp = workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    G = a.shards

    def shard_set():
        out = [Engine(wl, n_rows=a.rows, log_entries=1 << 16, shard_index=i, shard_count=G, flags=_lib.FLAG_SHARD_REPLICA) for i in range(G)]
        for e in out:
            e.populate(a.rows)
        return out

    prims, reps = shard_set(), shard_set()
    assert recovery.digest_sum(prims) == recovery.digest_sum(reps)
    rng = np.random.default_rng(3)
    changed = 0
    for e in prims:  # new values for 1 % of every shard's own rows of table 0, with the versions they have
        k, v, x = e.dump_rows(0)
        pick = rng.choice(len(k), max(1, len(k) // 100), replace=False)
        m = np.zeros(len(pick), wire.TATP_MSG if tatp else wire.SB_MSG)
        m["type"], m["table"], m["key"] = (wire.Tatp.COMMIT_PRIM if tatp else wire.Sb.COMMIT_PRIM), 0, k[pick]
        m["val"] = rng.integers(0, 256, m["val"].shape, dtype=np.uint8)
        e.submit(m)
        changed += len(pick)
    t0 = time.perf_counter()
    res = recovery.resync_set(prims, reps, blocks=a.blocks or None)
    dt = time.perf_counter() - t0
    out = {"workload": workload, "rows": a.rows, "shards": G, "blocks": a.blocks, "rows_changed": changed, "records": res["records"],
           "per_shard": [{k: v for k, v in r.items()} for r in res["shards"]], "resync_ms": round(dt * 1e3, 3),
           "digests_equal": res["digests_equal"], "runs": "one run"}
    out["ok"] = bool(res["digests_equal"] and 0 < res["records"] <= changed)
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


def child(a, workload):
    import numpy as np
    import torch

    from dint_amd import recovery, wire
    from dint_amd.engine import Engine, bench_access

    tatp = workload == "tatp"
    wl = wire.Workload.TATP if tatp else wire.Workload.SMALLBANK
    tables, stride = (5, 256) if tatp else (2, 128)
    T, S = wire.Tatp, wire.Sb
    msg = wire.TATP_MSG if tatp else wire.SB_MSG
    st = torch.cuda.current_stream().cuda_stream

    def fresh():
        e = Engine(wl, n_rows=a.rows, log_entries=1 << 20)
        e.populate(a.rows)
        return e

    def events(fn, reps):
        fn()  # warm: kernel load, scratch allocation
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    def host_equal(x, y):
        for t in range(tables):
            p, q = x.dump_rows(t), y.dump_rows(t)
            i, j = np.argsort(p[0], kind="stable"), np.argsort(q[0], kind="stable")
            if len(p[0]) != len(q[0]) or not all((u[i] == v[j]).all() for u, v in zip(p, q)):
                return False
        return True

    prim, rep = fresh(), fresh()
    out = {"workload": workload, "rows": a.rows, "runs": "one run each, same box"}
    # the entries a digest reads: one inline entry per bucket + the overflow entries of buckets with more than four rows
    dumps = [prim.dump_rows(t) for t in range(tables)]
    n_rows = sum(len(d[0]) for d in dumps)
    entries = 0
    for t, d in enumerate(dumps):
        hs = prim.hash_size(t)
        per = np.bincount(bucket_of(d[0], hs).astype(np.int64), minlength=hs)
        entries += hs + int(((np.maximum(per, 1) + 3) // 4 - 1).sum())
    nbytes = entries * stride
    keys = np.concatenate([d[0] for d in dumps])
    tabs = np.concatenate([np.full(len(d[0]), t, np.uint8) for t, d in enumerate(dumps)])
    del dumps

    ms = events(lambda: prim.state_digest(stream=st), a.repeats)
    gbs = nbytes / 1e6 / statistics.median(ms)
    bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)
    rd = bench_access(nbytes, nbytes // 16, "stream_rd", 16, 16)[0] * 16 / 1e9
    out["digest"] = {"ms": spread(ms), "rows": n_rows, "entry_bytes": nbytes, "GBps": round(gbs, 1), "stream_rd_GBps": round(rd, 1),
                     "fraction_of_stream_rd": round(gbs / rd, 3)}

    eq_d = [wall(lambda: prim.state_digest() == rep.state_digest()) for _ in range(a.repeats)]
    eq_h = wall(lambda: host_equal(prim, rep))
    assert all(r for r, _ in eq_d) and eq_h[0]
    out["equal"] = {"device_s": round(statistics.median(s for _, s in eq_d), 6), "host_s": round(eq_h[1], 3),
                    "speedup": round(eq_h[1] / statistics.median(s for _, s in eq_d), 1), "bytes_to_host": 64 * tables}

    buf = torch.empty(n_rows * 64, dtype=torch.uint8, device="cuda")

    def diff_ms():
        return spread(events(lambda: prim.state_diff(rep, buf, n_rows, stream=st), max(2, a.repeats // 2)))

    def writes(e, pick, logged):
        """an update of rows `pick` of engine e: the log record and the primary operation, or the backup operation alone"""
        rng = np.random.default_rng(len(pick))
        k = 2 if logged else 1
        for off in range(0, len(pick), e.pass_max // 2):
            p = pick[off:off + e.pass_max // 2]
            m = np.zeros(k * len(p), msg)
            val = rng.integers(0, 256, (len(p), 40 if tatp else 8), dtype=np.uint8)
            for j in range(k):
                m["table"][j::k], m["key"][j::k], m["val"][j::k] = tabs[p], keys[p], val
            if logged:
                m["type"][0::2], m["type"][1::2] = (T.COMMIT_LOG, T.COMMIT_PRIM) if tatp else (S.COMMIT_LOG, S.COMMIT_PRIM)
            else:
                m["type"] = T.COMMIT_BCK if tatp else S.COMMIT_BCK
            e.submit(m)

    out["diff"] = {"0pct": {"ms": diff_ms(), "total": prim.state_diff(rep)[1]["total"]}}
    # the replica falls 1 % behind: the primary logs and commits an update of one row in a hundred
    pick = np.random.default_rng(7).permutation(n_rows)[:n_rows // 100]
    prim.log_drain_device(buf, n_rows)  # (the cursor to the tail)
    writes(prim, pick, True)
    rec, lost = prim.log_drain(len(pick))
    assert lost == 0 and len(rec) == len(pick)
    out["diff"]["1pct"] = {"ms": diff_ms()}
    (n, dst), t_diff = wall(lambda: prim.state_diff(rep, buf, n_rows))
    rs, t_rep = wall(lambda: rep.state_repair(buf, n))
    assert n == dst["total"] == len(pick) == rs["applied"] and prim.state_digest() == rep.state_digest()
    out["diff"]["1pct"].update(total=n, repair_records_per_s=round(n / t_rep))
    (host, t_pop) = wall(fresh)
    _, t_apply = wall(lambda: recovery.apply_log(host, rec))
    assert host.state_digest() == prim.state_digest()
    out["behind_1pct"] = {"records": n, "device_diff_repair_s": round(t_diff + t_rep, 5), "host_populate_s": round(t_pop, 3),
                          "host_apply_log_s": round(t_apply, 3), "speedup": round((t_pop + t_apply) / (t_diff + t_rep), 1)}
    del host
    # every row different: one more version on each row of the replica
    writes(rep, np.arange(n_rows), False)
    out["diff"]["all"] = {"ms": diff_ms()}
    (n, dst), _ = wall(lambda: prim.state_diff(rep, buf, n_rows))
    rs, t_rep = wall(lambda: rep.state_repair(buf, n))
    assert n == dst["total"] == n_rows == rs["applied"] and prim.state_digest() == rep.state_digest()
    out["diff"]["all"].update(total=n, repair_records_per_s=round(n / t_rep))
    out["ok"] = host_equal(prim, rep)
    print(json.dumps(out), flush=True)
    return 0 if out["ok"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("tatp", "smallbank", "both"), default="both")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--timeout", type=int, default=540, help="seconds the GPU child may take")
    ap.add_argument("--blocks", type=int, default=0, help="buckets per block: measure the block path (recovery.resync_blocks) instead")
    ap.add_argument("--shards", type=int, default=0, help="G: the pairwise resync of two sets of G shards (recovery.resync_set)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    loads = ("tatp", "smallbank") if a.workload == "both" else (a.workload,)
    if a.child:
        for w in loads:
            if rc := (child_shards(a, w) if a.shards else child_blocks(a, w) if a.blocks else child(a, w)):
                return rc
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "--workload", a.workload,
           "--rows", str(a.rows), "--repeats", str(a.repeats), "--blocks", str(a.blocks), "--shards", str(a.shards)]
    return subprocess.run(cmd).returncode  # (124 / 137: the time limit; nothing else is started after a failure)


if __name__ == "__main__":
    sys.exit(main())
