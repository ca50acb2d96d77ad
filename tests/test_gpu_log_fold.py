"""The folded log replay (include/dint_abi.h dint_log_apply_folded_device, dint_amd/csrc/k_fold.hip over csrc/log_fold.h,
dint_amd/recovery.py apply_log_folded / LogShipper(fold=True)) against the unfolded path it must agree with
(dint_log_apply_device into a twin replica), the primary whose log is replayed, the host form (dint_log_fold_host) and the CPU
oracle.  Every comparison is exact."""
import numpy as np
import pytest

import log_fold_cases as lfc
import tracegen  # noqa: F401  (tests/ on the path, as the other GPU tests)
from dint_amd import _lib, recovery, wire
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ENOMEM, ESTATE = -1, -2, -5
SHARED = ("applied", "commits", "inserts", "deletes", "chunks")
HOST = SHARED + ("rows", "folded_records", "deferred_records", "deferred_buckets", "repair_records")
pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def _rows(e, t):
    k, v, x = e.dump_rows(t)
    o = np.lexsort((v, k))
    return k[o], v[o], x[o]


def _same_rows(a, b, tables=5):
    for t in range(tables):
        ra, rb = _rows(a, t), _rows(b, t)
        assert len(ra[0]) == len(rb[0]), t
        assert (ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and (ra[2] == rb[2]).all(), t
    assert a.state_digest() == b.state_digest()


def _clean(e):
    v = recovery.verify_tables([e])
    assert v["ok"] and v["clean"], v["tables"]


def _tatp(loads=(), **kw):
    from dint_amd.engine import Engine

    e = Engine(W.TATP, n_rows=300, log_entries=4096, **kw)
    e.populate(300)
    for t, keys, vers, vals in loads:
        e.load_rows(t, keys, vers, vals)
    return e


def _sb():
    from dint_amd.engine import Engine

    e = Engine(W.SMALLBANK, n_rows=lfc.N_ACCT, log_entries=1 << 16)
    e.populate(lfc.N_ACCT)
    return e


def _host(e, rec, tables=5):
    """the host form over the replica as it is now (one chunk)"""
    return recovery.fold_log_host(e.workload, [e.hash_size(t) for t in range(tables)], [e.dump_rows(t) for t in range(tables)], rec)


def _unfolded_with_host(twin, d_rec, rec, n, chunk, tables=5):
    """the unfolded path into `twin`, chunk by chunk as the call cuts the log, and before every chunk the host form over the twin as
    it is then: (log_apply_device's counts, the host form's) summed over the chunks"""
    c = min(chunk or twin.pass_max, twin.pass_max)
    raw, host = dict.fromkeys(SHARED, 0), dict.fromkeys(HOST, 0)
    for off in range(0, n, c):
        m = min(c, n - off)
        h = _host(twin, rec[off:off + m], tables)[2]
        r = twin.log_apply_device(d_rec[off * 64:], m, chunk=c)
        for k in HOST:
            host[k] += h[k]
        for k in SHARED:
            raw[k] += r[k]
    return raw, host


@pytest.fixture(scope="module")
def stream300():
    """test_gpu_log_replay.py's stream, rebuilt: 300 subscribers, 8 x 3,000 committed writes, drained on the device"""
    import torch

    cap = 4096
    prim = _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    dev = []
    for b in range(8):
        req = _committed_writes(o, 3000, seed=b)
        assert prim.submit(req).tobytes() == o.replay(req).tobytes()
        assert prim.log_drain_device(buf, cap) == (3000, 0)
        dev.append(buf[:3000 * 64].clone())
    d_rec = torch.cat(dev)
    return prim, d_rec, np.frombuffer(d_rec.cpu().numpy().tobytes(), wire.LOG_REC)


def _host_record_by_record(e, rec):
    """the host form with every record a chunk of its own, without a dump per chunk: a one-record chunk reads nothing of the
    replica but the rows that hold its key, so the host form is given exactly those, out of a row map {(table, key): [versions in
    chain order]} taken from the replica's dump once and kept up to date with the repair record every call returns.  Only for
    replicas that hold no key twice (nothing is deferred, so the repair records are all that changes a row).  The sums of HOST."""
    import ctypes as C

    L = _lib.load()
    rows = {}
    for t in range(5):
        k, v, _ = e.dump_rows(t)
        for key, ver in zip(k.tolist(), v.tolist()):
            rows.setdefault((t, key), []).append(ver)
    assert all(len(v) == 1 for v in rows.values())
    hs = np.array([e.hash_size(t) for t in range(5)], "<u8")
    off, keys, vers = np.zeros(6, "<u8"), np.zeros(1, "<u8"), np.zeros(1, "<u4")
    flag, out, st = np.zeros(1, np.uint8), np.zeros(1, wire.LOG_REC), _lib.FoldStats()
    rec = np.ascontiguousarray(rec)
    host = dict.fromkeys(HOST, 0)
    for i in range(len(rec)):
        t, key = int(rec["table"][i]), int(rec["key"][i])
        have = rows.get((t, key), [])
        off[:], keys[0] = 0, key
        off[t + 1:] = len(have)
        if have:
            vers[0] = have[0]
        got = L.dint_log_fold_host(int(W.TATP), 5, hs.ctypes.data, off.ctypes.data, keys.ctypes.data, vers.ctypes.data,
                                   rec[i:i + 1].ctypes.data, 1, flag.ctypes.data, out.ctypes.data, 1, C.byref(st))
        assert got in (0, 1) and not flag[0]
        if got and out["is_del"][0]:
            del rows[(t, key)]
        elif got:
            rows[(t, key)] = [int(out["ver"][0])]
        for k in HOST:
            host[k] += getattr(st, k)
    return host


@pytest.mark.parametrize("chunk", [0, 777, 1])
def test_the_stream_folded_equals_unfolded_and_the_primary(stream300, chunk):
    prim, d_rec, rec = stream300
    n = len(rec)
    rep, twin = _tatp(), _tatp()
    if chunk == 1:
        # every record a chunk of its own.  The unfolded twin takes the log in chunks of a pass -- what a record is as a backup
        # operation does not depend on where the log is cut, and 24,000 passes of one record would take a minute -- so of its counts
        # only `chunks` differs; the host form goes record by record over a row map
        want_host = _host_record_by_record(rep, rec)
        raw = twin.log_apply_device(d_rec, n)
        raw["chunks"] = n
    st = rep.log_apply_folded(d_rec, n, chunk=chunk)
    if chunk != 1:
        raw, want_host = _unfolded_with_host(twin, d_rec, rec, n, chunk)
    print("stream", chunk, st)
    assert {k: st[k] for k in SHARED} == {k: raw[k] for k in SHARED}
    assert st["deferred_records"] == 0 and st["deferred_buckets"] == 0  # the populations hold no key twice: nothing is deferred
    assert st["folded_records"] == n and st["refused"] == 0
    assert st["updated"] + st["inserted"] + st["deleted"] <= st["repair_records"] <= st["rows"]
    _same_rows(twin, rep)
    _same_rows(prim, rep)
    assert {k: st[k] for k in HOST} == {k: want_host[k] for k in HOST}
    _clean(rep)
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()  # the records stay untouched
    assert rep.stats()["missing_keys"] == 0


CASES = lfc.tatp_cases()


@pytest.mark.parametrize("name,chunk", [("one_row_5000", 0), ("alternating_present", 0), ("alternating_absent", 0), ("alternating_then_insert_absent", 0),
                                        ("duplicate_with_neighbour", 0), ("all_deferred", 0), ("version_wraps", 0), ("delete_first_absent", 0),
                                        ("one_record", 0), ("lengths", 0), ("lengths", 100), ("one_row_5000", 1333)])
def test_hand_built_logs(name, chunk):
    """chunk != 0: rows whose records straddle a chunk edge"""
    loads, rec = CASES[name]
    rep, twin = _tatp(loads), _tatp(loads)
    d_rec = _dev(rec)
    st = rep.log_apply_folded(d_rec, len(rec), chunk=chunk)
    raw, host = _unfolded_with_host(twin, d_rec, rec, len(rec), chunk)
    print(name, chunk, st)
    assert {k: st[k] for k in SHARED} == {k: raw[k] for k in SHARED}
    assert {k: st[k] for k in HOST} == {k: host[k] for k in HOST}
    if name in ("duplicate_with_neighbour", "all_deferred"):
        assert len(rec) <= rep.pass_max and st["deferred_records"] == host["deferred_records"] > 0 and st["deferred_buckets"] == 1
    else:
        assert st["deferred_records"] == 0
    _same_rows(twin, rep)
    _clean(rep)
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()


def test_smallbank_with_a_hot_account_and_absent_keys():
    loads, rec = lfc.smallbank_cases()["hot_account"]
    assert len(rec) == 50_000 and (rec["key"] == 77).sum() >= 20_000 and ((rec["key"] & lfc.ABSENT) != 0).sum() > 100
    rep, twin = _sb(), _sb()
    d_rec = _dev(rec)
    st = rep.log_apply_folded(d_rec, len(rec))
    raw, host = _unfolded_with_host(twin, d_rec, rec, len(rec), 0, tables=2)
    assert {k: st[k] for k in SHARED} == {k: raw[k] for k in SHARED} and st["inserts"] == st["deletes"] == 0
    assert {k: st[k] for k in HOST} == {k: host[k] for k in HOST} and st["deferred_records"] == 0
    assert st["updated"] == st["repair_records"] and st["inserted"] == st["deleted"] == st["refused"] == 0
    _same_rows(twin, rep, tables=2)
    o = lfc.oracle_for(W.SMALLBANK, loads)
    recovery.apply_log(lfc.OracleEngine(W.SMALLBANK, o), rec)
    for t in range(2):
        assert all((x == y).all() for x, y in zip(rep.dump_rows(t), o.dump(t)))  # updates in place: the oracle's own order
    _clean(rep)


def test_dry_run_counts_and_writes_nothing(stream300):
    from dint_amd.engine import Engine

    _, d_rec, rec = stream300
    rep = _tatp()
    before = rep.state_digest()
    dry = rep.log_apply_folded(d_rec, len(rec), chunk=777, dry_run=True)
    assert rep.state_digest() == before and rep.stats()["requests"] == 0
    assert (dry["updated"], dry["inserted"], dry["deleted"], dry["refused"]) == (0, 0, 0, 0)
    # (a dry run's later chunks see the tables as they were, a real run's as the earlier chunks left them: one chunk compares)
    n1 = min(len(rec), rep.pass_max)
    dry = rep.log_apply_folded(d_rec, n1, dry_run=True)
    wet = rep.log_apply_folded(d_rec, n1)
    assert dry["chunks"] == 1 and {k: dry[k] for k in HOST} == {k: wet[k] for k in HOST} and wet["updated"] + wet["inserted"] + wet["deleted"] > 0
    loads, drec = CASES["duplicate_with_neighbour"]
    dup = _tatp(loads)
    dry = dup.log_apply_folded(_dev(drec), len(drec), dry_run=True)
    wet = dup.log_apply_folded(_dev(drec), len(drec))
    assert {k: dry[k] for k in HOST} == {k: wet[k] for k in HOST} and dry["deferred_records"] > 0
    # a blank engine stays blank: it still takes an import
    blank, src = Engine(W.TATP, n_rows=300, log_entries=4096), _tatp()
    blank.log_apply_folded(d_rec, 3000, dry_run=True)
    buf, nbytes, _ = src.state_export(0, 1)
    blank.state_import(buf, nbytes)
    _same_rows(src, blank)


def test_refusals():
    import torch
    from dint_amd.engine import Engine

    buf = torch.zeros(64 * 64 + 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def apply(e, ptr=p, n=64, flags=0):
        return e._L.dint_log_apply_folded_device(e._h, ptr, n, 0, flags, None)

    for e in (Engine(W.FASST, n_slots=1024), Engine(W.TPL, n_slots=1024), Engine(W.LOG, log_entries=1024), Engine(W.STORE, n_rows=1000)):
        assert apply(e) == ESTATE, e.workload
    assert apply(Engine(W.TATP, n_rows=300, log_entries=4096, shard_index=0, shard_count=2)) == EINVAL
    e = _tatp()
    assert apply(e, None, 64) == EINVAL and apply(e, None, 0) == 0
    assert apply(e, p, 64, flags=2) == EINVAL and apply(e, p + 8, 64) == EINVAL
    o = orc.TatpOracle(300, log_entries=1 << 20)
    a, b = (_dev(_committed_writes(o, 1000, seed=s)) for s in (1, 2))
    e.submit_device(a, 2000, None, 0, ahead=(b, 2000, None))
    assert apply(e) == ESTATE and b"announced" in e._L.dint_last_error()
    e.submit_device(b, 2000)
    e.sync()
    assert apply(e) == 0
    e.sync()


def test_the_replicas_ring_tail_locks_and_counters_are_left_alone(stream300):
    _, d_rec, rec = stream300
    rep = _tatp()
    rep.submit(_committed_writes(orc.TatpOracle(300, log_entries=1 << 20), 500, seed=7))  # something in the replica's ring
    m = np.zeros(100, wire.TATP_MSG)
    m["type"], m["key"] = T.ACQUIRE_LOCK, np.arange(100)
    rep.submit(m)  # and some lock words held
    ring0, tail0 = rep.read_log(4096)
    locks0 = [rep.read_locks(t)[0].tobytes() for t in range(5)]
    s0 = rep.stats()
    assert tail0 == 500 and any(np.frombuffer(x, "<u4").any() for x in locks0)
    st = rep.log_apply_folded(d_rec, len(rec))
    assert st["deferred_records"] == 0
    ring1, tail1 = rep.read_log(4096)
    assert tail1 == tail0 and ring1.tobytes() == ring0.tobytes()
    assert [rep.read_locks(t)[0].tobytes() for t in range(5)] == locks0
    s1 = rep.stats()
    assert (s1["batches"], s1["requests"]) == (s0["batches"], s0["requests"])  # folded records are not requests


def test_a_pool_too_small_for_the_inserts():
    from dint_amd.engine import Engine

    src = _tatp()
    rng = np.random.default_rng(3)
    rows = [lfc.records(t, int(k), [False], rng) for t in range(5) for k in src.dump_rows(t)[0]]
    rec = lfc.interleave(rows, rng)  # one record per row of a populated engine: every one an insert into ...
    rep = Engine(W.TATP, n_rows=300, log_entries=4096, pool_entries=8)  # ... an empty one with next to no overflow entries
    with pytest.raises(_lib.DintError, match=rf"dint error {ENOMEM}: .*pool full"):  # DINT_ENOMEM
        rep.log_apply_folded(_dev(rec), len(rec))
    st = rep.last_fold
    print("pool exhaustion", st)
    assert st["refused"] > 0 and st["inserted"] == st["repair_records"] - st["refused"] and st["inserts"] == len(rec)
    assert rep.stats()["pool_exhausted"] == st["refused"]
    assert sum(len(rep.dump_rows(t)[0]) for t in range(5)) == st["inserted"]
    _clean(rep)


def test_log_shipper_with_fold_follows_a_primary():
    cap = 4096
    prim, rep = _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    ship = recovery.LogShipper(prim, rep, cap=cap, fold=True)
    for b in range(20):
        req = _committed_writes(o, 3000, seed=40 + b)
        assert prim.submit(req).tobytes() == o.replay(req).tobytes()
        st = ship.step()
        assert st["lost"] == 0 and st["applied"] == 3000 == st["commits"] + st["inserts"] + st["deletes"]
        assert st["folded"] == 3000 and st["deferred"] == 0
    assert ship.shipped == 60_000 and ship.lost == 0
    _same_rows(prim, rep)
    assert ship.step() == {"applied": 0, "lost": 0}
    _clean(rep)


def test_delete_insert_churn_over_many_folded_calls_reuses_the_pool():
    """Nothing is deferred, so no hot-path pass ever rotates the pool's pend lists: the fold rotates them itself in front of every
    repair.  Three buckets of an EMPTY table take 9 rows each -- an inline entry and two overflow entries -- and lose them again,
    40 times, on a pool of 8 overflow entries: without reuse the second round finds the pool full.  The unfolded twin, whose passes
    rotate, is the reference."""
    from dint_amd.engine import Engine
    from kvkeys import np_bucket

    t = 2
    rep, twin = (Engine(W.TATP, n_rows=300, log_entries=4096, pool_entries=8) for _ in range(2))  # (not populated: that alone would fill the pool)
    cand = np.arange(1, 5000, dtype=np.uint64) | lfc.ABSENT
    b = np_bucket(cand, rep.hash_size(t))
    ids, cnt = np.unique(b, return_counts=True)
    keys = [int(k) for bucket in ids[cnt >= 9][:3] for k in cand[b == bucket][:9]]
    assert len(keys) == 27
    rng = np.random.default_rng(8)
    for r in range(40):
        for dele in (False, True):
            rec = lfc.interleave([lfc.records(t, k, [dele], rng) for k in keys], rng)
            d_rec = _dev(rec)
            st = rep.log_apply_folded(d_rec, len(rec))  # (a full pool raises DintError)
            raw = twin.log_apply_device(d_rec, len(rec))
            assert {k: st[k] for k in SHARED} == {k: raw[k] for k in SHARED}
            assert st["deferred_records"] == 0 and st["refused"] == 0
            assert (st["inserted"], st["deleted"]) == ((0, 27) if dele else (27, 0))
            _same_rows(twin, rep)
    assert rep.stats()["pool_exhausted"] == 0 and twin.stats()["pool_exhausted"] == 0
    _clean(rep)
