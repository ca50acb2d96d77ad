"""Digest, diff and repair of two engines' rows on the GPU (include/dint_abi.h dint_state_digest / dint_state_diff /
dint_state_repair, dint_amd/csrc/k_state.hip, dint_amd/recovery.py resync / LogShipper.resync) against forms that share no code
with them: the digest in numpy (tests/test_state_sync_host.py np_digest: a vectorised fasthash64 pinned there against the CPU
oracle's) over the oracle's dump and the engine's own dump_rows, the diff in numpy set logic (np_diff) over dump_rows.  Every
comparison is exact."""
import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes
from test_gpu_log_replay import _dev, _same_rows, _tatp, _writes_in_rounds
from test_state_sync_host import np_diff, np_digest

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ENOMEM, ESTATE = -1, -2, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _np_digests(e):
    return [np_digest(t, *e.dump_rows(t)) for t in range(NTAB[e.workload])]


def _np_full_diff(a, b):
    """the whole diff a -> b in the contract's order, from the two engines' dumps"""
    recs, tot = [], {"total": 0, "only_a": 0, "only_b": 0, "val_differs": 0, "ver_only": 0}
    for t in range(NTAB[a.workload]):
        r, st = np_diff(t, a.hash_size(t), a.dump_rows(t), b.dump_rows(t))
        recs.append(r)
        for k in tot:
            tot[k] += st[k]
    return np.concatenate(recs), tot


def _diff(a, b, cap):
    """state_diff into a fresh HBM buffer of cap records: (records as LOG_REC, stats, the buffer)"""
    import torch

    buf = torch.full(((cap + 4) * 64,), 0xEE, dtype=torch.uint8, device="cuda")  # (4 records of room behind the cap)
    n, st = a.state_diff(b, buf, cap)
    return np.frombuffer(buf[:n * 64].cpu().numpy().tobytes(), wire.LOG_REC), st, buf


def _dumps(e):
    return [tuple(x.tobytes() for x in e.dump_rows(t)) for t in range(NTAB[e.workload])]


def _sb_writes(n_acct, n, seed):
    """committed smallbank writes as the client sends them (lock, log record, primary operation)"""
    rng = np.random.default_rng(seed)
    m = np.zeros(3 * n, wire.SB_MSG)
    key, tab = rng.integers(0, n_acct, n), rng.integers(0, 2, n)
    val = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    for j, ty in enumerate((S.ACQUIRE_EXCLUSIVE, S.COMMIT_LOG, S.COMMIT_PRIM)):
        m["type"][j::3], m["table"][j::3], m["key"][j::3], m["val"][j::3], m["ver"][j::3] = ty, tab, key, val, np.arange(n)
    return m


# ---------------------------------------------------------------------------------------------- 1. digest vs reference state
def test_digest_tatp_after_a_trace_with_inserts_and_deletes():
    e = _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    for b in range(3):
        req = _committed_writes(o, 3000, seed=20 + b)
        assert e.submit(req).tobytes() == o.replay(req).tobytes()
    existing = [o.dump(t)[0] for t in range(5)]
    req = tracegen.tatp_random(20_000, existing, seed=5, n_sub_touch=40)
    assert e.submit(req).tobytes() == o.replay(req).tobytes()
    got = e.state_digest()
    assert len(got) == 5
    for t in range(5):
        want = np_digest(t, *o.dump(t))
        print("tatp digest", t, got[t], want)
        assert got[t] == want and got[t] == np_digest(t, *e.dump_rows(t)) and got[t]["rows"] > 0, t


def test_digest_store_and_smallbank_after_a_trace():
    req = tracegen.store_random(40_000, seed=77, n_sub_touch=30, p_set=0.5, p_insert=0.05)
    o = orc.StoreOracle(4500, 60)
    e = _engine(W.STORE, n_rows=1000)
    e.populate(60)
    assert e.submit(req).tobytes() == o.replay(req).tobytes()
    got = e.state_digest()
    assert got == [np_digest(0, *o.dump())] == _np_digests(e) and got[0]["rows"] > 60 * 12
    req = tracegen.sb_random(30_000, seed=3, n_acct_touch=40)
    o = orc.SmallbankOracle(1000, log_entries=70_000, populate_n=500)
    e = _engine(W.SMALLBANK, n_rows=1000, log_entries=70_000)
    e.populate(500)
    assert e.submit(req).tobytes() == o.replay(req).tobytes()
    got = e.state_digest()
    assert got == [np_digest(t, *o.dump(t)) for t in range(2)] == _np_digests(e) and got[0]["rows"] == 500


def test_digest_tatp_one_million_subscribers_and_two_shards():
    n = 1_000_000
    e = _engine(W.TATP, n_rows=n)
    e.populate(n)
    got = e.state_digest()
    assert e.stats()["pool_exhausted"] == 0
    for t in range(5):
        want = np_digest(t, *e.dump_rows(t))
        print("tatp 1M digest", t, got[t], want)
        assert got[t] == want, t
    assert got[0]["rows"] == n and sum(d["rows"] for d in got) > 4 * n
    del e
    # two shards loaded with the same rows: their digests combine to the unsharded engine's
    n = 20_000
    whole = _engine(W.TATP, n_rows=n)
    whole.populate(n)
    parts = []
    for i in range(2):
        s = _engine(W.TATP, n_rows=n, shard_index=i, shard_count=2)
        s.populate(n)
        parts.append(s.state_digest())
        assert parts[-1] == _np_digests(s)
    want = whole.state_digest()
    assert want == _np_digests(whole)
    for t in range(5):
        p, q = parts[0][t], parts[1][t]
        assert p["rows"] > 0 and q["rows"] > 0
        assert {"rows": p["rows"] + q["rows"], "sum": (p["sum"] + q["sum"]) % (1 << 64), "xr": p["xr"] ^ q["xr"]} == want[t], t


# ---------------------------------------------------------------------------------------------- 2. layout independence
def test_digest_does_not_depend_on_the_chains_locks_or_the_log():
    import torch

    cap = 4096
    prim = _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    dev = []
    for b in range(8):
        req = _committed_writes(o, 3000, seed=b)
        assert prim.submit(req).tobytes() == o.replay(req).tobytes()
        n, lost = prim.log_drain_device(buf, cap)
        assert (n, lost) == (3000, 0)
        dev.append(buf[:n * 64].clone())
    d_rec = torch.cat(dev)
    rep = _tatp()
    rep.log_apply_device(d_rec, 24_000, chunk=777)  # rebuilt from the log: the same rows in chains of its own
    want = prim.state_digest()
    assert want == [np_digest(t, *o.dump(t)) for t in range(5)]
    assert rep.state_digest() == want
    # locks taken and log records appended on the replica are not state
    m = np.zeros(400, wire.TATP_MSG)
    m["type"][:200], m["type"][200:] = T.ACQUIRE_LOCK, T.COMMIT_LOG
    for t in range(5):
        m["table"][t::5] = t
    m["key"] = np.tile(o.dump(0)[0][:40], 10)
    m["val"] = 7
    ring0 = rep.read_log(cap)[1]
    r = rep.submit(m)
    assert (r["type"][:200] == T.GRANT_LOCK).sum() > 20 and rep.read_log(cap)[1] != ring0
    assert sum(int(rep.read_locks(t)[0].sum()) for t in range(5)) > 20
    assert rep.state_digest() == want
    assert prim.state_diff(rep)[1]["total"] == 0


def test_digest_after_pool_recycling_and_snapshot_restore():
    """the churn of test_gpu_ahead's small-pool test: ~360 CALL_FORWARDING rows inserted and deleted pass after pass, the
    overflow entries recycled through the pend lists; a freed entry must never leave a valid slot behind for the flat scan"""
    n_sub, touch, rounds = 40, 30, 61
    o = orc.TatpOracle(n_sub, log_entries=50_000, populate_n=touch)
    keys = np.array([s | (sf << 32) | (st << 40) for s in range(touch) for sf in (1, 2, 3, 4) for st in (0, 8, 16)], np.uint64)
    e = _engine(W.TATP, n_rows=n_sub, log_entries=50_000, pool_entries=1500)
    e.populate(touch)
    for r in range(rounds):
        m = np.zeros(len(keys), wire.TATP_MSG)
        m["table"], m["key"], m["val"] = 4, keys, (r * 7) & 0xFF
        m["type"] = T.INSERT_PRIM if r % 2 == 0 else T.DELETE_PRIM
        assert e.submit(m).tobytes() == o.replay(m).tobytes()
        if r in (0, 1, 30, 31, 59):
            assert e.state_digest() == _np_digests(e), r
    assert e.stats()["pool_exhausted"] == 0
    got = e.state_digest()
    assert got == _np_digests(e) == [np_digest(t, *o.dump(t)) for t in range(5)] and got[4]["rows"] >= 360
    e.snapshot()
    m = np.zeros(len(keys), wire.TATP_MSG)
    m["table"], m["key"], m["type"] = 4, keys, T.DELETE_PRIM
    e.submit(m)
    mid = e.state_digest()
    assert mid == _np_digests(e) and mid[4]["rows"] == got[4]["rows"] - len(keys) and mid[:4] == got[:4]
    e.restore()
    assert e.state_digest() == got == _np_digests(e)
    e.reset()
    assert e.state_digest() == [{"rows": 0, "sum": 0, "xr": 0}] * 5


# ---------------------------------------------------------------------------------------------- 3. single differences
@pytest.mark.parametrize("case", ["set", "version", "delete", "insert"])
def test_one_difference_changes_one_tables_digest_and_gives_one_record(case):
    a, b = _tatp(), _tatp()
    t = 2
    keys, vers, vals = a.dump_rows(t)
    key, ver, val = keys[5], vers[5], vals[5]
    m = np.zeros(1, wire.TATP_MSG)
    m["table"], m["key"] = t, key
    if case == "set":
        m["type"], m["val"] = T.COMMIT_BCK, val ^ 0x55
    elif case == "version":
        m["type"], m["val"] = T.COMMIT_BCK, val  # the same value once more: only the version moves
    elif case == "delete":
        m["type"] = T.DELETE_BCK
    else:
        m["type"], m["key"], m["val"] = T.INSERT_BCK, key | np.uint64(1 << 45), 9
    ack = {"set": T.COMMIT_BCK_ACK, "version": T.COMMIT_BCK_ACK, "delete": T.DELETE_BCK_ACK, "insert": T.INSERT_BCK_ACK}[case]
    assert b.submit(m)["type"][0] == ack
    da, db = a.state_digest(), b.state_digest()
    assert db == _np_digests(b)
    assert [x == y for x, y in zip(da, db)] == [True, True, False, True, True]
    rec, st, _ = _diff(a, b, 16)
    want = np.zeros(1, wire.LOG_REC)
    want["table"] = t
    if case == "insert":
        want["key"], want["is_del"] = m["key"][0], 1
    else:
        want["key"], want["ver"], want["val"] = key, ver, val
    field = {"set": "val_differs", "version": "ver_only", "delete": "only_a", "insert": "only_b"}[case]
    assert st == {"total": 1, "only_a": 0, "only_b": 0, "val_differs": 0, "ver_only": 0, **{field: 1}}
    assert rec.tobytes() == want.tobytes()
    assert (rec.tobytes(), st) == (lambda r: (r[0].tobytes(), r[1]))(_np_full_diff(a, b))


# ---------------------------------------------------------------------------------------------- 4. + 5. diff at size, repair
@pytest.fixture(scope="module")
def diverged():
    """two tatp engines of 100,000 subscribers that took different write streams"""
    kw = dict(n_rows=100_000, cap=1 << 19)
    a, b = _tatp(**kw), _tatp(**kw)
    for e, seed in ((a, 3), (b, 4)):
        for m in _writes_in_rounds(e, 3, 50_000, seed=seed):
            e.submit(m)
        assert e.stats()["missing_keys"] == 0
    return a, b


def test_diff_at_size_equals_numpy_byte_for_byte(diverged):
    a, b = diverged
    before = _dumps(a), _dumps(b)
    want, wst = _np_full_diff(a, b)
    n0, st0 = a.state_diff(b)  # count only
    print("diff at size", st0)
    assert n0 == 0 and st0 == wst
    assert wst["total"] > 50_000 and min(wst[k] for k in ("only_a", "only_b", "val_differs")) > 1000
    assert set(np.unique(want["table"]).tolist()) == {0, 1, 2, 3, 4}
    rec, st, _ = _diff(a, b, wst["total"] + 10)
    assert st == wst and len(rec) == wst["total"]
    assert rec.tobytes() == want.tobytes()
    cap = wst["total"] // 3
    part, pst, buf = _diff(a, b, cap)
    assert pst == wst and len(part) == cap and part.tobytes() == want[:cap].tobytes()
    assert (buf[cap * 64:].cpu().numpy() == 0xEE).all()  # nothing written behind the caller's cap
    assert (_dumps(a), _dumps(b)) == before  # neither engine was touched: same rows in the same bucket and chain order


def test_repair_makes_the_replica_equal_and_leaves_the_rest_alone(diverged):
    a, b = diverged
    m = np.zeros(100, wire.TATP_MSG)  # some locks on the replica: not state, and not the repair's business
    m["type"], m["key"] = T.ACQUIRE_LOCK, np.arange(100)
    b.submit(m)
    a_before = _dumps(a)
    locks = [b.read_locks(t)[0].tobytes() for t in range(5)]
    ring, tail = b.read_log(1 << 19)
    requests = b.stats()["requests"]
    assert sum(np.frombuffer(x, "<u4").sum() for x in locks) > 50 and tail > 0
    rec, st, buf = _diff(a, b, a.state_diff(b)[1]["total"])
    rs = b.state_repair(buf, len(rec))
    print("repair", st, rs)
    assert rs["refused"] == 0 and rs["applied"] == st["total"]
    assert (rs["updated"], rs["inserted"], rs["deleted"]) == (st["val_differs"] + st["ver_only"], st["only_a"], st["only_b"])
    assert a.state_diff(b)[1]["total"] == 0 and b.state_diff(a)[1]["total"] == 0
    assert a.state_digest() == b.state_digest() == _np_digests(b)
    _same_rows(a, b)
    assert [b.read_locks(t)[0].tobytes() for t in range(5)] == locks
    ring1, tail1 = b.read_log(1 << 19)
    assert tail1 == tail and ring1.tobytes() == ring.tobytes()
    sb = b.stats()
    assert sb["requests"] == requests and sb["missing_keys"] == 0 and sb["pool_exhausted"] == 0
    assert _dumps(a) == a_before
    assert buf[:len(rec) * 64].cpu().numpy().tobytes() == rec.tobytes()  # the records stay untouched
    # the repaired replica is an ordinary engine: the same writes on both keep them equal
    for m in _writes_in_rounds(a, 1, 20_000, seed=9):
        a.submit(m)
        b.submit(m)
    assert a.state_digest() == b.state_digest()
    _same_rows(a, b)


def test_diff_and_repair_smallbank_and_store():
    n_acct = 10_000
    a, b = (_engine(W.SMALLBANK, n_rows=n_acct, log_entries=1 << 16) for _ in range(2))
    for e, seed in ((a, 1), (b, 2)):
        e.populate(n_acct)
        e.submit(_sb_writes(n_acct, 20_000, seed))
    want, wst = _np_full_diff(a, b)
    assert wst["only_a"] == wst["only_b"] == 0 and wst["val_differs"] > 5000  # updates only
    rec, st, buf = _diff(a, b, wst["total"])
    assert st == wst and rec.tobytes() == want.tobytes() and (rec["val"][:, 8:] == 0).all()
    locks = [b.read_locks(t) for t in range(2)]
    rs = b.state_repair(buf, len(rec))
    assert rs == {"applied": wst["total"], "updated": wst["total"], "inserted": 0, "deleted": 0, "refused": 0}
    assert a.state_diff(b)[1]["total"] == 0 and a.state_digest() == b.state_digest() == _np_digests(a)
    _same_rows(a, b, tables=2)
    for t in range(2):
        assert all((x == y).all() for x, y in zip(b.read_locks(t), locks[t]))
    # store: SETs and INSERTs of fresh keys, different on the two sides
    a, b = (_engine(W.STORE, n_rows=1000) for _ in range(2))
    for e, seed in ((a, 1), (b, 2)):
        e.populate(80)
        e.submit(tracegen.store_random(30_000, seed=seed, n_sub_touch=40, p_set=0.4, p_insert=0.05))
    want, wst = _np_full_diff(a, b)
    assert min(wst["only_a"], wst["only_b"], wst["val_differs"]) > 100
    rec, st, buf = _diff(a, b, wst["total"])
    assert st == wst and rec.tobytes() == want.tobytes()
    rs = b.state_repair(buf, len(rec))
    assert rs["applied"] == wst["total"] and rs["refused"] == 0
    assert a.state_diff(b)[1]["total"] == 0 and a.state_digest() == b.state_digest() == _np_digests(b)
    _same_rows(a, b, tables=1)
    assert b.stats()["missing_keys"] == 0


# ---------------------------------------------------------------------------------------------- 6. the lapped shipper
@pytest.mark.parametrize("auto", [False, True])
def test_a_lapped_shipper_resyncs_and_goes_on(auto):
    cap = 4096  # smaller than two batches of 3,000 records
    prim, rep = _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    ship = recovery.LogShipper(prim, rep, cap=cap, resync_on_loss=auto)
    seed = iter(range(300, 400))

    def batch():
        req = _committed_writes(o, 3000, seed=next(seed))
        assert prim.submit(req).tobytes() == o.replay(req).tobytes()

    for _ in range(3):
        batch()
        assert ship.step()["lost"] == 0
    _same_rows(prim, rep)
    batch()
    batch()  # two batches without a step: the ring laps the reader
    st = ship.step()
    assert st["lost"] == 6000 - cap
    missed = rep.stats()["missing_keys"]  # (what a replay behind lost records may have sent to rows that are not there)
    if auto:
        assert missed == 0  # the records behind the gap were dropped, not replayed
        assert st["resync"]["digests_equal"] and st["resync"]["records"] > 0 and st["applied"] == 0 and ship.resyncs == 1
    else:
        assert st["applied"] == cap and prim.state_digest() != rep.state_digest()  # lost for good without a resync
        out = ship.resync()
        assert out["digests_equal"] and out["rounds"] >= 1 and out["records"] > 0
    assert prim.state_digest() == rep.state_digest()
    _same_rows(prim, rep)
    assert ship.step() == {"applied": 0, "lost": 0}  # the cursor stands at the tail: nothing is applied twice
    for _ in range(3):
        batch()
        st = ship.step()
        assert st["lost"] == 0 and st["applied"] == 3000
        _same_rows(prim, rep)  # rows AND versions
    assert prim.state_digest() == rep.state_digest() and rep.stats()["missing_keys"] == missed


# ---------------------------------------------------------------------------------------------- 7. rounds
def test_resync_takes_as_many_rounds_as_the_buffer_needs():
    a, b = _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    for s in range(2):
        req = _committed_writes(o, 3000, seed=70 + s)
        assert a.submit(req).tobytes() == o.replay(req).tobytes()  # (the generator follows the rows through o: no key inserted twice)
    total = a.state_diff(b)[1]["total"]
    assert total > 300
    cap = 100
    out = recovery.resync(a, b, cap=cap, max_rounds=64)
    assert out == {"rounds": -(-total // cap), "records": total, "digests_equal": True}
    _same_rows(a, b)
    assert recovery.resync(a, b, cap=cap) == {"rounds": 0, "records": 0, "digests_equal": True}
    # too few rounds allowed: it stops, and says that the two still differ
    c = _tatp()
    out = recovery.resync(a, c, cap=cap, max_rounds=2)
    assert out == {"rounds": 2, "records": 2 * cap, "digests_equal": False}
    # a key the replica holds TWICE and the primary not at all: the diff sees the visible row only, so the second row
    # surfaces once the first is deleted -- one more round
    d = _tatp()
    k, v, x = a.dump_rows(1)
    ghost = np.array([k[0] | np.uint64(1 << 46)] * 2, np.uint64)
    assert not np.isin(ghost, k).any()
    d.load_rows(1, ghost, np.array([3, 4], "<u4"), np.stack([x[0], x[1]]))
    assert (d.dump_rows(1)[0] == ghost[0]).sum() == 2
    out = recovery.resync(a, d, max_rounds=8)
    assert out["digests_equal"] and out["rounds"] == 2 and out["records"] == total + 2
    _same_rows(a, d)


# ---------------------------------------------------------------------------------------------- 8. pool exhaustion
def test_repair_with_a_full_pool_applies_the_rest_and_says_so():
    a = _tatp()
    b = _engine(W.TATP, n_rows=300, log_entries=4096, pool_entries=8)  # empty, and next to no overflow entries
    rec, st, buf = _diff(a, b, a.state_diff(b)[1]["total"])
    assert st["only_a"] == st["total"] == sum(len(a.dump_rows(t)[0]) for t in range(5))
    with pytest.raises(_lib.DintError, match="pool full"):
        b.state_repair(buf, len(rec))
    rs = b.last_repair
    print("pool exhaustion", st, rs)
    assert rs["refused"] > 0 and rs["inserted"] == rs["applied"] == st["total"] - rs["refused"]
    assert b.stats()["pool_exhausted"] == rs["refused"]
    left, lst, _ = _diff(a, b, st["total"])
    want, wst = _np_full_diff(a, b)
    assert lst == wst and left.tobytes() == want.tobytes()
    assert lst["total"] == lst["only_a"] == rs["refused"]  # exactly the refused rows are still missing
    # the engine goes on answering: rows the repair stored read as they do on a fully populated reference server
    o = orc.TatpOracle(300, log_entries=4096)
    m = np.zeros(2000, wire.TATP_MSG)
    m["type"] = T.READ
    for t in range(5):
        k = a.dump_rows(t)[0]
        k = k[~np.isin(k, left["key"][left["table"] == t])]
        m["table"][t::5], m["key"][t::5] = t, k[np.arange(400) % len(k)]
    got = b.submit(m)  # (and dint_wait does not report the repair's refused inserts a second time)
    assert got.tobytes() == o.replay(m).tobytes() and (got["type"] == T.GRANT_READ).all()


# ---------------------------------------------------------------------------------------------- 9. refusals
def test_refusals():
    import torch

    buf = torch.zeros(4096 * 64, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def diff(x, y, ptr=None, cap=0):
        return x._L.dint_state_diff(x._h, y._h, ptr, cap, None, None)

    def repair(x, n=0, ptr=p):
        return x._L.dint_state_repair(x._h, ptr, n, None, None)

    def digest(x, cap=5):
        return x._L.dint_state_digest(x._h, (_lib.TableDigest * 5)(), cap, None)

    a, b = _tatp(), _tatp()
    assert diff(a, a) == EINVAL and diff(a, b) == 0
    assert diff(a, b, None, 10) == EINVAL and diff(a, b, p + 4, 10) == EINVAL  # no buffer / not 8-byte aligned
    assert digest(a, 4) == EINVAL and digest(a) == 5
    sb = _engine(W.SMALLBANK, n_rows=300, log_entries=4096)
    assert diff(a, sb) == EINVAL and diff(sb, a) == EINVAL  # another workload
    assert diff(a, _tatp(n_rows=400)) == EINVAL              # another size
    sh = _engine(W.TATP, n_rows=300, log_entries=4096, shard_index=0, shard_count=2)
    assert diff(a, sh) == EINVAL and diff(sh, a) == EINVAL and repair(sh, 1) == EINVAL and digest(sh) == 5
    for e in (_engine(W.FASST, n_slots=1024), _engine(W.TPL, n_slots=1024), _engine(W.LOG, log_entries=1024)):
        assert diff(a, e) == ESTATE and diff(e, a) == ESTATE and repair(e, 1) == ESTATE and digest(e) == ESTATE, e.workload
    assert repair(a, 5, None) == EINVAL and repair(a, 0, None) == 0
    # records out of bucket order: refused, nothing applied
    o = orc.TatpOracle(300, log_entries=1 << 20)
    a.submit(_committed_writes(o, 2000, seed=5))
    rec, st, good = _diff(a, b, a.state_diff(b)[1]["total"])
    assert len(rec) > 100
    before = _dumps(b)
    d_rev = _dev(rec[::-1].copy())
    assert repair(b, len(rec), d_rev.data_ptr()) == EINVAL and b"grouped" in b._L.dint_last_error()
    bad = rec.copy()
    bad["table"][7] = 5  # a table tatp has not
    d_bad = _dev(bad)
    assert repair(b, len(rec), d_bad.data_ptr()) == EINVAL
    assert _dumps(b) == before
    # an announced batch is the engine's next submission (as dint_snapshot): none of the three calls runs in front of it
    wx = _committed_writes(o, 1000, seed=11)
    o.replay(wx)  # (the second batch is generated for the rows the first leaves: no key inserted twice)
    x, y = _dev(wx), _dev(_committed_writes(o, 1000, seed=12))
    b.submit_device(x, 2000, None, 0, ahead=(y, 2000, None))
    assert digest(b) == ESTATE and b"announced" in b._L.dint_last_error()
    assert diff(a, b) == ESTATE and diff(b, a) == ESTATE and repair(b, len(rec), good.data_ptr()) == ESTATE
    b.submit_device(y, 2000)  # the announced batch after all: the engine goes on
    b.sync()
    assert digest(b) == 5 and diff(a, b) == 0
    n, st = a.state_diff(b, buf, 4096)
    assert n == st["total"] <= 4096 and repair(b, n) == 0
    assert a.state_digest() == b.state_digest()
    _same_rows(a, b)
