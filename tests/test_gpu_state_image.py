"""A server's tables moved to another shard layout on the GPU (include/dint_abi.h dint_state_export / dint_state_import,
dint_amd/csrc/k_image.hip, dint_amd/recovery.py reshard / save_state / load_state) against forms that share no code with
it: numpy over dump_rows and read_locks with the fasthash of tests/shard_double.py (tests/test_state_image_host.py
np_reshard / np_locks_*), and engines that were sharded that way from the start.  Every comparison is exact."""
import struct

import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from shard_double import fasthash_lid, kv_home, lid_home
from test_state_image_host import np_bucket, np_locks_global, np_locks_shard, np_reshard, same_dump

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ENOMEM, ESTATE = -1, -2, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _set(wl, G, **kw):
    return [_engine(wl, shard_index=s, shard_count=G, **kw) for s in range(G)]


def _routed(engines, req, home):
    """each shard's requests, in order, to that shard's engine; the replies scattered back"""
    h = home(req)
    rep = np.zeros_like(req)
    for s, e in enumerate(engines):
        idx = np.nonzero(h == s)[0]
        if len(idx):
            rep[idx] = e.submit(req[idx])
    return rep


def _kv_home(e, G):
    return kv_home([e.hash_size(t) for t in range(NTAB[e.workload])], G, 0)


def _dumps(e):
    return [e.dump_rows(t) for t in range(NTAB[e.workload])]


def _locks(e):
    return [e.read_locks(t) for t in range(NTAB[e.workload])] if e.workload != W.STORE else []


def _same_engine_state(a, b):
    return all(same_dump(x, y) for x, y in zip(_dumps(a), _dumps(b))) and all(same_dump(x, y) for x, y in zip(_locks(a), _locks(b)))


def _check_against_numpy(src, dst):
    """dst (H engines) holds what the numpy forms make of src's (G engines) dumps and lock words"""
    H, wl = len(dst), src[0].workload
    for t in range(NTAB[wl]):
        hs = src[0].hash_size(t)
        want = np_reshard([e.dump_rows(t) for e in src], hs, H)
        for j, e in enumerate(dst):
            assert same_dump(e.dump_rows(t), want[j]), (t, j)
        if wl != W.STORE:
            A, B = np_locks_global([e.read_locks(t) for e in src], hs)
            for j, e in enumerate(dst):
                assert same_dump(e.read_locks(t), np_locks_shard(A, B, hs, j, H)), (t, j)


def _digest_sum(engines):
    out = None
    for e in engines:
        d = e.state_digest()
        if out is None:
            out = [dict(x) for x in d]
        else:
            for x, y in zip(out, d):
                x["rows"] += y["rows"]; x["sum"] = (x["sum"] + y["sum"]) % (1 << 64); x["xr"] ^= y["xr"]
    return out


def _self_stats(e):
    s = _lib.ImageStats()
    _lib.check(e._L.dint_state_export(e._h, e.shard_index, e.shard_count, None, 0, s, 0))
    return {"buckets": s.buckets, "overflow_entries": s.overflow_entries, "rows": s.rows, "bytes": s.bytes}


# ---------------------------------------------------------------------------------------------- 1. chains
def _store_with_chains(n=20_000):
    e = _engine(W.STORE, n_rows=256, pool_entries=8192)
    m = np.zeros(n, wire.STORE_MSG)
    m["type"], m["key"] = wire.Store.INSERT, tracegen.store_key(3_000_000_000 + np.arange(n), 1, 0)
    m["val"] = (np.arange(n)[:, None] * 7 + np.arange(40)[None, :]) & 0xFF
    assert (e.submit(m)["type"] == wire.Store.INSERT_ACK).all()
    s = m[::3].copy()
    s["type"], s["val"] = wire.Store.SET, 0x5A
    e.submit(s)
    assert e.stats()["pool_exhausted"] == 0
    return e


def test_store_chains_one_to_two_three_eight():
    src = _store_with_chains()
    keys = src.dump_rows(0)[0]
    assert len(keys) == 20_000 and src.hash_size(0) == 1152
    assert np.bincount(np_bucket(keys, 1152).astype(np.int64)).max() > 8  # chains of at least three entries, or the test is void
    mine = _self_stats(src)
    assert mine["rows"] == 20_000 and mine["buckets"] == 1152 and mine["overflow_entries"] >= (20_000 - 4 * 1152) // 4
    for H in (2, 3, 8):
        dst = _set(W.STORE, H, n_rows=256, pool_entries=8192)
        tot = recovery.reshard([src], dst)
        _check_against_numpy([src], dst)
        assert tot["pieces"] == H and tot["rows"] == mine["rows"] and tot["overflow_entries"] == mine["overflow_entries"] and tot["buckets"] == 1152
        assert _digest_sum(dst) == src.state_digest()
        for e in dst:
            e.close()


# ---------------------------------------------------------------------------------------------- 2. against a set sharded from the start
def _tatp_t1(existing, seed):
    return np.concatenate([tracegen.tatp_random(6000, existing, seed=seed, n_sub_touch=40),
                           tracegen.tatp_random(3000, existing, seed=seed + 1, n_sub_touch=40, well_formed=False)])  # (duplicate inserts)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LOCK_SAME_KEY])
def test_tatp_resharded_equals_sharded_from_the_start(flags):
    kw = dict(n_rows=300, log_entries=1 << 16, flags=flags)
    U, F = _engine(W.TATP, **kw), _set(W.TATP, 3, **kw)
    for e in [U] + F:
        e.populate(300)
    home = _kv_home(U, 3)
    t1 = _tatp_t1([U.dump_rows(t)[0] for t in range(5)], 40)
    U.submit(t1)
    _routed(F, t1, home)
    assert any(U.read_locks(t)[0].any() for t in range(5))  # ACQUIREs left held
    stats0 = U.stats()
    M = _set(W.TATP, 3, **kw)
    log0 = [e.read_log(64)[1] for e in M]
    recovery.reshard([U], M)
    for s in range(3):
        assert _same_engine_state(M[s], F[s]), s
        assert M[s].read_log(64)[1] == log0[s] and M[s].stats()["requests"] == 0  # log ring and stats as they were
    _check_against_numpy([U], M)
    assert _digest_sum(M) == U.state_digest() and U.stats() == stats0  # (5. the digests add up; the source is untouched)
    t2 = _tatp_t1([U.dump_rows(t)[0] for t in range(5)], 50)
    ru, rm, rf = U.submit(t2), _routed(M, t2, home), _routed(F, t2, home)
    assert ru.tobytes() == rm.tobytes() == rf.tobytes()
    for s in range(3):
        assert _same_engine_state(M[s], F[s]), s


# ---------------------------------------------------------------------------------------------- 3. counters, non-trivial pieces
def test_smallbank_counters_round_trip_and_every_kind_of_piece():
    kw = dict(n_rows=1000, log_entries=1 << 16)
    U = _engine(W.SMALLBANK, **kw)
    U.populate(500)
    U.submit(tracegen.sb_random(30_000, seed=3, n_acct_touch=400))
    a, b = U.read_locks(0)
    assert a.any() and b.any()  # num_ex and num_sh non-zero at export
    D2, U2 = _set(W.SMALLBANK, 2, **kw), _engine(W.SMALLBANK, **kw)
    recovery.reshard([U], D2)
    _check_against_numpy([U], D2)
    assert _digest_sum(D2) == U.state_digest()
    recovery.reshard(D2, [U2])
    assert _same_engine_state(U, U2)  # 1 -> 2 -> 1: bit for bit
    D3, D4 = _set(W.SMALLBANK, 3, **kw), _set(W.SMALLBANK, 4, **kw)
    assert recovery.reshard(D2, D3)["pieces"] == 6  # every piece non-empty
    _check_against_numpy(D2, D3)
    _check_against_numpy([U], D3)
    for i in range(2):  # 2 -> 4: half the pieces are empty, and valid images of zero buckets
        for j in range(4):
            buf, n, st = D2[i].state_export(j, 4)
            assert (st["buckets"] == 0 and n == 320) == (i % 2 != j % 2), (i, j)
            assert D4[j].state_import(buf, n)["buckets"] == st["buckets"]
    _check_against_numpy(D2, D4)
    assert _digest_sum(D4) == U.state_digest() == _digest_sum(D3)
    D2b = _set(W.SMALLBANK, 2, **kw)
    assert recovery.reshard(D4, D2b)["pieces"] == 4
    for s in range(2):
        assert _same_engine_state(D2b[s], D2[s])


# ---------------------------------------------------------------------------------------------- 4. lock tables
@pytest.mark.parametrize("wl", [W.FASST, W.TPL])
def test_lock_tables_one_to_three_and_back(wl):
    gen = tracegen.fasst_random if wl == W.FASST else tracegen.tpl_random
    U = _engine(wl, n_slots=1000)
    req = gen(40_000, seed=9, key_space=20_000)
    assert len(np.unique(fasthash_lid(req["lid"]) % np.uint64(1000))) == 1000  # every slot is hit
    U.submit(req)
    a, b = U.read_locks()
    assert len(a) == 1000 and (a | b).any()
    D = _set(wl, 3, n_slots=1000)
    tot = recovery.reshard([U], D)
    assert tot["buckets"] == 1000 and tot["rows"] == int(((a | b) != 0).sum())
    for j, e in enumerate(D):
        x, y = e.read_locks()
        assert len(x) == 334  # local sizes are ceil-divided
        wa, wb = np.zeros(334, "<u4"), np.zeros(334, "<u4")
        wa[:len(a[j::3])], wb[:len(b[j::3])] = a[j::3], b[j::3]
        assert same_dump((x, y), (wa, wb)), j
    U2 = _engine(wl, n_slots=1000)
    recovery.reshard(D, [U2])
    assert same_dump(U2.read_locks(), (a, b))
    more = gen(5000, seed=10, key_space=20_000)
    assert U.submit(more).tobytes() == U2.submit(more).tobytes() == _routed(D, more, lid_home(1000, 3)).tobytes()


# ---------------------------------------------------------------------------------------------- 6. pool life on both sides
def test_pool_recycling_on_the_source_and_on_the_destinations():
    """the source after the churn of test_gpu_state_sync.py test_digest_after_pool_recycling_and_snapshot_restore (its
    recipe: ~360 CALL_FORWARDING rows inserted and deleted pass after pass through a pool of 1,500 entries, which leaves
    entries on the free and the pend lists), stopped after an insert round; then the same churn goes on on both sides"""
    n_sub, touch, rounds = 40, 30, 61
    keys = np.array([s | (sf << 32) | (st << 40) for s in range(touch) for sf in (1, 2, 3, 4) for st in (0, 8, 16)], np.uint64)
    kw = dict(n_rows=n_sub, log_entries=50_000, pool_entries=1500)
    U = _engine(W.TATP, **kw)
    U.populate(touch)

    def churn(r):
        m = np.zeros(len(keys), wire.TATP_MSG)
        m["table"], m["key"], m["val"] = 4, keys, (r * 7) & 0xFF
        m["type"] = T.INSERT_PRIM if r % 2 == 0 else T.DELETE_PRIM
        return m

    taken = freed = 0
    held = _self_stats(U)["overflow_entries"]
    for r in range(rounds):
        U.submit(churn(r))
        now = _self_stats(U)["overflow_entries"]
        taken, freed, held = taken + max(0, now - held), freed + max(0, held - now), now
    assert U.stats()["pool_exhausted"] == 0 and len(U.dump_rows(4)[0]) >= 360
    # the precondition: entries were freed and handed out again -- the insert rounds took more overflow entries than the pool
    # has, and none was refused, so the free and pend lists were in use (pool_top never reached pool_entries)
    print("pool churn: taken", taken, "freed", freed, "held at export", held)
    assert taken > 1500 > held > 0 and freed > 0
    D = _set(W.TATP, 2, **kw)
    tot = recovery.reshard([U], D)
    assert tot["overflow_entries"] > 0
    _check_against_numpy([U], D)
    home = _kv_home(U, 2)
    for r in range(rounds, rounds + 12):  # deletes and re-inserts: the destinations' imported entries are freed and recycled
        m = churn(r)
        if r % 4 == 0:
            m = m[::-1].copy()  # (other slot positions than before)
        assert U.submit(m).tobytes() == _routed(D, m, home).tobytes(), r
    assert all(e.stats()["pool_exhausted"] == 0 for e in [U] + D)
    _check_against_numpy([U], D)
    assert _digest_sum(D) == U.state_digest()


# ---------------------------------------------------------------------------------------------- 7. at size
def test_tatp_twenty_thousand_subscribers_one_to_eight():
    from dint_amd.driver import Driver
    from dint_amd.replay import ShardGroup

    n_sub, clients = 20_000, 5000
    g = ShardGroup(W.TATP, n_sub, log_entries=200_000)
    d = Driver(W.TATP, clients, n_sub, zipf_theta=0.8)
    for _ in range(25):
        d.consume(g.submit(d.next()))
    U = g.engines[0]
    assert any(U.read_locks(t)[0].any() for t in range(5))
    D = _set(W.TATP, 8, n_rows=n_sub, log_entries=1024, max_pass=4096)
    tot = recovery.reshard([U], D)
    assert tot["pieces"] == 8 and tot["rows"] == sum(len(U.dump_rows(t)[0]) for t in range(5))
    _check_against_numpy([U], D)
    assert _digest_sum(D) == U.state_digest()


# ---------------------------------------------------------------------------------------------- 7b. more workgroups than scan threads
def _by_key(dump):
    o = np.argsort(dump[0], kind="stable")
    return tuple(x[o] for x in dump)


def test_store_of_more_than_1024_workgroups_export_import_and_rehash():
    """270,000 buckets = 1,055 workgroups of 256: a thread of the one-workgroup scan of the workgroups' counts (export, the
    import's check, the rehash) owns two counts.  About 300 chained buckets in workgroups of either parity up to the last
    one, so a dropped second count shifts the `first` of every later bucket's run."""
    kw = dict(n_rows=60_000, pool_entries=4096)
    src = _engine(W.STORE, **kw)
    hs = src.hash_size(0)
    assert hs == 270_000 and -(-hs // 256) == 1055
    cand = tracegen.store_key(7_000_000_000 + np.arange(1_500_000), 1, 0)
    b = np_bucket(cand, hs).astype(np.int64)
    chained = cand[(b % 900 == 899) | (b == hs - 1)]  # every candidate of 301 buckets: 5.5 on average
    keys = np.unique(np.concatenate([cand[:3000], chained]))
    np.random.default_rng(5).shuffle(keys)
    vals = ((keys[:, None] >> np.uint64(2)) + np.arange(40, dtype=np.uint64)[None, :] * np.uint64(3)).astype("u1")
    src.load_rows(0, keys, np.arange(len(keys), dtype="<u4"), vals)
    assert src.stats()["pool_exhausted"] == 0
    want, digest = _by_key(src.dump_rows(0)), src.state_digest()
    assert len(want[0]) == len(keys) and digest[0]["rows"] == len(keys)
    # export (0, 1) -> (0, 1)
    buf, n, st = src.state_export(0, 1)
    assert st["buckets"] == hs and st["rows"] == len(keys) and 200 < st["overflow_entries"] < 4096
    img = buf[:n].cpu().numpy()
    assert _lib.load().dint_state_image_check_host(img.ctypes.data, n) == 0
    off, n_b, n_ovf = (struct.unpack_from("<Q", img, 64 + k)[0] for k in (32, 8, 16))
    d = np.frombuffer(img, np.dtype([("id", "<u8"), ("first", "<u4"), ("count", "<u4")]), n_b, off)
    wg = np.nonzero(d["count"])[0] // 256
    assert n_b == hs and (wg % 2 == 0).any() and (wg % 2 == 1).any() and wg.max() == 1054  # or the test is void
    count = d["count"].astype(np.int64)
    assert count.sum() == n_ovf == st["overflow_entries"]
    assert (d["first"] == np.cumsum(count) - count).all()
    # ... imported into a blank twin
    twin = _engine(W.STORE, **kw)
    assert twin.state_import(buf, n)["rows"] == len(keys)
    assert twin.state_digest() == digest and same_dump(_by_key(twin.dump_rows(0)), want)
    # rehashed into a blank engine of the same n_rows
    dst = _engine(W.STORE, **kw)
    rs = dst.state_rehash([src])
    assert rs["rows_placed"] == len(keys) and rs["rows_foreign"] == 0
    assert dst.state_digest() == digest and same_dump(_by_key(dst.dump_rows(0)), want)
    for e in (src, twin, dst):
        e.close()


# ---------------------------------------------------------------------------------------------- 8. file
def _small_tatp(flags=0):
    e = _engine(W.TATP, n_rows=300, log_entries=1 << 16, flags=flags)
    e.populate(300)
    e.submit(_tatp_t1([e.dump_rows(t)[0] for t in range(5)], 60))
    return e


def test_save_and_load_state_and_a_corrupt_file(tmp_path):
    U = _small_tatp()
    path = tmp_path / "u.img"
    st = recovery.save_state(U, path)
    assert path.stat().st_size == st["bytes"] and st["overflow_entries"] > 0
    img = np.fromfile(path, np.uint8)
    # flip one link word: the head of the first bucket of table 0 whose chain is its inline entry alone
    off, n_b = struct.unpack_from("<Q", img, 64 + 32)[0], struct.unpack_from("<Q", img, 64 + 8)[0]
    heads = [struct.unpack_from("<I", img, off + 16 * n_b + 256 * b + 56)[0] for b in range(n_b)]
    at = off + 16 * n_b + 256 * heads.index(1) + 56
    bad = img.copy()
    bad[at:at + 4] = np.frombuffer(struct.pack("<I", 0x7FFFFFF0), np.uint8)
    bad.tofile(tmp_path / "bad.img")
    V = _engine(W.TATP, n_rows=300, log_entries=1 << 16)
    with pytest.raises(_lib.DintError, match="image refused"):
        recovery.load_state(V, tmp_path / "bad.img")
    assert all(len(V.dump_rows(t)[0]) == 0 for t in range(5))
    got = recovery.load_state(V, path)  # ... and V is still blank
    assert got == st
    assert _same_engine_state(U, V)
    t2 = _tatp_t1([U.dump_rows(t)[0] for t in range(5)], 70)
    assert U.submit(t2).tobytes() == V.submit(t2).tobytes()
    assert _same_engine_state(U, V)


# ---------------------------------------------------------------------------------------------- 9. refusals
def _raw_import(e, buf, n):
    s = _lib.ImageStats()
    rc = e._L.dint_state_import(e._h, buf.data_ptr(), n, s, 0)
    return rc, e._L.dint_last_error().decode()


def _empty(e):
    return all(len(e.dump_rows(t)[0]) == 0 for t in range(NTAB[e.workload])) and not any(a.any() or b.any() for a, b in _locks(e))


def test_import_refusals_leave_the_destination_untouched():
    import torch

    U = _small_tatp()
    buf, n, st = U.state_export()
    kw = dict(n_rows=300, log_entries=1 << 16)
    # a destination that is not blank
    V = _engine(W.TATP, **kw)
    V.populate(10)
    before = [tuple(x.tobytes() for x in d) for d in _dumps(V)]
    assert _raw_import(V, buf, n)[0] == ESTATE and before == [tuple(x.tobytes() for x in d) for d in _dumps(V)]
    V.reset()  # ... blank again
    assert _raw_import(V, buf, n)[0] == 0 and _same_engine_state(U, V)
    # the same piece twice
    assert _raw_import(V, buf, n)[0] == ESTATE and _same_engine_state(U, V)
    # other n_rows, other workload, other flags
    for e in (_engine(W.TATP, n_rows=400, log_entries=1 << 16), _engine(W.STORE, n_rows=300), _engine(W.TATP, flags=_lib.FLAG_LOCK_SAME_KEY, **kw)):
        rc, msg = _raw_import(e, buf, n)
        assert rc == EINVAL and "image refused" in msg and _empty(e), msg
    # an image for (1, 2) into engine (0, 2)
    half, hn, _ = U.state_export(1, 2)
    Z = _set(W.TATP, 2, **kw)
    assert _raw_import(Z[0], half, hn)[0] == EINVAL and _empty(Z[0])
    assert _raw_import(Z[1], half, hn)[0] == 0 and not _empty(Z[1])
    # truncated
    assert _raw_import(_engine(W.TATP, **kw), buf, n - 16)[0] == EINVAL
    # an out-of-range link word patched in where the image lies: the check kernel refuses before a table is touched
    host = buf[:n].cpu().numpy()
    off, n_b = struct.unpack_from("<Q", host, 64 + 40 * 4 + 32)[0], struct.unpack_from("<Q", host, 64 + 40 * 4 + 8)[0]
    at = off + 16 * n_b + 56  # `head` of the first bucket of table 4
    patched = buf.clone()
    patched[at:at + 4] = torch.tensor([0, 0xFF, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")
    X = _engine(W.TATP, **kw)
    rc, msg = _raw_import(X, patched, n)
    assert rc == EINVAL and "link" in msg and _empty(X), msg
    assert _raw_import(X, buf, n)[0] == 0 and _same_engine_state(U, X)  # (still blank, and the image itself was good)


def test_export_refusals_and_the_pool():
    import torch

    src = _store_with_chains(8000)
    mine = _self_stats(src)
    assert mine["overflow_entries"] > 16
    # a buffer one byte short: DINT_ENOMEM, the size reported, nothing written
    buf = torch.full((mine["bytes"] + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    s = _lib.ImageStats()
    assert src._L.dint_state_export(src._h, 0, 1, buf.data_ptr(), mine["bytes"] - 1, s, 0) == ENOMEM
    assert s.bytes == mine["bytes"] and bool((buf == 0xEE).all())
    assert src._L.dint_state_export(src._h, 0, 1, buf.data_ptr(), mine["bytes"], s, 0) == 0
    assert bool((buf[mine["bytes"]:] == 0xEE).all()) and not bool((buf[:mine["bytes"]] == 0xEE).all())
    assert src._L.dint_state_export(src._h, 2, 2, None, 0, s, 0) == EINVAL
    # a destination whose pool is smaller than the image's need
    small = _engine(W.STORE, n_rows=256, pool_entries=16)
    rc, msg = _raw_import(small, buf, mine["bytes"])
    assert rc == ENOMEM and "pool" in msg and _empty(small)
    # overflow entries in a table without buckets (they belong to no run): refused, the pool and the digest as they were
    from test_state_image_host import _orphans

    orphans = torch.from_numpy(_orphans()).cuda()
    blank = _engine(W.STORE, n_rows=256, pool_entries=8192)
    d0 = blank.state_digest()
    rc, msg = _raw_import(blank, orphans, orphans.numel())
    assert rc == EINVAL and "sizes in the header" in msg and _empty(blank) and blank.state_digest() == d0 == [{"rows": 0, "sum": 0, "xr": 0}]
    assert _self_stats(blank)["overflow_entries"] == 0
    assert _raw_import(blank, buf, mine["bytes"])[0] == 0 and _self_stats(blank) == mine  # (still blank; every pool entry it takes is the good image's)
    # a pending announcement, on the source and on the destination
    req = tracegen.store_random(40_000, seed=8, n_sub_touch=40, p_set=0.4, p_insert=0.05)
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()
    e = _engine(W.STORE, n_rows=1000)
    e.populate(80)
    a, b = up(req[:20_000]), up(req[20_000:])
    e.submit_device(a, 20_000, None, 0, ahead=(b, 20_000, None))
    assert e._L.dint_state_export(e._h, 0, 1, None, 0, s, 0) == ESTATE and b"announced" in e._L.dint_last_error()
    assert _raw_import(e, buf, mine["bytes"])[0] == ESTATE
    e.submit_device(b, 20_000)
    e.sync()
    assert e._L.dint_state_export(e._h, 0, 1, None, 0, s, 0) == 0
    # log_server
    lg = _engine(W.LOG, log_entries=4096)
    assert lg._L.dint_state_export(lg._h, 0, 1, None, 0, s, 0) == ESTATE
    assert _raw_import(lg, buf, mine["bytes"])[0] == ESTATE
