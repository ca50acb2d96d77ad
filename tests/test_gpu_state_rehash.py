"""A server's tables rehashed to another bucket count on the GPU (include/dint_abi.h dint_state_rehash,
dint_amd/csrc/k_rehash.hip, dint_amd/recovery.py rehash) against forms that share no code with it: numpy over dump_rows
with the fasthash of tests/shard_double.py (tests/test_state_rehash_host.py np_rehash), the digests, the state image's
check as an independent judge of the links, and the replies of the source itself.  Every comparison is exact."""
import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from test_state_image_host import np_bucket, same_dump
from test_state_rehash_host import np_foreign, np_rehash

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ENOMEM, ESTATE = -1, -2, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _set(wl, G, **kw):
    return [_engine(wl, shard_index=s, shard_count=G, **kw) for s in range(G)]


def _dumps(e):
    return [e.dump_rows(t) for t in range(NTAB[e.workload])]


def _refused(rc, dst, srcs, **kw):
    """the call is refused with rc, and the destination still dumps empty"""
    with pytest.raises(_lib.DintError, match=f"dint error {rc}:"):
        dst.state_rehash(srcs, **kw)
    for t in range(NTAB.get(dst.workload, 0)):
        assert len(dst.dump_rows(t)[0]) == 0
    return dst.last_rehash


def _check_against_numpy(srcs, dst):
    """dst holds what the numpy form makes of the sources' dumps, in srcs order; returns the rows that were foreign"""
    foreign = 0
    for t in range(NTAB[dst.workload]):
        dumps = [e.dump_rows(t) for e in srcs]
        assert same_dump(dst.dump_rows(t), np_rehash(dumps, dst.hash_size(t), dst.shard_index, dst.shard_count)), t
        foreign += np_foreign(dumps, dst.hash_size(t), dst.shard_index, dst.shard_count)
    return foreign


def _np_longest(keys, dst, t=0):
    g = np_bucket(keys, dst.hash_size(t)).astype(np.int64)
    g = g[g % dst.shard_count == dst.shard_index]
    return int(-(-np.bincount(g).max() // 4)) if len(g) else 0


def _vals(keys, tag):
    keys = np.asarray(keys, np.uint64)
    return (((keys[:, None] >> np.uint64(3)) + np.arange(40, dtype=np.uint64)[None, :] * np.uint64(5) + np.uint64(tag)) & np.uint64(0xFF)).astype("u1")


def _delete_rows(e, keys, table=0):
    """DELETE of the visible row of every key through the repair (the store has no delete on the wire): holes and freed entries"""
    import torch

    keys = np.asarray(keys, np.uint64)
    keys = keys[np.argsort(np_bucket(keys, e.hash_size(table)), kind="stable")]
    rec = np.zeros(len(keys), wire.LOG_REC)
    rec["key"], rec["is_del"], rec["table"] = keys, 1, table
    buf = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).cuda()
    assert e.state_repair(buf, len(rec))["deleted"] == len(keys)


def _store_insert(e, keys, tag):
    m = np.zeros(len(keys), wire.STORE_MSG)
    m["type"], m["key"], m["val"] = wire.Store.INSERT, keys, _vals(keys, tag)
    assert (e.submit(m)["type"] == wire.Store.INSERT_ACK).all()


def _store_read(e, keys):
    m = np.zeros(len(keys), wire.STORE_MSG)
    m["type"], m["key"] = wire.Store.READ, keys
    return e.submit(m)


# ---------------------------------------------------------------------------------------------- 1. store with chains
@pytest.fixture(scope="module")
def chained():
    """288 buckets, about 3,000 rows loaded in a shuffled order (10 rows, 3 entries a bucket), then INSERT / DELETE churn:
    holes, freed and reused pool entries, chains whose inline entry is not the head"""
    e = _engine(W.STORE, n_rows=64, pool_entries=4096)
    rng = np.random.default_rng(17)
    keys = tracegen.store_key(rng.permutation(1000)[:, None], np.arange(1, 4)[None, :], 0).ravel()
    rng.shuffle(keys)
    e.load_rows(0, keys, np.arange(len(keys), dtype="<u4"), _vals(keys, 1))
    _delete_rows(e, keys[::5])
    fresh = tracegen.store_key(3_000_000 + np.arange(500), 1, 0)
    _store_insert(e, fresh, 2)
    left = np.delete(keys, np.arange(0, len(keys), 5))
    _delete_rows(e, np.concatenate([left[1::7], fresh[::4]]))
    _store_insert(e, tracegen.store_key(4_000_000 + np.arange(300), 2, 8), 3)
    assert e.stats()["pool_exhausted"] == 0 and e.hash_size(0) == 288
    n = len(e.dump_rows(0)[0])
    assert 2600 < n < 3400
    yield e
    e.close()


@pytest.mark.parametrize("n_rows", [16, 64, 1024])
def test_store_chains_to_long_chains_a_compaction_and_a_sparse_table(chained, n_rows):
    src = chained
    before = src.dump_rows(0)
    dst = _engine(W.STORE, n_rows=n_rows, pool_entries=4096)
    st = dst.state_rehash([src])
    print(n_rows, st)
    assert _check_against_numpy([src], dst) == 0
    assert dst.state_digest() == src.state_digest()
    n = len(before[0])
    k = np.bincount(np_bucket(before[0], dst.hash_size(0)).astype(np.int64))
    assert st["rows_seen"] == st["rows_placed"] == st["tables"][0]["rows"] == n and st["rows_foreign"] == 0 and st["locks_held"] == 0
    assert st["tables"][0]["longest_chain"] == _np_longest(before[0], dst) == -(-k.max() // 4)
    assert st["tables"][0]["overflow_entries"] == int(np.maximum(-(-k // 4) - 1, 0).sum())
    if n_rows == 16:
        assert st["tables"][0]["longest_chain"] >= 10  # long chains, or the case is void
    # the image's check is an independent judge of the links: export -> import into a third blank engine
    third = _engine(W.STORE, n_rows=n_rows, pool_entries=4096)
    buf, nbytes, ist = dst.state_export(0, 1)
    assert ist["rows"] == n and ist["overflow_entries"] == st["tables"][0]["overflow_entries"]
    assert third.state_import(buf, nbytes)["rows"] == n
    assert same_dump(third.dump_rows(0), dst.dump_rows(0))
    assert same_dump(src.dump_rows(0), before)  # the source was only read
    dst.close(); third.close()


# ---------------------------------------------------------------------------------------------- 2. visibility with duplicates
def _same_bucket_keys(hash_size, bucket, n, start):
    cand = tracegen.store_key(start + np.arange(40_000), 1, 0)
    cand = cand[np_bucket(cand, hash_size).astype(np.int64) == bucket]
    assert len(cand) >= n
    return cand[:n]


def _visible(dump):
    """per key the first row in dump order: what a READ returns"""
    keys, vers, vals = dump
    _, first = np.unique(keys, return_index=True)
    return {int(keys[i]): (int(vers[i]), vals[i].tobytes()) for i in first}


def test_visible_row_of_every_key_stays_visible_and_the_host_way_does_not_keep_it():
    src = _engine(W.STORE, n_rows=64, pool_entries=1024)
    hs = src.hash_size(0)

    def load(keys, tag, ver):
        src.load_rows(0, keys, np.full(len(keys), ver, "<u4"), _vals(keys, tag))

    # bucket 5: the issue's case.  a b c d | e with d a second row of a's key: inline [a b c a'], then a newer entry [e]
    a, b, c, e = _same_bucket_keys(hs, 5, 4, 10_000_000)
    load([a, b, c], 1, 1); load([a], 2, 2); load([e], 1, 1)
    # bucket 9: copies in an older and a newer entry, and both orders inside one entry
    k = _same_bucket_keys(hs, 9, 8, 20_000_000)
    load(k[:4], 1, 1)                      # inline [k0 k1 k2 k3]
    load([k[4], k[0], k[5]], 2, 2); load([k[5]], 5, 5)  # a newer entry [k4 k0' k5 k5']: k0 in an older and a newer entry, k5 first copy first
    _delete_rows(src, [k[4]])              # a hole in front of them ...
    load([k[5]], 3, 3)                     # ... takes the copy loaded last: [k5'' k0' k5 k5']
    load([k[6]], 4, 4); load([k[6], k[7]], 6, 6)        # and a third entry [k6 k6' k7]
    # filler with chains, every key twice in a shuffled order
    rng = np.random.default_rng(4)
    fill = tracegen.store_key(rng.permutation(400), 2, 0)
    fill = fill[~np.isin(np_bucket(fill, hs).astype(np.int64), (5, 9))]
    twice = np.concatenate([fill, fill]); vers = np.concatenate([np.full(len(fill), 7, "<u4"), np.full(len(fill), 8, "<u4")])
    o = rng.permutation(len(twice))
    src.load_rows(0, twice[o], vers[o], _vals(twice[o], 0) + vers[o][:, None].astype("u1"))
    d = src.dump_rows(0)
    in9 = np_bucket(d[0], hs).astype(np.int64) == 9
    assert d[0][in9].tolist() == [k[6], k[6], k[7], k[5], k[0], k[5], k[5], k[0], k[1], k[2], k[3]]  # chain order as built
    assert d[1][in9].tolist() == [4, 6, 6, 3, 2, 2, 5, 1, 1, 1, 1]
    in5 = np_bucket(d[0], hs).astype(np.int64) == 5
    assert d[0][in5].tolist() == [e, a, b, c, a] and d[1][in5].tolist() == [1, 1, 1, 1, 2]
    allk = np.unique(d[0])
    want = _store_read(src, allk)
    vis = _visible(d)
    assert (want["type"] == wire.Store.GRANT_READ).all()
    assert all(vis[int(x)] == (int(v), val.tobytes()) for x, v, val in zip(allk, want["ver"], want["val"]))  # numpy agrees with the source
    for n_rows in (16, 64, 1024):
        dst = _engine(W.STORE, n_rows=n_rows, pool_entries=1024)
        dst.state_rehash([src])
        assert _check_against_numpy([src], dst) == 0
        assert _store_read(dst, allk).tobytes() == want.tobytes(), n_rows
        assert _visible(dst.dump_rows(0)) == vis
        dst.close()
    # the reason for the rule: dump_rows + load_rows into a twin of the same size answers a READ of `a` with its second row
    twin = _engine(W.STORE, n_rows=64, pool_entries=1024)
    twin.load_rows(0, *d)
    assert twin.state_digest() == src.state_digest()  # the same rows ...
    got = _store_read(twin, allk)
    differs = allk[(got["ver"] != want["ver"])]
    print("keys the host way answers differently:", len(differs), "of", len(allk))
    assert a in differs.tolist() and got["ver"][allk.tolist().index(a)] == 2  # ... another one visible
    src.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 3. later requests
@pytest.mark.parametrize("n_rows", [400, 100])
def test_store_later_requests_answer_the_same(n_rows):
    src = _engine(W.STORE, n_rows=200, pool_entries=8192)
    src.populate(200)
    dst = _engine(W.STORE, n_rows=n_rows, pool_entries=8192)
    dst.state_rehash([src])
    trace = tracegen.store_random(30_000, seed=6, n_sub_touch=200, p_set=0.4, p_insert=0.08)
    assert (trace["type"] == wire.Store.INSERT).sum() > 1500
    rs, rd = src.submit(trace), dst.submit(trace)
    assert rs.tobytes() == rd.tobytes()
    assert src.state_digest() == dst.state_digest() and dst.stats()["pool_exhausted"] == 0
    assert _visible(src.dump_rows(0)) == _visible(dst.dump_rows(0))
    src.close(); dst.close()


def _tatp_keys(t, s, a=1, st=0):
    s = np.asarray(s, np.uint64)
    if t < 2:
        return s
    return s | np.uint64(a << 32) | (np.uint64(st << 40) if t == 4 else np.uint64(0))


def _tatp_trace(existing, n_units, seed):
    """READ, COMMIT_BCK, INSERT_BCK / DELETE_BCK, and ACQUIRE_LOCK immediately followed by COMMIT_PRIM or ABORT of the same key:
    no two locks are ever open together.  Inserts only of absent keys: the tables never hold a key twice."""
    rng = np.random.default_rng(seed)
    live = [set(int(x) for x in ks) for ks in existing]
    cand = [np.concatenate([np.asarray(ks[:: max(1, len(ks) // 300)], np.uint64), _tatp_keys(t, 900_000 + np.arange(150), 2, 8)])
            for t, ks in enumerate(existing)]
    out = []
    kind = rng.integers(0, 5, n_units); tb = rng.integers(0, 5, n_units); pick = rng.integers(0, 1 << 30, n_units)
    for i in range(n_units):
        t = int(tb[i]); key = int(cand[t][pick[i] % len(cand[t])]); ex = key in live[t]
        if kind[i] == 0:
            ops = [T.READ]
        elif kind[i] == 1:
            ops = [T.COMMIT_BCK if ex else T.INSERT_BCK]
        elif kind[i] == 2:
            ops = [T.DELETE_BCK if ex else T.INSERT_BCK]
        elif kind[i] == 3:
            ops = [T.ACQUIRE_LOCK, T.COMMIT_PRIM] if ex else [T.READ]
        else:
            ops = [T.ACQUIRE_LOCK, T.ABORT] if ex else [T.READ]
        if ops[0] == T.INSERT_BCK:
            live[t].add(key)
        elif ops[0] == T.DELETE_BCK:
            live[t].discard(key)
        out += [(op, t, key) for op in ops]
    m = np.zeros(len(out), wire.TATP_MSG)
    m["type"], m["table"], m["key"] = [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
    m["val"] = rng.integers(0, 256, (len(out), 40), dtype=np.uint8)
    m["ver"] = rng.integers(0, 2**32, len(out), dtype=np.uint64).astype("<u4")
    return m


@pytest.mark.parametrize("flags", [0, _lib.FLAG_LOCK_SAME_KEY])
@pytest.mark.parametrize("n_rows", [4000, 1000])
def test_tatp_later_requests_answer_the_same_then_churn_on_the_pool(n_rows, flags):
    src = _engine(W.TATP, n_rows=2000, log_entries=1 << 16, flags=flags)
    src.populate(2000)
    d0 = _dumps(src)
    assert all(len(np.unique(d[0])) == len(d[0]) for d in d0) and len(d0[0][0]) == 2000  # no key twice
    dst = _engine(W.TATP, n_rows=n_rows, log_entries=1 << 16, flags=flags, pool_entries=16384)
    st = dst.state_rehash([src])
    assert _check_against_numpy([src], dst) == 0 and st["rows_placed"] == sum(len(d[0]) for d in d0)
    trace = _tatp_trace([d[0] for d in d0], 6000, seed=21)
    for op in (T.READ, T.COMMIT_BCK, T.INSERT_BCK, T.DELETE_BCK, T.ACQUIRE_LOCK, T.COMMIT_PRIM, T.ABORT):
        assert (trace["type"] == op).sum() > 200, op
    rs, rd = src.submit(trace), dst.submit(trace)
    assert (rs["type"][trace["type"] == T.ACQUIRE_LOCK] == T.GRANT_LOCK).all()
    assert rs.tobytes() == rd.tobytes()
    assert src.state_digest() == dst.state_digest()
    for t in range(5):
        assert not src.read_locks(t)[0].any() and not dst.read_locks(t)[0].any()
    # churn on the destination against a numpy row set: the pool is used on from pool_top, with empty free lists
    rng = np.random.default_rng(5)
    rows = [set(int(x) for x in dst.dump_rows(t)[0]) for t in range(5)]
    for rnd in range(3):
        t = 4 if rnd != 1 else 2
        fresh = _tatp_keys(t, 2_000_000 + 10_000 * rnd + np.arange(3000), 3, 16)
        gone = rng.choice(np.array(sorted(rows[t]), np.uint64), 1500, replace=False)
        m = np.zeros(4500, wire.TATP_MSG)
        m["table"] = t
        m["type"][:3000], m["key"][:3000] = T.INSERT_BCK, fresh
        m["type"][3000:], m["key"][3000:] = T.DELETE_BCK, gone
        m = m[rng.permutation(4500)]
        rep = dst.submit(m)
        assert set(rep["type"].tolist()) == {int(T.INSERT_BCK_ACK), int(T.DELETE_BCK_ACK)}
        rows[t] |= set(int(x) for x in fresh)
        rows[t] -= set(int(x) for x in gone)
    assert dst.stats()["pool_exhausted"] == 0
    for t in range(5):
        k = dst.dump_rows(t)[0]
        assert len(k) == len(rows[t]) and set(int(x) for x in k) == rows[t], t
    src.close(); dst.close()


# ---------------------------------------------------------------------------------------------- 4. shard sets
def _move(srcs, dsts):
    tot = recovery.rehash(srcs, dsts)
    want_foreign = [_check_against_numpy(srcs, d) for d in dsts]
    assert [p["rows_foreign"] for p in tot["per_engine"]] == want_foreign
    assert recovery.digest_sum(srcs) == recovery.digest_sum(dsts)
    assert tot["rows_placed"] == tot["rows_seen"] == sum(x["rows"] for x in recovery.digest_sum(srcs))
    return tot


def test_tatp_shard_sets_one_to_three_to_two_and_eight_to_one():
    kw = dict(log_entries=1 << 12)
    U = _engine(W.TATP, n_rows=2000, **kw)
    U.populate(2000)
    D3 = _set(W.TATP, 3, n_rows=4000, **kw)
    tot = _move([U], D3)  # 1 -> 3 at double size
    assert all(p["rows_foreign"] > 0 for p in tot["per_engine"])
    D2 = _set(W.TATP, 2, n_rows=2000, **kw)
    _move(D3, D2)  # 3 -> 2 at half size
    for t in range(5):  # ... which is where a set of two sharded from the start has them, row for row (no key twice: order is free of history)
        assert sorted(np.concatenate([e.dump_rows(t)[0] for e in D2]).tolist()) == sorted(U.dump_rows(t)[0].tolist())
    S8 = _set(W.TATP, 8, n_rows=2000, **kw)
    for e in S8:
        e.populate(2000)
    one = _engine(W.TATP, n_rows=2000, **kw)
    tot = _move(S8, [one])  # 8 -> 1
    assert tot["per_engine"][0]["rows_foreign"] == 0 and one.state_digest() == U.state_digest()
    for e in [U, one] + D3 + D2 + S8:
        e.close()


def test_smallbank_two_to_three():
    S2 = _set(W.SMALLBANK, 2, n_rows=5000, log_entries=1 << 12)
    for e in S2:
        e.populate(5000)
    D3 = _set(W.SMALLBANK, 3, n_rows=7000, log_entries=1 << 12)
    tot = _move(S2, D3)
    assert tot["rows_seen"] == 10_000 and all(p["rows_foreign"] > 3000 for p in tot["per_engine"])
    for e in S2 + D3:
        e.close()


# ---------------------------------------------------------------------------------------------- 5. locks
def _still_blank(dst, **kw):
    """dumps empty and takes an image: the import's own rule says it is blank"""
    twin = _engine(dst.workload, **kw)
    twin.populate(50)
    buf, n, st = twin.state_export(0, 1)
    assert all(len(d[0]) == 0 for d in _dumps(dst))
    assert dst.state_import(buf, n)["rows"] == st["rows"] > 0
    twin.close()


@pytest.mark.parametrize("wl", [W.TATP, W.SMALLBANK])
def test_held_locks_are_refused_or_dropped(wl):
    src = _engine(wl, n_rows=500, log_entries=1 << 12)
    src.populate(500)
    m = np.zeros(1, wire.MSG_DTYPE[wl])
    m["type"], m["key"] = (T.ACQUIRE_LOCK, 7) if wl == W.TATP else (S.ACQUIRE_SHARED, 7)
    assert src.submit(m)["type"][0] == (T.GRANT_LOCK if wl == W.TATP else S.GRANT_SHARED)
    a, b = src.read_locks(0)
    assert int((a != 0).sum() + (b != 0).sum()) == 1
    kw = dict(n_rows=1000, log_entries=1 << 12)
    dst = _engine(wl, **kw)
    st = _refused(ESTATE, dst, [src])
    assert st["locks_held"] == 1 and st["rows_placed"] == 0
    _still_blank(dst, **kw)
    dst2 = _engine(wl, **kw)
    st = dst2.state_rehash([src], drop_locks=True)
    assert st["locks_held"] == 1 and st["rows_placed"] == st["rows_seen"] == sum(len(d[0]) for d in _dumps(src)) >= 1000
    assert _check_against_numpy([src], dst2) == 0 and dst2.state_digest() == src.state_digest()
    for t in range(NTAB[wl]):
        assert not any(x.any() for x in dst2.read_locks(t))
    assert int(sum((x != 0).sum() for x in src.read_locks(0))) == 1  # the source keeps its lock
    for e in (src, dst, dst2):
        e.close()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_destination_untouched_and_blank(chained):
    src = chained
    n = len(src.dump_rows(0)[0])
    dst = _engine(W.STORE, n_rows=16, pool_entries=4096)
    _refused(EINVAL, dst, [src, dst])            # the destination among the sources
    _refused(EINVAL, dst, [])                    # no source
    _refused(EINVAL, dst, [src, src])            # a source twice
    tatp = _engine(W.TATP, n_rows=100)
    _refused(EINVAL, dst, [src, tatp])           # mixed workloads
    _refused(EINVAL, dst, [tatp])
    f1, f2 = _engine(W.FASST, n_slots=1000), _engine(W.FASST, n_slots=2000)
    _refused(ESTATE, f2, [f1])                   # lock tables keep no keys
    full = _engine(W.STORE, n_rows=16)
    full.populate(4)
    with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
        full.state_rehash([src])                 # a destination that is not blank
    assert len(full.dump_rows(0)[0]) == 4 * 12
    # a pool that is too small: the need is reported, and a destination created with it fits exactly
    small = _engine(W.STORE, n_rows=16, pool_entries=8)
    st = _refused(ENOMEM, small, [src])
    need = st["tables"][0]["overflow_entries"]
    assert need > 8 and st["rows_placed"] == n
    fits = _engine(W.STORE, n_rows=16, pool_entries=need)
    assert fits.state_rehash([src])["tables"][0]["overflow_entries"] == need
    assert _check_against_numpy([src], fits) == 0
    # after all that `dst` and `small` are still blank: the rehash itself is the proof
    for e in (dst, small):
        if e is small:
            with pytest.raises(_lib.DintError, match=f"dint error {ENOMEM}:"):
                e.state_rehash([src])
        else:
            assert e.state_rehash([src])["rows_placed"] == n
            with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
                e.state_rehash([src])            # ... and no longer afterwards
    for e in (dst, tatp, f1, f2, full, small, fits):
        e.close()


def test_a_bucket_over_the_chain_bound_is_refused_and_an_empty_source_is_not():
    big = _engine(W.STORE, n_rows=20_000, pool_entries=4096)
    keys = tracegen.store_key(np.arange(70_000), 1, 0)
    big.load_rows(0, keys, None, np.zeros((70_000, 40), "u1"))
    assert big.stats()["pool_exhausted"] == 0
    tiny = _engine(W.STORE, n_rows=1, pool_entries=32768)
    assert tiny.hash_size(0) == 4  # about 4,375 entries a bucket: over SI_MAX_RUN = 4095 overflow entries
    st = _refused(ESTATE, tiny, [big])
    assert st["rows_placed"] == 70_000 and st["tables"][0]["longest_chain"] > 4096
    empty = _engine(W.STORE, n_rows=64)
    st = tiny.state_rehash([empty])  # still blank; an empty source is fine ...
    assert st["rows_seen"] == 0 and st["rows_placed"] == 0 and len(tiny.dump_rows(0)[0]) == 0
    with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
        tiny.state_rehash([empty])  # ... and leaves a destination that is no longer blank
    for e in (big, tiny, empty):
        e.close()
