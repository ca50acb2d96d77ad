"""Rows loaded and the population generated without leaving the GPU (dint_load_rows_device / dint_populate_device; the rule is
dint_amd/csrc/state_load.h) against twins that take the same rows through the host path (dint_populate / dint_load_rows, unchanged):
dumps in order, digests, table reports, a clean verify, lock words, then replies to a mixed trace against the twin and the CPU
oracle, and the refusals.  Engines are small (n_rows = 64: 24 / 60 / 90 buckets for tatp) and populated with 2,500 subscribers, so
chains reach tens of entries; one engine has the ordinary shape."""
import ctypes as C

import numpy as np
import pytest
import torch

import tracegen
from dint_amd import _lib, wire
from dint_amd.engine import Engine
from dint_amd import recovery
from kvkeys import keys_by_bucket, np_bucket, overflow_need, raw_submit
from load_helpers import dev, load_dev, pool_need, rows_host, same_state
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W = wire.Workload
EINVAL, ENOMEM, ESTATE = -1, -2, -5
N_TABLES = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
N_POP = 2500
PER = [0, 1, 4, 5, 8, 9, 41]

SHAPES = [(W.TATP, 64, N_POP, None), (W.STORE, 64, N_POP, None), (W.SMALLBANK, 64, N_POP, None), (W.TATP, 20000, 20000, 0)]


@pytest.mark.parametrize("wl,n_rows,n_pop,pool", SHAPES, ids=["tatp", "store", "smallbank", "tatp-ordinary"])
def test_populate_device_equals_a_host_populated_twin(wl, n_rows, n_pop, pool):
    pool = pool_need(wl, n_rows, n_pop) if pool is None else pool
    a, b = Engine(wl, n_rows=n_rows, pool_entries=pool), Engine(wl, n_rows=n_rows, pool_entries=pool)
    b.populate(n_pop)
    r = a.populate_device(n_pop)
    assert r is a.last_load and r["direct"] == 1 and all(t["direct"] == 1 for t in r["tables"]) and r["foreign_rows"] == 0
    assert r["rows_loaded"] == sum(d["rows"] for d in b.state_digest()) and r["temp_bytes"] > 0
    for t, hs in enumerate(recovery.hash_sizes(wl, n_rows)):
        g = np_bucket(rows_host(wl, t, n_pop)[0], hs).astype(np.int64)
        per = np.bincount(g, minlength=hs)
        assert r["tables"][t] == {"rows": len(g), "overflow_entries": overflow_need(per), "longest_chain_entries": -(-int(per.max()) // 4), "direct": 1}
    same_state(a, b)
    # what is direct once is not direct twice: the engine is not blank any more
    with pytest.raises(_lib.DintError, match="dint error -5"):
        a.populate_device(n_pop)
    a.close(); b.close()


def test_a_three_shard_set_keeps_its_home_rows():
    wl, n_rows = W.TATP, 64
    pools = [pool_need(wl, n_rows, N_POP, (i, 3)) for i in range(3)]
    dev_set = [Engine(wl, n_rows=n_rows, pool_entries=pools[i], shard_index=i, shard_count=3) for i in range(3)]
    host_set = [Engine(wl, n_rows=n_rows, pool_entries=pools[i], shard_index=i, shard_count=3) for i in range(3)]
    tot = recovery.populate_set(dev_set, N_POP)
    all_rows = 0
    for i in range(3):
        host_set[i].populate(N_POP)
        same_state(dev_set[i], host_set[i])
        foreign = 0
        for t, hs in enumerate(recovery.hash_sizes(wl, n_rows)):
            g = np_bucket(rows_host(wl, t, N_POP)[0], hs).astype(np.int64)
            foreign += int((g % 3 != i).sum())
            all_rows += int((g % 3 == i).sum())
        assert dev_set[i].last_load["foreign_rows"] == foreign and dev_set[i].last_load["direct"] == 1
    assert tot["rows_loaded"] == all_rows
    for e in dev_set + host_set:
        e.close()


def bucket_rows(hs, seed, dup=True):
    """keys with PER rows per bucket (the pattern repeated over the table), insertion order mixed; rows 3 and 4 of the last
    41-row bucket share a key; explicit versions"""
    per = (PER * (hs // len(PER) + 1))[:hs]
    keys = keys_by_bucket(hs, per, seed=seed)
    keys = keys[np.random.default_rng(seed).permutation(len(keys))]
    dup_key = None
    if dup:
        b = max(i for i, p in enumerate(per) if p == 41)
        at = np.nonzero(np_bucket(keys, hs) == np.uint64(b))[0]
        keys[at[4]] = keys[at[3]]
        dup_key = int(keys[at[3]])
    vers = (np.arange(len(keys)) + 900).astype("<u4")
    vals = ((np.arange(len(keys))[:, None] * 5 + np.arange(40)[None, :]) % 253).astype(np.uint8)
    return keys, vers, vals, per, dup_key


def store_read(key):
    m = np.zeros(1, wire.STORE_MSG)
    m["type"], m["key"] = int(wire.Store.READ), key
    return m


def test_load_rows_device_equals_load_rows_and_a_second_load_takes_the_passes():
    a, b = Engine(W.STORE, n_rows=16, pool_entries=512), Engine(W.STORE, n_rows=16, pool_entries=512)
    hs = a.hash_size(0)
    assert hs == 72
    keys, vers, vals, per, dup_key = bucket_rows(hs, seed=4)
    r = load_dev(a, 0, keys, vers, vals)
    b.load_rows(0, keys, vers, vals)
    assert (r["direct"], r["rows_loaded"], r["foreign_rows"]) == (1, len(keys), 0)
    assert r["tables"][0] == {"rows": len(keys), "overflow_entries": overflow_need(per), "longest_chain_entries": 11, "direct": 1}
    same_state(a, b)
    ra, rb = raw_submit(a, store_read(dup_key)), raw_submit(b, store_read(dup_key))
    assert ra[0] == rb[0] == 0 and ra[1].tobytes() == rb[1].tobytes() and ra[1]["type"][0] == int(wire.Store.GRANT_READ)
    # more rows into the same table: the passes, formed on the device; versions left out
    k2, _, v2, _, _ = bucket_rows(hs, seed=5, dup=False)
    r = load_dev(a, 0, k2, None, v2)
    b.load_rows(0, k2, None, v2)
    assert (r["direct"], r["rows_loaded"], r["tables"][0]["direct"]) == (0, len(k2), 0)
    same_state(a, b)
    a.close(); b.close()


def test_a_load_after_a_request_takes_the_passes():
    a, b = Engine(W.STORE, n_rows=16, pool_entries=512), Engine(W.STORE, n_rows=16, pool_entries=512)
    keys, vers, vals, per, dup_key = bucket_rows(72, seed=6)
    for e in (a, b):
        assert raw_submit(e, store_read(12345))[0] == 0
    r = load_dev(a, 0, keys, vers, vals)
    b.load_rows(0, keys, vers, vals)
    assert r["direct"] == 0 and r["rows_loaded"] == len(keys)
    same_state(a, b)
    # ... and after a reset the table is untouched again
    a.reset()
    assert load_dev(a, 0, keys, vers, vals)["direct"] == 1
    same_state(a, b)
    a.close(); b.close()


def test_smallbank_rows_and_the_second_table():
    """8-byte values in 128-byte entries; a direct load into one table leaves the other untouched and still direct"""
    a, b = Engine(W.SMALLBANK, n_rows=64, pool_entries=256), Engine(W.SMALLBANK, n_rows=64, pool_entries=256)
    hs = a.hash_size(1)
    keys, vers, vals, per, _ = bucket_rows(hs, seed=8)
    vals = vals[:, :8].copy()
    for t in (1, 0):
        r = load_dev(a, t, keys, vers, vals)
        b.load_rows(t, keys, vers, vals)
        assert r["direct"] == 1 and r["tables"][t]["overflow_entries"] == overflow_need(per)
    same_state(a, b)
    a.close(); b.close()


def test_replies_after_loading_equal_the_twin_and_the_oracle():
    n_rows, n_pop = 64, 600
    pool = 4 * pool_need(W.TATP, n_rows, n_pop) + 2000
    a, b = (Engine(W.TATP, n_rows=n_rows, log_entries=1 << 16, pool_entries=pool) for _ in range(2))
    a.populate_device(n_pop)
    b.populate(n_pop)
    o = orc.TatpOracle(n_rows, log_entries=1 << 16, populate_n=n_pop)
    req = tracegen.tatp_random(6000, [o.dump(t)[0] for t in range(5)], seed=21, n_sub_touch=n_pop)
    assert np.isin(req["type"], (int(wire.Tatp.INSERT_PRIM), int(wire.Tatp.DELETE_PRIM))).sum() > 100
    want = o.replay(req)
    for e in (a, b):
        got = np.concatenate([e.submit(req[k:k + 1500]) for k in range(0, len(req), 1500)])
        assert got.tobytes() == want.tobytes()
    for t in range(5):
        x, y, z = a.dump_rows(t), b.dump_rows(t), o.dump(t)
        assert all((p == q).all() and (p == s).all() for p, q, s in zip(x, y, z))
    a.close(); b.close()


def empty(e):
    return all(len(e.dump_rows(t)[0]) == 0 for t in range(N_TABLES[e.workload])) and all(d["rows"] == 0 for d in e.state_digest())


def test_refusals_leave_the_tables_empty():
    keys, vers, vals, per, _ = bucket_rows(72, seed=4)
    need = overflow_need(per)
    e = Engine(W.STORE, n_rows=16, pool_entries=need - 1)
    with pytest.raises(_lib.DintError, match="dint error -2"):
        load_dev(e, 0, keys, vers, vals)
    assert e.last_load["tables"][0]["overflow_entries"] == need and empty(e)
    assert e.state_stats()[0]["pool_top"] == 0
    # (still untouched: a smaller load goes the direct way)
    assert load_dev(e, 0, keys[:50], vers[:50], vals[:50])["direct"] == 1
    e.close()
    e = Engine(W.STORE, n_rows=16, pool_entries=need)  # exactly the need: fits
    assert load_dev(e, 0, keys, vers, vals)["direct"] == 1 and e.state_stats()[0]["pool_top"] == need
    e.reset()
    # misaligned arrays
    dk, dv, dx = dev(keys), dev(vers), dev(vals)
    L, s = _lib.load(), _lib.LoadStats()
    for kp, vp, xp in ((dk.data_ptr() + 4, dv.data_ptr(), dx.data_ptr()), (dk.data_ptr(), dv.data_ptr() + 2, dx.data_ptr()),
                       (dk.data_ptr(), dv.data_ptr(), dx.data_ptr() + 4)):
        assert L.dint_load_rows_device(e._h, 0, kp, vp, xp, 10, C.byref(s), None) == EINVAL
    assert L.dint_load_rows_device(e._h, 1, dk.data_ptr(), None, dx.data_ptr(), 10, C.byref(s), None) == EINVAL
    assert L.dint_load_rows_device(e._h, 0, None, None, dx.data_ptr(), 10, C.byref(s), None) == EINVAL
    assert empty(e)
    # an announced batch pending
    q = torch.from_numpy(np.frombuffer(tracegen.store_random(64, seed=1).tobytes(), np.uint8).copy()).cuda()
    q2 = q.clone()
    e.submit_device(q, 64, ahead=(q2, 64, None))
    assert L.dint_load_rows_device(e._h, 0, dk.data_ptr(), None, dx.data_ptr(), 10, C.byref(s), None) == ESTATE and b"announced" in L.dint_last_error()
    assert L.dint_populate_device(e._h, 10, C.byref(s), None) == ESTATE
    e.submit_device(q2, 64)
    e.sync()
    assert empty(e)  # (the batches only read and set)
    e.close()
    # a lock-table engine
    lk = Engine(W.FASST, n_slots=1024)
    assert L.dint_load_rows_device(lk._h, 0, dk.data_ptr(), None, dx.data_ptr(), 10, C.byref(s), None) == ESTATE
    assert L.dint_populate_device(lk._h, 10, C.byref(s), None) == ESTATE
    lk.close()
    # populate_device on an engine that is not blank
    e = Engine(W.STORE, n_rows=16, pool_entries=512)
    load_dev(e, 0, keys[:8], None, vals[:8])
    assert L.dint_populate_device(e._h, 10, C.byref(s), None) == ESTATE and len(e.dump_rows(0)[0]) == 8
    e.reset()
    assert L.dint_populate_device(e._h, 10, C.byref(s), None) == 0 and s.direct == 1 and len(e.dump_rows(0)[0]) == 120
    e.close()
