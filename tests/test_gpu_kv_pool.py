"""The store and tatp tables at the edge of their overflow pool (dint_config.pool_entries): passes that start with head-room
and end with none, exact fits, tatp's REJECT_COMMIT and its untouched lock byte, the device path.  Every case runs the
filtered-replay check of tests/kvkeys.py in full: the oracle's replay of the trace without the refused INSERTs gives every other
reply, the rows and the lock words; the refusals are counted, reported and complete ("the refusal is
never silent").

The shapes: every bucket of the table holds four rows (its inline entry is full, the pool untouched), then ONE fresh key per
bucket is inserted -- every inserting run is one key in its bucket and needs exactly one pool entry, no refusal changes a later
request, so the number refused is exactly max(0, buckets - pool_entries) whatever order the workgroups reach the allocator in."""
import functools

import numpy as np
import pytest

import kvkeys
from dint_amd import _lib, wire
from kvkeys import ENOMEM, Trace, check_filtered_replay, keys_by_bucket
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W, S, T = wire.Workload, wire.Store, wire.Tatp
ROUNDS = _lib.FLAG_KV_ROUNDS

STORE_ROWS = 14_564  # 65,538 buckets (n_rows * 18 / 4): ~17 MB of inline entries
STORE_HS = STORE_ROWS * 18 // 4
STORE_POOLS = [4096, 4097, 8192, 20_000, 65_537, 65_538, 70_000]  # 4096: always "low" (the control); 65,538: the exact fit


def _engine(*a, **k):
    from dint_amd.engine import Engine

    return Engine(*a, **k)


def _msgs(dtype, types, keys, seed, table=None):
    rng = np.random.default_rng(seed)
    m = np.zeros(len(keys), dtype)
    m["type"], m["key"] = types, keys
    m["val"] = rng.integers(0, 256, (len(keys), 40), dtype=np.uint8)
    m["ver"] = rng.integers(0, 2**32, len(keys), dtype=np.uint64).astype("<u4")
    if table is not None:
        m["table"] = table
        m["ord"] = rng.integers(0, 256, len(keys))
    return m


# ---------------------------------------------------------------------------------------------------------------- store
@functools.lru_cache(maxsize=None)
def _store_shape():
    """{fill: four INSERTs per bucket, ins: one INSERT of a fresh key per bucket, rd: READs of the fresh keys}, shuffled"""
    assert STORE_HS == 65_538
    rng = np.random.default_rng(7)
    k = keys_by_bucket(STORE_HS, 5, seed=3).reshape(STORE_HS, 5)
    fill, fresh = k[:, :4].ravel(), k[:, 4].copy()
    fill = fill[rng.permutation(len(fill))]
    out = {"fill_keys": fill, "fresh": fresh,
           "fill": _msgs(wire.STORE_MSG, S.INSERT, fill, 11),
           "ins": _msgs(wire.STORE_MSG, S.INSERT, fresh[rng.permutation(STORE_HS)], 12),
           "rd": _msgs(wire.STORE_MSG, S.READ, fresh[rng.permutation(STORE_HS)], 13)}
    for v in out.values():
        v.setflags(write=False)
    return out


def _store_filled(pool, flags):
    sh = _store_shape()
    e = _engine(W.STORE, n_rows=STORE_ROWS, pool_entries=pool, flags=flags)
    assert e.hash_size(0) == STORE_HS
    tr = Trace(e)
    rc, rep = tr.submit(sh["fill"])
    assert rc == 0 and (rep["type"] == S.INSERT_ACK).all()
    (v,) = e.state_verify()
    assert v["pool_top"] == 0 and v["rows"] == 4 * STORE_HS  # the inline entries are full, the pool is untouched
    return e, tr, sh


def _store_ends(e, tr, sh, pool, R):
    n_ref = max(0, STORE_HS - pool)
    assert int(R.sum()) == n_ref
    (v,) = e.state_verify()
    assert v["pool_top"] == min(STORE_HS, pool) == v["linked"] and v["rows"] == 5 * STORE_HS - n_ref
    e.close()


@pytest.mark.parametrize("flags", [0, ROUNDS], ids=["closed", "rounds"])
@pytest.mark.parametrize("pool", STORE_POOLS)
def test_store_one_pass_across_the_margin(pool, flags):
    """a. ONE pass of 65,538 INSERTs, one fresh key per full bucket, then one pass of READs of all of them"""
    e, tr, sh = _store_filled(pool, flags)
    tr.submit(sh["ins"])
    tr.submit(sh["rd"])
    R = check_filtered_replay(tr, orc.StoreOracle(STORE_HS, 0), harmless=sh["rd"][:10])
    _store_ends(e, tr, sh, pool, R)


@functools.lru_cache(maxsize=None)
def _store_mixed():
    """the INSERTs of case a, the READs of the fresh keys and READ / SET noise on the loaded keys (p_set 0.3: plain closed-form
    segments beside the inserting ones), shuffled into one trace whose length 4 and 16 divide"""
    sh = _store_shape()
    rng = np.random.default_rng(21)
    n_noise = STORE_HS + (-3 * STORE_HS) % 16
    nk = sh["fill_keys"][rng.integers(0, len(sh["fill_keys"]), n_noise)]
    noise = _msgs(wire.STORE_MSG, np.where(rng.random(n_noise) < 0.3, S.SET, S.READ), nk, 22)
    m = np.concatenate([sh["ins"], sh["rd"], noise])
    m = m[rng.permutation(len(m))]
    assert len(m) % 16 == 0
    m.setflags(write=False)
    return m


@pytest.mark.parametrize("flags", [0, ROUNDS], ids=["closed", "rounds"])
@pytest.mark.parametrize("passes", [4, 16])
@pytest.mark.parametrize("pool", STORE_POOLS)
def test_store_crossing_inside_mixed_passes(pool, passes, flags):
    """b. the same INSERTs in 4 and in 16 passes of equal size with READs of the fresh keys and READ / SET noise mixed in: the
    crossing falls inside a pass that also carries plain closed-form segments"""
    e, tr, sh = _store_filled(pool, flags)
    m = _store_mixed()
    n = len(m) // passes
    for p in range(passes):
        tr.submit(m[p * n:(p + 1) * n])
    R = check_filtered_replay(tr, orc.StoreOracle(STORE_HS, 0), harmless=sh["rd"][:10])
    _store_ends(e, tr, sh, pool, R)


# ---------------------------------------------------------------------------------------------------------------- the device path
def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


@pytest.mark.parametrize("ahead", [False, True], ids=["plain", "ahead"])
def test_store_device_path_across_the_margin(ahead):
    """f. case a with 20,000 pool entries through submit_device, and with the next batch announced (its partition runs beside
    this batch's hot keys): same check; DINT_ENOMEM comes from the sync behind the batch that held the refused INSERTs"""
    pool = 20_000
    e, tr, sh = _store_filled(pool, 0)
    half = STORE_HS // 2
    parts = [sh["ins"][:half], sh["ins"][half:], sh["rd"]]
    d = [_up(p) for p in parts]
    for k, p in enumerate(parts):
        nxt = (d[k + 1], len(parts[k + 1]), None) if ahead and k + 1 < len(parts) else None
        e.submit_device(d[k], len(p), None, 0, ahead=nxt)
    rc = e._L.dint_sync(e._h)
    for k, p in enumerate(parts):
        tr.add(p, np.frombuffer(d[k].cpu().numpy().tobytes(), wire.STORE_MSG), None)
    n_ref = int(kvkeys.refused_mask(W.STORE, np.concatenate(parts), np.concatenate(tr.rep[-3:])).sum())
    assert rc == (ENOMEM if n_ref else 0) and e._L.dint_sync(e._h) == 0  # reported once
    R = check_filtered_replay(tr, orc.StoreOracle(STORE_HS, 0), harmless=sh["rd"][:10])
    _store_ends(e, tr, sh, pool, R)


# ---------------------------------------------------------------------------------------------------------------- tatp
@functools.lru_cache(maxsize=None)
def _tatp_shape():
    """CALL_FORWARDING (table 4) at the smallest n_rows whose table-4 hash size is >= 16,384; the passes of case c"""
    n_rows = next(n for n in range(11_000, 13_000) if n * 45 // 8 // 4 >= 16_384)
    o = orc.TatpOracle(n_rows, log_entries=1 << 12, populate_n=0)
    hs = o.hash_size(4)
    assert hs >= 16_384 and orc.TatpOracle(n_rows - 1, log_entries=1 << 12, populate_n=0).hash_size(4) < 16_384
    rng = np.random.default_rng(5)
    k = keys_by_bucket(hs, 5, seed=9, key_of=kvkeys.cf_key_of).reshape(hs, 5)
    fill, fresh = k[:, :4].ravel(), k[:, 4].copy()
    fresh = fresh[rng.permutation(hs)]
    prim, bck = fresh[:hs // 2], fresh[hs // 2:]  # one fresh key per bucket: no two of them share a lock byte
    ins = np.concatenate([_msgs(wire.TATP_MSG, T.INSERT_PRIM, prim, 31, 4), _msgs(wire.TATP_MSG, T.INSERT_BCK, bck, 32, 4)])
    after = np.concatenate([_msgs(wire.TATP_MSG, T.ACQUIRE_LOCK, prim, 33, 4), _msgs(wire.TATP_MSG, T.READ, fresh, 34, 4)])
    out = {"n_rows": n_rows, "hs": hs, "prim": prim,
           "fill": _msgs(wire.TATP_MSG, T.INSERT_BCK, fill[rng.permutation(len(fill))], 35, 4),
           "lock": _msgs(wire.TATP_MSG, T.ACQUIRE_LOCK, prim[rng.permutation(len(prim))], 36, 4),
           "ins": ins[rng.permutation(len(ins))], "after": after[rng.permutation(len(after))]}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("flags", [0, ROUNDS], ids=["closed", "rounds"])
@pytest.mark.parametrize("pool", ["4097", "half", "buckets-1", "buckets"])
def test_tatp_call_forwarding_across_the_margin(pool, flags):
    """c. every bucket of CALL_FORWARDING full, then one pass of INSERT_PRIM / INSERT_BCK (half each) of one fresh key per
    bucket.  Every INSERT_PRIM's key was locked by an ACQUIRE_LOCK of an earlier pass and is asked for again in a later one:
    REJECT_LOCK exactly when the insert was refused -- a refused INSERT_PRIM must not have released the lock."""
    sh = _tatp_shape()
    hs = sh["hs"]
    pool = {"4097": 4097, "half": hs // 2, "buckets-1": hs - 1, "buckets": hs}[pool]
    e = _engine(W.TATP, n_rows=sh["n_rows"], log_entries=1 << 12, pool_entries=pool, flags=flags)
    assert e.hash_size(4) == hs
    tr = Trace(e)
    rc, rep = tr.submit(sh["fill"])
    assert rc == 0 and (rep["type"] == T.INSERT_BCK_ACK).all() and e.state_verify()[4]["pool_top"] == 0
    rc, rep = tr.submit(sh["lock"])
    assert rc == 0 and (rep["type"] == T.GRANT_LOCK).all()
    rc, rep = tr.submit(sh["ins"])
    refused = sh["ins"]["key"][rep["type"] == T.REJECT_COMMIT]
    rc, rep = tr.submit(sh["after"])
    acq = sh["after"]["type"] == T.ACQUIRE_LOCK
    again = np.isin(sh["after"]["key"][acq], refused)
    assert ((rep["type"][acq] == T.REJECT_LOCK) == again).all() and (rep["type"][acq][~again] == T.GRANT_LOCK).all()
    R = check_filtered_replay(tr, orc.TatpOracle(sh["n_rows"], log_entries=1 << 12, populate_n=0), harmless=sh["after"][~acq][:10])
    n_ref = max(0, hs - pool)
    assert int(R.sum()) == n_ref and (np.concatenate(tr.req)["table"][R] == 4).all()
    v = e.state_verify()
    assert v[4]["pool_top"] == min(hs, pool) == v[4]["linked"] and all(v[t]["pool_top"] == 0 for t in range(4))
    e.close()


# ---------------------------------------------------------------------------------------------------------------- the hot-row paths
from test_gpu_kv import SPLIT_KNOBS, _hot_tatp  # noqa: E402

HOT_KNOBS = [SPLIT_KNOBS[0], SPLIT_KNOBS[2], SPLIT_KNOBS[4], SPLIT_KNOBS[5]]
HOT_IDS = ["t16", "default", "late_big", "nofuse"]
HOT_CF = (4, 7 | (1 << 32))


def _need(keys, hs):
    return kvkeys.overflow_need(np.bincount(kvkeys.np_bucket(keys, hs).astype(np.int64), minlength=hs))


def _hot_pools(needs, hot_rows, cross_after):
    """the two pool sizes of a hot-row case from the UNBOUNDED oracle's table after each pass: {issue: 4096 + the entries the
    hot bucket links after the third pass -- at these table sizes no INSERT is refused with it: the control, every closed form
    taken with the pool never low; crossing: what the table links after pass `cross_after` -- the pool is used up while
    the later passes pile duplicate rows onto the hot bucket.  With that size pool_top + a pass's INSERTs exceeds the pool from
    the first pass (pieces) or the second (dominant, store) on, so the inserting runs of the hot bucket go request by request
    and the refusals happen there; the inserting closed forms of the pieces and of the bucket-group path run with the first
    size}.  The crossing is real:
    the unbounded table ends with more entries than that pool has, so an engine that refused nothing cannot hold it."""
    third = min(2, len(hot_rows) - 1)
    pools = {"issue": 4096 + max(-(-hot_rows[third] // 4) - 1, 0), "crossing": needs[cross_after]}
    assert needs[-1] > pools["crossing"] > 0 and -(-hot_rows[-1] // 4) < 1000  # (KV_MAX_CHAIN is 4096)
    return pools


@functools.lru_cache(maxsize=None)
def _tatp_hot(p_hot, sizes, cross_after):
    n_sub = 3000
    o = orc.TatpOracle(n_sub, log_entries=400_000)
    existing = [o.dump(t)[0] for t in range(5)]
    hs = o.hash_size(4)
    hb = int(kvkeys.np_bucket(np.array([HOT_CF[1]], np.uint64), hs)[0])
    mix = {0: 85, 1: 10, 2: 2, 18: 6, 22: 2}  # INSERT_PRIM of the hot row three times as often as DELETE_PRIM: duplicate rows pile up
    passes = [_hot_tatp(n, p_hot, mix, seed=17 * k + 5, hot_key=HOT_CF, existing=existing, n_noise_sub=n_sub) for k, n in enumerate(sizes)]
    needs, hot_rows = [], []
    for p in passes:
        o.replay(p)
        keys = o.dump(4)[0]
        needs.append(_need(keys, hs))
        hot_rows.append(int((kvkeys.np_bucket(keys, hs).astype(np.int64) == hb).sum()))
    return n_sub, passes, _hot_pools(needs, hot_rows, cross_after)


@pytest.mark.parametrize("knobs", HOT_KNOBS, ids=HOT_IDS)
@pytest.mark.parametrize("pool", ["issue", "crossing"])
@pytest.mark.parametrize("p_hot,sizes,cross_after", [(0.5, (900, 3000, 500, 6000, 9000, 250, 2500, 14_000, 600), 2),
                                                    (0.3, (6000, 40_000, 150_000), 1)], ids=["pieces", "dominant"])
def test_tatp_hot_row_piles_up_duplicates_across_the_margin(p_hot, sizes, cross_after, pool, knobs, monkeypatch):
    """e. the hot CALL_FORWARDING row inserted (also when it exists: duplicate rows) and deleted, as in
    test_tatp_hot_key_in_pieces / test_tatp_dominant_key_vs_oracle, with a pool that runs out on the way"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    n_sub, passes, pools = _tatp_hot(p_hot, sizes, cross_after)
    e = _engine(W.TATP, n_rows=n_sub, log_entries=400_000, pool_entries=pools[pool])
    e.populate(n_sub)
    assert e.stats()["pool_exhausted"] == 0
    tr = Trace(e)
    for p in passes:
        tr.submit(p)
    rd = passes[0][:10].copy()
    rd["type"] = T.READ
    R = check_filtered_replay(tr, orc.TatpOracle(n_sub, log_entries=400_000), harmless=rd)
    assert e.stats()["big_bin_requests"] > 0 and (pool != "crossing" or R.sum() > 0)
    e.close()


@functools.lru_cache(maxsize=None)
def _store_hot():
    import tracegen

    n_sub = 5000
    hs = n_sub * 18 // 4
    o = orc.StoreOracle(hs, n_sub)
    rng = np.random.default_rng(4)
    passes, needs, hot_rows = [], [], []
    for n, key in ((1500, tracegen.store_key(11, 2, 8)), (5000, tracegen.store_key(11, 2, 8)), (8000, tracegen.store_key(4999, 4, 16)),
                   (6000, tracegen.store_key(77_777, 1, 0))):  # the last one is not in the table
        req = tracegen.store_random(n, seed=n, n_sub_touch=n_sub, p_set=0.3, p_missing=0.05, p_insert=0.05)
        hot = rng.random(n) < 0.7
        req["key"][hot] = key
        req["type"][hot & (rng.random(n) < 0.1)] = S.INSERT  # INSERTs of the hot key: duplicate rows when it exists
        passes.append(req)
        o.replay(req)
        keys = o.dump()[0]
        needs.append(_need(keys, hs))
        hb = int(kvkeys.np_bucket(np.array([key], np.uint64), hs)[0])
        hot_rows.append(int((kvkeys.np_bucket(keys, hs).astype(np.int64) == hb).sum()))
    return n_sub, passes, _hot_pools(needs, hot_rows, 2)


@pytest.mark.parametrize("knobs", HOT_KNOBS, ids=HOT_IDS)
@pytest.mark.parametrize("pool", ["issue", "crossing"])
def test_store_hot_key_inserted_across_the_margin(pool, knobs, monkeypatch):
    """e. test_store_hot_key_in_pieces with INSERTs of the hot key and of fresh keys, with a pool that runs out on the way"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    n_sub, passes, pools = _store_hot()
    e = _engine(W.STORE, n_rows=n_sub, pool_entries=pools[pool])
    e.populate(n_sub)
    assert e.stats()["pool_exhausted"] == 0
    tr = Trace(e)
    for p in passes:
        tr.submit(p)
    rd = passes[0][:10].copy()
    rd["type"] = S.READ
    R = check_filtered_replay(tr, orc.StoreOracle(n_sub * 18 // 4, n_sub), harmless=rd)
    assert e.stats()["big_bin_requests"] > 0 and (pool != "crossing" or R.sum() > 0)
    e.close()


# ---------------------------------------------------------------------------------------------------------------- churn
@functools.lru_cache(maxsize=None)
def _churn(wl, kind):
    passes = kvkeys.churn_trace(wl, kind)
    return passes, kvkeys.churn_pool(wl, passes, kind)


@pytest.mark.parametrize("flags", [0, ROUNDS], ids=["closed", "rounds"])
@pytest.mark.parametrize("kind", ["issue", "crossing"])
@pytest.mark.parametrize("wl", [W.STORE, W.TATP], ids=["store", "tatp"])
def test_churn_at_a_pool_that_is_too_small(wl, kind, flags):
    """d. 240,000 requests over a populated server whose pool is too small: inserts are refused while tatp's deletes free
    entries, which become poppable two passes later and are handed out again.  Two pool sizes (kvkeys.churn_pool): "issue", half
    of what the unbounded oracle's fullest table links after four of 12 passes -- with it every inserting run of every pass
    goes request by request; "crossing", with which the first passes take their closed forms, then kv_pool_low turns true
    beside freed, pending and recycled entries -- which it ignores: that may only send more runs request by request, never
    acknowledge an INSERT that fails --, then the pool runs out.  tests/test_kv_core_host.py shows on the host build that
    both sizes refuse some INSERTs and fewer than half, and that the second really crosses."""
    passes, pool = _churn(wl, kind)
    n = kvkeys.CHURN_SUBS[wl]
    kw = {} if wl == W.STORE else {"log_entries": 1 << 16}
    e = _engine(wl, n_rows=n, pool_entries=pool, flags=flags, **kw)
    e.populate(n)
    assert e.stats()["pool_exhausted"] == 0
    tr = Trace(e)
    for p in passes:
        tr.submit(p)
    rd = passes[0][:10].copy()
    rd["type"] = 0  # READ
    R = check_filtered_replay(tr, kvkeys.churn_oracle(wl), harmless=rd)
    n_ins = int(np.isin(np.concatenate(tr.req)["type"], kvkeys.INSERT_TYPES[wl]).sum())
    assert 0 < R.sum() < n_ins // 2, (pool, n_ins, int(R.sum()))
    if kind == "crossing":  # pass 0 had head-room for every INSERT it holds: none of them is refused
        assert not R[:len(passes[0])].any()
    e.close()
