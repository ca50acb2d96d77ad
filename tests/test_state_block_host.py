"""The block sync's rule without a GPU (dint_amd/csrc/state_block.h through dint_state_block_digest_host / _rows_host / _diff_host,
include/dint_driver.h) against numpy over dumps of hand-built tables: the block of a key is np_bucket // shard count // B, a
block's digest np_digest over the rows of its buckets, the rows the first row of every key in bucket and chain order, the block
diff np_diff (tests/test_state_sync_host.py) over the rows of the listed blocks.  The tables are the verify and compaction tests'
(tests/test_state_verify_host.py, tests/test_state_compact_host.py): chains with the inline entry at the head, in the middle, at the
tail and unlinked, holes, an all-invalid entry, duplicate keys, a sharded table, the smallbank shape.  The dump below walks the raw
bytes by the layout comment of dint_kv_core.h and shares no code with the rule.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from dint_amd import _lib, wire
from test_state_compact_host import _chain, hand_view
from test_state_sync_host import np_bucket, np_diff, np_digest
from test_state_verify_host import SHAPE, keys_of, sound_view

W = wire.Workload
EINVAL = -1
FILL = 0xEE
BS = (64, 256, 1 << 20)
VIEWS = {"hand": lambda: hand_view(1), "hand_smallbank": lambda: hand_view(1, stride=128), "sharded": lambda: sound_view("sharded"),
         "sound": lambda: sound_view("store")}


# ------------------------------------------------------------------------------------------------ numpy over the raw bytes
def dump(view, ti):
    """(keys, vers, vals, local bucket) of table ti's valid chained rows in bucket order, chain order inside a bucket"""
    t, vs = view.tabs[ti], SHAPE[view.workload][2]
    k, v, x, bk = [], [], [], []
    for b in range(t.n_local):
        for e in _chain(t, b):
            for s in range(4):
                if t.entries[e, 48 + s]:
                    k.append(int(t.entries[e, 8 * s:8 * s + 8].view("<u8")[0]))
                    v.append(t.u32(e, 32 + 4 * s))
                    x.append(t.entries[e, 64 + vs * s:64 + vs * (s + 1)].copy())
                    bk.append(b)
    return (np.array(k, "<u8"), np.array(v, "<u4"), np.array(x, np.uint8).reshape(len(k), vs), np.array(bk, np.int64))


def geometry(view, B):
    """first block id of every table, and the number of blocks"""
    per = [-(-t.n_local // B) for t in view.tabs]
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64), per


def np_visible(view, ids, B):
    """the visible rows of the listed blocks as LOG_REC records, in the contract's order"""
    first, _ = geometry(view, B)
    out = []
    for ti in range(len(view.tabs)):
        k, v, x, bk = dump(view, ti)
        vis = np.sort(np.unique(k, return_index=True)[1]) if len(k) else np.zeros(0, np.int64)  # (a key lives in one bucket)
        keep = vis[np.isin(first[ti] + bk[vis] // B, ids)]
        r = np.zeros(len(keep), wire.LOG_REC)
        r["key"], r["ver"], r["table"] = k[keep], v[keep], ti
        r["val"][:, :x.shape[1]] = x[keep]
        out.append(r)
    return np.concatenate(out)


def digest_of(ti, k, ver, x):
    return np_digest(ti, k, ver, x) if len(k) else {"rows": 0, "sum": 0, "xr": 0}  # (np_digest wants a row)


def _one_sided(ti, rows, is_del):
    """np_diff when the other side has no row at all: every visible row of this side, in dump order"""
    k, ver, x = rows
    vis = np.sort(np.unique(k, return_index=True)[1]) if len(k) else np.zeros(0, np.int64)
    r = np.zeros(len(vis), wire.LOG_REC)
    r["key"], r["table"] = k[vis], ti
    if is_del:
        r["is_del"] = 1
    else:
        r["ver"] = ver[vis]
        r["val"][:, :x.shape[1]] = x[vis]
    st = {"total": len(r), "only_a": 0 if is_del else len(r), "only_b": len(r) if is_del else 0, "val_differs": 0, "ver_only": 0}
    return r, st


def np_block_diff(a, b, ids, B):
    """np_diff of the rows of the listed blocks, table after table"""
    first, _ = geometry(a, B)
    recs, stats = [], {"total": 0, "only_a": 0, "only_b": 0, "val_differs": 0, "ver_only": 0}
    for ti, t in enumerate(a.tabs):
        rows = []
        for v in (a, b):
            k, ver, x, bk = dump(v, ti)
            keep = np.isin(first[ti] + bk // B, ids)
            rows.append((k[keep], ver[keep], x[keep]))
        if len(rows[0][0]) and len(rows[1][0]):
            r, st = np_diff(ti, t.hash_size, rows[0], rows[1])
        else:  # (np_diff wants a row on both sides)
            r, st = _one_sided(ti, rows[1], True) if len(rows[1][0]) else _one_sided(ti, rows[0], False)
        recs.append(r)
        stats = {key: stats[key] + st[key] for key in stats}
    return np.concatenate(recs), stats


# ------------------------------------------------------------------------------------------------ the host exports
def host_digest(view, B, cap=None):
    L = _lib.load()
    st = _lib.BlockStats()
    n = L.dint_state_block_digest_host(C.byref(view.c_view()), B, None, 0, C.byref(st))
    if n < 0:
        return n, None, None
    cap = n if cap is None else cap
    out = np.full((max(cap, 1), 4), 0xEEEEEEEEEEEEEEEE, "<u8")
    rc = L.dint_state_block_digest_host(C.byref(view.c_view()), B, out.ctypes.data, cap, C.byref(st))
    return rc, out, st.as_dict()


def host_rows(view, B, ids, cap=None):
    """(rc, the whole output buffer, total)"""
    L = _lib.load()
    ids = np.ascontiguousarray(ids, "<u4")
    st = _lib.BlockStats()
    if cap is None:
        cap = L.dint_state_block_rows_host(C.byref(view.c_view()), B, ids.ctypes.data, len(ids), None, 0, C.byref(st))
        if cap < 0:
            cap = 16
        else:
            cap = st.total
    buf = np.full(max(cap, 1) * 64, FILL, np.uint8)
    rc = L.dint_state_block_rows_host(C.byref(view.c_view()), B, ids.ctypes.data, len(ids), buf.ctypes.data, cap, C.byref(st))
    return rc, buf, st.total


def host_diff(view, B, ids, rows, cap=None):
    """(rc, the whole output buffer, stats)"""
    L = _lib.load()
    ids = np.ascontiguousarray(ids, "<u4")
    rows = np.ascontiguousarray(rows)
    st = _lib.DiffStats()
    cap = 4 * len(rows) + 2000 if cap is None else cap
    buf = np.full(max(cap, 1) * 64, FILL, np.uint8)
    rc = L.dint_state_block_diff_host(C.byref(view.c_view()), B, ids.ctypes.data, len(ids), rows.ctypes.data, len(rows), buf.ctypes.data, cap,
                                      C.byref(st))
    return rc, buf, {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}


def as_records(buf, n):
    return np.frombuffer(buf[:64 * n].tobytes(), wire.LOG_REC)


def behind(view):
    """a copy of `view` that differs from it in every way the diff tells apart, in several blocks of table 0: values, versions, rows
    missing, rows it alone has"""
    b = view.copy()
    t, vs = b.tabs[0], SHAPE[view.workload][2]
    rows = [(e, s) for bk in range(t.n_local) for e in _chain(t, bk) for s in range(4) if t.entries[e, 48 + s]]
    for i, (e, s) in enumerate(rows):
        if i % 7 == 0:
            t.entries[e, 64 + vs * s] ^= 0x55  # value
        elif i % 7 == 1:
            t.set_u32(e, 32 + 4 * s, t.u32(e, 32 + 4 * s) + 9)  # version alone
        elif i % 7 == 2:
            t.entries[e, 48 + s] = 0  # b lacks the row
    free = [bk for bk in range(t.n_local) if t.u32(bk, 56) == 0 and t.u32(bk, 48) == 0][3:60:9]
    assert len(free) >= 3
    for bk in free:  # a row only b has: an empty bucket's inline entry linked, the row in its slot 3
        t.set_u32(bk, 56, 1)
        t.set_u32(bk, 52, 0)
        key = keys_of(t.hash_size, view.shard, bk, 1, 90)[0]
        t.entries[bk, 24:32] = np.frombuffer(np.uint64(key).tobytes(), np.uint8)
        t.entries[bk, 51] = 1
    return b


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_block_digests_are_numpys_and_merge_to_the_table_digest(name, B):
    v = VIEWS[name]()
    first, per = geometry(v, B)
    rc, got, st = host_digest(v, B)
    assert rc == sum(per) == st["n_blocks"] == st["total"] and st["blocks"] == per and st["block_buckets"] == B
    M = (1 << 64) - 1
    for ti in range(len(v.tabs)):
        k, ver, x, bk = dump(v, ti)
        merged = {"rows": 0, "sum": 0, "xr": 0}
        for j in range(per[ti]):  # (a short last block; with B = 2^20 a table smaller than one block)
            m = bk // B == j
            want = digest_of(ti, k[m], ver[m], x[m])
            g = got[first[ti] + j]
            assert (int(g[0]), int(g[1]), int(g[2]), int(g[3])) == (want["rows"], want["sum"], want["xr"], 0), (name, B, ti, j)
            merged = {"rows": merged["rows"] + want["rows"], "sum": (merged["sum"] + want["sum"]) & M, "xr": merged["xr"] ^ want["xr"]}
        assert merged == digest_of(ti, k, ver, x)  # the invariant the device call is held to against dint_state_digest
    if B == 1 << 20:
        assert per == [1] * len(v.tabs)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_every_key_lies_in_the_block_its_hash_gives(name, B):
    v = VIEWS[name]()
    first, per = geometry(v, B)
    seen = 0
    for i in range(sum(per)):
        rc, buf, total = host_rows(v, B, [i])
        assert rc == total
        r = as_records(buf, rc)
        seen += rc
        for ti in np.unique(r["table"]):
            k = r["key"][r["table"] == ti]
            g = np_bucket(k, v.tabs[ti].hash_size).astype(np.int64)
            assert (g % v.shard[1] == v.shard[0]).all()
            assert (first[ti] + g // v.shard[1] // B == i).all()
    assert seen == len(np_visible(v, np.arange(sum(per)), B))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_rows_are_the_visible_rows_in_id_bucket_and_chain_order(name, B):
    v = VIEWS[name]()
    _, per = geometry(v, B)
    n = sum(per)
    for ids in (np.arange(n), np.arange(n)[::2], np.array([n - 1])):
        want = np_visible(v, ids, B)
        rc, buf, total = host_rows(v, B, ids)
        assert rc == total == len(want)
        assert buf[:64 * rc].tobytes() == want.tobytes()
        # count only; a cap shorter than the total gives the first cap of the order and touches nothing behind them
        L = _lib.load()
        st = _lib.BlockStats()
        a = np.ascontiguousarray(ids, "<u4")
        assert L.dint_state_block_rows_host(C.byref(v.c_view()), B, a.ctypes.data, len(a), None, 0, C.byref(st)) == 0 and st.total == len(want)
        if len(want) > 3:
            rc, buf, total = host_rows(v, B, ids, cap=len(want) - 3)
            assert rc == len(want) - 3 and total == len(want) and buf.tobytes() == want[:rc].tobytes()
    if name == "hand":  # the duplicate key of bucket 9: the digest counts both rows, the rows list the first
        k = dump(v, 0)[0]
        assert len(np.unique(k)) < len(k) and len(np_visible(v, np.arange(n), B)) == len(np.unique(k))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("name", list(VIEWS))
def test_block_diff_is_numpys_diff_of_the_listed_blocks(name, B):
    a = VIEWS[name]()
    b = behind(a)
    _, per = geometry(a, B)
    n = sum(per)
    before = b.raw()
    da, db = host_digest(a, B)[1], host_digest(b, B)[1]
    differ = np.nonzero((da[:n] != db[:n]).any(axis=1))[0]
    assert len(differ) >= 1
    for ids in (differ, np.arange(n), differ[:1]):
        rc, buf, _ = host_rows(a, B, ids)
        rows = as_records(buf, rc)
        want, wst = np_block_diff(a, b, ids, B)
        rc, out, st = host_diff(b, B, ids, rows)
        assert rc == len(want) and st == wst, (name, B, st, wst)
        assert out[:64 * rc].tobytes() == want.tobytes()
        assert (out[64 * rc:] == FILL).all()
        if len(want) > 2:  # a short buffer: the first cap records, the full total
            rc, out, st = host_diff(b, B, ids, rows, cap=len(want) - 2)
            assert rc == len(want) - 2 and st["total"] == len(want) and out.tobytes() == want[:rc].tobytes()
    # every block whose VISIBLE rows differ is among the blocks whose digests differ
    full, _ = np_block_diff(a, b, np.arange(n), B)
    sel, _ = np_block_diff(a, b, differ, B)
    assert full.tobytes() == sel.tobytes()
    assert b.raw() == before  # nothing is modified
    # equal tables: nothing to do
    rc, buf, _ = host_rows(a, B, np.arange(n))
    rc, out, st = host_diff(a, B, np.arange(n), as_records(buf, rc))
    assert rc == 0 and st["total"] == 0 and (out == FILL).all()


def test_a_key_listed_twice_in_a_run_the_first_wins():
    a = VIEWS["hand"]()
    b = behind(a)
    ids = np.arange(5)
    rc, buf, _ = host_rows(a, 64, ids)
    rows = as_records(buf, rc)
    want = host_diff(b, 64, ids, rows)
    i = len(rows) // 2
    twin = rows[i:i + 1].copy()
    twin["val"][0, 0] ^= 0xFF
    twin["ver"] += 5
    doubled = np.concatenate([rows[:i + 1], twin, rows[i + 1:]])
    got = host_diff(b, 64, ids, doubled)
    assert got[0] == want[0] and got[2] == want[2] and got[1][:64 * got[0]].tobytes() == want[1][:64 * want[0]].tobytes()


def test_refusals_leave_the_output_as_it_was():
    L = _lib.load()
    a = VIEWS["hand"]()
    b = behind(a)
    before = b.raw()
    ids = np.arange(5)
    rc, buf, _ = host_rows(a, 64, ids)
    rows = as_records(buf, rc)
    assert rc > 40

    def refused_diff(B, ids, rows, what):
        rc, out, _ = host_diff(b, B, ids, rows)
        assert rc == EINVAL and (out == FILL).all(), what
        assert b.raw() == before

    refused_diff(64, ids, rows[::-1].copy(), "rows out of order")
    swapped = rows.copy()
    swapped[[3, 30]] = swapped[[30, 3]]
    refused_diff(64, ids, swapped, "two rows swapped")
    refused_diff(64, ids[1:], rows, "a row home to an unlisted block")
    t7 = rows.copy()
    t7["table"][5] = 7
    refused_diff(64, ids, t7, "table 7")
    t1 = rows.copy()
    t1["table"][5] = 1  # (the store has one table)
    refused_diff(64, ids, t1, "table 1 of 1")
    dl = rows.copy()
    dl["is_del"][0] = 1
    refused_diff(64, ids, dl, "a delete record")
    alien = rows.copy()
    alien["key"][7] ^= np.uint64(0x5A5A5A)
    refused_diff(64, ids[:1], alien[:12], "a key that is home to another bucket")
    for bad_ids, what in ((ids[::-1].copy(), "descending"), (np.array([0, 1, 1, 2]), "duplicate"), (np.array([0, 5]), "out of range"),
                          (np.array([0xFFFFFFFF]), "out of range")):
        refused_diff(64, bad_ids, rows, what)
        rc, out, _ = host_rows(a, 64, bad_ids, cap=400)
        assert rc == EINVAL and (out == FILL).all(), what
    for B in (96, 32, 0, 1 << 21, 63):
        refused_diff(B, ids, rows, B)
        rc, out, _ = host_rows(a, B, ids, cap=400)
        assert rc == EINVAL and (out == FILL).all()
        assert host_digest(a, B)[0] == EINVAL
    # the digest: room for fewer blocks than there are
    rc, out, _ = host_digest(a, 64, cap=4)
    assert rc == EINVAL and (out == 0xEEEEEEEEEEEEEEEE).all()
    # a sharded table: a row of another shard
    s = VIEWS["sharded"]()
    rc, buf, _ = host_rows(s, 64, np.arange(5))
    srows = as_records(buf, rc).copy()
    foreign = keys_of(899, (2, 3), 0, 1)[0]
    srows["key"][0] = foreign
    rc, out, _ = host_diff(s, 64, np.arange(5), srows)
    assert rc == EINVAL and (out == FILL).all()
    # null arguments and a view that fails the check
    assert L.dint_state_block_digest_host(None, 64, None, 0, None) == EINVAL
    assert L.dint_state_block_rows_host(C.byref(a.c_view()), 64, None, 3, None, 0, None) == EINVAL
    assert L.dint_state_block_diff_host(C.byref(a.c_view()), 64, ids.astype("<u4").ctypes.data, 5, None, 3, None, 0, None) == EINVAL
    cv = a.c_view()
    cv.table[0].stride = 128
    assert L.dint_state_block_digest_host(C.byref(cv), 64, None, 0, None) == EINVAL


def test_struct_layout_and_symbols():
    assert C.sizeof(_lib.BlockDigest) == 32 and C.sizeof(_lib.BlockStats) == 64
    L = _lib.load()
    for name in ("dint_state_block_digest", "dint_state_block_select", "dint_state_block_rows", "dint_state_block_diff"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    # the device calls check their arguments before they touch a device
    assert L.dint_state_block_digest(None, 64, None, 0, None, None) == EINVAL
    assert L.dint_state_block_rows(None, 64, None, 0, None, 0, None, None) == EINVAL
    assert L.dint_state_block_diff(None, 64, None, 0, None, 0, None, 0, None, None) == EINVAL
    assert L.dint_state_block_select(None, None, 0, None, 0, None) == 0
    assert L.dint_state_block_select(None, None, 5, None, 0, None) == EINVAL
