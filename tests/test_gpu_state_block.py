"""Replicas compared block by block on the GPU (include/dint_abi.h dint_state_block_digest / _select / _rows / _diff,
dint_amd/csrc/k_block.hip, dint_amd/recovery.py resync_blocks) against forms that share no code with them: per block np_digest
(tests/test_state_sync_host.py) over the engine's dump_rows cut by np_bucket // B, the visible rows by first occurrence in dump
order, the block diff held byte for byte to dint_state_diff of the same two engines, and the host form of the same rule
(dint_state_block_digest_host) over a view rebuilt from the dump.  Shapes: tatp of 300 subscribers (112 / 112 / 281 / 281 / 421
buckets: with B = 64 every table's last block is short, with B = 256 single short blocks stand beside two-block tables, with
B = 2^20 a block is a table), smallbank and store of 1,000, two tatp shards of 20,000.  Chains of three entries in the last
bucket of one block and the first of the next, a hole, a key held twice.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from dint_amd import _lib, recovery, wire
from kvkeys import keys_by_bucket
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes
from test_gpu_log_replay import _dev, _tatp
from test_state_sync_host import np_bucket, np_digest
from test_state_verify_host import Tab, View

W, T = wire.Workload, wire.Tatp
EINVAL, ESTATE = -1, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
BS = (64, 256, 1 << 20)
M64 = (1 << 64) - 1
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


# ------------------------------------------------------------------------------------------------ numpy
def _geom(e, B):
    n_local = [-(-e.hash_size(t) // e.shard_count) for t in range(NTAB[e.workload])]
    per = [-(-n // B) for n in n_local]
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64), per


def _dump_blocks(e, t, B, first):
    k, v, x = e.dump_rows(t)
    local = np_bucket(k, e.hash_size(t)).astype(np.int64) // e.shard_count
    return k, v, x, first[t] + local // B


def _np_block_digests(e, B):
    first, per = _geom(e, B)
    out = np.zeros((sum(per), 4), "<u8")
    for t in range(NTAB[e.workload]):
        k, v, x, blk = _dump_blocks(e, t, B, first)
        for i in np.unique(blk):
            d = np_digest(t, k[blk == i], v[blk == i], x[blk == i])
            out[i, :3] = d["rows"], d["sum"], d["xr"]
    return out


def _np_rows(e, B, ids):
    """the visible rows of the listed blocks, in the contract's order (dump_rows: bucket order, chain order inside a bucket)"""
    first, _ = _geom(e, B)
    out = []
    for t in range(NTAB[e.workload]):
        k, v, x, blk = _dump_blocks(e, t, B, first)
        vis = np.sort(np.unique(k, return_index=True)[1]) if len(k) else np.zeros(0, np.int64)
        keep = vis[np.isin(blk[vis], ids)]
        r = np.zeros(len(keep), wire.LOG_REC)
        r["key"], r["ver"], r["table"] = k[keep], v[keep], t
        r["val"][:, :x.shape[1]] = x[keep]
        out.append(r)
    return np.concatenate(out)


def _merge(d, lo, hi):
    rows = sum(int(r) for r in d[lo:hi, 0])
    s = sum(int(r) for r in d[lo:hi, 1]) & M64
    x = 0
    for r in d[lo:hi, 2]:
        x ^= int(r)
    return {"rows": rows, "sum": s, "xr": x}


def _view_of(e):
    """a host view that holds the engine's rows bucket by bucket in its chain order: the inline entry, then overflow entries"""
    tabs = []
    for t in range(NTAB[e.workload]):
        hs = e.hash_size(t)
        k, v, x = e.dump_rows(t)
        g = np_bucket(k, hs).astype(np.int64)
        need = int(np.maximum(-(-np.bincount(g, minlength=hs) // 4) - 1, 0).sum())
        tab = Tab(hs, hs, max(need, 1), 256 if e.val_size == 40 else 128)
        pool = 0
        for b in np.unique(g):
            idx = np.nonzero(g == b)[0]
            seq = ["I"] + list(range(pool, pool + (len(idx) + 3) // 4 - 1))
            pool += len(seq) - 1
            tab.chain(int(b), seq)
            for j, i in enumerate(idx):
                row, s = (int(b) if j < 4 else tab.pool(seq[j // 4])), j % 4
                tab.entries[row, 8 * s:8 * s + 8] = np.frombuffer(k[i].tobytes(), np.uint8)
                tab.set_u32(row, 32 + 4 * s, int(v[i]))
                tab.entries[row, 48 + s] = 1
                tab.entries[row, 64 + e.val_size * s:64 + e.val_size * (s + 1)] = x[i]
        tab.top = pool
        tabs.append(tab)
    return View(e.workload, tabs)


# ------------------------------------------------------------------------------------------------ the device calls
def _digests(e, B):
    d, n, st = e.state_block_digest(B)
    return d[:n].cpu().numpy().view("<u8").reshape(n, 4), st


def _ids(ids):
    import torch

    return torch.from_numpy(np.ascontiguousarray(ids, "<i4").copy()).cuda() if len(ids) else torch.zeros(1, dtype=torch.int32, device="cuda")


def _rows(e, B, ids, cap=None, shift=0):
    """state_block_rows into a 0xEE-filled buffer, `shift` bytes into it: (n, total, records, the whole buffer as bytes)"""
    import torch

    if cap is None:
        cap = e.state_block_rows(B, _ids(ids), len(ids))[1]
    buf = torch.full((shift + (cap + 2) * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    n, total = e.state_block_rows(B, _ids(ids), len(ids), buf[shift:], cap)
    raw = buf.cpu().numpy()
    return n, total, np.frombuffer(raw[shift:shift + 64 * n].tobytes(), wire.LOG_REC), raw


def _block_diff(e, B, ids, rows, cap=None, shift=0):
    import torch

    d_rows = torch.cat([torch.zeros(shift, dtype=torch.uint8, device="cuda"), _dev(rows)]) if len(rows) else torch.zeros(shift + 64, dtype=torch.uint8, device="cuda")
    cap = 2 * len(rows) + 4096 if cap is None else cap
    buf = torch.full((shift + (cap + 2) * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    n, st = e.state_block_diff(B, _ids(ids), len(ids), d_rows[shift:], len(rows), buf[shift:], cap)
    raw = buf.cpu().numpy()
    return n, st, np.frombuffer(raw[shift:shift + 64 * n].tobytes(), wire.LOG_REC), buf


def _copy_of(e):
    """a blank engine of e's shape filled with e's image: chains, holes and duplicates included"""
    c = _engine(e.workload, n_rows=300, log_entries=4096)
    buf, n, _ = e.state_export()
    c.state_import(buf, n)
    return c


def _image(e):
    buf, n, _ = e.state_export()
    return buf[:n].cpu().numpy().tobytes()


def _select(a, b, B):
    da, n, _ = a.state_block_digest(B)
    db, n2, _ = b.state_block_digest(B)
    assert n == n2
    ids, nd = b.state_block_select(da, db, n)
    return ids[:nd].cpu().numpy().astype(np.int64), nd


def _with_chains(e, table=4):
    """rows loaded into the LAST bucket of block 0 and the FIRST of block 1 (B = 64) of `table`: three entries each; then a hole
    in the first chain and a key held twice in the second"""
    hs = e.hash_size(table)
    per = np.zeros(hs, np.int64)
    per[63], per[64] = 10, 9
    keys = keys_by_bucket(hs, per, seed=9)
    vals = (np.arange(len(keys))[:, None] + np.arange(40)[None, :]).astype(np.uint8)
    e.load_rows(table, keys, np.arange(100, 100 + len(keys), dtype="<u4"), vals)
    m = np.zeros(1, wire.TATP_MSG)
    m["type"], m["table"], m["key"] = T.DELETE_PRIM, table, keys[5]
    e.submit(m)
    assert keys[5] not in e.dump_rows(table)[0]  # a hole in the chain of bucket 63
    e.load_rows(table, keys[12:13], np.array([7], "<u4"), vals[:1] + 1)  # a second row of a key of bucket 64: shadowed
    return keys


@pytest.fixture(scope="module")
def prim():
    e = _tatp()
    _with_chains(e)
    return e


class Carry:
    """moves a tensor "to the other device" -- a clone on this one -- and counts the bytes"""

    def __init__(self):
        self.bytes, self.calls = 0, 0

    def __call__(self, t):
        self.bytes += t.numel() * t.element_size()
        self.calls += 1
        return t.clone()


# ---------------------------------------------------------------------------------------------- 1. digests
@pytest.mark.parametrize("B", BS)
def test_block_digests_device_host_form_and_numpy(prim, B):
    got, st = _digests(prim, B)
    want = _np_block_digests(prim, B)
    first, per = _geom(prim, B)
    assert st["blocks"] == per == {64: [2, 2, 5, 5, 7], 256: [1, 1, 2, 2, 2], 1 << 20: [1] * 5}[B] and st["n_blocks"] == sum(per)
    assert got.tobytes() == want.tobytes(), np.nonzero((got != want).any(axis=1))[0]
    v = _view_of(prim)
    host = np.zeros((sum(per), 4), "<u8")
    assert _lib.load().dint_state_block_digest_host(C.byref(v.c_view()), B, host.ctypes.data, sum(per), None) == sum(per)
    assert host.tobytes() == got.tobytes()
    table = prim.state_digest()
    for t in range(5):
        assert _merge(got, first[t], first[t + 1]) == table[t], t
    if B == 64:  # the overflow rows land in the right block: bucket 63 closes block 0 of table 4, bucket 64 opens block 1
        assert got[first[4], 0] >= 9 and got[first[4] + 1, 0] >= 10
        k, _, _, blk = _dump_blocks(prim, 4, 64, first)
        local = np_bucket(k, prim.hash_size(4)).astype(np.int64)
        assert (local == 63).sum() >= 9 and (local == 64).sum() >= 10 and (local == 64).sum() - len(np.unique(k[local == 64])) == 1
    # count only
    s = _lib.BlockStats()
    assert prim._L.dint_state_block_digest(prim._h, B, None, 0, C.byref(s), None) == sum(per) and list(s.blocks) == per


@pytest.mark.parametrize("wl", ["smallbank", "store"])
def test_block_digests_smallbank_and_store(wl):
    import tracegen

    if wl == "smallbank":
        e = _engine(W.SMALLBANK, n_rows=1000, log_entries=70_000)
        e.populate(500)
        e.submit(tracegen.sb_random(20_000, seed=3, n_acct_touch=40))
        assert e.hash_size(0) == 375
    else:
        e = _engine(W.STORE, n_rows=1000)
        e.populate(60)
        e.submit(tracegen.store_random(30_000, seed=77, n_sub_touch=30, p_set=0.5, p_insert=0.05))
        assert e.hash_size(0) == 4500
    table = e.state_digest()
    for B in (64, 256, 1 << 20):
        got, st = _digests(e, B)
        first, per = _geom(e, B)
        assert st["blocks"] == per and got.tobytes() == _np_block_digests(e, B).tobytes(), B
        for t in range(NTAB[e.workload]):
            assert _merge(got, first[t], first[t + 1]) == table[t]
    n = sum(_geom(e, 256)[1])
    ids = np.arange(n)[1::2]
    want = _np_rows(e, 256, ids)
    got_n, total, rec, _ = _rows(e, 256, ids)
    assert got_n == total == len(want) > 0 and rec.tobytes() == want.tobytes()


def test_two_shards_each_against_its_twin():
    n = 20_000
    for i in range(2):
        a, b = (_engine(W.TATP, n_rows=n, shard_index=i, shard_count=2) for _ in range(2))
        a.populate(n); b.populate(n)
        for B in (256, 1 << 20):
            got, _ = _digests(a, B)
            first, per = _geom(a, B)
            assert got.tobytes() == _np_block_digests(a, B).tobytes()
            table = a.state_digest()
            for t in range(5):
                assert _merge(got, first[t], first[t + 1]) == table[t]
        assert _select(a, b, 256)[1] == 0
        # the primary gets three rows more in one bucket of table 2: one block differs, its rows and its diff are numpy's
        hs = a.hash_size(2)
        per_b = np.zeros(hs, np.int64)
        per_b[2 * 700 + i] = 3  # (global bucket of local bucket 700 of shard i)
        keys = keys_by_bucket(hs, per_b, seed=5)
        a.load_rows(2, keys, np.array([4, 5, 6], "<u4"), np.full((3, 40), 9, "u1"))
        first, _ = _geom(a, 256)
        ids, nd = _select(a, b, 256)
        assert ids.tolist() == [first[2] + 700 // 256]
        _, _, rows, _ = _rows(a, 256, ids)
        assert rows.tobytes() == _np_rows(a, 256, ids).tobytes()
        before = _image(b)
        nrec, st, rec, _ = _block_diff(b, 256, ids, rows)
        assert nrec == 3 and st == {"total": 3, "only_a": 3, "only_b": 0, "val_differs": 0, "ver_only": 0}
        assert sorted(rec["key"].tolist()) == sorted(keys.tolist()) and (rec["table"] == 2).all() and (rec["is_del"] == 0).all()
        # a row of the OTHER shard is home to no listed block here
        other = rows.copy()
        other["key"][0] = keys_by_bucket(hs, np.eye(1, hs, 2 * 700 + 1 - i, dtype=np.int64)[0], seed=6)[0]
        with pytest.raises(_lib.DintError):
            _block_diff(b, 256, ids, other)
        assert _image(b) == before
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 2. layout independence
def test_a_replica_rebuilt_from_the_log_has_the_primarys_block_digests():
    import torch

    cap = 4096
    p = _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    dev = []
    for b in range(3):
        req = _committed_writes(o, 1500, seed=b)
        assert p.submit(req).tobytes() == o.replay(req).tobytes()
        n, lost = p.log_drain_device(buf, cap)
        assert (n, lost) == (1500, 0)
        dev.append(buf[:n * 64].clone())
    rep = _tatp()
    rep.log_apply_device(torch.cat(dev), 4500, chunk=777)  # the same rows in chains of its own
    m = np.zeros(400, wire.TATP_MSG)  # lock words and log records on the replica are not state
    m["type"][:200], m["type"][200:] = T.ACQUIRE_LOCK, T.COMMIT_LOG
    for t in range(5):
        m["table"][t::5] = t
    m["key"] = np.tile(o.dump(0)[0][:40], 10)
    assert (rep.submit(m)["type"][:200] == T.GRANT_LOCK).sum() > 20
    for B in BS:
        assert _digests(rep, B)[0].tobytes() == _digests(p, B)[0].tobytes() == _np_block_digests(p, B).tobytes()
        assert _select(p, rep, B)[1] == 0


# ---------------------------------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize("B", BS)
def test_block_rows_are_numpys_visible_rows_in_order(prim, B):
    n_blocks = sum(_geom(prim, B)[1])
    before = _image(prim)
    for ids in (np.arange(n_blocks), np.arange(n_blocks)[::2], np.array([n_blocks - 1])):
        want = _np_rows(prim, B, ids)
        n, total, rec, raw = _rows(prim, B, ids, shift=8)  # (an 8-byte aligned address that is not 64-byte aligned)
        assert n == total == len(want) and rec.tobytes() == want.tobytes()
        assert (raw[:8] == 0xEE).all() and (raw[8 + 64 * n:] == 0xEE).all()
        assert prim.state_block_rows(B, _ids(ids), len(ids)) == (0, len(want))  # count only
        n, total, rec, raw = _rows(prim, B, ids, cap=len(want) - 5)
        assert n == len(want) - 5 and total == len(want) and rec.tobytes() == want[:n].tobytes() and (raw[64 * n:] == 0xEE).all()
    assert prim.state_block_rows(B, _ids([]), 0) == (0, 0)
    assert _image(prim) == before
    if B == 64:  # the shadowed second row of a key of bucket 64 is in the digest and not in the rows
        first, _ = _geom(prim, 64)
        assert len(_np_rows(prim, 64, [first[4] + 1])) == _digests(prim, 64)[0][first[4] + 1, 0] - 1


# ---------------------------------------------------------------------------------------------- 4. - 7. a replica behind
@pytest.fixture(scope="module")
def behind():
    """(primary, replica, replica's image): the primary 400 committed writes ahead, inserts and deletes among them, and with chains"""
    p, r = _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    keys = _with_chains(p)
    _with_chains(r)
    req = _committed_writes(o, 400, seed=31)
    p.submit(req)
    m = np.zeros(1, wire.TATP_MSG)  # and the replica holds a row of the chains the primary has deleted
    m["type"], m["table"], m["key"] = T.DELETE_PRIM, 4, keys[2]
    p.submit(m)
    assert keys[2] not in p.dump_rows(4)[0] and keys[2] in r.dump_rows(4)[0]
    return p, r


@pytest.mark.parametrize("B", BS)
def test_select_diff_and_repair_of_a_replica_behind(behind, B):
    import torch

    p, r0 = behind
    r = _copy_of(r0)
    img_p, img_r = _image(p), _image(r)
    np_p, np_r = _np_block_digests(p, B), _np_block_digests(r, B)
    want_ids = np.nonzero((np_p != np_r).any(axis=1))[0]
    ids, nd = _select(p, r, B)
    assert nd == len(want_ids) > 0 and ids.tolist() == want_ids.tolist()
    # a cap shorter than the list: the first ids, the full count
    da, n, _ = p.state_block_digest(B)
    db, _, _ = r.state_block_digest(B)
    short = torch.full((nd + 2,), -1, dtype=torch.int32, device="cuda")
    assert r.state_block_select(da, db, n, short, nd - 1)[1] == nd
    assert short.cpu().numpy().tolist() == want_ids[:nd - 1].tolist() + [-1] * 3
    # with all of them listed the block diff IS the diff of the two engines
    _, _, rows, _ = _rows(p, B, ids)
    assert rows.tobytes() == _np_rows(p, B, ids).tobytes()
    total = p.state_diff(r)[1]["total"]
    full = torch.full(((total + 2) * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    n_full, st_full = p.state_diff(r, full, total)
    n, st, rec, d_rec = _block_diff(r, B, ids, rows, shift=8)
    assert n == n_full == total > 100 and st == st_full
    assert rec.tobytes() == full[:64 * total].cpu().numpy().tobytes()
    # a short buffer: the first records of the order
    n2, st2, rec2, _ = _block_diff(r, B, ids, rows, cap=total - 7)
    assert n2 == total - 7 and st2 == st and rec2.tobytes() == rec[:n2].tobytes()
    assert _image(p) == img_p and _image(r) == img_r  # none of the four calls modifies an engine
    rs = r.state_repair(d_rec[8:], n)
    assert rs["applied"] == total and rs["refused"] == 0
    assert _select(p, r, B)[1] == 0 and r.state_digest() == p.state_digest()
    for v in r.state_verify():
        assert not any(v[k] for k in recovery.VERIFY_VIOLATIONS), v
    r.close()


def test_one_damaged_row_gives_one_id_and_equal_engines_carry_digests_only(behind):
    p = behind[0]
    r = _copy_of(p)
    c = Carry()
    out = recovery.resync_blocks(p, r, block_buckets=64, carry=c)
    assert _select(p, r, 64)[1] == 0
    assert out == {"rounds": 0, "records": 0, "blocks_differing": 0, "digest_bytes": 32 * 21, "id_bytes": 0, "row_bytes": 0, "digests_equal": True}
    assert (c.bytes, c.calls) == (32 * 21, 1)
    k = r.dump_rows(3)[0][17]
    m = np.zeros(1, wire.TATP_MSG)
    m["type"], m["table"], m["key"], m["val"] = T.COMMIT_PRIM, 3, k, 0x5A
    r.submit(m)
    assert not recovery.digests_equal(p, r)
    for B in BS:
        first, _ = _geom(r, B)
        ids, nd = _select(p, r, B)
        assert ids.tolist() == [first[3] + int(np_bucket(np.array([k], "<u8"), r.hash_size(3))[0]) // B]
    rows = len(_np_rows(p, 64, _select(p, r, 64)[0]))
    c = Carry()
    out = recovery.resync_blocks(p, r, block_buckets=64, carry=c)
    assert out["rounds"] == 1 and out["records"] == 1 and out["blocks_differing"] == 1 and out["digests_equal"]
    assert (out["digest_bytes"], out["id_bytes"], out["row_bytes"]) == (2 * 32 * 21, 4, 64 * rows) and rows > 0
    assert c.bytes == out["digest_bytes"] + out["id_bytes"] + out["row_bytes"]
    r.close()


@pytest.mark.parametrize("B,cap", [(64, 1 << 16), (256, 1 << 16), (64, 700)])
def test_resync_blocks_carries_the_rows_of_the_differing_blocks(behind, B, cap):
    p, r0 = behind
    r = _copy_of(r0)
    want_ids = _select(p, r, B)[0]
    want_rows = len(_np_rows(p, B, want_ids))
    image_bytes = p.state_export()[1]
    c = Carry()
    out = recovery.resync_blocks(p, r, block_buckets=B, cap=cap, carry=c)
    print("resync_blocks", B, cap, out, "image", image_bytes)
    assert out["digests_equal"] and out["blocks_differing"] == len(want_ids)
    assert c.bytes == out["digest_bytes"] + out["id_bytes"] + out["row_bytes"]
    if cap >= want_rows:
        assert out["rounds"] == 1 and out["row_bytes"] == 64 * want_rows and out["id_bytes"] == 4 * len(want_ids)
        assert out["digest_bytes"] == 2 * 32 * sum(_geom(p, B)[1])
    else:
        assert out["rounds"] > 1 and out["row_bytes"] >= 64 * want_rows
    assert c.bytes < image_bytes
    assert r.state_digest() == p.state_digest() and p.state_diff(r)[1]["total"] == 0
    r.close()


def test_a_replica_a_few_writes_behind_carries_far_less_than_an_image():
    """three writes to SUBSCRIBER rows: at most the two blocks of table 0 differ.  They hold its 300 rows, 19,200 bytes of records;
    with the digests of two rounds (2 x 2 x 21 x 32) and the ids that is under 23 KB, and the image holds 256 bytes for every
    one of the 1,207 buckets alone: an eighth of the image is a bound with room"""
    p, r = _tatp(), _tatp()
    m = np.zeros(3, wire.TATP_MSG)
    m["type"], m["table"], m["key"], m["val"] = T.COMMIT_PRIM, 0, p.dump_rows(0)[0][[5, 150, 290]], 0x77
    p.submit(m)
    ids, nd = _select(p, r, 64)
    assert 1 <= nd <= 2 and (ids < 2).all()
    rows = len(_np_rows(p, 64, ids))
    image_bytes = p.state_export()[1]
    c = Carry()
    out = recovery.resync_blocks(p, r, block_buckets=64, carry=c)
    print("resync_blocks, three writes behind", out, "image", image_bytes)
    assert out["rounds"] == 1 and out["records"] == 3 and out["blocks_differing"] == nd and out["digests_equal"]
    assert (out["digest_bytes"], out["id_bytes"], out["row_bytes"]) == (2 * 32 * 21, 4 * nd, 64 * rows)
    assert c.bytes == out["digest_bytes"] + out["id_bytes"] + out["row_bytes"] < image_bytes // 8


# ---------------------------------------------------------------------------------------------- 8. a shadowed duplicate
def test_a_shadowed_duplicate_takes_a_second_round():
    p, r = _tatp(), _tatp()
    hs = r.hash_size(2)
    key = keys_by_bucket(hs, np.eye(1, hs, 100, dtype=np.int64)[0], seed=3)
    for ver in (3, 4):  # the replica holds a key twice that the primary lacks: deleting the visible row uncovers the other
        r.load_rows(2, key, np.array([ver], "<u4"), np.full((1, 40), ver, "u1"))
    out = recovery.resync_blocks(p, r, block_buckets=64, carry=Carry())
    assert out["rounds"] == 2 and out["records"] == 2 and out["blocks_differing"] == 1 and out["digests_equal"]
    assert out["row_bytes"] == 2 * 64 * len(_np_rows(p, 64, [_geom(p, 64)[0][2] + 100 // 64]))
    # LogShipper.resync(blocks=) is the same path
    r.load_rows(2, key, np.array([9], "<u4"), np.full((1, 40), 9, "u1"))
    sh = recovery.LogShipper(p, r, cap=4096)
    assert not recovery.digests_equal(p, r)
    out = sh.resync(blocks=64)
    assert out["rounds"] == 1 and out["digests_equal"] and "row_bytes" in out
    assert "row_bytes" not in sh.resync()


# ---------------------------------------------------------------------------------------------- 9. - 10. hostile input
def test_hostile_lists_are_refused_with_nothing_written(behind):
    import torch

    p, r = behind
    B = 64
    n_blocks = sum(_geom(p, B)[1])
    ids = np.arange(n_blocks)
    rows = _np_rows(p, B, ids)
    image = _image(r)
    L = r._L

    def refused(B, ids, rows, rows_too=False):
        """the return code of block_diff (and of block_rows with the same ids); the 0xEE-filled outputs and b's image untouched"""
        d_rows = _dev(rows)
        out = torch.full((4096 * 64,), 0xEE, dtype=torch.uint8, device="cuda")
        d_ids = _ids(ids)
        st = _lib.DiffStats()
        rc = L.dint_state_block_diff(r._h, B, d_ids.data_ptr(), len(ids), d_rows.data_ptr(), len(rows), out.data_ptr(), 4096, C.byref(st), None)
        rc2 = L.dint_state_block_rows(r._h, B, d_ids.data_ptr(), len(ids), out.data_ptr(), 4096, None, None) if rows_too else None
        assert bool((out == 0xEE).all()) and _image(r) == image
        return rc if rc2 is None else (rc, rc2)

    assert refused(B, ids, rows[::-1].copy()) == EINVAL and b"grouped" in L.dint_last_error()
    swapped = rows.copy()
    swapped[[10, 900]] = swapped[[900, 10]]
    assert refused(B, ids, swapped) == EINVAL
    assert refused(B, ids[1:], rows) == EINVAL and b"listed" in L.dint_last_error()  # rows home to an unlisted block
    t7 = rows.copy()
    t7["table"][5] = 7
    assert refused(B, ids, t7) == EINVAL and b"table" in L.dint_last_error()
    for bad in (ids[::-1].copy(), np.array([0, 1, 1, 2]), np.array([0, n_blocks]), np.array([2, 0xFFFFFFFF], np.uint32).view(np.int32)):
        assert refused(B, bad, rows, True) == (EINVAL, EINVAL), bad
        assert b"ascending" in L.dint_last_error()
    for bad_b in (96, 32):
        assert refused(bad_b, ids, rows, True) == (EINVAL, EINVAL)
        assert L.dint_state_block_digest(r._h, bad_b, None, 0, None, None) == EINVAL
    # unaligned buffers, a digest buffer that is too small
    out = torch.full((4096,), 0xEE, dtype=torch.uint8, device="cuda")
    assert L.dint_state_block_digest(r._h, B, out.data_ptr(), n_blocks - 1, None, None) == EINVAL
    assert L.dint_state_block_digest(r._h, B, out.data_ptr() + 4, n_blocks, None, None) == EINVAL
    assert L.dint_state_block_rows(r._h, B, _ids(ids).data_ptr(), 1, out.data_ptr() + 4, 8, None, None) == EINVAL
    assert bool((out == 0xEE).all()) and _image(r) == image
    # the good list goes through
    n, st, rec, _ = _block_diff(r, B, ids, rows)
    assert n == st["total"] == p.state_diff(r)[1]["total"]


def test_a_key_listed_twice_in_a_run_the_first_wins(behind):
    p, r = behind
    ids = np.arange(sum(_geom(p, 64)[1]))
    rows = _np_rows(p, 64, ids)
    want = _block_diff(r, 64, ids, rows)
    i = int(np.nonzero(rows["table"] == 4)[0][20])
    twin = rows[i:i + 1].copy()
    twin["val"][0, 0] ^= 0xFF
    twin["ver"] += 5
    got = _block_diff(r, 64, ids, np.concatenate([rows[:i + 1], twin, rows[i + 1:]]))
    assert got[0] == want[0] and got[1] == want[1] and got[2].tobytes() == want[2].tobytes()
    first_twin = _block_diff(r, 64, ids, np.concatenate([rows[:i], twin, rows[i:]]))  # the other way round: the changed copy is the visible one
    assert first_twin[2].tobytes() != want[2].tobytes() and twin.tobytes() in first_twin[2].tobytes()


# ---------------------------------------------------------------------------------------------- 11. refusals
def test_engines_without_kv_tables_and_a_pending_batch_are_refused():
    import torch

    out = torch.zeros(4096 * 64, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()

    def calls(e):
        L = e._L
        return (L.dint_state_block_digest(e._h, 64, p, 4096, None, None), L.dint_state_block_rows(e._h, 64, p, 1, p, 16, None, None),
                L.dint_state_block_diff(e._h, 64, p, 1, p, 0, p, 16, None, None))

    for e in (_engine(W.FASST, n_slots=1024), _engine(W.TPL, n_slots=1024), _engine(W.LOG, log_entries=1024)):
        assert calls(e) == (ESTATE, ESTATE, ESTATE), e.workload
    b = _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    wx = _committed_writes(o, 500, seed=11)
    o.replay(wx)
    x, y = _dev(wx), _dev(_committed_writes(o, 500, seed=12))
    b.submit_device(x, 1000, None, 0, ahead=(y, 1000, None))
    assert calls(b) == (ESTATE, ESTATE, ESTATE) and b"announced" in b._L.dint_last_error()
    b.submit_device(y, 1000)
    b.sync()
    # the announced batch after all: the engine goes on
    assert b.state_block_digest(64)[1] == 21 and b.state_block_rows(64, _ids([0]), 1)[1] > 0
    assert _block_diff(b, 64, [0], _np_rows(b, 64, [0]))[0] == 0
