"""Records routed to the shards of another layout on the GPU (include/dint_abi.h dint_records_route, dint_amd/csrc/k_rroute.hip over
csrc/state_route.h) and the consumers that take a shard (DINT_FLAG_SHARD_REPLICA: dint_state_repair, dint_state_diff,
dint_log_apply_device, dint_log_apply_folded_device; dint_amd/recovery.py route_records / resync / resync_blocks / resync_set /
ShardSetShipper), against forms that share no code with them: the route as numpy's stable argsort by home
(tests/test_state_route_host.py: the home from tests/kvkeys.py np_bucket) and the host form, the consumers against an UNSHARDED
twin that takes the same records unrouted, the primary whose records they are, and the CPU oracle's rows.  Every comparison is
exact."""
import ctypes as C

import numpy as np
import pytest

import tracegen
from dint_amd import _lib, recovery, wire
from kvkeys import keys_by_bucket
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes
from test_gpu_state_sync import _sb_writes
from test_state_route_host import HS, SHAPES, hash_sizes, np_home, np_route, records, route_host

W = wire.Workload
EINVAL, ENOMEM, ESTATE = -1, -2, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
TILE = _lib.ROUTE_TILE
FLAG = _lib.FLAG_SHARD_REPLICA
pytestmark = pytest.mark.gpu


def _engine(wl, n_rows, **kw):
    from dint_amd.engine import Engine

    if wl != W.STORE:
        kw.setdefault("log_entries", 1 << 16)
    return Engine(wl, n_rows=n_rows, **kw)


def _set(wl, n_rows, H, populate, flags=FLAG, **kw):
    """a complete set of H shards (H = 1: one unsharded engine), every shard loaded by `populate` rows as an unsharded engine is"""
    out = [_engine(wl, n_rows, shard_index=i, shard_count=H, flags=flags if H > 1 else 0, **kw) for i in range(H)]
    for e in out:
        e.populate(populate)
    return out


def _dev(a):
    import torch

    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def _host(t, n):
    return np.frombuffer(t[:n * 64].cpu().numpy().tobytes(), wire.LOG_REC)


def _dumps(e):
    return [tuple(x.tobytes() for x in e.dump_rows(t)) for t in range(NTAB[e.workload])]


def _sorted_rows(engines, t):
    k, v, x = (np.concatenate(c) for c in zip(*(e.dump_rows(t) for e in engines)))
    o = np.lexsort((v, k))
    return k[o], v[o], x[o]


def _same_rows(a_set, b_set):
    for t in range(NTAB[a_set[0].workload]):
        ra, rb = _sorted_rows(a_set, t), _sorted_rows(b_set, t)
        assert all(x.shape == y.shape and (x == y).all() for x, y in zip(ra, rb)), t


def _route(geom, H, d_rec, n, cap=None, guard=4):
    """dint_records_route into a fresh buffer of cap records filled with 0xEE, `guard` records of room behind it: (rc, buffer,
    offsets); the write stage has finished"""
    import torch

    cap = n if cap is None else cap
    out = torch.full(((cap + guard) * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    off = (C.c_uint64 * (H + 2))(*([0xEEEEEEEE] * (H + 2)))
    rc = geom._L.dint_records_route(geom._h, H, d_rec.data_ptr() if d_rec is not None else None, n, out.data_ptr(), cap, off, None)
    geom.sync()
    return rc, out, list(off)


@pytest.fixture(scope="module")
def tatp300():
    """an unsharded tatp primary of 300 subscribers after 3 x 2,000 committed writes (updates, inserts and deletes of rows of all five
    tables, CALL_FORWARDING among them), its log drained on the device, the oracle that took the same requests, and the requests"""
    import torch

    a = _set(W.TATP, 300, 1, 300)[0]
    o = orc.TatpOracle(300, log_entries=1 << 20)
    buf = torch.zeros(4096 * 64, dtype=torch.uint8, device="cuda")
    dev, reqs = [], []
    for b in range(3):
        req = _committed_writes(o, 2000, seed=20 + b)
        assert a.submit(req).tobytes() == o.replay(req).tobytes()
        assert a.log_drain_device(buf, 4096) == (2000, 0)
        dev.append(buf[:2000 * 64].clone())
        reqs.append(req)
    d_rec = torch.cat(dev)
    rec = _host(d_rec, 6000)
    assert set(np.unique(rec["table"]).tolist()) == {0, 1, 2, 3, 4} and rec["is_del"].any()
    return a, o, d_rec, rec, reqs


# ---------------------------------------------------------------------------------------------- 1. the route
def _sizes():
    return [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 65_537]


@pytest.mark.parametrize("wl,n_rows", SHAPES)
def test_route_is_numpys_stable_partition_byte_for_byte(wl, n_rows, tatp300):
    a, _, _, log, _ = tatp300
    if wl == W.TATP:  # a drained log and a state_diff list, repeated to the length asked for
        stale = _set(wl, n_rows, 1, n_rows)[0]
        tot = a.state_diff(stale)[1]["total"]
        assert tot > 300
        import torch

        dbuf = torch.zeros(tot * 64, dtype=torch.uint8, device="cuda")
        assert a.state_diff(stale, dbuf, tot)[0] == tot
        sources = [log, _host(dbuf, tot)]
        geom = a
    else:
        sources = [records(wl, 6000, seed=11)]
        geom = _set(wl, n_rows, 1, n_rows)[0]
    before, digest = _dumps(geom), geom.state_digest()
    for k, n in enumerate(_sizes()):
        src = sources[k % len(sources)]
        rec = np.resize(src, n) if n else src[:0]
        d_rec = _dev(rec) if n else None
        for H in HS:
            want, woff = np_route(rec, wl, n_rows, H)
            rc, out, off = _route(geom, H, d_rec, n)
            assert rc == n, (n, H, geom._L.dint_last_error())
            assert off[:H + 1] == woff.tolist() and off[H + 1] == 0xEEEEEEEE, (n, H)
            got = out.cpu().numpy()
            assert got[:n * 64].tobytes() == want.tobytes(), (n, H)
            assert (got[n * 64:] == 0xEE).all()  # nothing behind the n records
            if H == 1:
                assert got[:n * 64].tobytes() == rec.tobytes()  # one shard: a copy
            if n in (TILE + 1, 65_537) and H in (3, 255):
                rc2, out2, off2 = _route(geom, H, d_rec, n)  # two runs: the same bytes
                assert rc2 == n and off2 == off and (out2 == out).all()
                hrc, hout, hoff = route_host(wl, n_rows, H, rec)  # ... and the host form's
                assert hrc == n and hoff[:H + 1].tolist() == off[:H + 1] and hout[:n * 64].tobytes() == got[:n * 64].tobytes()
            if n:
                assert d_rec.cpu().numpy().tobytes() == rec.tobytes()  # the records stay untouched
    assert _dumps(geom) == before and geom.state_digest() == digest  # geom lends its sizes: its tables are not touched


def test_route_ignores_the_geom_engines_own_layout_and_leaves_a_blank_one_blank(tatp300):
    a, _, d_rec, rec, _ = tatp300
    blank = _engine(W.TATP, 300, shard_index=1, shard_count=2)  # a shard, never loaded
    want, woff = np_route(rec, W.TATP, 300, 3)
    out, off = blank.records_route(3, d_rec, len(rec))
    assert off == woff.tolist() and out.cpu().numpy().tobytes() == want.tobytes()
    pieces = recovery.route_records(blank, d_rec, len(rec), 3)
    assert [m for _, m in pieces] == np.diff(woff.astype(np.int64)).tolist()
    assert b"".join(v.cpu().numpy().tobytes() for v, _ in pieces) == want.tobytes()
    assert all(d["rows"] == 0 for d in blank.state_digest())
    twin = _set(W.TATP, 300, 2, 300, flags=0)[1]
    buf, nbytes, _ = twin.state_export(1, 2)
    blank.state_import(buf, nbytes)  # (an import takes a BLANK engine only)
    assert blank.state_digest() == twin.state_digest()


def test_route_refusals_leave_the_output_as_it_was(tatp300):
    import torch

    a, _, d_rec, rec, _ = tatp300
    n = 1000

    def call(geom, H, src, n, dst, cap):
        off = (C.c_uint64 * 300)(*([7] * 300))
        rc = geom._L.dint_records_route(geom._h, H, src, n, dst, cap, off, None)
        geom.sync()
        return rc, list(off)

    out = torch.full((2 * n * 64,), 0xEE, dtype=torch.uint8, device="cuda")
    p, q = d_rec.data_ptr(), out.data_ptr()
    for H in (0, 256, 1 << 20):
        assert call(a, H, p, n, q, n)[0] == EINVAL
    assert call(a, 3, p + 8, n, q, n)[0] == EINVAL and call(a, 3, p, n, q + 8, n)[0] == EINVAL  # not 16-byte aligned
    assert call(a, 3, None, n, q, n)[0] == EINVAL and call(a, 3, p, n, None, n)[0] == EINVAL
    assert call(a, 3, p, n, q, n - 1)[0] == ENOMEM and call(a, 3, p, n, q, 0)[0] == ENOMEM
    both = torch.cat([d_rec[:n * 64], out])  # input and output in one allocation: overlapping either way round
    b0 = both.data_ptr()
    ref = both.clone()
    assert call(a, 3, b0, n, b0 + 64 * (n - 1), n)[0] == EINVAL and call(a, 3, b0 + 64, n, b0, n)[0] == EINVAL
    assert call(a, 3, b0, n, b0, n)[0] == EINVAL
    assert (both == ref).all()
    assert call(a, 3, b0, n, b0 + 64 * n, n)[0] == n  # adjacent: fine
    assert both[n * 64:2 * n * 64].cpu().numpy().tobytes() == np_route(rec[:n], W.TATP, 300, 3)[0].tobytes()
    for e in (_engine_lock(W.FASST), _engine_lock(W.TPL), _engine_log()):
        assert call(e, 3, p, n, q, n)[0] == ESTATE
    # records without a home: the message names the first one, wherever the second is
    bad = rec[:3 * TILE + 17].copy()
    bad["table"][2 * TILE + 5] = 5
    bad["table"][TILE - 1] = 200
    rc, off = call(a, 3, _dev(bad).data_ptr(), len(bad), q, 2 * n)
    assert rc == EINVAL and f"record {TILE - 1} ".encode() in a._L.dint_last_error() and off == [7] * 300
    sb = _set(W.SMALLBANK, 1000, 1, 0)[0]
    rc, _ = call(sb, 2, _dev(bad).data_ptr(), len(bad), q, 2 * n)  # smallbank has two tables: the log holds rows of five
    assert rc == EINVAL and b"record " in sb._L.dint_last_error()
    assert (out == 0xEE).all()
    # no records: every offset 0
    rc, off = call(a, 4, None, 0, None, 0)
    assert rc == 0 and off[:5] == [0] * 5 and off[5] == 7


def _engine_lock(wl):
    from dint_amd.engine import Engine

    return Engine(wl, n_slots=1024)


def _engine_log():
    from dint_amd.engine import Engine

    return Engine(W.LOG, log_entries=1024)


# ---------------------------------------------------------------------------------------------- 2. repair through the route
def _diff_list(a, r):
    import torch

    tot = a.state_diff(r)[1]["total"]
    buf = torch.zeros(max(tot, 1) * 64, dtype=torch.uint8, device="cuda")
    n, st = a.state_diff(r, buf, tot)
    assert n == tot
    return buf, n, st


def _home_rows(a, wl, n_rows, H, i, t):
    """a's rows of table t that are home to shard i of H, sorted by key"""
    k, v, x = a.dump_rows(t)
    m = np_home(np.rec.fromarrays([k, np.full(len(k), t, np.uint8)], names="key,table"), wl, n_rows, H) == i
    o = np.argsort(k[m], kind="stable")
    return k[m][o], v[m][o], x[m][o]


def _repair_through_route(a, wl, n_rows, populate):
    r = _set(wl, n_rows, 1, populate)[0]
    buf, n, st = _diff_list(a, r)
    assert n > 100
    for H in (2, 3, 5):
        shards = _set(wl, n_rows, H, populate)
        assert recovery.digest_sum(shards) == r.state_digest()  # loaded as r was
        before = [_dumps(e) for e in shards]
        with pytest.raises(_lib.DintError):  # the un-routed list holds rows of every shard
            shards[1].state_repair(buf, n)
        assert [_dumps(e) for e in shards] == before
        pieces = recovery.route_records(a, buf, n, H)
        tot = dict.fromkeys(("applied", "updated", "inserted", "deleted", "refused"), 0)
        for e, (view, m) in zip(shards, pieces):
            rs = e.state_repair(view, m)
            for k in tot:
                tot[k] += rs[k]
        assert recovery.digest_sum(shards) == a.state_digest(), H
        for i, e in enumerate(shards):
            for t in range(NTAB[wl]):
                k, v, x = e.dump_rows(t)
                o = np.argsort(k, kind="stable")
                wk, wv, wx = _home_rows(a, wl, n_rows, H, i, t)
                assert (k[o] == wk).all() and (v[o] == wv).all() and (x[o] == wx).all(), (H, i, t)
            assert e.stats()["missing_keys"] == 0
        if H == 5:
            rs = r.state_repair(buf, n)  # the same records, unrouted, into the unsharded twin
            assert {k: rs[k] for k in tot} == tot and tot["applied"] == st["total"] and tot["refused"] == 0
            assert r.state_digest() == a.state_digest()
        for e in shards:
            e.close()


def test_repair_through_the_route_tatp(tatp300):
    a = tatp300[0]
    _repair_through_route(a, W.TATP, 300, 300)


def test_repair_through_the_route_smallbank_and_store():
    a = _set(W.SMALLBANK, 1000, 1, 1000)[0]
    a.submit(_sb_writes(1000, 4000, seed=1))
    _repair_through_route(a, W.SMALLBANK, 1000, 1000)
    a = _set(W.STORE, 1000, 1, 80)[0]
    a.submit(tracegen.store_random(20_000, seed=1, n_sub_touch=40, p_set=0.4, p_insert=0.05))
    _repair_through_route(a, W.STORE, 1000, 80)


# ---------------------------------------------------------------------------------------------- 3. diff on shards
def _local_place(rec, wl, n_rows, H):
    """(table << 40 | local bucket) per record"""
    from kvkeys import np_bucket

    out = np.zeros(len(rec), np.int64)
    for t, hs in enumerate(hash_sizes(wl, n_rows)):
        m = rec["table"] == t
        out[m] = (t << 40) | (np_bucket(rec["key"][m], hs).astype(np.int64) // H)
    return out


def test_diff_of_a_flagged_pair_is_the_routed_unsharded_diff(tatp300):
    a = tatp300[0]
    wl, n_rows, H = W.TATP, 300, 3
    r = _set(wl, n_rows, 1, 300)[0]
    buf, n, st = _diff_list(a, r)
    pieces = recovery.route_records(a, buf, n, H)
    A, R = _set(wl, n_rows, H, 300), _set(wl, n_rows, H, 300)
    for e, (view, m) in zip(A, pieces):  # set A := a's rows
        e.state_repair(view, m)
    assert recovery.digest_sum(A) == a.state_digest()
    tot = dict.fromkeys(st, 0)
    for i in range(H):
        sbuf, sn, sst = _diff_list(A[i], R[i])
        for k in tot:
            tot[k] += sst[k]
        got, want = _host(sbuf, sn), _host(pieces[i][0], pieces[i][1])
        place = _local_place(got, wl, n_rows, H)
        assert (np.diff(place) >= 0).all()  # ascending table, then ascending LOCAL bucket
        assert (np_home(got, wl, n_rows, H) == i).all()
        # the same records per (table, local bucket); the order inside a bucket is the chains' business
        assert sn == pieces[i][1]
        key = lambda x, pl: np.lexsort((x["is_del"], x["key"], pl))  # noqa: E731
        wplace = _local_place(want, wl, n_rows, H)
        assert got[key(got, place)].tobytes() == want[key(want, wplace)].tobytes()
        rs = R[i].state_repair(sbuf, sn)
        assert rs["applied"] == sn and rs["refused"] == 0
        again = recovery.resync(A[i], R[i], cap=4096)
        assert again == {"rounds": 0, "records": 0, "digests_equal": True}
    assert tot == st
    assert recovery.digest_sum(R) == a.state_digest()
    # pairs of different index or count, and a sharded side without the flag
    L = a._L
    other = _set(wl, n_rows, 2, 300)
    plain = _set(wl, n_rows, H, 300, flags=0)
    for x, y in ((A[0], A[1]), (A[0], other[0]), (a, A[0]), (A[0], a), (A[1], plain[1]), (plain[1], A[1])):
        assert L.dint_state_diff(x._h, y._h, None, 0, None, None) == EINVAL
    assert L.dint_state_diff(A[1]._h, R[1]._h, None, 0, None, None) == 0
    res = recovery.resync_set(A, R)
    assert res["digests_equal"] and res["records"] == 0 and len(res["shards"]) == H
    with pytest.raises(_lib.DintError, match="reshard"):
        recovery.resync_set(A, other)


# ---------------------------------------------------------------------------------------------- 4. log replay on shards
def _apply_pieces(replicas, pieces, folded, chunk=0):
    """every destination's pieces one after the other; the counts summed"""
    tot = {}
    for j, view, m in pieces:
        if m == 0:
            continue
        st = replicas[j].log_apply_folded(view, m, chunk) if folded else replicas[j].log_apply_device(view, m, chunk)
        for k in ("applied", "commits", "inserts", "deletes") + (("deferred_records", "folded_records") if folded else ()):
            tot[k] = tot.get(k, 0) + st[k]
    return tot


def _oracle_rows_agree(o, engines):
    for t in range(5):
        k, v, x = _sorted_rows(engines, t)
        ok, ov, ox = o.dump(t)
        oo = np.lexsort((ov, ok))
        assert (k == ok[oo]).all() and (v == ov[oo]).all() and (x == ox[oo]).all(), t


@pytest.mark.parametrize("folded", [False, True])
def test_an_unsharded_primarys_log_replayed_into_shard_sets(tatp300, folded):
    a, o, d_rec, rec, _ = tatp300
    n = len(rec)
    twin = _set(W.TATP, 300, 1, 300)[0]
    want = twin.log_apply_folded(d_rec, n, 1500) if folded else twin.log_apply_device(d_rec, n, 1500)
    assert twin.state_digest() == a.state_digest()
    for H in (2, 3):
        reps = _set(W.TATP, 300, H, 300)
        pieces = [(j, v, m) for j, (v, m) in enumerate(recovery.route_records(a, d_rec, n, H))]
        before = [_dumps(e) for e in reps]
        if folded:
            for j, v, m in pieces:  # a dry run counts and writes nothing
                dry = reps[j].log_apply_folded(v, m, 1500, dry_run=True)
                assert dry["applied"] == m
            assert [_dumps(e) for e in reps] == before
        # a piece with one record of another shard: refused whole, nothing applied
        j, v, m = pieces[0]
        foreign = v.clone()
        foreign[64 * (m // 2):64 * (m // 2) + 64] = pieces[1][1][:64]
        for dry in ((False, True) if folded else (False,)):
            with pytest.raises(_lib.DintError, match="another shard"):
                reps[0].log_apply_folded(foreign, m, 1500, dry_run=dry) if folded else reps[0].log_apply_device(foreign, m, 1500)
        with pytest.raises(_lib.DintError):
            reps[0].log_apply_folded(d_rec, n) if folded else reps[0].log_apply_device(d_rec, n)  # the un-routed log
        assert [_dumps(e) for e in reps] == before
        got = _apply_pieces(reps, pieces, folded, 1500)
        assert recovery.digest_sum(reps) == a.state_digest(), H
        assert {k: got[k] for k in ("applied", "commits", "inserts", "deletes")} == {k: want[k] for k in ("applied", "commits", "inserts", "deletes")}
        if folded:
            assert got["deferred_records"] + got["folded_records"] == n and "deferred_records" in want
        _oracle_rows_agree(o, reps)
        _same_rows([a], reps)
        assert all(e.stats()["missing_keys"] == 0 for e in reps)
        for e in reps:
            e.close()


@pytest.mark.parametrize("folded", [False, True])
def test_a_primary_set_of_two_replayed_into_a_replica_set_of_three(tatp300, folded):
    import torch

    a, o, _, rec, reqs = tatp300
    G, H = 2, 3
    prims = _set(W.TATP, 300, G, 300, flags=0, log_entries=4096)
    reps = _set(W.TATP, 300, H, 300)
    twin = _set(W.TATP, 300, 1, 300)[0]
    buf = torch.zeros(4096 * 64, dtype=torch.uint8, device="cuda")
    want = dict.fromkeys(("applied", "commits", "inserts", "deletes"), 0)
    got = dict(want)
    for b, req in enumerate(reqs):
        home = np_home(req, W.TATP, 300, G)
        for i, p in enumerate(prims):  # every primary shard gets its home requests, in order
            p.submit(req[home == i])
        st = twin.log_apply_device(_dev(rec[2000 * b:2000 * (b + 1)]), 2000)
        for k in want:
            want[k] += st[k]
        for i, p in enumerate(prims):
            n, lost = p.log_drain_device(buf, 4096)
            assert lost == 0 and n == int((home[0::2] == i).sum())
            pieces = [(j, v, m) for j, (v, m) in enumerate(recovery.route_records(p, buf, n, H))]
            assert sum(m for _, _, m in pieces) == n
            st = _apply_pieces(reps, pieces, folded)
            for k in want:
                got[k] += st[k]
    assert recovery.digest_sum(prims) == a.state_digest() == twin.state_digest()
    assert recovery.digest_sum(reps) == a.state_digest()
    assert got == want
    _oracle_rows_agree(o, reps)
    assert all(e.stats()["missing_keys"] == 0 for e in reps)


# ---------------------------------------------------------------------------------------------- 5. block sync of a flagged pair
def test_resync_blocks_on_a_flagged_pair_of_shards():
    n, B = 2000, 64
    P = _engine(W.TATP, n, shard_index=1, shard_count=2)
    R = _engine(W.TATP, n, shard_index=1, shard_count=2, flags=FLAG)
    P.populate(n); R.populate(n)
    assert recovery.digests_equal(P, R)
    hs = P.hash_size(0)
    per = np.zeros(hs, np.int64)
    per[2 * 63 + 1] = per[2 * 64 + 1] = 2  # local buckets 63 and 64 of shard 1: the last of block 0, the first of block 1
    keys = keys_by_bucket(hs, per, seed=8)
    P.load_rows(0, keys, np.arange(4, dtype="<u4") + 9, np.full((4, 40), 5, "u1"))
    all_rows = sum(len(P.dump_rows(t)[0]) for t in range(5))
    out = recovery.resync_blocks(P, R, block_buckets=B)
    print("resync_blocks on shard 1 of 2:", out)
    assert out["digests_equal"] and out["blocks_differing"] == 2 and out["records"] == 4
    assert 0 < out["row_bytes"] < all_rows * 64
    again = recovery.resync_blocks(P, R, block_buckets=B)  # (the primary needs no flag: only block calls read it)
    assert again["digests_equal"] and again["blocks_differing"] == 0 and again["rounds"] == 0 and again["row_bytes"] == 0
    plain = _engine(W.TATP, n, shard_index=1, shard_count=2)
    plain.populate(n)
    with pytest.raises(_lib.DintError):  # without the flag the repair still refuses a shard
        recovery.resync_blocks(P, plain, block_buckets=B)


# ---------------------------------------------------------------------------------------------- 6. the set shipper
@pytest.mark.parametrize("fold", [False, True])
def test_shard_set_shipper_two_to_three(tatp300, fold):
    a, _, _, _, reqs = tatp300
    prims = _set(W.TATP, 300, 2, 300, flags=0, log_entries=4096)
    reps = _set(W.TATP, 300, 3, 300)
    sh = recovery.ShardSetShipper(prims, reps, cap=4096, fold=fold)
    for req in reqs:  # three steps
        home = np_home(req, W.TATP, 300, 2)
        for i, p in enumerate(prims):
            p.submit(req[home == i])
        st = sh.step()
        assert st["applied"] == 2000 and st["lost"] == [0, 0] and sum(m for _, _, m in st["pieces"]) == 2000
        if fold:
            assert st["folded"] + st["deferred"] == 2000
    assert sh.routes == 6 and sh.shipped == 6000
    assert recovery.digest_sum(reps) == recovery.digest_sum(prims) == a.state_digest()
    with pytest.raises(_lib.DintError, match="reshard"):
        sh.resync()
    # equal layouts: a shard's log is its replica's piece as it stands -- no route call
    reps2 = _set(W.TATP, 300, 2, 300)
    prims2 = _set(W.TATP, 300, 2, 300, log_entries=4096)  # (flagged too: their resync diffs shard against shard)
    sh2 = recovery.ShardSetShipper(prims2, reps2, cap=4096, fold=fold)
    for req in reqs[:2]:
        home = np_home(req, W.TATP, 300, 2)
        for i, p in enumerate(prims2):
            p.submit(req[home == i])
        assert sh2.step()["applied"] == 2000
    assert sh2.routes == 0 and recovery.digest_sum(reps2) == recovery.digest_sum(prims2)
    prims2[0].submit(reqs[2][np_home(reqs[2], W.TATP, 300, 2) == 0])  # the replicas fall behind; a resync pairs the shards
    res = sh2.resync()
    assert res["digests_equal"] and res["records"] > 0 and sh2.step()["applied"] == 0
