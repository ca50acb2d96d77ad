"""A server's tables and overflow pool compacted in place on the GPU (include/dint_abi.h dint_state_compact,
dint_amd/csrc/k_compact.hip, dint_amd/recovery.py compact_tables / compact_advice): every view of
tests/test_state_compact_host.py run through the kernels (include/dint_driver.h dint_state_compact_view) against the host form and
the numpy form, and live engines against what the other calls report -- dump_rows, state_digest, state_stats, state_verify, the
exported image of a rehashed twin, read_locks, an uncompacted twin's replies and the CPU oracle's.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import kvkeys
import tracegen
from dint_amd import _lib, recovery, wire
from test_gpu_state_rehash import _delete_rows, _same_bucket_keys, _store_insert, _store_read, _tatp_trace, _vals, chained  # noqa: F401
from test_state_compact_host import CFIELDS, DRY, all_cases, expected, host_compact
from test_state_image_host import np_bucket
from test_state_verify_host import assert_identities, is_clean

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ESTATE = -1, -5
NTAB = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
pytestmark = pytest.mark.gpu
CASES = all_cases()


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def dev_compact(view, flags=0):
    """the view uploaded and run through dint_state_compact_view: (rc, reports, the bytes downloaded afterwards)"""
    import torch

    dev = [[_up(x) for x in (t.entries, t.pool_next, t.ctl)] for t in view.tabs]
    cv = view.c_view()
    for i, (e, n, c) in enumerate(dev):
        cv.table[i].entries, cv.table[i].pool_next, cv.table[i].ctl = e.data_ptr(), n.data_ptr() if n.numel() else 0, c.data_ptr()
    out = (_lib.TableCompact * 5)()
    torch.cuda.synchronize()
    rc = _lib.load().dint_state_compact_view(torch.cuda.current_device(), C.byref(cv), out, 5, flags, None)
    torch.cuda.synchronize()
    return rc, [out[t].as_dict() for t in range(len(view.tabs))], [tuple(x.cpu().numpy().tobytes() for x in d) for d in dev]


def _dumps(e):
    return [[x.tobytes() for x in e.dump_rows(t)] for t in range(NTAB[e.workload])]


def _image(e):
    buf, n, _ = e.state_export(e.shard_index, e.shard_count)
    return buf[:n].cpu().numpy().tobytes()


def _compacted(e, **kw):
    """compact, and what must hold after every compaction: the pool one range, nothing listed or leaked, a second one a no-op"""
    rep = e.state_compact(**kw)
    for r, v in zip(rep, e.state_verify()):
        assert is_clean(v) and v["free_entries"] == v["pending_entries"] == v["unaccounted"] == 0, v
        assert v["linked"] == v["pool_top"] == r["pool_top_after"] == r["overflow_after"] and v["rows"] == r["rows"] == r["verify"]["rows"]
        assert_identities(v)
    return rep


def _np_shape(e, t):
    """(holes, overflow entries, non-empty buckets) a packed table of e's rows has, from dump_rows and the keys' buckets"""
    g = np_bucket(e.dump_rows(t)[0], e.hash_size(t)).astype(np.int64)
    k = np.bincount(g[g % e.shard_count == e.shard_index] // e.shard_count) if len(g) else np.zeros(0, np.int64)
    k = k[k > 0]
    ent = -(-k // 4)
    return int((4 * ent - k).sum()), int((ent - 1).sum()), len(k)


def _packed(e):
    for t, st in enumerate(e.state_stats()):
        holes, ovf, nonempty = _np_shape(e, t)
        assert st["holes"] == holes and st["overflow_entries"] == ovf == st["pool_top"] and st["inline_first"] == nonempty, (t, st)
        assert st["inline_unlinked"] == 0 and st["entries"] == nonempty + ovf


# ---------------------------------------------------------------------------------------------- 1. views on the device
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_view_on_the_device_equals_the_host_form_equals_the_numpy_form(name):
    _, view, flags = next(c for c in CASES if c[0] == name)
    want_rc, want, after = expected(view, flags)
    rc, got, raw = dev_compact(view, flags)
    host = view.copy()
    hrc, hgot = host_compact(host, flags)
    assert rc == hrc == want_rc, _lib.load().dint_last_error()
    for t, (g, h, w) in enumerate(zip(got, hgot, want)):
        assert g == h == w, (name, t, {k: (g[k], h[k], w[k]) for k in w if not g[k] == h[k] == w[k]})
    assert raw == after.raw() == host.raw()
    if want_rc == ESTATE or flags & DRY:
        assert raw == view.raw()  # a refusal and a dry run leave the device buffers as they were


# ---------------------------------------------------------------------------------------------- 2. store: chains with holes
def test_the_chained_store_keeps_every_row_in_order_and_is_packed_afterwards(chained):  # noqa: F811
    e = chained
    per = np.zeros(e.hash_size(0), np.int64)
    per[:16] = 9
    mates = kvkeys.keys_by_bucket(e.hash_size(0), per, seed=3)  # nine keys in each of sixteen buckets ...
    _store_insert(e, mates, 4)
    _delete_rows(e, mates[np.arange(len(mates)) % 3 != 0])  # ... six of them gone again: holes in the middle of their chains
    before, digest = _dumps(e), e.state_digest()
    (st0,) = e.state_stats()
    (dry,) = e.state_compact(dry_run=True)
    assert _dumps(e) == before and e.state_stats() == [st0]
    (r,) = _compacted(e)
    print(r)
    assert {k: r[k] for k in CFIELDS} == {k: dry[k] for k in CFIELDS} and r["verify"] == dry["verify"]
    assert _dumps(e) == before and e.state_digest() == digest  # the same sequence: chain order kept
    assert r["holes_before"] == st0["holes"] > r["holes_after"] and r["entries_before"] == st0["entries"] and r["overflow_before"] == st0["overflow_entries"]
    assert r["pool_top_before"] == st0["pool_top"] > r["pool_top_after"] and r["buckets_rewritten"] > 0
    assert r["verify"]["free_entries"] + r["verify"]["pending_entries"] > 0  # or the case is void
    _packed(e)
    (again,) = _compacted(e)
    assert again["buckets_rewritten"] == 0 and again["holes_before"] == again["holes_after"] and _dumps(e) == before
    s = recovery.compact_tables([e], dry_run=True)
    assert s["tables"] == s["engines"][0] == [again]


# ---------------------------------------------------------------------------------------------- 3. against rehash
def _churned_store(pool_entries=2048):
    e = _engine(W.STORE, n_rows=64, pool_entries=pool_entries)
    rng = np.random.default_rng(5)
    keys = tracegen.store_key(rng.permutation(600)[:, None], np.arange(1, 4)[None, :], 0).ravel()
    rng.shuffle(keys)
    e.load_rows(0, keys, np.arange(len(keys), dtype="<u4"), _vals(keys, 1))
    _delete_rows(e, keys[::3])
    _store_insert(e, tracegen.store_key(3_000_000 + np.arange(200), 1, 0), 2)
    _delete_rows(e, keys[1::9])  # some buckets are emptied: their inline entries keep the deleted rows' bytes
    return e, keys


def test_the_image_afterwards_is_the_image_of_a_blank_twin_rehashed_from_it():
    e, _ = _churned_store()
    twin = _engine(W.STORE, n_rows=64, pool_entries=2048)
    twin.state_rehash([e])
    assert _image(e) != _image(twin)
    _compacted(e)
    assert _image(e) == _image(twin)  # every byte, the header included: no field differs by construction
    assert e.state_digest() == twin.state_digest()
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 4. locks stay
@pytest.mark.parametrize("flags", [0, _lib.FLAG_LOCK_SAME_KEY])
def test_tatp_lock_words_stay_and_held_keys_are_still_refused(flags):
    pair = [_engine(W.TATP, n_rows=2000, log_entries=1 << 16, flags=flags) for _ in range(2)]
    for x in pair:
        x.populate(2000)
    e, twin = pair
    existing = [e.dump_rows(t)[0] for t in range(5)]
    churn = _tatp_trace(existing, 3000, seed=31)
    assert e.submit(churn).tobytes() == twin.submit(churn).tobytes()
    live = [e.dump_rows(t)[0] for t in range(5)]
    acq = np.zeros(250, wire.TATP_MSG)
    acq["type"] = T.ACQUIRE_LOCK
    acq["table"] = np.arange(250) % 5
    acq["key"] = [live[t][(7 * i) % len(live[t])] for i, t in enumerate(acq["table"])]
    first = e.submit(acq)
    assert first.tobytes() == twin.submit(acq).tobytes()
    granted = first["type"] == T.GRANT_LOCK
    assert granted.sum() > 150
    locks = [[x.tobytes() for x in e.read_locks(t)] for t in range(5)]
    assert sum(np.count_nonzero(e.read_locks(t)[0]) for t in range(5)) > 0
    owners = _image(e)
    rep = _compacted(e)
    assert sum(r["buckets_rewritten"] for r in rep) > 0
    assert [[x.tobytes() for x in e.read_locks(t)] for t in range(5)] == locks
    assert e.state_digest() == twin.state_digest()
    if flags:  # the owner keys travel in the image's inline entries: the same bytes at the same place in every one
        def owner_keys(image):
            raw, hdr = np.frombuffer(image, np.uint8), np.frombuffer(image[:320], "<u8")
            out = []
            for t in range(5):  # table t of the header: {global size, buckets, overflow entries, rows, offset}; dir, then the inline entries
                n_b, off = int(hdr[8 + 5 * t + 1]), int(hdr[8 + 5 * t + 4])
                out.append(raw[off + 16 * n_b: off + 16 * n_b + 256 * n_b].reshape(n_b, 256)[:, 224:].tobytes())
            return out

        was = owner_keys(owners)
        assert owner_keys(_image(e)) == was and any(was[0]) and any(was[4])
    second, second_twin = e.submit(acq), twin.submit(acq)
    assert second.tobytes() == second_twin.tobytes()
    if not flags:
        assert (second["type"][granted] == T.REJECT_LOCK).all()  # still held
    rel = acq[granted].copy()
    rel["type"] = np.where(np.arange(len(rel)) % 2 == 0, int(T.COMMIT_PRIM), int(T.ABORT))
    rel["val"] = 7
    out = e.submit(rel)
    assert out.tobytes() == twin.submit(rel).tobytes()
    for t in range(5):
        assert not e.read_locks(t)[0].any() and not twin.read_locks(t)[0].any()
    assert e.state_digest() == twin.state_digest()
    e.close(); twin.close()


def test_smallbank_counters_stay_and_the_trace_goes_on_as_on_a_twin():
    from oracle import oracle as orc

    pair = [_engine(W.SMALLBANK, n_rows=5000, log_entries=1 << 16) for _ in range(2)]
    trace = tracegen.sb_random(8000, seed=9, n_acct_touch=300)
    reps = []
    for i, x in enumerate(pair):
        x.populate(5000)
        for t in range(2):
            k = np.sort(x.dump_rows(t)[0])
            _delete_rows(x, k[k >= 1000][t::3], table=t)  # accounts the trace never names: holes, freed entries
        r1 = x.submit(trace[:4000])
        if i == 0:
            locks = [[a.tobytes() for a in x.read_locks(t)] for t in range(2)]
            ex, sh = x.read_locks(0)
            assert ex.any() and sh.any()  # exclusive and shared counters outstanding
            rep = _compacted(x)
            assert sum(r["buckets_rewritten"] for r in rep) > 0 and sum(r["verify"]["free_entries"] + r["verify"]["pending_entries"] for r in rep) > 0
            assert [[a.tobytes() for a in x.read_locks(t)] for t in range(2)] == locks
            _packed(x)
        reps.append(np.concatenate([r1, x.submit(trace[4000:])]))
    e, twin = pair
    assert reps[0].tobytes() == reps[1].tobytes() == orc.SmallbankOracle(5000, log_entries=1 << 16).replay(trace).tobytes()
    assert e.state_digest() == twin.state_digest()
    assert [[a.tobytes() for a in e.read_locks(t)] for t in range(2)] == [[a.tobytes() for a in twin.read_locks(t)] for t in range(2)]
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 5. answers stay
def test_store_answers_stay_between_two_halves_of_a_trace():
    from oracle import oracle as orc

    pair = [_engine(W.STORE, n_rows=200, pool_entries=8192) for _ in range(2)]
    trace = tracegen.store_random(20_000, seed=6, n_sub_touch=200, p_set=0.4, p_insert=0.08)
    reps = []
    for i, x in enumerate(pair):
        x.populate(200)
        r1 = x.submit(trace[:10_000])
        if i == 0:
            (r,) = _compacted(x)
            _packed(x)
        reps.append(np.concatenate([r1, x.submit(trace[10_000:])]))
    assert reps[0].tobytes() == reps[1].tobytes() == orc.StoreOracle(200 * 18 // 4, 200).replay(trace).tobytes()
    assert pair[0].state_digest() == pair[1].state_digest() and pair[0].stats()["pool_exhausted"] == 0
    for x in pair:
        x.close()


def test_tatp_answers_stay_on_three_shards_each_compacted_mid_trace():
    from oracle import oracle as orc

    sets = [[_engine(W.TATP, n_rows=2000, log_entries=1 << 16, shard_index=s, shard_count=3) for s in range(3)] for _ in range(2)]
    for x in sets[0] + sets[1]:
        x.populate(2000)
    existing = [np.concatenate([x.dump_rows(t)[0] for x in sets[0]]) for t in range(5)]
    trace = _tatp_trace(existing, 6000, seed=21)
    hs = np.array([sets[0][0].hash_size(t) for t in range(5)], np.uint64)
    home = np.zeros(len(trace), np.int64)
    for t in range(5):
        m = trace["table"] == t
        home[m] = np_bucket(trace["key"][m], int(hs[t])).astype(np.int64) % 3
    half = len(trace) // 2
    reps = []
    for i, shards in enumerate(sets):
        rep = np.zeros_like(trace)
        for s, x in enumerate(shards):
            idx1, idx2 = np.nonzero(home[:half] == s)[0], half + np.nonzero(home[half:] == s)[0]
            rep[idx1] = x.submit(trace[idx1])
            if i == 0:
                out = _compacted(x)
                assert sum(r["buckets_rewritten"] for r in out) > 0
                _packed(x)
            rep[idx2] = x.submit(trace[idx2])
        reps.append(rep)
    assert reps[0].tobytes() == reps[1].tobytes()
    assert reps[0].tobytes() == orc.TatpOracle(2000, log_entries=1 << 16).replay(trace).tobytes()
    assert recovery.digest_sum(sets[0]) == recovery.digest_sum(sets[1])
    for x in sets[0] + sets[1]:
        assert x.stats()["pool_exhausted"] == 0
        x.close()


def test_a_read_of_a_key_with_a_duplicate_row_answers_the_same_row():
    e = _engine(W.STORE, n_rows=64, pool_entries=1024)
    hs = e.hash_size(0)

    def load(keys, tag, ver):
        e.load_rows(0, keys, np.full(len(keys), ver, "<u4"), _vals(keys, tag))

    a, b, c, d = _same_bucket_keys(hs, 5, 4, 10_000_000)
    load([a, b, c], 1, 1); load([a], 2, 2); load([d], 1, 1)  # [d] -> inline [a b c a']: a twice
    k = _same_bucket_keys(hs, 9, 8, 20_000_000)
    load(k[:4], 1, 1); load([k[4], k[0], k[5]], 2, 2); load([k[5]], 5, 5)
    _delete_rows(e, [k[4]])  # a hole in front of the copies
    load([k[6]], 4, 4); load([k[6], k[7]], 6, 6)
    keys = np.unique(e.dump_rows(0)[0])
    want, before = _store_read(e, keys), _dumps(e)
    assert len(keys) < len(e.dump_rows(0)[0])  # duplicates are there
    (r,) = _compacted(e)
    assert r["buckets_rewritten"] >= 1 and _dumps(e) == before
    assert _store_read(e, keys).tobytes() == want.tobytes()
    e.close()


# ---------------------------------------------------------------------------------------------- 6. pool head-room returns
def test_a_full_pool_has_room_again_after_a_compaction():
    cap = 64
    e = _engine(W.STORE, n_rows=64, pool_entries=cap)
    hs = e.hash_size(0)
    per = np.zeros(hs, np.int64)
    per[:cap] = 8        # 64 full buckets of 8 rows: one overflow entry each ...
    per[cap:cap + 40] = 8  # ... and 40 more for later
    keys = kvkeys.keys_by_bucket(hs, per, seed=8)
    b = np_bucket(keys, hs).astype(np.int64)
    first, later = keys[b < cap], keys[b >= cap]
    _store_insert(e, first, 1)
    (st,) = e.state_stats()
    assert st["pool_top"] == st["pool_cap"] == cap and e.stats()["pool_exhausted"] == 0
    _delete_rows(e, first[np_bucket(first, hs).astype(np.int64) >= 16])  # 48 of the 64 overflow entries are free now
    (dry,) = e.state_compact(dry_run=True)
    assert dry["pool_top_before"] == cap and dry["overflow_before"] == 16 and dry["verify"]["free_entries"] + dry["verify"]["pending_entries"] == 48
    (r,) = _compacted(e)
    assert r["pool_top_after"] == 16 and e.state_stats()[0]["pool_top"] == 16
    m = np.zeros(len(later), wire.STORE_MSG)  # ONE pass: 320 INSERTs, 40 overflow entries -- more than pool_cap - pool_top_before = 0, fewer than the 48 regained
    m["type"], m["key"], m["val"] = wire.Store.INSERT, later, _vals(later, 3)
    assert len(m) > cap - dry["pool_top_before"] and 40 <= cap - r["pool_top_after"]
    rep = e.submit(m)
    assert (rep["type"] == wire.Store.INSERT_ACK).all() and e.stats()["pool_exhausted"] == 0
    got = _store_read(e, later)
    assert (got["type"] == wire.Store.GRANT_READ).all() and (got["val"] == _vals(later, 3)).all()
    (v,) = e.state_verify()
    assert is_clean(v) and v["pool_top"] == 56 and v["linked"] == 56
    e.close()


# ---------------------------------------------------------------------------------------------- 7. refusals, a blank engine
def test_refusals():
    for e in (_engine(W.FASST, n_slots=1000), _engine(W.TPL, n_slots=1000), _engine(W.LOG, log_entries=1 << 10)):
        for dry in (False, True):
            with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
                e.state_compact(dry_run=dry)
        e.close()
    e = _engine(W.TATP, n_rows=100)
    out = (_lib.TableCompact * 5)()
    assert e._L.dint_state_compact(e._h, out, 4, 0, None) == EINVAL and b"room for" in e._L.dint_last_error()
    assert e._L.dint_state_compact(e._h, None, 5, 0, None) == EINVAL
    assert e._L.dint_state_compact(e._h, out, 5, 2, None) == EINVAL  # an unknown flag
    assert e._L.dint_state_compact(e._h, out, 5, 0, None) == 5 and out[4].verify.pool_cap == e.hash_size(4) // 4 + 4096
    e.close()


def test_refused_with_a_batch_announced_and_the_batch_is_still_answered():
    pair = [_engine(W.TATP, n_rows=2000, log_entries=1 << 16) for _ in range(2)]
    for x in pair:
        x.populate(2000)
    e, twin = pair
    existing = [e.dump_rows(t)[0] for t in range(5)]
    trace = _tatp_trace(existing, 3000, seed=50)
    n = len(trace) // 2
    a, b = _up(trace[:n]), _up(trace[n:2 * n])
    want = np.concatenate([twin.submit(trace[:n]), twin.submit(trace[n:2 * n])])
    e.submit_device(a, n, None, 0, ahead=(b, n, None))
    out = (_lib.TableCompact * 5)()
    for flags in (0, DRY):
        assert e._L.dint_state_compact(e._h, out, 5, flags, None) == ESTATE and b"announced" in e._L.dint_last_error()
    e.submit_device(b, n)
    e.sync()
    got = np.concatenate([np.frombuffer(x.cpu().numpy().tobytes(), wire.TATP_MSG) for x in (a, b)])
    assert got.tobytes() == want.tobytes() and e.state_digest() == twin.state_digest()  # nothing changed, and the batch was answered
    assert _dumps(e) == _dumps(twin)
    _compacted(e)
    assert _dumps(e) == _dumps(twin)
    e.close(); twin.close()


@pytest.mark.parametrize("wl", [W.STORE, W.TATP, W.SMALLBANK])
def test_a_blank_engine_stays_blank(wl):
    kw = dict(n_rows=64) if wl == W.STORE else dict(n_rows=64, log_entries=1 << 12)
    e = _engine(wl, **kw)
    for dry in (True, False, False):
        rep = e.state_compact(dry_run=dry)
        assert len(rep) == NTAB[wl]
        for t, r in enumerate(rep):
            assert r["verify"]["pool_cap"] == e.hash_size(t) // 4 + 4096
            assert all(r[k] == 0 for k in CFIELDS) and all(v == 0 for k, v in r["verify"].items() if k != "pool_cap"), r
    twin = _engine(wl, **kw)
    twin.populate(50)
    buf, n, st = twin.state_export(0, 1)
    assert e.state_import(buf, n)["rows"] == st["rows"] > 0  # the import's own rule says it was blank
    assert e.state_digest() == twin.state_digest()
    e.close(); twin.close()


# ---------------------------------------------------------------------------------------------- 8. snapshot and restore
def test_a_snapshot_taken_before_a_compaction_restores_the_engine_whole():
    e, keys = _churned_store()
    image, dumps, (v0,), (s0,) = _image(e), _dumps(e), e.state_verify(), e.state_stats()
    e.snapshot()
    (r,) = _compacted(e)
    assert r["buckets_rewritten"] > 0 and _image(e) != image
    e.restore()
    assert _image(e) == image and _dumps(e) == dumps and e.state_verify() == [v0] and e.state_stats() == [s0]  # pool_top and the lists too
    fresh = tracegen.store_key(5_000_000 + np.arange(300), 2, 0)
    _store_insert(e, fresh, 7)  # the restored lists and pool_top are used on
    (v,) = e.state_verify()
    assert is_clean(v) and v["unaccounted"] == 0 and (_store_read(e, fresh)["type"] == wire.Store.GRANT_READ).all()
    e.close()


# ---------------------------------------------------------------------------------------------- 9. more buckets than one stride covers
def test_a_table_of_more_buckets_than_2048_workgroups_cover():
    e = _engine(W.STORE, n_rows=120_000)
    assert e.hash_size(0) > 2048 * 256  # the scan crosses workgroups and every kernel's stride loops
    rng = np.random.default_rng(12)
    keys = np.unique(rng.integers(1, 1 << 40, 1_400_000, dtype=np.uint64))
    keys = keys[rng.permutation(len(keys))]
    e.load_rows(0, keys, np.arange(len(keys), dtype="<u4"), _vals(keys, 1))
    _delete_rows(e, keys[::3])
    before, digest = _dumps(e), e.state_digest()
    (st0,) = e.state_stats()
    (r,) = _compacted(e)
    print({k: r[k] for k in CFIELDS})
    assert _dumps(e) == before and e.state_digest() == digest
    assert r["rows"] == st0["rows"] and r["holes_before"] == st0["holes"] and r["overflow_before"] == st0["overflow_entries"] > r["overflow_after"] > 256
    assert r["buckets_rewritten"] > 2048 and r["pool_top_before"] == st0["pool_top"]
    _packed(e)
    e.close()


# ---------------------------------------------------------------------------------------------- 10. the advice
def test_compact_tables_and_compact_advice_on_a_three_shard_tatp_set():
    shards = [_engine(W.TATP, n_rows=2000, log_entries=1 << 16, shard_index=s, shard_count=3, pool_entries=600) for s in range(3)]
    for x in shards:
        x.populate(2000)
    assert recovery.compact_advice(shards)["action"] == "none"
    fresh = np.arange(2_000_000, 2_004_200, dtype=np.uint64) | np.uint64(3 << 32) | np.uint64(16 << 40)  # CALL_FORWARDING rows that come and go
    home = np_bucket(fresh, shards[0].hash_size(4)).astype(np.int64) % 3
    for op, ack in ((T.INSERT_BCK, T.INSERT_BCK_ACK), (T.DELETE_BCK, T.DELETE_BCK_ACK)):
        for s, x in enumerate(shards):
            m = np.zeros(int((home == s).sum()), wire.TATP_MSG)
            m["type"], m["table"], m["key"] = op, 4, fresh[home == s]
            assert (x.submit(m)["type"] == ack).all()
    assert all(x.stats()["pool_exhausted"] == 0 for x in shards)
    a, r = recovery.compact_advice(shards, max_pool_top_fill=0.5), recovery.rehash_advice(shards)
    print({k: a[k] for k in ("action", "hole_share", "pool_top_fill", "pool_top_fill_after", "load")})
    assert a["pool_top_fill"] > 0.5 > a["pool_top_fill_after"] and max(a["load"]) < 4.0  # churned but not overloaded, or the case is void
    assert a["action"] == "compact" and a["n_rows"] == r["n_rows"] and a["load"] == r["load"]
    dry = recovery.compact_tables(shards, dry_run=True)
    assert a["compact"] == dry["tables"] and len(dry["engines"]) == 3
    digest = recovery.digest_sum(shards)
    done = recovery.compact_tables(shards)
    for t in range(5):
        for k in CFIELDS:
            assert done["tables"][t][k] == dry["tables"][t][k] == sum(p[t][k] for p in done["engines"])
    assert recovery.digest_sum(shards) == digest and recovery.verify_tables(shards)["clean"]
    assert recovery.compact_advice(shards, max_pool_top_fill=0.5)["action"] == "none"
    for x in shards:
        x.close()
    # overloaded: five times the rows the bucket count was made for
    small = [_engine(W.TATP, n_rows=400, log_entries=1 << 12, shard_index=s, shard_count=3, pool_entries=8192) for s in range(3)]
    for x in small:
        x.populate(2000)
    a, r = recovery.compact_advice(small), recovery.rehash_advice(small)
    assert a["action"] == "rehash" and r["needed"] and a["n_rows"] == r["n_rows"] > 400
    for x in small:
        x.close()
