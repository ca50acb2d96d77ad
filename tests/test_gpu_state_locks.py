"""The lock units a server holds listed from the GPU and orphaned ones released (include/dint_abi.h dint_state_locks /
dint_state_unlock, dint_amd/csrc/k_locks_state.hip, dint_amd/recovery.py held_locks / release_locks).  The lists are held to a
numpy form over read_locks and dump_rows with the fasthash of tests/shard_double.py, to the CPU oracle's own lock arrays, and to
the host form over the engine's downloaded own image; the releases to a twin engine that got the matching release REQUESTS, and
to the oracle's replies afterwards.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import shardsplit as ss
import tracegen
from dint_amd import _lib, recovery, wire
from oracle import oracle as orc
from shard_double import fasthash_key, fasthash_lid
from test_state_locks_host import KEY_OWNER, KEY_ROW, REC, host_first_bad, host_locks

W, F, P, T, S = wire.Workload, wire.Fasst, wire.Tpl, wire.Tatp, wire.Sb
EINVAL, ESTATE = -1, -5
LOCKS, KV = (W.FASST, W.TPL), (W.TATP, W.SMALLBANK)
ALL = LOCKS + KV
NTAB = {W.FASST: 1, W.TPL: 1, W.TATP: 5, W.SMALLBANK: 2}
N_ROWS = 64
pytestmark = pytest.mark.gpu


def _engine(*a, **kw):
    from dint_amd.engine import Engine

    return Engine(*a, **kw)


def mk(wl, H=1, i=0, n_slots=1000, n_rows=N_ROWS, flags=0, populate=True):
    if wl in LOCKS:
        return _engine(wl, n_slots=n_slots, shard_index=i, shard_count=H, flags=flags)
    e = _engine(wl, n_rows=n_rows, log_entries=1 << 12, shard_index=i, shard_count=H, flags=flags, pool_entries=4096)
    if populate:
        e.populate(n_rows)
    return e


def mk_oracle(wl, n_slots=1000, n_rows=N_ROWS, same_key=False):
    if wl == W.FASST:
        return orc.FasstOracle(n_slots)
    if wl == W.TPL:
        return orc.TplOracle(n_slots)
    if wl == W.TATP:
        o = orc.TatpOracle(n_rows, log_entries=1 << 12)
        if same_key:
            o.same_key_mode()
        return o
    return orc.SmallbankOracle(n_rows, log_entries=1 << 12)


def sizes(wl, o, n_slots=1000):
    return [n_slots] if wl in LOCKS else [int(o.hash_size(t)) for t in range(NTAB[wl])]


def trace(wl, n, seed, o, formed=False, n_slots=1000):
    """a random trace; formed: without the RELEASEs of lock_2pl / smallbank that find their counter at 0 (the reference lets it wrap
    to 2^32 - 1 -- the listing takes such counters, but no twin can be sent that many release requests)"""
    if wl == W.FASST:
        return tracegen.fasst_random(n, seed=seed, n_hot=48, key_space=4000, p_hot=0.5)
    if wl == W.TATP:
        return tracegen.tatp_random(n, [o.dump(t)[0] for t in range(5)], seed=seed, n_sub_touch=40)
    if wl == W.TPL:
        m = tracegen.tpl_random(n, seed=seed, n_hot=48, key_space=4000, p_hot=0.5)
        unit = (fasthash_lid(np.ascontiguousarray(m["lid"], "<u4")) % np.uint64(n_slots)).astype(np.int64)
        acq, rel, excl = m["action"] == P.ACQUIRE_LOCK, m["action"] == P.RELEASE_LOCK, m["type"] == P.EXCLUSIVE
    else:
        m = tracegen.sb_random(n, seed=seed, n_acct_touch=40)
        hs = np.array([o.hash_size(t) for t in range(2)], np.uint64)[m["table"]]
        unit = (fasthash_key(np.ascontiguousarray(m["key"], "<u8")) % (np.uint64(4) * hs)).astype(np.int64) * 2 + m["table"]
        acq, rel = m["type"] <= S.ACQUIRE_EXCLUSIVE, (m["type"] == S.RELEASE_SHARED) | (m["type"] == S.RELEASE_EXCLUSIVE)
        excl = (m["type"] == S.ACQUIRE_EXCLUSIVE) | (m["type"] == S.RELEASE_EXCLUSIVE)
    if not formed:
        return m
    keep, cnt = np.ones(n, bool), {}
    for i in range(n):
        ex, sh = cnt.get(int(unit[i]), (0, 0))
        if acq[i]:
            if excl[i] and ex == 0 and sh == 0:
                ex = 1
            elif not excl[i] and ex == 0:
                sh += 1
        elif rel[i]:
            if (ex if excl[i] else sh) == 0:
                keep[i] = False
            elif excl[i]:
                ex -= 1
            else:
                sh -= 1
        cnt[int(unit[i])] = (ex, sh)
    return m[keep]


def same_replies(wl, got, want):
    name = {W.TATP: "tatp", W.SMALLBANK: "smallbank"}.get(wl)
    if name:  # (bytes of populated rows the reference never assigns)
        got, want = orc.mask_populate_garbage(name, got), orc.mask_populate_garbage(name, want)
    return got.tobytes() == want.tobytes()


def oracle_words(wl, o, t):
    if wl == W.FASST:
        return np.array(o.locks), np.array(o.vers)
    if wl == W.TPL:
        return np.array(o.num_ex), np.array(o.num_sh)
    if wl == W.TATP:
        a = np.array(o.locks(t)).astype("<u4")
        return a, np.zeros_like(a)
    return np.array(o.num_ex(t)), np.array(o.num_sh(t))


# ------------------------------------------------------------------------------------------------ the numpy form
def np_list(wl, tables, H=1, i=0, owner=None):
    """tables: per table (a, b, keys of the shard's rows in dump order or None, global size) with a, b as read_locks numbers them.
    owner: {(table, slot): key} on a DINT_FLAG_LOCK_SAME_KEY engine"""
    recs, st = [], {"total": 0, "held": [0] * 5, "sum_a": 0, "sum_b": 0, "no_row": 0, "walk_cut": 0}
    for t, (a, b, keys, size) in enumerate(tables):
        held = (a != 0) if wl == W.FASST else ((a != 0) | (b != 0))
        if wl in LOCKS:
            for s in np.flatnonzero(held):
                recs.append((int(s), int(a[s]), int(b[s]), 0, 0, t, 0, 0))
            continue
        nl = len(a) // 4
        lh = fasthash_key(np.ascontiguousarray(keys, "<u8")) % np.uint64(4 * size)
        for l in range(nl):
            for q in range(4):
                s = q * nl + l
                if not held[s]:
                    continue
                cand = keys[lh == np.uint64(q * size + l * H + i)]
                key, fl = (int(cand[0]), KEY_ROW) if len(cand) else (0, 0)
                if owner is not None:
                    key, fl = owner[(t, s)], KEY_OWNER
                st["no_row"] += len(cand) == 0
                recs.append((s, int(a[s]), int(b[s]), key, len(cand), t, fl, 0))
    for r in recs:
        st["total"] += 1
        st["held"][r[5]] += 1
        st["sum_a"] += r[1]
        st["sum_b"] += r[2]
    return (np.array(recs, REC) if recs else np.zeros(0, REC)), st


def engine_tables(e):
    out = []
    for t in range(NTAB[e.workload]):
        a, b = e.read_locks(t)
        kv = e.workload in KV
        out.append((a, b, e.dump_rows(t)[0] if kv else None, e.hash_size(t) if kv else 0))
    return out


def listing(e):
    from dint_amd.engine import lock_records

    buf, n, st = e.state_locks()
    assert n == st["total"]
    return lock_records(buf, n), st, buf


def image_of(e):
    buf, n, _ = e.state_export(e.shard_index, e.shard_count)
    return buf[:n].cpu().numpy()


def check(e, owner=None):
    """the device list of `e` against the numpy form over read_locks / dump_rows and against the host form over its own image;
    returns (records, stats, device buffer)"""
    r, st, buf = listing(e)
    want, wst = np_list(e.workload, engine_tables(e), e.shard_count, e.shard_index, owner)
    assert r.tobytes() == want.tobytes(), (r, want)
    assert st == wst
    n, hr, hst = host_locks(image_of(e))
    assert n == len(r) and hr.tobytes() == r.tobytes() and hst == st
    if e.workload in KV:
        assert [d["locks_held"] for d in e.state_stats()] == st["held"][:NTAB[e.workload]]
    return r, st, buf


def up(rec, e):
    import torch

    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).copy()).to(e._torch_device())


# ------------------------------------------------------------------------------------------------ requests on units
def lids_by_slot(n_slots):
    """lid[s] hashes to slot s"""
    lid = np.arange(1, 40 * n_slots + 4000, dtype="<u4")
    slot = (fasthash_lid(lid) % np.uint64(n_slots)).astype(np.int64)
    first = np.full(n_slots, -1, np.int64)
    first[slot[::-1]] = lid[::-1]
    assert (first >= 0).all()
    return first.astype("<u4")


def keys_by_lock_hash(size, per=1, start=1 << 33):
    """key[h][k] hashes to lock slot h of a table of `size` buckets (keys no population holds)"""
    c = np.arange(start, start + 400 * size * per + 40_000, dtype="<u8")
    lh = (fasthash_key(c) % np.uint64(4 * size)).astype(np.int64)
    out = []
    for h in range(4 * size):
        hit = c[lh == h]
        assert len(hit) >= per
        out.append(hit[:per])
    return np.array(out, "<u8")


def acquire(wl, keys, table=0, shared=False):
    m = np.zeros(len(keys), wire.MSG_DTYPE[wl])
    if wl == W.FASST:
        m["type"], m["lid"] = F.ACQUIRE_LOCK, keys
    elif wl == W.TPL:
        m["action"], m["type"], m["lid"] = P.ACQUIRE_LOCK, (P.SHARED if shared else P.EXCLUSIVE), keys
    elif wl == W.TATP:
        m["type"], m["table"], m["key"] = T.ACQUIRE_LOCK, table, keys
    else:
        m["type"], m["table"], m["key"] = (S.ACQUIRE_SHARED if shared else S.ACQUIRE_EXCLUSIVE), table, keys
    return m


def releases(wl, units):
    """the release requests of units [(table, key, a, b)]: ABORT per key, num_ex / num_sh RELEASEs"""
    rows = []
    for t, k, a, b in units:
        if wl == W.FASST:
            rows.append((F.ABORT, 0, k))
        elif wl == W.TATP:
            rows.append((T.ABORT, t, k))
        elif wl == W.TPL:
            rows += [(P.EXCLUSIVE, 0, k)] * a + [(P.SHARED, 0, k)] * b
        else:
            rows += [(S.RELEASE_EXCLUSIVE, t, k)] * a + [(S.RELEASE_SHARED, t, k)] * b
    m = np.zeros(len(rows), wire.MSG_DTYPE[wl])
    if rows:
        ty, tb, k = (np.array(x) for x in zip(*rows))
        m["type"] = ty
        if wl in LOCKS:
            m["lid"] = k
        else:
            m["table"], m["key"] = tb, k
        if wl == W.TPL:
            m["action"] = P.RELEASE_LOCK
    return m


def unit_keys(wl, req, sz):
    """{(table, unsharded slot): a key of the trace that hashes there}"""
    if wl in LOCKS:
        s = (fasthash_lid(np.ascontiguousarray(req["lid"], "<u4")) % np.uint64(sz[0])).astype(np.int64)
        return {(0, int(x)): int(k) for x, k in zip(s, req["lid"])}
    ok = req["table"] < len(sz)
    hs = np.array(sz, np.uint64)[np.minimum(req["table"], len(sz) - 1)]
    s = (fasthash_key(np.ascontiguousarray(req["key"], "<u8")) % (np.uint64(4) * hs)).astype(np.int64)
    return {(int(t), int(x)): int(k) for t, x, k, o in zip(req["table"], s, req["key"], ok) if o}


def release_requests(wl, rec, keymap):
    return releases(wl, [(int(r["table"]), keymap[(int(r["table"]), int(r["slot"]))], int(r["a"]), int(r["b"])) for r in rec])


@pytest.fixture(scope="module")
def traced():
    """per workload: an unsharded engine and the oracle after one random trace, with the trace"""
    made = {}

    def get(wl):
        if wl not in made:
            o = mk_oracle(wl)
            req = trace(wl, 3000, 41, o, formed=True)
            e = mk(wl)
            assert same_replies(wl, e.submit(req), o.replay(req))
            made[wl] = (e, o, req)
        return made[wl]

    yield get
    for e, _, _ in made.values():
        e.close()


def twin_of(wl, req, **kw):
    e = mk(wl, **kw)
    e.submit(req)
    return e


# ---------------------------------------------------------------------------------------------- 1. nothing held
@pytest.mark.parametrize("wl", ALL)
def test_nothing_held_and_a_blank_engine_stays_blank(wl):
    src = mk(wl)
    blank = mk(wl, populate=False)
    for e in (blank, src):
        r, st, _ = check(e)
        assert len(r) == 0 and st == {"total": 0, "held": [0] * 5, "sum_a": 0, "sum_b": 0, "no_row": 0, "walk_cut": 0}
        assert e.state_unlock(all=True) == {"released": 0, "stale": 0, "released_a": 0, "released_b": 0, "per_table": [0] * 5}
    buf, n, _ = src.state_export(0, 1)
    blank.state_import(buf, n)  # still blank: the listing and the empty sweep changed no gate
    assert image_of(blank).tobytes() == image_of(src).tobytes()
    if wl in KV:
        fresh = mk(wl, populate=False)
        check(fresh)
        assert fresh.populate_device(N_ROWS)["direct"] == 1  # the freshness gate of the direct load as well
        fresh.close()
    src.close(); blank.close()


# ---------------------------------------------------------------------------------------------- 2. after a random trace
@pytest.mark.parametrize("wl,H,n_slots", [(W.FASST, 1, 1), (W.FASST, 1, 257), (W.FASST, 1, 1000), (W.FASST, 3, 1000), (W.TPL, 1, 1), (W.TPL, 1, 257),
                                          (W.TPL, 1, 1000), (W.TPL, 3, 1000), (W.TATP, 1, 0), (W.TATP, 3, 0), (W.SMALLBANK, 1, 0), (W.SMALLBANK, 3, 0)])
def test_listing_after_a_random_trace(wl, H, n_slots):
    o = mk_oracle(wl, n_slots=n_slots)
    req = trace(wl, 3000, 7 + H, o, n_slots=n_slots)
    sz = sizes(wl, o, n_slots)
    hm = ss.home(wl, req, sz, H)
    o.replay(req)
    total = 0
    for i in range(H):
        e = mk(wl, H, i, n_slots=n_slots)
        e.submit(req[hm == i])
        r, st, _ = check(e)
        tabs = []
        for t in range(NTAB[wl]):  # ... and the oracle's own arrays, projected onto the shard
            a, b = oracle_words(wl, o, t)
            if wl in LOCKS:
                a, b = ss.project_slots(a, b, n_slots, i, H)
                tabs.append((a, b, None, 0))
            else:
                keys = ss.project_rows(o.dump(t), sz[t], i, H)[0]
                tabs.append((ss.project_kv_locks(a, sz[t], i, H), ss.project_kv_locks(b, sz[t], i, H), keys, sz[t]))
        want, wst = np_list(wl, tabs, H, i)
        assert r.tobytes() == want.tobytes() and st == wst
        assert st["total"] == sum(st["held"]) == len(r) and st["sum_a"] == int(r["a"].sum()) and st["sum_b"] == int(r["b"].sum())
        total += st["total"]
        e.close()
    assert n_slots == 1 or total > 20  # or the case is void


# ---------------------------------------------------------------------------------------------- 3. cap and alignment
@pytest.mark.parametrize("wl", [W.FASST, W.TATP])
def test_cap_count_only_guard_bytes_and_alignment(wl, traced):
    import torch

    e, _, _ = traced(wl)
    full, st, _ = listing(e)
    n = len(full)
    assert n > 8
    for cap in (0, 1, n // 2, n - 1, n, n + 5):
        guard = torch.full((32 * (n + 8) + 64,), 0xA5, dtype=torch.uint8, device=e._torch_device())
        s = _lib.LockStats()
        body = guard[32:]
        got = _lib.check(e._L.dint_state_locks(e._h, body.data_ptr(), cap, C.byref(s), None))
        assert got == min(cap, n) and s.as_dict() == st
        h = guard.cpu().numpy()
        assert h[32:32 + 32 * got].tobytes() == full[:got].tobytes()
        assert (h[:32] == 0xA5).all() and (h[32 + 32 * got:] == 0xA5).all()
    s = _lib.LockStats()
    assert e._L.dint_state_locks(e._h, None, 0, C.byref(s), None) == 0 and s.total == n  # count only
    assert e._L.dint_state_locks(e._h, None, 4, C.byref(s), None) == EINVAL
    buf = torch.zeros(32 * n + 64, dtype=torch.uint8, device=e._torch_device())
    for off in (1, 4):
        assert e._L.dint_state_locks(e._h, buf.data_ptr() + off, n, C.byref(s), None) == EINVAL and b"aligned" in e._L.dint_last_error()
        assert e._L.dint_state_unlock(e._h, buf.data_ptr() + off, 1, 0, None, None) == EINVAL
    assert _lib.check(e._L.dint_state_locks(e._h, buf.data_ptr() + 8, n, C.byref(s), None)) == n  # 8-byte aligned is enough
    assert buf.cpu().numpy()[8:8 + 32 * n].tobytes() == full.tobytes()


# ---------------------------------------------------------------------------------------------- 4. ranks across waves and workgroups
@pytest.mark.parametrize("wl", ALL)
@pytest.mark.parametrize("which", ["every_unit", "last_unit"])
def test_ranks_across_waves_and_workgroups(wl, which):
    e = mk(wl, n_slots=1000, n_rows=768, populate=False)  # 1000 slots / 288 buckets in table 0: more than one workgroup, no multiple of 256
    if wl in LOCKS:
        keys = lids_by_slot(1000)
        units = 1000
    else:
        assert e.hash_size(0) == 288
        keys = keys_by_lock_hash(288)[:, 0]
        units = 4 * 288
    pick = keys if which == "every_unit" else keys[-1:]
    rep = e.submit(acquire(wl, pick))
    assert len(set(rep["type"].tolist())) == 1  # every one granted
    r, st, _ = check(e)
    if which == "every_unit":
        assert len(r) == units and (r["a"] == 1).all()
        if wl in KV:
            assert (r["slot"] == (np.arange(units) % 4) * 288 + np.arange(units) // 4).all() and st["no_row"] == units  # bucket-major, then q
        else:
            assert (r["slot"] == np.arange(units)).all()
    else:
        assert r["slot"].tolist() == [units - 1] and st["held"][0] == 1
    e.close()


# ---------------------------------------------------------------------------------------------- 5. lock_fasst versions
def test_fasst_versions_alone_hold_nothing_and_survive_a_release(traced):
    e, o, _ = traced(W.FASST)
    lock, ver = e.read_locks()
    assert ((ver != 0) & (lock == 0)).sum() > 20 and ((ver != 0) & (lock != 0)).sum() > 5  # or the case is void
    r, _, buf = check(e)
    assert set(r["slot"].tolist()) == set(np.flatnonzero(lock).tolist()) and (r["b"] == ver[r["slot"].astype(np.int64)]).all()
    tw = twin_of(W.FASST, traced(W.FASST)[2])
    assert tw.state_unlock(buf, len(r))["released"] == len(r)
    l2, v2 = tw.read_locks()
    assert not l2.any() and (v2 == ver).all()
    tw.close()


# ---------------------------------------------------------------------------------------------- 6. candidates
def _vals(e, n):
    return np.full((n, e.val_size), 7, np.uint8)


@pytest.mark.parametrize("wl", KV)
def test_candidates_in_an_overflowing_bucket(wl):
    e = mk(wl, populate=False)
    ntab = 1 if wl == W.TATP else 2
    for t in range(ntab):
        hs, g = e.hash_size(t), 5 + t
        k = keys_by_lock_hash(hs, per=6, start=(1 << 33) + t * (1 << 20))
        u = lambda q, j: int(k[q * hs + g][j])  # noqa: E731  key j of unit (bucket g, q)
        rows = [u(0, 0), u(0, 1), u(1, 0), u(1, 1), u(1, 2), u(0, 2), u(3, 0), u(1, 0), u(0, 3), u(1, 3)]  # ten rows, u(1, 0) twice: three entries
        e.load_rows(t, np.array(rows, "<u8"), np.arange(len(rows), dtype="<u4"), _vals(e, len(rows)))
        if wl == W.TATP:  # a deleted row leaves a hole that is not counted
            m = np.zeros(1, wire.TATP_MSG)
            m["type"], m["table"], m["key"] = T.DELETE_PRIM, t, u(0, 1)
            assert e.submit(m)["type"][0] == T.DELETE_PRIM_ACK
        e.submit(acquire(wl, [u(0, 0), u(1, 0), u(2, 0), u(3, 1)], table=t))  # a row; a key held twice; no row at all; a unit whose row is another key's
        other = keys_by_lock_hash(hs, start=1 << 36)[:, 0]
        e.submit(acquire(wl, [other[2 * hs + g + 1]], table=t))  # ... and a unit of a bucket without rows
    r, st, _ = check(e)
    for t in range(ntab):
        hs, g = e.hash_size(t), 5 + t
        mine = r[r["table"] == t]
        assert mine["slot"].tolist() == [0 * hs + g, 1 * hs + g, 2 * hs + g, 3 * hs + g, 2 * hs + g + 1]
        assert mine["cand_rows"].tolist() == [3 if wl == W.TATP else 4, 5, 0, 1, 0]
        assert mine["flags"].tolist() == [KEY_ROW, KEY_ROW, 0, KEY_ROW, 0] and mine["key"][2] == 0
        dump = e.dump_rows(t)[0]
        lh = fasthash_key(dump) % np.uint64(4 * hs)
        assert mine["key"][1] == dump[lh == np.uint64(hs + g)][0]  # the first in chain order
    assert st["no_row"] == 2 * ntab and st["walk_cut"] == 0
    e.close()


# ---------------------------------------------------------------------------------------------- 7. DINT_FLAG_LOCK_SAME_KEY
def test_same_key_records_carry_the_owner_and_a_changed_key_is_stale():
    e = mk(W.TATP, flags=_lib.FLAG_LOCK_SAME_KEY)
    keys = e.dump_rows(2)[0][:12]
    rep = e.submit(acquire(W.TATP, keys, table=2))
    granted = keys[rep["type"] == T.GRANT_LOCK]
    assert len(granted) >= 8
    hs = e.hash_size(2)
    owner = {(2, int(h)): int(k) for h, k in zip(fasthash_key(granted) % np.uint64(4 * hs), granted)}
    r, st, _ = check(e, owner)
    assert len(r) == len(granted) and (r["flags"] == KEY_OWNER).all() and set(r["key"].tolist()) == set(granted.tolist())
    bent = r.copy()
    bent["key"][1] ^= 1
    bent["key"][4] += 2
    image = image_of(e)
    assert e.state_unlock(up(bent, e), len(bent), dry_run=True)["stale"] == 2 and image_of(e).tobytes() == image.tobytes()
    u = e.state_unlock(up(bent, e), len(bent))
    assert u["stale"] == 2 and u["released"] == len(r) - 2 and u["per_table"] == [0, 0, len(r) - 2, 0, 0]
    left, _, _ = check(e, owner)
    assert left.tobytes() == r[[1, 4]].tobytes()
    e.close()


# ---------------------------------------------------------------------------------------------- 9. release of the full list
@pytest.mark.parametrize("wl", ALL)
def test_release_of_the_full_list_equals_the_release_requests(wl, traced):
    _, o0, req = traced(wl)
    sz = sizes(wl, o0)
    a, b = twin_of(wl, req), twin_of(wl, req)
    r, st, buf = check(a)
    assert len(r) > 20
    u = a.state_unlock(buf, len(r))
    assert u["released"] == len(r) and u["stale"] == 0 and u["released_a"] == st["sum_a"] and u["per_table"] == st["held"]
    assert u["released_b"] == (0 if wl == W.FASST else st["sum_b"])
    assert len(check(a)[0]) == 0
    rel = release_requests(wl, r, unit_keys(wl, req, sz))
    b.submit(rel)
    assert image_of(a).tobytes() == image_of(b).tobytes()
    o = mk_oracle(wl)  # a following pass is answered as the oracle answers it after the same releases
    o.replay(req); o.replay(rel)
    nxt = trace(wl, 2000, 99, mk_oracle(wl))
    assert same_replies(wl, a.submit(nxt), o.replay(nxt))
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 10. a partial list
@pytest.mark.parametrize("wl", ALL)
def test_every_third_record_frees_exactly_those_units(wl, traced):
    _, _, req = traced(wl)
    e = twin_of(wl, req)
    r, _, _ = check(e)
    part = r[::3]
    u = e.state_unlock(up(part, e), len(part))
    assert u["released"] == len(part) and u["stale"] == 0
    left, _, _ = check(e)
    keep = np.ones(len(r), bool)
    keep[::3] = False
    assert left.tobytes() == r[keep].tobytes()
    e.close()


def test_two_of_the_four_units_of_one_tatp_bucket():
    e = mk(W.TATP)
    hs, g = e.hash_size(0), 3
    k = keys_by_lock_hash(hs)[:, 0]
    e.submit(acquire(W.TATP, [k[q * hs + g] for q in range(4)] + [k[g + 1]]))
    r, _, _ = check(e)
    assert r["slot"].tolist() == [g, hs + g, 2 * hs + g, 3 * hs + g, g + 1]
    u = e.state_unlock(up(r[1:3], e), 2)
    assert u["released"] == 2
    assert check(e)[0].tobytes() == r[[0, 3, 4]].tobytes()  # q = 0 and q = 3 stay held: a byte store each, not the word
    e.close()


# ---------------------------------------------------------------------------------------------- 11. stale
@pytest.mark.parametrize("wl", ALL)
def test_stale_records_are_counted_and_their_units_left_alone(wl, traced):
    _, o0, req = traced(wl)
    sz = sizes(wl, o0)
    e = twin_of(wl, req)
    r, _, _ = check(e)
    km = unit_keys(wl, req, sz)
    e.submit(release_requests(wl, r[[2, 5]], km))  # two units released by requests since the listing: free by now ...
    want = None
    if wl in (W.TPL, W.SMALLBANK):  # ... and one of them taken again with another count: shared twice (three times, had it been twice)
        key, k = km[(int(r["table"][5]), int(r["slot"][5]))], 3 if (int(r["a"][5]), int(r["b"][5])) == (0, 2) else 2
        e.submit(acquire(wl, [key] * k, table=int(r["table"][5]), shared=True))
        want = (0, k)
    u = e.state_unlock(up(r, e), len(r))
    assert u["stale"] == 2 and u["released"] == len(r) - 2
    left, _, _ = check(e)
    if want:  # untouched
        assert len(left) == 1 and (int(left["a"][0]), int(left["b"][0])) == want and left["slot"][0] == r["slot"][5]
    else:  # (a lock byte has one value: taken again it would be the record's {a, b} and released)
        assert len(left) == 0
    e.close()


# ---------------------------------------------------------------------------------------------- 12. dry run, DINT_UNLOCK_ALL
@pytest.mark.parametrize("wl", ALL)
def test_dry_run_writes_nothing_and_the_sweep_equals_the_list(wl, traced):
    _, _, req = traced(wl)
    a, b = twin_of(wl, req), twin_of(wl, req)
    r, st, buf = check(a)
    image = image_of(a)
    d1, d2 = a.state_unlock(buf, len(r), dry_run=True), a.state_unlock(all=True, dry_run=True)
    assert d1 == d2 and d1["released"] == len(r) and image_of(a).tobytes() == image.tobytes()
    assert a.state_unlock(buf, len(r)) == d1 and b.state_unlock(all=True) == d1
    assert image_of(a).tobytes() == image_of(b).tobytes() and len(check(b)[0]) == 0
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 13. refusals
@pytest.mark.parametrize("wl", ALL)
def test_a_refused_list_leaves_the_image_and_names_the_first_bad_record(wl, traced):
    _, _, req = traced(wl)
    e = twin_of(wl, req)
    r, _, _ = check(e)
    image = image_of(e)
    geom = (0, 1, [1000] if wl in LOCKS else [e.hash_size(t) for t in range(NTAB[wl])])
    lists = []
    x = r.copy(); x["table"][4] = NTAB[wl]; lists.append(x)
    x = r.copy(); x["slot"][len(r) - 1] = 1 << 40; lists.append(x)
    x = r.copy(); x[[6, 7]] = x[[7, 6]]; lists.append(x)
    x = r.copy(); x[3] = x[2]; lists.append(x)
    x = r.copy(); x["a"][9] = 0; x["b"][9] = 0; lists.append(x)
    for x in lists:
        bad = host_first_bad(wl, geom, x)
        assert bad < len(x)
        for flags in (0, _lib.UNLOCK_DRY_RUN):
            assert e._L.dint_state_unlock(e._h, up(x, e).data_ptr(), len(x), flags, None, None) == EINVAL
            assert f"record {bad}:".encode() in e._L.dint_last_error()
        assert image_of(e).tobytes() == image.tobytes()
    L, d = e._L, up(r, e)
    assert L.dint_state_unlock(e._h, d.data_ptr(), len(r), 4, None, None) == EINVAL  # an unknown flag
    assert L.dint_state_unlock(e._h, d.data_ptr(), len(r), _lib.UNLOCK_ALL, None, None) == EINVAL
    assert L.dint_state_unlock(e._h, None, 3, 0, None, None) == EINVAL
    assert L.dint_state_unlock(e._h, d.data_ptr(), (1 << 32) - 16, 0, None, None) == EINVAL
    assert image_of(e).tobytes() == image.tobytes()
    assert e.state_unlock(d, len(r))["released"] == len(r)  # and the good list goes through
    e.close()


def test_engines_without_lock_units_and_a_pending_announcement():
    import torch

    for e in (_engine(W.STORE, n_rows=64), _engine(W.LOG, log_entries=1 << 10)):
        for call in (e.state_locks, lambda: e.state_unlock(all=True)):
            with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:.*no lock table"):
                call()
        e.close()
    e = mk(W.SMALLBANK)
    keys = e.dump_rows(0)[0]
    req = [acquire(W.SMALLBANK, keys[:20]), acquire(W.SMALLBANK, keys[20:40])]
    d = [torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).cuda() for x in req]
    e.submit_device(d[0], 20, None, 0, ahead=(d[1], 20, None))
    for call in (e.state_locks, lambda: e.state_unlock(all=True)):
        with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:.*pending"):
            call()
    e.submit_device(d[1], 20)  # it stayed announced: the announced batch is taken
    e.sync()
    r, st, _ = check(e)
    assert st["total"] == len(np.unique(fasthash_key(keys[:40]) % np.uint64(4 * e.hash_size(0)))) > 15
    e.close()


# ---------------------------------------------------------------------------------------------- 14. beside the other state calls
def test_compact_and_an_image_clone_keep_the_list(traced):
    _, _, req = traced(W.TATP)
    e = twin_of(W.TATP, req)
    r, st, _ = check(e)
    e.state_compact()
    assert check(e)[0].tobytes() == r.tobytes()
    clone = mk(W.TATP, populate=False)
    buf, n, _ = e.state_export(0, 1)
    clone.state_import(buf, n)
    assert check(clone)[0].tobytes() == r.tobytes()
    e.close(); clone.close()


def test_a_refused_rehash_goes_through_after_release_locks(traced):
    _, _, req = traced(W.TATP)
    src = twin_of(W.TATP, req)
    dst = _engine(W.TATP, n_rows=128, log_entries=1 << 12, pool_entries=4096)
    with pytest.raises(_lib.DintError, match=f"dint error {ESTATE}:"):
        recovery.rehash([src], [dst])
    held = recovery.held_locks([src])
    assert len(held) == dst.last_rehash["locks_held"] > 0
    assert recovery.release_locks([src], held, dry_run=True)["released"] == len(held)
    assert recovery.release_locks([src], held)["released"] == len(held)
    assert recovery.rehash([src], [dst])["locks_held"] == 0
    src.close(); dst.close()


@pytest.mark.parametrize("wl", [W.TPL, W.SMALLBANK, W.TATP])
def test_held_locks_of_three_shards_are_the_oracles_global_ids(wl):
    H = 3
    o = mk_oracle(wl)
    req = trace(wl, 3000, 23, o)
    sz = sizes(wl, o)
    hm = ss.home(wl, req, sz, H)
    o.replay(req)
    shards = [mk(wl, H, i) for i in range(H)]
    for i, e in enumerate(shards):
        e.submit(req[hm == i])
    held = recovery.held_locks(shards)
    want = set()
    for t in range(NTAB[wl]):
        a, b = oracle_words(wl, o, t)
        want |= {(t, int(s), int(a[s]), int(b[s])) for s in np.flatnonzero((a != 0) | (b != 0))}
    assert {(int(h["table"]), int(h["lock_hash"]), int(h["a"]), int(h["b"])) for h in held} == want and len(held) == len(want) > 20
    if wl in KV:
        hs = np.array(sz, np.uint64)[held["table"]]
        assert (held["bucket"] == held["lock_hash"] % hs).all() and (held["q"] == held["lock_hash"] // hs).all()
        assert (held["bucket"] % np.uint64(H) == held["shard"]).all()
    third = held[::3]
    u = recovery.release_locks(shards, third)
    assert u["released"] == len(third) and u["stale"] == 0
    left = recovery.held_locks(shards)
    keep = np.ones(len(held), bool)
    keep[::3] = False
    assert left.tobytes() == held[keep].tobytes()
    assert recovery.release_locks(shards)["released"] == len(left) and len(recovery.held_locks(shards)) == 0
    for e in shards:
        e.close()


@pytest.mark.parametrize("wl", LOCKS)
def test_a_piped_inputs_ready_engine_is_listed_behind_its_passes(wl):
    """DINT_FLAG_INPUTS_READY: the first half of a pass runs on a helper stream; the calls order themselves behind the second half,
    which owns the table, as dint_state_export does"""
    import torch

    o = mk_oracle(wl)
    e = mk(wl, flags=_lib.FLAG_INPUTS_READY)
    reqs = [trace(wl, 3000, 60 + k, o, formed=True) for k in range(4)]
    d = [torch.from_numpy(np.frombuffer(x.tobytes(), np.uint8).copy()).cuda() for x in reqs]
    torch.cuda.synchronize()
    for k in range(4):
        e.submit_device(d[k], len(reqs[k]))
    buf, n, st = e.state_locks()  # (no sync in between: the call waits for the passes itself)
    for x in reqs:
        o.replay(x)
    a, b = oracle_words(wl, o, 0)
    want, wst = np_list(wl, [(a, b, None, 0)])
    from dint_amd.engine import lock_records
    assert lock_records(buf, n).tobytes() == want.tobytes() and st == wst and n > 20
    e.submit_device(d[0], len(reqs[0]))
    assert e.state_unlock(all=True)["released"] > 0 and check(e)[1]["total"] == 0
    e.close()
