"""Keys by bucket, the overflow need of a table, and the filtered-replay check of the kv tables at the edge of their overflow
pool (test tooling, numpy only; tests/test_gpu_kv_pool.py and tests/test_kv_core_host.py use it).

The oracle has no pool: the reference `new`s entries without bound.  Which INSERTs an engine with a full pool refuses may depend
on the order in which workgroups reach the allocator, so the check takes the refusals from the replies and holds everything
else to the oracle: with R = the INSERTs answered with the reject code, the oracle's replay of the trace WITHOUT R must give
the other replies byte for byte, the same rows in bucket and chain order and the same lock words; the refused requests come
back unchanged but for their type; R is counted in dint_stats.pool_exhausted and reported by DINT_ENOMEM from exactly the
submissions that hold one; and the tables and their pool verify clean."""
from __future__ import annotations

import ctypes as C

import numpy as np

from dint_amd import wire
from shard_double import fasthash_key

W = wire.Workload
ENOMEM = -2
INSERT_TYPES = {W.STORE: (int(wire.Store.INSERT),), W.TATP: (int(wire.Tatp.INSERT_PRIM), int(wire.Tatp.INSERT_BCK))}
REJECT = {W.STORE: int(wire.Store.REJECT_INSERT), W.TATP: int(wire.Tatp.REJECT_COMMIT)}
N_TABLES = {W.STORE: 1, W.TATP: 5}


def np_bucket(keys, hash_size: int) -> np.ndarray:
    """global bucket of every key: fasthash64(&key, 8, 0xdeadbeef) % hash_size (store/udp/kvs.h:37-40)"""
    return fasthash_key(np.ascontiguousarray(keys, "<u8")) % np.uint64(hash_size)


def cf_key_of(cand: np.ndarray) -> np.ndarray:
    """well-formed CALL_FORWARDING keys from 48-bit candidates: s_id | sf_type (1..4) << 32 | start_time (0, 8, 16) << 40"""
    cand = np.asarray(cand, np.uint64)
    s_id = cand & np.uint64(0xFFFFFFFF)
    sf = (cand >> np.uint64(32)) % np.uint64(4) + np.uint64(1)
    st = ((cand >> np.uint64(34)) % np.uint64(3)) * np.uint64(8)
    return s_id | (sf << np.uint64(32)) | (st << np.uint64(40))


def keys_by_bucket(hash_size: int, per_bucket, seed: int = 1, key_of=None) -> np.ndarray:
    """distinct keys, exactly per_bucket[b] of them in global bucket b of hash_size (a scalar: that many in every bucket), in
    bucket order; `key_of` maps the 48-bit candidates to keys of the form a workload wants"""
    per = np.broadcast_to(np.asarray(per_bucket, np.int64), (hash_size,))
    rng = np.random.default_rng(seed)
    keys = np.zeros(0, np.uint64)
    draw = 8 * int(per.sum()) + 20 * hash_size + 4000
    for _ in range(8):
        cand = rng.integers(1, 1 << 48, draw, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, key_of(cand) if key_of else cand]))
        keys = keys[rng.permutation(len(keys))]
        b = np_bucket(keys, hash_size).astype(np.int64)
        o = np.argsort(b, kind="stable")
        sb = b[o]
        rank = np.arange(len(o)) - np.searchsorted(sb, sb, side="left")
        take = rank < per[sb]
        if (np.bincount(sb[take], minlength=hash_size) == per).all():
            return keys[o][take]
        draw *= 2
    raise AssertionError("not enough candidate keys for every bucket")


def overflow_need(rows_per_bucket) -> int:
    """overflow entries an insert-only table without holes links: sum of max(ceil(r / 4) - 1, 0)"""
    r = np.asarray(rows_per_bucket, np.int64)
    return int(np.maximum(-(-r // 4) - 1, 0).sum())


def raw_submit(e, req: np.ndarray):
    """dint_submit on raw buffers: (rc, replies) -- Engine.submit raises on DINT_ENOMEM"""
    req = np.ascontiguousarray(req)
    rep = np.empty_like(req)
    rc = e._L.dint_submit(e._h, req.ctypes.data, len(req), rep.ctypes.data)
    return rc, rep


class Trace:
    """every submission of one engine from its creation on: the requests, the replies, the return code of each"""

    def __init__(self, e):
        self.e, self.req, self.rep, self.rc = e, [], [], []

    def submit(self, req):
        rc, rep = raw_submit(self.e, req)
        self.add(req, rep, rc)
        return rc, rep

    def add(self, req, rep, rc):
        self.req.append(np.ascontiguousarray(req).copy()); self.rep.append(rep); self.rc.append(rc)


def refused_mask(workload, req, got) -> np.ndarray:
    return (got["type"] == REJECT[workload]) & np.isin(req["type"], INSERT_TYPES[workload])


def _first_diff(a, b, item):
    x, y = np.frombuffer(a.tobytes(), "u1"), np.frombuffer(b.tobytes(), "u1")
    return (np.nonzero(x != y)[0][:5] // item).tolist()


def check_filtered_replay(trace: Trace, oracle, harmless=None):
    """the whole check (module docstring) of an engine's history `trace` against `oracle`, a FRESH oracle of the same tables.
    `harmless` = a batch without INSERTs submitted first of all here: it must return 0 whatever came before.  Returns R, the
    mask of the refused INSERTs over the concatenated trace."""
    e = trace.e
    wl = e.workload
    if harmless is not None:
        rc, _ = trace.submit(harmless)
        assert rc == 0, rc  # refusals of earlier submissions are not reported again
    req, got = np.concatenate(trace.req), np.concatenate(trace.rep)
    R = refused_mask(wl, req, got)
    want = oracle.replay(req[~R])
    assert got[~R].tobytes() == want.tobytes(), ("replies differ from the oracle's replay without the refused INSERTs",
                                                 int(R.sum()), _first_diff(got[~R], want, req.dtype.itemsize))
    back = got[R].copy()
    back["type"] = req["type"][R]
    assert back.tobytes() == req[R].tobytes()  # a refused INSERT comes back as it was sent, but for its type
    for t in range(N_TABLES[wl]):
        a, b = e.dump_rows(t), (oracle.dump() if wl == W.STORE else oracle.dump(t))
        assert all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b)), ("rows differ", t, len(a[0]), len(b[0]))
        if wl == W.TATP:
            assert (e.read_locks(t)[0] == oracle.locks(t)).all(), ("lock words differ", t)
    assert int(R.sum()) == e.stats()["pool_exhausted"]
    at = 0
    for k, (q, rc) in enumerate(zip(trace.req, trace.rc)):
        share = int(R[at:at + len(q)].sum())
        at += len(q)
        if rc is not None:  # (None: a device submission, reported by the sync that follows -- the caller checks that one)
            assert rc == (ENOMEM if share else 0), (k, rc, share)
    for r in e.state_verify():
        bad = {k: v for k, v in r.items() if k in ("bad_chains", "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries",
                                                   "stray_rows", "misplaced_rows", "odd_valid_bytes", "unaccounted") and v}
        assert not bad, r
        assert r["linked"] + r["free_entries"] + r["pending_entries"] == r["pool_top"] <= r["pool_cap"], r
    return R


# ---- churn at a pool that is too small (case d of the pool tests; sizes shown on the host build in tests/test_kv_core_host.py) --------
CHURN_PASSES, CHURN_N = 12, 20_000
CHURN_SUBS = {W.STORE: 2000, W.TATP: 400}  # engine rows = populated subscribers (tatp: all of them touched; store: the first 300)


def churn_oracle(wl):
    from oracle import oracle as orc

    n = CHURN_SUBS[wl]
    return orc.StoreOracle(n * 18 // 4, n) if wl == W.STORE else orc.TatpOracle(n, log_entries=1 << 16)


def churn_trace(wl, kind="issue"):
    """240,000 requests: store_random(p_insert=0.1) with fresh keys that differ from pass to pass / tatp_random(well_formed=True)
    over every subscriber -- inserts and deletes of CALL_FORWARDING, SPECIAL_FACILITY, ACCESS_INFO and SUBSCRIBER rows.  kind
    "issue": 12 passes of 20,000.  kind "crossing": the same requests, tatp's in 48 passes of 5,000 (churn_pool says why)."""
    import tracegen

    if wl == W.STORE:
        out = []
        for p in range(CHURN_PASSES):
            m = tracegen.store_random(CHURN_N, seed=100 + p, n_sub_touch=300, p_set=0.4, p_insert=0.1)
            fresh = (m["key"] & np.uint64(0xFFFFFFFF)) >= np.uint64(3_000_000_000)
            m["key"][fresh] += np.uint64(p * CHURN_N)  # (s_id stays below 2^32)
            out.append(m)
        return out
    o = churn_oracle(wl)
    m = tracegen.tatp_random(CHURN_PASSES * CHURN_N, [o.dump(t)[0] for t in range(5)], seed=77, n_sub_touch=CHURN_SUBS[wl])
    n = CHURN_N if kind == "issue" else 5000
    return [m[k:k + n] for k in range(0, len(m), n)]


def table_needs(wl, o):
    out = []
    for t in range(N_TABLES[wl]):
        keys = o.dump()[0] if wl == W.STORE else o.dump(t)[0]
        hs = CHURN_SUBS[wl] * 18 // 4 if wl == W.STORE else o.hash_size(t)
        out.append(overflow_need(np.bincount(np_bucket(keys, hs).astype(np.int64), minlength=hs)))
    return out


def pass_inserts(wl, m):
    """INSERT requests of one pass per table: what the engine's partition counts"""
    ins = np.isin(m["type"], INSERT_TYPES[wl])
    return [int(ins.sum())] if wl == W.STORE else [int((ins & (m["table"] == t)).sum()) for t in range(5)]


def churn_pool(wl, passes, kind="issue"):
    """pool_entries of the churn case; the population fits it.
    "issue": half of what the UNBOUNDED oracle's fullest table links after the first four passes of 20,000.  An INSERT takes an
    entry only when its chain has no free slot, at most every fourth, so what four passes add is less than one pass's INSERTs
    and half of it lies below population + the INSERTs of pass 0: with this pool every inserting run of every pass goes request
    by request (kv_pool_low counts an entry per INSERT).  The case is refusals beside freed, pending and recycled entries.
    "crossing": what the fullest table's population links + 1.2 times (tatp) / 1.5 times (store) the most INSERTs a pass holds on
    it: the first passes take their closed forms, then pool_top + the pass's INSERTs passes pool_cap, then the pool runs out --
    for tatp only with passes short enough that a pass's INSERTs are fewer than the entries the whole trace adds."""
    o = churn_oracle(wl)
    pop = table_needs(wl, o)
    if kind == "crossing":
        ins = np.array([pass_inserts(wl, m) for m in passes]).max(axis=0)
        t = int(np.argmax(pop))
        return pop[t] + int(ins[t]) * (6 if wl == W.TATP else 3) // (5 if wl == W.TATP else 2)
    for p in passes[:4]:
        o.replay(p)
    pool = max(table_needs(wl, o)) // 2
    assert pool >= max(pop) > 0, (pool, pop)
    return pool


# ---- keys that share a bucket and the 9 key-hash bits of the kv pass (tests/kv_collide.py builds its traces from these) -------------
def key_sig(keys, hash_size: int):
    """(bucket, lock quadrant, key-hash bits) of every key as the kv pass's partition computes them from h = fasthash64(key):
    h % hash_size, (h % (4 * hash_size)) // hash_size, (h >> 40) & 511"""
    h = fasthash_key(np.ascontiguousarray(np.atleast_1d(keys), "<u8"))
    hs = np.uint64(hash_size)
    return h % hs, (h % (np.uint64(4) * hs)) // hs, (h >> np.uint64(40)) & np.uint64(511)


_LIKE, _GROUPS = {}, {}


def keys_like(key: int, hash_size: int, n: int, *, same_kh: bool, same_quadrant: bool, seed: int, key_of=None, exclude=()) -> np.ndarray:
    """n distinct keys other than `key` (and than `exclude`) in key's bucket of hash_size, whose key-hash bits / lock quadrant
    equal key's or differ from them as asked (same_quadrant=None: either); `key_of` maps the 48-bit candidates to keys of the form a workload wants.
    Results are kept per argument set: a parametrized test searches once."""
    memo = (int(key), hash_size, n, same_kh, same_quadrant, seed, key_of, tuple(int(x) for x in exclude))
    if memo in _LIKE:
        return _LIKE[memo].copy()
    b0, q0, k0 = (int(x[0]) for x in key_sig([key], hash_size))
    rng = np.random.default_rng(seed)
    out = np.zeros(0, np.uint64)
    bad = np.array([int(key), *memo[-1]], np.uint64)
    for _ in range(4000):
        cand = rng.integers(1, 1 << 48, 1 << 20, dtype=np.uint64)
        cand = key_of(cand) if key_of else cand
        b, q, k = key_sig(cand, hash_size)
        ok = (b == np.uint64(b0)) & ((k == np.uint64(k0)) == same_kh)
        if same_quadrant is not None:  # (None: any quadrant -- the store has no lock bytes)
            ok &= (q == np.uint64(q0)) == same_quadrant
        if ok.any():
            new = cand[ok]
            out = np.concatenate([out, new[~np.isin(new, bad) & ~np.isin(new, out)]])
            out = out[np.sort(np.unique(out, return_index=True)[1])]
            if len(out) >= n:
                _LIKE[memo] = out[:n].copy()
                return out[:n]
    raise AssertionError("no such keys among 2^32 candidates")


def keys_in_cells(hash_size: int, cells, per: int, seed: int, key_of=None, exclude=()) -> np.ndarray:
    """(len(cells), per) distinct keys, row c in cell cells[c] = (global bucket, lock quadrant) of hash_size, none of `exclude`:
    the keys of the shard-aware layout "edge" (tests/opwords.py), whose places are chosen by bucket and quadrant"""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    want = cells[:, 1] * hash_size + cells[:, 0]  # = the lock word
    assert len(np.unique(want)) == len(want)
    rng = np.random.default_rng(seed)
    out = np.zeros((len(cells), per), np.uint64)
    have = np.zeros(len(cells), np.int64)
    order = np.argsort(want)
    for _ in range(64):
        cand = rng.integers(1 << 33, 1 << 48, 1 << 20, dtype=np.uint64)
        cand = np.unique(key_of(cand) if key_of else cand)
        cand = cand[~np.isin(cand, np.asarray(exclude, np.uint64)) & ~np.isin(cand, out)]
        b, q, _ = key_sig(cand, hash_size)
        lw = (q * np.uint64(hash_size) + b).astype(np.int64)
        at = np.searchsorted(want[order], lw)
        hit = np.nonzero(want[order][np.minimum(at, len(want) - 1)] == lw)[0]
        for k, c in zip(cand[hit], order[at[hit]]):
            if have[c] < per:
                out[c, have[c]] = k
                have[c] += 1
        if (have == per).all():
            return out
    raise AssertionError("not enough candidate keys for every cell")


def collision_groups(hash_size: int, n_groups: int, per_group: int, seed: int, key_of=None) -> np.ndarray:
    """(n_groups, per_group) distinct keys: a row shares bucket and key-hash bits, different rows lie in different buckets.
    A birthday search over the cells (bucket, key hash) of 200,000 candidates, doubled until there are enough."""
    memo = (hash_size, n_groups, per_group, seed, key_of)
    if memo in _GROUPS:
        return _GROUPS[memo].copy()
    rng = np.random.default_rng(seed)
    keys = np.zeros(0, np.uint64)
    draw = 200_000
    for _ in range(8):
        cand = rng.integers(1, 1 << 48, draw, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, key_of(cand) if key_of else cand]))
        b, _, k = key_sig(keys, hash_size)
        cell = b * np.uint64(512) + k
        o = np.argsort(cell, kind="stable")
        sc = cell[o]
        first = np.searchsorted(sc, sc, side="left")
        rank = np.arange(len(o)) - first
        heads = first[rank == per_group - 1]  # cells with at least per_group keys
        _, pick = np.unique(sc[heads] // np.uint64(512), return_index=True)  # one cell per bucket
        if len(pick) >= n_groups:
            heads = heads[pick][rng.permutation(len(pick))[:n_groups]]
            out = keys[o][heads[:, None] + np.arange(per_group)[None, :]]
            _GROUPS[memo] = out.copy()
            return out
        draw *= 2
    raise AssertionError("not enough candidate keys for the groups")


def colliding_pairs(keys, hash_size: int, same_quadrant: bool) -> np.ndarray:
    """all pairs (a, b), a before b, among `keys` (distinct) that share bucket and key-hash bits and whose lock quadrants are equal or
    not as asked: the pairs a populated table holds"""
    keys = np.ascontiguousarray(keys, "<u8")
    b, q, k = key_sig(keys, hash_size)
    cell = b * np.uint64(512) + k
    o = np.argsort(cell, kind="stable")
    sc, sq, sk = cell[o], q[o], keys[o]
    out = []
    for i in np.nonzero(sc[1:] == sc[:-1])[0]:
        if (sq[i] == sq[i + 1]) == same_quadrant:
            out.append((int(sk[i]), int(sk[i + 1])))
    return np.array(out, np.uint64).reshape(-1, 2)
