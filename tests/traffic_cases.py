"""Traces for the traffic report and an independent numpy form of it (test tooling, numpy only; tests/test_traffic_host.py and
tests/test_gpu_traffic.py use it).

np_report restates struct dint_traffic_report (include/dint_abi.h) with np.unique / np.bincount, the vectorised fasthash64 of
tests/shard_double.py and class / flag tables written here from dint_amd/wire.py; it shares no code with
dint_amd/csrc/traffic_report.h.  The bucket counts are the formulas the reference's servers use."""
from __future__ import annotations

import numpy as np

from dint_amd import wire
from shard_double import fasthash_key, fasthash_lid

W, F, P, S, T, B = wire.Workload, wire.Fasst, wire.Tpl, wire.Store, wire.Tatp, wire.Sb
WORKLOADS = [W.FASST, W.TPL, W.STORE, W.TATP, W.SMALLBANK]
IDS = ["fasst", "2pl", "store", "tatp", "smallbank"]
N_ROWS = 64      # kv tables: small, so that keys share buckets and lock slots
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1025, 70001]
READ, LOCK, UNLOCK, WRITE, LOG, OTHER = range(6)

CLASS = {
    W.FASST: {F.READ: READ, F.ACQUIRE_LOCK: LOCK, F.ABORT: UNLOCK, F.COMMIT: WRITE},
    W.TPL: {P.ACQUIRE_LOCK: LOCK, P.RELEASE_LOCK: UNLOCK},
    W.STORE: {S.READ: READ, S.SET: WRITE, S.INSERT: WRITE},
    W.TATP: {T.READ: READ, T.ACQUIRE_LOCK: LOCK, T.ABORT: UNLOCK, T.COMMIT_PRIM: WRITE, T.COMMIT_BCK: WRITE, T.INSERT_PRIM: WRITE,
             T.INSERT_BCK: WRITE, T.DELETE_PRIM: WRITE, T.DELETE_BCK: WRITE, T.COMMIT_LOG: LOG, T.DELETE_LOG: LOG},
    W.SMALLBANK: {B.ACQUIRE_SHARED: LOCK, B.ACQUIRE_EXCLUSIVE: LOCK, B.RELEASE_SHARED: UNLOCK, B.RELEASE_EXCLUSIVE: UNLOCK,
                  B.COMMIT_PRIM: WRITE, B.COMMIT_BCK: WRITE, B.COMMIT_LOG: LOG, B.WARMUP_READ: READ},
}
#: requests that work on the key's lock slot: acquires, releases and the primary's writes (tatp / smallbank)
SLOT = {W.TATP: (T.ACQUIRE_LOCK, T.ABORT, T.COMMIT_PRIM, T.INSERT_PRIM, T.DELETE_PRIM),
        W.SMALLBANK: (B.ACQUIRE_SHARED, B.ACQUIRE_EXCLUSIVE, B.RELEASE_SHARED, B.RELEASE_EXCLUSIVE, B.COMMIT_PRIM)}
REJECT = {W.FASST: (F.REJECT_LOCK,), W.TPL: (P.REJECT_LOCK, P.RETRY), W.STORE: (S.REJECT_READ, S.REJECT_SET, S.REJECT_INSERT),
          W.TATP: (T.REJECT_READ, T.REJECT_LOCK, T.REJECT_COMMIT, 28), W.SMALLBANK: (B.REJECT_SHARED, B.REJECT_EXCLUSIVE, B.RETRY)}
MISS = {W.FASST: (), W.TPL: (), W.STORE: (S.NOT_EXIST,), W.TATP: (T.NOT_EXIST,), W.SMALLBANK: ()}
SCALARS = ("n", "keyed", "bad_table", "log_requests", "reads", "locks", "unlocks", "writes", "others", "rejects", "misses", "distinct_keys",
           "distinct_units", "distinct_lock_slots", "max_key_requests", "max_unit_requests", "max_unit", "max_unit_table", "shared_units",
           "shared_unit_requests", "shared_unit_rejects", "shared_slots", "shared_slot_requests", "shared_slot_rejects", "n_by_requests",
           "n_by_rejects")
LISTS = ("key_hist", "unit_hist", "req_types", "rep_types", "by_requests", "by_rejects")


def is_lock(wl):
    return wl in (W.FASST, W.TPL)


def sizes(wl, n_slots=16, n_rows=N_ROWS):
    """lock tables: n_slots; kv: the bucket counts of store/udp/server.cc:112-114, tatp/udp/server_shard.cc:75-79,
    smallbank/udp/server_shard.cc:75-76"""
    if is_lock(wl):
        return [n_slots]
    if wl == W.STORE:
        return [n_rows * 18 // 4]
    if wl == W.TATP:
        return [n_rows * 3 // 2 // 4] * 2 + [n_rows * 15 // 4 // 4] * 2 + [n_rows * 45 // 8 // 4]
    return [n_rows * 3 // 2 // 4] * 2


def fields(wl, m):
    """(table, key as u64, type byte) of a message array"""
    n = len(m)
    if wl == W.FASST:
        return np.zeros(n, np.int64), m["lid"].astype(np.uint64), m["type"].astype(np.int64)
    if wl == W.TPL:
        return np.zeros(n, np.int64), m["lid"].astype(np.uint64), m["action"].astype(np.int64)
    if wl == W.STORE:
        return np.zeros(n, np.int64), m["key"].astype(np.uint64), m["type"].astype(np.int64)
    return m["table"].astype(np.int64), m["key"].astype(np.uint64), m["type"].astype(np.int64)


def _hash(wl, keys):
    return fasthash_lid(keys.astype(np.uint32)) if is_lock(wl) else fasthash_key(keys)


def _log2_hist(counts):
    h = np.zeros(25, np.int64)
    if len(counts):
        b = np.minimum(np.floor(np.log2(counts.astype(np.float64))).astype(np.int64), 24)
        h += np.bincount(b, minlength=25)
    return [int(x) for x in h]


def _groups(t, ids, req, rej):
    """per distinct (t, id): distinct, shared, shared requests, shared rejects, the per-group request sums and the sorted pairs"""
    if not len(t):
        return 0, 0, 0, 0, np.zeros(0, np.int64), np.zeros((0, 2), np.uint64)
    pair = np.stack([t.astype(np.uint64), ids.astype(np.uint64)], axis=1)
    uq, inv = np.unique(pair, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    members = np.bincount(inv, minlength=len(uq))
    greq = np.bincount(inv, weights=req, minlength=len(uq)).astype(np.int64)
    grej = np.bincount(inv, weights=rej, minlength=len(uq)).astype(np.int64)
    sh = members >= 2
    return len(uq), int(sh.sum()), int(greq[sh].sum()), int(grej[sh].sum()), greq, uq


def np_report(wl, reqs, reps, size, top):
    """the report dict of Engine.traffic_report / traffic.report_host, without temp_bytes"""
    nt, n = len(size), len(reqs)
    t, key, y = fields(wl, reqs)
    cls = np.full(n, OTHER, np.int64)
    for code, c in CLASS[wl].items():
        cls[y == int(code)] = c
    if wl == W.TPL:
        cls[reqs["type"] > 1] = OTHER
    in_t = t < nt
    keyed = in_t & (cls != LOG)
    has = reps is not None
    yr = fields(wl, reps)[2] if has else np.zeros(n, np.int64)
    rej = np.isin(yr, [int(c) for c in REJECT[wl]]) & keyed & has
    mis = np.isin(yr, [int(c) for c in MISS[wl]]) & keyed & has
    slot_cls = np.isin(y, [int(c) for c in SLOT.get(wl, ())]) & keyed
    r = {"n": n, "keyed": int(keyed.sum()), "bad_table": int((~in_t).sum()), "log_requests": int((in_t & (cls == LOG)).sum()),
         "reads": int((keyed & (cls == READ)).sum()), "locks": int((keyed & (cls == LOCK)).sum()),
         "unlocks": int((keyed & (cls == UNLOCK)).sum()), "writes": int((keyed & (cls == WRITE)).sum()),
         "others": int((keyed & (cls == OTHER)).sum()), "rejects": int(rej.sum()), "misses": int(mis.sum())}
    r["req_types"] = np.bincount(t[in_t] * 32 + np.minimum(y[in_t], 31), minlength=160).reshape(5, 32).tolist()
    r["rep_types"] = (np.bincount(t[in_t] * 32 + np.minimum(yr[in_t], 31), minlength=160) if has else np.zeros(160, np.int64)).reshape(5, 32).tolist()
    idx = np.nonzero(keyed)[0]
    kt, kk = t[idx], key[idx]
    pair = np.stack([kt.astype(np.uint64), kk], axis=1) if len(idx) else np.zeros((0, 2), np.uint64)
    uq, first, inv = np.unique(pair, axis=0, return_index=True, return_inverse=True) if len(idx) else (pair, np.zeros(0, np.int64), np.zeros(0, np.int64))
    inv = inv.reshape(-1)
    D = len(uq)

    def per_key(mask):
        return np.bincount(inv, weights=mask[idx], minlength=D).astype(np.int64)

    ent = {"requests": per_key(keyed), "reads": per_key(cls == READ), "locks": per_key(cls == LOCK), "unlocks": per_key(cls == UNLOCK),
           "writes": per_key(cls == WRITE), "rejects": per_key(rej), "misses": per_key(mis)}
    sreq, srej = per_key(slot_cls), per_key(slot_cls & rej)
    ut, uk = uq[:, 0].astype(np.int64), uq[:, 1]
    r["distinct_keys"] = D
    r["key_hist"] = _log2_hist(ent["requests"])
    r["max_key_requests"] = int(ent["requests"].max()) if D else 0
    h = _hash(wl, uk)
    hs = np.array(size, np.uint64)
    unit = h % hs[ut] if D else np.zeros(0, np.uint64)
    du, su, sreqs, srejs, greq, gid = _groups(ut, unit, ent["requests"], ent["rejects"])
    r.update(distinct_units=du, shared_units=su, shared_unit_requests=sreqs, shared_unit_rejects=srejs, unit_hist=_log2_hist(greq))
    if du:
        g = int(np.argmax(greq))  # (the first maximum of the ascending (table, unit) list)
        r.update(max_unit_requests=int(greq[g]), max_unit=int(gid[g, 1]), max_unit_table=int(gid[g, 0]))
    else:
        r.update(max_unit_requests=0, max_unit=0, max_unit_table=0)
    if wl in SLOT and D:
        m = sreq > 0
        ds, ss, a, b, _, _ = _groups(ut[m], h[m] % (np.uint64(4) * hs[ut[m]]), sreq[m], srej[m])
    else:
        ds = ss = a = b = 0
    r.update(distinct_lock_slots=ds, shared_slots=ss, shared_slot_requests=a, shared_slot_rejects=b)

    def top_list(by, need_positive):
        order = np.lexsort((uk, ut, -ent[by])) if D else np.zeros(0, np.int64)
        if need_positive:
            order = order[ent[by][order] > 0]
        return [dict(key=int(uk[d]), table=int(ut[d]), first_index=int(idx[first[d]]), **{k: int(v[d]) for k, v in ent.items()}) for d in order[:top]]

    r["by_requests"] = top_list("requests", False)
    r["by_rejects"] = top_list("rejects", True) if has else []
    r["n_by_requests"], r["n_by_rejects"] = len(r["by_requests"]), len(r["by_rejects"])
    return r


def assert_same(got, want, what=""):
    for k in SCALARS + LISTS:
        assert got[k] == want[k], (what, k, got[k], want[k])


# ---- trace builders --------------------------------------------------------------------------------------------------------------
MIX = {  # request codes of the ordinary mixes (no inserts: the tables stay as populated)
    W.FASST: [F.READ, F.READ, F.ACQUIRE_LOCK, F.ACQUIRE_LOCK, F.ABORT, F.COMMIT],
    W.TPL: [P.ACQUIRE_LOCK, P.ACQUIRE_LOCK, P.RELEASE_LOCK],
    W.STORE: [S.READ, S.READ, S.SET],
    W.TATP: [T.READ, T.READ, T.ACQUIRE_LOCK, T.ACQUIRE_LOCK, T.ABORT, T.COMMIT_PRIM, T.COMMIT_BCK, T.COMMIT_LOG],
    W.SMALLBANK: [B.ACQUIRE_SHARED, B.ACQUIRE_EXCLUSIVE, B.RELEASE_SHARED, B.RELEASE_EXCLUSIVE, B.COMMIT_PRIM, B.COMMIT_BCK, B.COMMIT_LOG,
                  B.WARMUP_READ],
}
N_TABLES = {W.FASST: 1, W.TPL: 1, W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}


def batch(wl, keys, seed, types=None, tables=None):
    """one message per key: types (default: drawn from MIX) and tables (default: drawn from the workload's) as given; values,
    versions and -- lock_2pl -- the lock type random"""
    rng = np.random.default_rng(seed)
    n = len(keys)
    m = np.zeros(n, wire.MSG_DTYPE[wl])
    ty = np.asarray(types if types is not None else rng.choice([int(c) for c in MIX[wl]], n), np.uint8)
    if wl == W.TPL:
        m["action"], m["type"] = ty, rng.integers(0, 2, n)
    else:
        m["type"] = ty
    if is_lock(wl):
        m["lid"] = np.asarray(keys, np.uint64).astype(np.uint32)
    else:
        m["key"] = np.asarray(keys, np.uint64)
    if wl in (W.TATP, W.SMALLBANK):
        m["table"] = rng.integers(0, N_TABLES[wl], n) if tables is None else tables
        m["ord"] = rng.integers(0, 256, n)
    if wl == W.FASST:
        m["ver"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    elif wl != W.TPL:
        m["val"] = rng.integers(0, 256, m["val"].shape, dtype=np.uint8)
        m["ver"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4")
    return m


def key_mix(wl, n, mix, seed):
    rng = np.random.default_rng(seed)
    top = (1 << 32) if is_lock(wl) else (1 << 64)
    if mix == "one":
        return np.full(n, 5, np.uint64)
    if mix == "distinct":
        k = np.arange(n, dtype=np.uint64) * np.uint64(2654435761 if is_lock(wl) else 0x9E3779B97F4A7C15)
        k = k % np.uint64(top) if is_lock(wl) else k
        assert len(np.unique(k)) == n
        return k[rng.permutation(n)]
    return (rng.zipf(1.3, n) % 5000).astype(np.uint64)  # zipf: a few hot keys, a long tail


def edge_batches(wl, seed=7):
    """name -> batch: the key and table edge cases of the issue"""
    rng = np.random.default_rng(seed)
    lock = is_lock(wl)
    hi = np.uint64(0xFFFFFFFF if lock else 0xFFFFFFFFFFFFFFFF)
    out = {}
    out["extreme_keys"] = batch(wl, np.array([0, hi, 0, hi, 1, hi, 0, 7] * 9, np.uint64), seed)
    if lock:
        top_byte = np.array([(b << 24) | 0x123456 for b in range(0, 256, 5)] * 3, np.uint64)
        low = np.array([0xABCD0000 | b for b in range(70)] * 2, np.uint64)
    else:
        top_byte = np.array([(b << 56) | 0x123456789ABC for b in range(0, 256, 5)] * 3, np.uint64)
        low = np.array([(0x5EED << 32) | rng.integers(0, 1 << 32) for _ in range(70)] * 2, np.uint64)
    out["top_byte"] = batch(wl, top_byte, seed + 1)
    out["low_32_bits"] = batch(wl, low, seed + 2)
    nt = N_TABLES[wl]
    if nt > 1:
        k = np.repeat(np.array([3, 3, 9, 1 << 40], np.uint64), 25)
        out["same_key_two_tables"] = batch(wl, k, seed + 3, tables=np.arange(100) % nt)
        tb = rng.integers(0, nt, 300)
        tb[::7] = 5
        tb[3::11] = 255
        out["bad_tables"] = batch(wl, rng.integers(0, 40, 300).astype(np.uint64), seed + 4, tables=tb)
        logt = int(T.COMMIT_LOG if wl == W.TATP else B.COMMIT_LOG)
        ty = rng.choice([int(c) for c in MIX[wl]], 400)
        ty[::3] = logt
        out["logs_between"] = batch(wl, rng.integers(0, 30, 400).astype(np.uint64), seed + 5, types=ty)
    every = np.arange(41, dtype=np.uint8)
    out["every_type_byte"] = batch(wl, rng.integers(0, 20, 41).astype(np.uint64), seed + 6, types=every)
    # many keys tied at the cut: 40 keys, 3 requests each
    out["ties"] = batch(wl, np.repeat(np.arange(100, 140, dtype=np.uint64), 3)[rng.permutation(120)], seed + 8,
                        types=np.full(120, int(MIX[wl][0])), tables=np.zeros(120, np.int64))
    return out


def aliased_lids(n_slots, groups, per, seed=3):
    """`groups` groups of `per` lids that share one lock slot"""
    rng = np.random.default_rng(seed)
    lids = np.unique(rng.integers(1, 1 << 32, 40 * n_slots * per + 4000, dtype=np.uint64))
    slot = (fasthash_lid(lids.astype(np.uint32)) % np.uint64(n_slots)).astype(np.int64)
    out = []
    for s in np.unique(slot):
        g = lids[slot == s]
        if len(g) >= per:
            out.append(g[:per])
        if len(out) == groups:
            return np.array(out)
    raise AssertionError("not enough aliased lids")


def sharing_batch(wl, groups, seed=5):
    """`groups`: rows of 3 keys that share a unit (and, kv, a lock slot).  Every key of a group ACQUIREs in turn, twice over, with
    no release in between: the second and third key are rejected because ANOTHER key holds the slot, the second round also the
    first key -- because it holds it itself.  Then releases.  kv: every key in table 0"""
    acq = {W.FASST: F.ACQUIRE_LOCK, W.TPL: P.ACQUIRE_LOCK, W.STORE: S.READ, W.TATP: T.ACQUIRE_LOCK, W.SMALLBANK: B.ACQUIRE_EXCLUSIVE}[wl]
    rel = {W.FASST: F.ABORT, W.TPL: P.RELEASE_LOCK, W.STORE: S.SET, W.TATP: T.ABORT, W.SMALLBANK: B.RELEASE_EXCLUSIVE}[wl]
    keys, types = [], []
    for g in groups:
        keys += list(g) * 2 + [g[0]]
        types += [int(acq)] * (2 * len(g)) + [int(rel)]
    m = batch(wl, np.array(keys, np.uint64), seed, types=types, tables=np.zeros(len(keys), np.int64))
    if wl == W.TPL:
        m["type"] = P.EXCLUSIVE
    return m


def sharing_groups(wl, n_slots=16):
    """4 groups of 3 keys that share a unit: lids aliased to one slot; kv keys of one bucket of table 0 that also share the lock
    slot (hash % 4 hash_size) -- 12 keys are drawn per bucket and a triple of one slot kept"""
    if is_lock(wl):
        return aliased_lids(n_slots, 4, 3)
    from kvkeys import keys_by_bucket, np_bucket

    hs = sizes(wl)[0]
    keys = keys_by_bucket(hs, 12, seed=2).reshape(hs, 12)
    out = []
    for row in keys[:8]:
        slot = np_bucket(row, 4 * hs)
        for s in np.unique(slot):
            if (slot == s).sum() >= 3:
                out.append(row[slot == s][:3])
                break
    assert len(out) >= 4
    return np.array(out[:4])
