"""Traces for the kv passes on keys that share a bucket AND the 9 key-hash bits the pass sorts by (test tooling, numpy only;
tests/test_gpu_kv_collide.py runs them on the GPU, tests/test_kvkeys_host.py checks on the host that every one of them holds
what its case is about).

A case is built once per argument set and kept: its passes, the oracle's replies to them and the oracle's final state, so that
a test parametrized over the engine's knobs replays nothing twice.  `Case.pairs` names the colliding keys and the passes meant
to exercise them, `Case.cold` / `Case.hot` the per-pass request counts the case promises."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import kvkeys
import tracegen
from dint_amd import wire
from oracle import oracle as orc

W = wire.Workload
T, S, B = wire.Tatp, wire.Store, wire.Sb
HOT_PASSES = (900, 3000, 500, 6000, 14_000, 600)  # solo items, pieces, one stretch, several stretches; the last one without N
SB_PASSES = (3000, 900, 20_000, 6000, 40_000)
CHUNK_PASSES = (300, 1000, 4000)
TATP_SIMPLE = ([T.READ, T.ACQUIRE_LOCK, T.ABORT, T.COMMIT_PRIM, T.COMMIT_BCK], [0.6, 0.15, 0.05, 0.1, 0.1])
CF_MIXES = {0.3: {0: 85, 1: 10, 2: 2, 18: 1.5, 22: 1.5}, 0.02: {0: 85, 1: 12, 2: 1, 18: 1, 22: 1}}  # test_tatp_dominant_key_vs_oracle's
CF_HOT = (4, 7 | (1 << 32))
STORE_HOT = int(tracegen.store_key(11, 2, 8))
N_SUB, N_STORE = 3000, 5000
STORE_HS = N_STORE * 18 // 4


@dataclass
class Case:
    wl: object
    engine: dict                       # Engine(wl, **engine)
    populate: int
    passes: list
    pairs: list = field(default_factory=list)  # (table, [keys that share bucket and key hash], [passes every one of them occurs in])
    cold: list = field(default_factory=list)   # (table, key, [passes]): 1 .. 8 requests in each
    hot: list = field(default_factory=list)    # (table, key, {pass: at least that many requests})
    control: tuple = None              # (table, hot key, N'): a control case -- N' shares the bucket, not the key hash, not the quadrant
    want: list = None                  # the oracle's replies, pass by pass
    rows: list = None                  # its rows per table afterwards, its lock words, its log
    locks: list = None
    ring: np.ndarray = None
    tail: int = 0
    errors: int = 0
    log_cap: int = 0

    def oracle(self):
        if self.wl == W.STORE:
            return orc.StoreOracle(STORE_HS, self.populate)
        if self.wl == W.TATP:
            return orc.TatpOracle(self.engine["n_rows"], log_entries=self.log_cap, populate_n=self.populate)
        return orc.SmallbankOracle(self.engine["n_rows"], log_entries=self.log_cap, populate_n=self.populate)

    def replayed(self):
        o = self.oracle()
        self.want = [o.replay(p) for p in self.passes]
        self.errors = getattr(o, "errors", 0)
        if self.wl == W.STORE:
            self.rows = [tuple(x.copy() for x in o.dump())]
        elif self.wl == W.TATP:
            self.rows = [tuple(x.copy() for x in o.dump(t)) for t in range(5)]
            self.locks = [o.locks(t).copy() for t in range(5)]
        else:
            self.rows = [tuple(x.copy() for x in o.dump(t)) for t in range(2)]
            self.locks = [(o.num_ex(t).copy(), o.num_sh(t).copy()) for t in range(2)]
        if self.wl != W.STORE:
            self.ring, self.tail = o.ring.copy(), int(o.tail)
        return self


def count(case: Case, k: int, table: int, key: int) -> int:
    p = case.passes[k]
    sel = p["key"] == np.uint64(key)
    if case.wl != W.STORE:
        sel &= p["table"] == table
    return int(sel.sum())


def cold_count(n: int) -> int:
    """requests of a cold neighbour in a pass of n: about 0.3 %, and between 1 and 8 (a handful per pass)"""
    return min(8, max(1, round(0.003 * n)))


def _overlay(req, rng, table, key, sel, types, p):
    if table is not None:
        req["table"][sel] = table
    req["key"][sel] = key
    req["type"][sel] = rng.choice(types, int(sel.sum()), p=np.array(p, float) / sum(p))


def _cold_sel(rng, free, n_cold):
    sel = np.zeros(len(free), bool)
    sel[rng.choice(np.nonzero(free)[0], n_cold, replace=False)] = True
    return sel


# ---- tatp ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def tatp_base(n_sub=N_SUB):
    o = orc.TatpOracle(n_sub, log_entries=16)
    return [o.dump(t)[0].copy() for t in range(5)], [o.hash_size(t) for t in range(5)]


def sf_key_of(cand):
    """ACCESS_INFO / SPECIAL_FACILITY keys from 48-bit candidates: s_id | type (1..4) << 32"""
    cand = np.asarray(cand, np.uint64)
    return (cand & np.uint64(0xFFFFFFFF)) | (((cand >> np.uint64(32)) % np.uint64(4) + np.uint64(1)) << np.uint64(32))


TATP_KEY_OF = (None, None, sf_key_of, sf_key_of, kvkeys.cf_key_of)


@functools.lru_cache(None)
def _tatp_pools(avoid):
    """tatp_random's own pools for every subscriber (the populated rows and the plausible missing ones), without the keys of the
    (table, bucket) pairs in `avoid`: noise that stays out of a hot row's bucket"""
    existing, hs = tatp_base()
    s = np.arange(N_SUB, dtype=np.uint64)
    a = (np.arange(1, 5, dtype=np.uint64) << np.uint64(32))[None, :]
    sf = (s[:, None] | a).ravel()
    cf = (sf[:, None] | (np.array([0, 8, 16], np.uint64) << np.uint64(40))[None, :]).ravel()
    plausible = [s, np.zeros(0, np.uint64), sf, sf, cf]
    pools = []
    for t in range(5):
        pool = np.unique(np.concatenate([existing[t], plausible[t]]))
        for tb, b in avoid:
            if tb == t:
                pool = pool[kvkeys.np_bucket(pool, hs[t]) != np.uint64(b)]
        pools.append(pool.tolist())
    return tuple(pools)


def tatp_noise(n, seed, avoid):
    existing, _ = tatp_base()
    return tracegen.tatp_random(n, existing, seed=seed, pools=_tatp_pools(avoid))


def tatp_insert_pass(rows, seed, avoid):
    """a first small pass that INSERTs the (table, key) rows in `rows`, so that the neighbours exist"""
    req = tatp_noise(200, seed, avoid)
    for k, (tb, key) in enumerate(rows):
        at = 20 + 30 * k
        req["type"][at], req["table"][at], req["key"][at] = T.INSERT_PRIM, tb, key
    return req


def tatp_bucket_of(table, key):
    return (table, int(kvkeys.np_bucket(np.array([key], np.uint64), tatp_base()[1][table])[0]))


@functools.lru_cache(None)
def tatp_hot_pair(same_quadrant: bool, share: str, control: bool = False, hot: int = 7) -> Case:
    """case b: subscriber `hot` (55 .. 60 % of every pass, 35 % in "equal") and a neighbour N in its bucket behind its key-hash bits,
    in its lock quadrant or not; N is inserted by pass 0, requested in passes 1 .. 5 and absent from pass 6.  `share`: "cold" = 1 .. 8
    requests of N per pass (about 0.3 %), "warm" = 6 %, "equal" = 35 % each.  control: the same trace with N' instead of N, a key
    of the bucket with OTHER key-hash bits in another quadrant."""
    hs = tatp_base()[1][0]
    n_key = int(kvkeys.keys_like(hot, hs, 1, same_kh=not control, same_quadrant=same_quadrant and not control, seed=11)[0])
    avoid = (tatp_bucket_of(0, hot),)
    rng = np.random.default_rng(5)
    passes = [tatp_insert_pass([(0, n_key)], 3, avoid)]
    c = Case(W.TATP, dict(n_rows=N_SUB, log_entries=400_000), N_SUB, passes, log_cap=400_000)
    p_h = 0.35 if share == "equal" else 0.6
    hot_min = {}
    for k, n in enumerate(HOT_PASSES):
        req = tatp_noise(n, 17 * k + 5, avoid)
        u = rng.random(n)
        h_sel = u < p_h
        _overlay(req, rng, 0, hot, h_sel, *TATP_SIMPLE)
        if k < len(HOT_PASSES) - 1:
            n_sel = _cold_sel(rng, ~h_sel, cold_count(n)) if share == "cold" else (u >= p_h) & (u < p_h + (0.06 if share == "warm" else 0.35))
            _overlay(req, rng, 0, n_key, n_sel, *TATP_SIMPLE)
        passes.append(req)
        hot_min[k + 1] = int(0.8 * p_h * n)
    ex = list(range(1, len(HOT_PASSES)))
    c.pairs = [] if control else [(0, [hot, n_key], ex)]
    c.control = (0, hot, n_key) if control else None
    c.hot = [(0, hot, hot_min)] + ([(0, n_key, {k: hot_min[k] for k in ex})] if share == "equal" else [])
    c.cold = [(0, n_key, ex)] if share == "cold" else []
    return c.replayed()


@functools.lru_cache(None)
def tatp_cf_pair(p_hot: float, n_writes: bool) -> Case:
    """case c: the hot CALL_FORWARDING row (4, 7 | 1 << 32) inserted and deleted by its own requests, beside a well-formed
    CALL_FORWARDING key N behind its key-hash bits (another lock quadrant).  N is inserted by pass 0; then it is only read
    (1 % of a pass) or, n_writes, takes the hot row's own mix at 2 % -- inserted and deleted as well."""
    hs = tatp_base()[1][4]
    n_key = int(kvkeys.keys_like(CF_HOT[1], hs, 1, same_kh=True, same_quadrant=False, seed=12, key_of=kvkeys.cf_key_of)[0])
    avoid = (tatp_bucket_of(*CF_HOT),)
    rng = np.random.default_rng(6)
    mix = CF_MIXES[p_hot]
    passes = [tatp_insert_pass([(4, n_key)], 4, avoid)]
    c = Case(W.TATP, dict(n_rows=N_SUB, log_entries=400_000), N_SUB, passes, log_cap=400_000)
    hot_min, ex = {}, []
    for k, n in enumerate(HOT_PASSES):
        req = tatp_noise(n, 19 * k + 7, avoid)
        u = rng.random(n)
        _overlay(req, rng, 4, CF_HOT[1], u < p_hot, list(mix), list(mix.values()))
        if k < len(HOT_PASSES) - 1:
            p_n = 0.02 if n_writes else 0.01
            n_sel = (u >= p_hot) & (u < p_hot + p_n)
            _overlay(req, rng, 4, n_key, n_sel, *((list(mix), list(mix.values())) if n_writes else ([T.READ], [1])))
            ex.append(k + 1)
        passes.append(req)
        hot_min[k + 1] = max(1, int(p_hot * n - 4 * (p_hot * n) ** 0.5))  # (binomial: the mean less four standard deviations)
    c.pairs = [(4, [CF_HOT[1], n_key], ex)]
    c.hot = [(4, CF_HOT[1], hot_min)]
    return c.replayed()


@functools.lru_cache(None)
def tatp_rem_pair(hot: int = 7) -> Case:
    """case d: subscriber `hot` is hot; N1 and N2 lie in its bucket in ANOTHER lock quadrant, behind key-hash bits that are each
    other's and not the hot key's: the hot key stays in closed form, the two go through the remainder's chunks in rounds"""
    hs = tatp_base()[1][0]
    n1 = int(kvkeys.keys_like(hot, hs, 1, same_kh=False, same_quadrant=False, seed=13)[0])
    n2 = int(kvkeys.keys_like(n1, hs, 1, same_kh=True, same_quadrant=True, seed=14, exclude=(hot,))[0])
    avoid = (tatp_bucket_of(0, hot),)
    rng = np.random.default_rng(7)
    passes = [tatp_insert_pass([(0, n1), (0, n2)], 5, avoid)]
    c = Case(W.TATP, dict(n_rows=N_SUB, log_entries=400_000), N_SUB, passes, log_cap=400_000)
    hot_min = {}
    for k, n in enumerate(HOT_PASSES):
        req = tatp_noise(n, 23 * k + 9, avoid)
        u = rng.random(n)
        h_sel = u < 0.6
        _overlay(req, rng, 0, hot, h_sel, *TATP_SIMPLE)
        free = ~h_sel
        for key in (n1, n2):
            sel = _cold_sel(rng, free, cold_count(n))
            free &= ~sel
            _overlay(req, rng, 0, key, sel, *TATP_SIMPLE)
        passes.append(req)
        hot_min[k + 1] = int(0.5 * n)
    ex = list(range(1, len(HOT_PASSES) + 1))
    c.pairs = [(0, [n1, n2], ex)]
    c.cold = [(0, n1, ex), (0, n2, ex)]
    c.hot = [(0, hot, hot_min)]
    return c.replayed()


@functools.lru_cache(None)
def tatp_chunks() -> Case:
    """case a: per table eight groups of three keys behind one (bucket, key hash) and some 130 populated rows, tatp_random over them
    with all eleven op types, well formed -- INSERTs and DELETEs restructure chains that hold colliding keys; cold throughout"""
    existing, hs = tatp_base()
    groups = [kvkeys.collision_groups(hs[t], 8, 3, seed=20 + t, key_of=TATP_KEY_OF[t]) for t in range(5)]
    pools = [sorted(set(groups[t].ravel().tolist()) | set(np.sort(existing[t])[:130].tolist())) for t in range(5)]
    req = tracegen.tatp_random(sum(CHUNK_PASSES), existing, seed=41, pools=pools)
    cuts = np.cumsum((0,) + CHUNK_PASSES)
    c = Case(W.TATP, dict(n_rows=N_SUB, log_entries=400_000), N_SUB, [req[a:b] for a, b in zip(cuts[:-1], cuts[1:])], log_cap=400_000)
    c.pairs = [(t, g.tolist(), []) for t in range(5) for g in groups[t]]
    return c.replayed()


# ---- store --------------------------------------------------------------------------------------------------------------------
def store_noise(n, seed, avoid_bucket=None):
    req = tracegen.store_random(n, seed=seed, n_sub_touch=N_STORE, p_set=0.3, p_missing=0.05)
    if avoid_bucket is not None:  # (the noise stays out of the hot key's bucket)
        hit = kvkeys.np_bucket(req["key"], STORE_HS) == np.uint64(avoid_bucket)
        req["key"][hit] = tracegen.store_key(1, 1, 0) if avoid_bucket != int(kvkeys.np_bucket([tracegen.store_key(1, 1, 0)], STORE_HS)[0]) else tracegen.store_key(2, 1, 0)
    return req


@functools.lru_cache(None)
def store_hot_pair(share: str, exists: bool = True, control: bool = False) -> Case:
    """case e: case b for the store (no lock quadrants).  N is inserted by pass 0 -- or, exists=False, never: NOT_EXIST for its READs
    and SETs beside the hot key's successful ones"""
    n_key = int(kvkeys.keys_like(STORE_HOT, STORE_HS, 1, same_kh=not control, same_quadrant=None, seed=15)[0])
    hb = int(kvkeys.np_bucket([STORE_HOT], STORE_HS)[0])
    rng = np.random.default_rng(8)
    first = store_noise(200, 2, hb)
    if exists:
        first["type"][20], first["key"][20] = S.INSERT, n_key
    passes = [first]
    c = Case(W.STORE, dict(n_rows=N_STORE), N_STORE, passes)
    p_h = 0.35 if share == "equal" else 0.6
    hot_min = {}
    for k, n in enumerate(HOT_PASSES):
        req = store_noise(n, 17 * k + 6, hb)
        u = rng.random(n)
        h_sel = u < p_h
        _overlay(req, rng, None, STORE_HOT, h_sel, [S.READ, S.SET], [0.7, 0.3])
        if k < len(HOT_PASSES) - 1:
            n_sel = _cold_sel(rng, ~h_sel, cold_count(n)) if share == "cold" else (u >= p_h) & (u < p_h + (0.06 if share == "warm" else 0.35))
            _overlay(req, rng, None, n_key, n_sel, [S.READ, S.SET], [0.7, 0.3])
        passes.append(req)
        hot_min[k + 1] = int(0.8 * p_h * n)
    ex = list(range(1, len(HOT_PASSES)))
    c.pairs = [] if control else [(0, [STORE_HOT, n_key], ex)]
    c.control = (0, STORE_HOT, n_key) if control else None
    c.hot = [(0, STORE_HOT, hot_min)] + ([(0, n_key, {k: hot_min[k] for k in ex})] if share == "equal" else [])
    c.cold = [(0, n_key, ex)] if share == "cold" else []
    return c.replayed()


@functools.lru_cache(None)
def store_rem_pair() -> Case:
    """case d for the store: N1 and N2 behind one key hash that is not the hot key's, in its bucket, a handful of requests each"""
    n1 = int(kvkeys.keys_like(STORE_HOT, STORE_HS, 1, same_kh=False, same_quadrant=None, seed=16)[0])
    n2 = int(kvkeys.keys_like(n1, STORE_HS, 1, same_kh=True, same_quadrant=None, seed=17, exclude=(STORE_HOT,))[0])
    hb = int(kvkeys.np_bucket([STORE_HOT], STORE_HS)[0])
    rng = np.random.default_rng(9)
    first = store_noise(200, 3, hb)
    first["type"][20], first["key"][20] = S.INSERT, n1
    first["type"][50], first["key"][50] = S.INSERT, n2
    passes = [first]
    c = Case(W.STORE, dict(n_rows=N_STORE), N_STORE, passes)
    hot_min = {}
    for k, n in enumerate(HOT_PASSES):
        req = store_noise(n, 29 * k + 6, hb)
        u = rng.random(n)
        h_sel = u < 0.6
        _overlay(req, rng, None, STORE_HOT, h_sel, [S.READ, S.SET], [0.7, 0.3])
        free = ~h_sel
        for key in (n1, n2):
            sel = _cold_sel(rng, free, cold_count(n))
            free &= ~sel
            _overlay(req, rng, None, key, sel, [S.READ, S.SET], [0.5, 0.5])
        passes.append(req)
        hot_min[k + 1] = int(0.5 * n)
    ex = list(range(1, len(HOT_PASSES) + 1))
    c.pairs = [(0, [n1, n2], ex)]
    c.cold = [(0, n1, ex), (0, n2, ex)]
    c.hot = [(0, STORE_HOT, hot_min)]
    return c.replayed()


@functools.lru_cache(None)
def store_chunks() -> Case:
    """case a: eight groups of three keys behind one (bucket, key hash), READ / SET / INSERT of them among ordinary noise.  A key is
    inserted by the trace the first time the draw says INSERT (a later INSERT of it becomes a SET), read and set before and after;
    one key of every group is never inserted.  At most ~10 requests per key and pass."""
    groups = kvkeys.collision_groups(STORE_HS, 8, 3, seed=30)
    keys = groups.ravel()
    never = set(groups[:, 2].tolist())
    rng = np.random.default_rng(10)
    live, passes = set(), []
    for k, n in enumerate(CHUNK_PASSES):
        req = tracegen.store_random(n, seed=50 + k, n_sub_touch=900, p_set=0.4, p_insert=0.05)
        at = np.sort(rng.choice(n, min(n // 4, 240), replace=False))
        for i in at:
            key = int(keys[rng.integers(len(keys))])
            ty = rng.choice([S.READ, S.SET, S.INSERT], p=[0.45, 0.3, 0.25])
            if ty == S.INSERT and (key in live or key in never):
                ty = S.SET
            if ty == S.INSERT:
                live.add(key)
            req["key"][i], req["type"][i] = key, ty
        passes.append(req)
    c = Case(W.STORE, dict(n_rows=N_STORE), 1500, passes)
    c.pairs = [(0, g.tolist(), []) for g in groups]
    return c.replayed()


# ---- smallbank ----------------------------------------------------------------------------------------------------------------
SB_MIX = ([0, 1, 2, 3, 4, 5], [0.3, 0.25, 0.15, 0.12, 0.1, 0.08])
SB_ACCT = 200_000


@functools.lru_cache(None)
def sb_hs(n_acct):
    return orc.SmallbankOracle(n_acct, log_entries=16, populate_n=1).hash_size(0)


@functools.lru_cache(None)
def sb_pair(same_quadrant: bool, populated: bool = True):
    """(H, N, n_acct): two POPULATED accounts of an engine of 200,000 behind one (bucket, key hash) -- or account 7 of an engine of
    2,000 and a searched key that is no account (counted in missing_keys)"""
    if populated:
        p = kvkeys.colliding_pairs(np.arange(SB_ACCT, dtype=np.uint64), sb_hs(SB_ACCT), same_quadrant)
        return int(p[0][0]), int(p[0][1]), SB_ACCT
    n = int(kvkeys.keys_like(7, sb_hs(2000), 1, same_kh=True, same_quadrant=same_quadrant, seed=18)[0])
    return 7, n, 2000


def sb_noise(n, seed, n_acct, avoid):
    """sb_random over the first 2,000 accounts, kept off the accounts in `avoid`' buckets"""
    req = tracegen.sb_random(n, seed=seed, n_acct_touch=2000)
    hs = sb_hs(n_acct)
    bad = np.isin(kvkeys.np_bucket(req["key"], hs), kvkeys.np_bucket(np.array(avoid, np.uint64), hs))
    ok = np.nonzero(~np.isin(kvkeys.np_bucket(np.arange(2000, dtype=np.uint64), hs), kvkeys.np_bucket(np.array(avoid, np.uint64), hs)))[0]
    req["key"][bad] = ok[(req["key"][bad] % np.uint64(len(ok))).astype(np.int64)]
    return req


@functools.lru_cache(None)
def sb_hot_pair(same_quadrant: bool, share: str, populated: bool = True, both_rows: bool = False) -> Case:
    """case f: the savings row of account H is hot (60 % of a pass; both_rows: its savings and its checking row, 30 % each) and
    account N collides with it, in table 0 only; "cold" = 1 .. 8 requests of N per pass, "warm" = 10 %"""
    h_key, n_key, n_acct = sb_pair(same_quadrant, populated)
    rng = np.random.default_rng(3)
    c = Case(W.SMALLBANK, dict(n_rows=n_acct, log_entries=400_000), n_acct, [], log_cap=400_000)
    hot_rows = [(0, h_key), (1, h_key)] if both_rows else [(0, h_key)]
    mins = [{} for _ in hot_rows]
    for k, n in enumerate(SB_PASSES):
        req = sb_noise(n, 50 + k, n_acct, (h_key, n_key))
        u = rng.random(n)
        h_sel = u < 0.6
        for j, (tb, key) in enumerate(hot_rows):
            _overlay(req, rng, tb, key, (u >= 0.6 * j / len(hot_rows)) & (u < 0.6 * (j + 1) / len(hot_rows)), *SB_MIX)
            mins[j][k] = int(0.5 * n / len(hot_rows))
        n_sel = _cold_sel(rng, ~h_sel, cold_count(n)) if share == "cold" else (u >= 0.6) & (u < 0.7)
        _overlay(req, rng, 0, n_key, n_sel, *SB_MIX)
        c.passes.append(req)
    ex = list(range(len(SB_PASSES)))
    c.pairs = [(0, [h_key, n_key], ex)]
    c.hot = [(tb, key, m) for (tb, key), m in zip(hot_rows, mins)]
    c.cold = [(0, n_key, ex)] if share == "cold" else []
    return c.replayed()


@functools.lru_cache(None)
def sb_chunks() -> Case:
    """case a: all seven ops on accounts that collide, both tables -- eight pairs of POPULATED accounts of an engine of 200,000
    (it holds about one triple) and four groups of three keys that are no accounts, among sb_random's noise"""
    hs = sb_hs(SB_ACCT)
    pop = kvkeys.collision_groups(hs, 8, 2, seed=31, key_of=lambda cand: np.asarray(cand, np.uint64) % np.uint64(SB_ACCT))
    miss = kvkeys.collision_groups(hs, 4, 3, seed=32)
    keys = np.concatenate([pop.ravel(), miss.ravel()])
    rng = np.random.default_rng(11)
    passes = []
    for k, n in enumerate(CHUNK_PASSES):
        req = tracegen.sb_random(n, seed=60 + k, n_acct_touch=2000)
        at = rng.choice(n, min(n // 4, 280), replace=False)
        req["key"][at] = keys[rng.integers(0, len(keys), len(at))]
        passes.append(req)
    c = Case(W.SMALLBANK, dict(n_rows=SB_ACCT, log_entries=400_000), SB_ACCT, passes, log_cap=400_000)
    c.pairs = [(t, g.tolist(), []) for t in range(2) for g in list(pop) + list(miss)]
    return c.replayed()


# ---- every case the GPU tests run, by name (the host tests check each one's preconditions) ------------------------------------------
SHARES = ("cold", "warm", "equal")
CASES = {"a-store": store_chunks, "a-tatp": tatp_chunks, "a-smallbank": sb_chunks, "d-tatp": tatp_rem_pair, "d-store": store_rem_pair}
for _sh in SHARES:
    for _sq in (False, True):
        CASES[f"b-{'same' if _sq else 'other'}-quadrant-{_sh}"] = functools.partial(tatp_hot_pair, _sq, _sh)
    CASES[f"b-control-{_sh}"] = functools.partial(tatp_hot_pair, False, _sh, True)
    CASES[f"e-{_sh}"] = functools.partial(store_hot_pair, _sh)
    CASES[f"e-control-{_sh}"] = functools.partial(store_hot_pair, _sh, True, True)
for _sh in ("cold", "warm"):
    CASES[f"e-missing-{_sh}"] = functools.partial(store_hot_pair, _sh, False)
    for _sq in (False, True):
        CASES[f"f-{'same' if _sq else 'other'}-quadrant-{_sh}"] = functools.partial(sb_hot_pair, _sq, _sh)
    CASES[f"f-no-account-{_sh}"] = functools.partial(sb_hot_pair, True, _sh, False)
    CASES[f"f-both-rows-{_sh}"] = functools.partial(sb_hot_pair, False, _sh, True, True)
for _p in CF_MIXES:
    for _nw in (False, True):
        CASES[f"c-{_p}-{'writes' if _nw else 'reads'}"] = functools.partial(tatp_cf_pair, _p, _nw)
