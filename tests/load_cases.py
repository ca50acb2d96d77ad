"""Row sets for the bulk load (dint_load_rows_device; the rule is dint_amd/csrc/state_load.h) whose rows per bucket are chosen so
that runs, totals and chains sit at the edges of the load kernels' tiles, workgroups and waves (test tooling, numpy only;
tests/test_gpu_load_edges.py runs them on the GPU, tests/test_load_cases_host.py checks from the keys alone that every one of
them holds what it promises, and holds the host form of the rule and the serial kvs_insert twin to the same promise).

The direct load decides every row's position by arithmetic over the rows SORTED by local bucket: a stable radix sort, a max-scan
for the run heads, a sum-scan whose low half is the pool index, a build that reads scan[p - 4] and scan[h + 4 * last].  Whether
that arithmetic is right depends on where a bucket's run starts and ends in the sorted order, which no random row set chooses.
A case here is planned as rows per GLOBAL bucket; keys come from kvkeys.keys_by_bucket, the insertion order is a permutation, and
the promise is computed from the plan, never from the keys:

    n_local, per_local   rows per local bucket, in sorted order (the foreign rows sort last)
    runs                 {name: (sorted position where the bucket's run starts, its rows)}
    rows, foreign        rows home to the shard / to another
    need, longest        overflow entries sum(max(ceil(k / 4) - 1, 0)), entries of the longest chain ceil(max k / 4)
    pool_top             pool_top afterwards (= need; with rows held before, the need of both row sets together)
    direct, refused      1 / 0: the table is built directly / by passes; None or the error the load returns
    visible              (dup) {key: row number of the row a lookup must see}

The constants the cases depend on are read from the headers and asserted: a changed constant makes someone look here again."""
from __future__ import annotations

import functools
import os
import re
import zlib
from collections import namedtuple

import numpy as np

from dint_amd import wire
from kvkeys import keys_by_bucket, np_bucket, overflow_need

W = wire.Workload
ESTATE = -5
CSRC = os.path.join(os.path.dirname(os.path.abspath(wire.__file__)), "csrc")


def _const(name, pattern):
    with open(os.path.join(CSRC, name)) as f:
        m = re.search(pattern, f.read())
    assert m, pattern
    return int(m.group(1))


SL_TILE = _const("state_load.h", r"#define SL_TILE (\d+)u")            # subscribers per workgroup of the generation kernel
KV_MAX_CHAIN = _const("dint_kv_core.h", r"#define KV_MAX_CHAIN (\d+)u")  # entries a walk visits at most: the longest chain a load accepts
SD_TB = _const("state_dev.h", r"#define SD_TB (\d+)u")                  # threads per workgroup of the plan kernels
WAVE = 64
assert (SL_TILE, KV_MAX_CHAIN, SD_TB) == (256, 4096, 256)

Case = namedtuple("Case", "name workload engine table keys vers vals promise prior offset")
# workload, table, value bytes: the store's 256-byte entries and smallbank's 128-byte ones (CHECKING, its second table)
TARGETS = {"store": (W.STORE, 0, 40), "smallbank": (W.SMALLBANK, 1, 8)}
CYCLE = (1, 4, 5, 8, 9)          # rows per bucket around the named runs: 1, a full entry, one more, two entries, one more
PER = (0, 1, 4, 5, 8, 9, 41)     # the pattern of tests/test_gpu_state_load.py
N_EDGES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)
ONE_BUCKET = (1, 3, 4, 5, 8, 9, 12, 13, 16, 17)
MIN_PASS = 64                    # the smallest max_pass an engine accepts (engine.hip: smaller values are raised to it)
MAX_ROWS = 20_000


def hash_size(wl, n_rows):
    """recovery.hash_sizes for the two tables used here"""
    return n_rows * 18 // 4 if wl == W.STORE else n_rows * 3 // 2 // 4


def engine_rows(wl, hs):
    """the n_rows that gives the table exactly hs buckets"""
    n = -(-4 * hs // 18) if wl == W.STORE else -(-8 * hs // 3)
    assert hash_size(wl, n) == hs, (wl, hs)
    return n


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _vals(n, vs, salt=0):
    return ((np.arange(n)[:, None] * 7 + np.arange(vs)[None, :] + salt) % 251).astype(np.uint8)


def _filler(total, start=0):
    """runs from CYCLE, in its order, that hold exactly `total` rows"""
    out, i = [], start
    while total > 0:
        c = CYCLE[i % len(CYCLE)]
        i += 1
        if c > total:
            c = max(x for x in CYCLE if x <= total)
        out.append(c)
        total -= c
    return out


def _pad(per, hs):
    assert len(per) <= hs, (len(per), hs)
    return np.array(list(per) + [0] * (hs - len(per)), np.int64)


def local_plan(hs, shard, per_global):
    """(rows per local bucket, foreign rows) of a plan under shard = (index, count)"""
    index, count = shard
    g = np.arange(hs)
    home = g % count == index
    per_local = np.zeros(-(-hs // count), np.int64)
    per_local[g[home] // count] = per_global[home]
    return per_local, int(per_global[~home].sum())


def _case(name, target, hs, per_global, keys, *, shard=(0, 1), runs=None, versions=True, max_pass=0, pool=None, prior=None, offset=0,
          refused=None, visible=None, vers_from=1000, salt=None):
    """a case from its plan and keys that follow it (in insertion order)"""
    wl, table, vs = TARGETS[target]
    per_local, foreign = local_plan(hs, shard, per_global)
    starts = np.concatenate([[0], np.cumsum(per_local)])[:-1]
    together = per_local if prior is None else per_local + local_plan(hs, shard, prior[3])[0]
    need = overflow_need(per_local)
    promise = {
        "hash_size": hs, "n_local": len(per_local), "per_local": tuple(int(x) for x in per_local),
        "runs": {k: (int(starts[b // shard[1]]), int(per_global[b])) for k, b in (runs or {}).items()},
        "rows": int(per_local.sum()), "foreign": foreign, "need": need, "longest": -(-int(per_local.max()) // 4),
        "pool_top": overflow_need(together), "direct": 0 if prior is not None else 1, "refused": refused, "visible": visible or {},
    }
    engine = {"n_rows": engine_rows(wl, hs), "pool_entries": max(1, promise["pool_top"]) if pool is None else pool, "shard_index": shard[0],
              "shard_count": shard[1], "max_pass": max_pass}
    n = len(keys)
    assert n == int(per_global.sum())
    vers = (np.arange(n) + vers_from).astype("<u4") if versions else None
    return Case(name, wl, engine, table, np.ascontiguousarray(keys, "<u8"), vers, _vals(n, vs, _seed(name) % 97 if salt is None else salt), promise,
                None if prior is None else prior[:3], offset)


def _planned(name, target, hs, per_global, *, fix=None, **kw):
    """keys for the plan, insertion order permuted; fix(keys, bucket of every key) may overwrite keys (duplicates) and returns `visible`"""
    per_global = _pad(per_global, hs)
    keys = keys_by_bucket(hs, per_global, seed=_seed(name))
    keys = keys[np.random.default_rng(_seed(name)).permutation(len(keys))]
    if fix:
        kw["visible"] = fix(keys, np_bucket(keys, hs).astype(np.int64))
    return _case(name, target, hs, per_global, keys, **kw)


# ---- the cases --------------------------------------------------------------------------------------------------------------
_REG, GROUPS = {}, {}


def _reg(group, name, fn):
    assert name not in _REG
    _REG[name] = fn
    GROUPS.setdefault(group, []).append(name)


def _cycle_to(total, cycle):
    per, i = [], 0
    while total > 0:
        per.append(min(cycle[i % len(cycle)], total))
        total -= per[-1]
        i += 1
    return per


def _straddle_plan(variant):
    """(rows per bucket, {run name: bucket}): "a" = 9 rows from sorted position 60 (over the wave's edge at 64) and 17 from 250 (over
    the workgroup's at 256), "b" = 17 from 63 and 9 from 253; runs of CYCLE before, between and after"""
    (p0, k0), (p1, k1) = (((WAVE - 4, 9), (SD_TB - 6, 17)) if variant == "a" else ((WAVE - 1, 17), (SD_TB - 3, 9)))
    per = _filler(p0)
    b0 = len(per)
    per += [k0] + _filler(p1 - p0 - k0, start=2)
    b1 = len(per)
    per += [k1] + list(CYCLE) * 2
    return per, {"run%d" % k0: b0, "run%d" % k1: b1}


def _longest_plan(where, hs):
    per = (list((4, 3, 1, 2, 4, 0, 4)) * (hs // 7 + 1))[:hs]
    b = {"first": 0, "middle": hs // 2, "last": hs - 1}[where]
    per[b] = 41
    if where == "last":
        assert all(p == 0 for p in per[b + 1:])
    return per, {"longest": b}


@functools.lru_cache(maxsize=None)
def _chain_keys():
    """4 * KV_MAX_CHAIN + 1 distinct keys of the last bucket of 72"""
    hs, want = 72, 4 * KV_MAX_CHAIN + 1
    cand = np.unique(np.random.default_rng(41).integers(1, 1 << 48, 110 * want, dtype=np.uint64))
    keys = cand[np_bucket(cand, hs) == np.uint64(hs - 1)]
    assert len(keys) >= want
    return keys[np.random.default_rng(42).permutation(len(keys))[:want]]


def _chain(name, over):
    hs, n = 72, 4 * KV_MAX_CHAIN + (1 if over else 0)
    per = np.zeros(hs, np.int64)
    per[hs - 1] = n
    return _case(name, "store", hs, per, _chain_keys()[:n], runs={"chain": hs - 1}, pool=KV_MAX_CHAIN + (8 if over else -1),
                 refused=ESTATE if over else None, salt=5)


def _dup_fix(bucket):
    """in `bucket` (13 rows): the key of row 2 again in rows 5 and 12 (entries 0, 1 and 3), the key of row 8 again in row 10 (entry 2 twice)"""
    def fix(keys, g):
        at = np.nonzero(g == bucket)[0]
        assert len(at) == 13
        keys[at[5]] = keys[at[12]] = keys[at[2]]
        keys[at[10]] = keys[at[8]]
        # a lookup sees the first row in chain order: the earliest row of the NEWEST entry that holds the key
        return {int(keys[at[2]]): int(at[12]), int(keys[at[8]]): int(at[8])}
    return fix


def _shard_per(hs):
    return np.array((list(PER) * (hs // len(PER) + 1))[:hs], np.int64)


PRIOR_PER = {1: 5, 4: 3}  # the 8 rows a table of the `passes` cases holds before: global buckets 1 and 4 (home to shard 1 of 3 as well)


@functools.lru_cache(maxsize=None)
def _prior(target):
    hs, vs = 72, TARGETS[target][2]
    per = np.zeros(hs, np.int64)
    for b, k in PRIOR_PER.items():
        per[b] = k
    keys = keys_by_bucket(hs, per, seed=977)
    return keys, (np.arange(len(keys)) + 50).astype("<u4"), _vals(len(keys), vs, 13), per


def _build_registry():
    for target in TARGETS:
        def reg(group, variant, fn, target=target):
            name = f"{group}-{variant}-{target}" if variant else f"{group}-{target}"
            _reg(group, name, functools.partial(fn, name, target))

        for n in N_EDGES:
            reg("n-edges", str(n), lambda name, target, n=n: _planned(name, target, 360, _cycle_to(n, (3, 0, 1, 2))))
        for v in "ab":
            def straddle(name, target, v=v, **kw):
                per, runs = _straddle_plan(v)
                return _planned(name, target, 72, per, runs=runs, **kw)
            reg("run-straddle", v, straddle)
            if v == "a":
                for off in (8, 24):
                    reg("offset-arrays", str(off), functools.partial(straddle, offset=off))
        for where in ("first", "middle", "last"):
            def longest(name, target, where=where):
                per, runs = _longest_plan(where, 270)
                return _planned(name, target, 270, per, runs=runs)
            reg("longest", where, longest)
        for k in ONE_BUCKET:
            def one(name, target, k=k):
                per = np.zeros(72, np.int64)
                per[37] = k
                return _planned(name, target, 72, per, runs={"all": 37})
            reg("one-bucket", str(k), one)

        def dup(name, target):
            per = _pad((list(CYCLE) * 5)[:24], 72)
            per[20] = 13
            return _planned(name, target, 72, per, runs={"dup": 20}, fix=_dup_fix(20))
        reg("dup", "", dup)
        # 72 buckets over 9 shards: n_local = 8, a power of two (the foreign rows' sort key is 8 itself); over 11: n_local = 7
        for count in (9, 11):
            for index in range(count):
                reg("shard-pow2", f"{index}of{count}", lambda name, target, s=(index, count): _planned(name, target, 72, _shard_per(72), shard=s))
        reg("all-foreign", "", lambda name, target: _planned(name, target, 72, [0 if g % 3 == 1 else CYCLE[g % 5] for g in range(72)], shard=(1, 3), pool=64))
        for n in (MIN_PASS - 1, MIN_PASS, MIN_PASS + 1, 3 * MIN_PASS + 7):
            for versions in (True, False):
                for shard in ((0, 1), (1, 3)):
                    v = f"{n}-{'vers' if versions else 'nover'}-{'whole' if shard[1] == 1 else '1of3'}"
                    reg("passes", v, lambda name, target, n=n, versions=versions, shard=shard: _planned(
                        name, target, 72, _filler(n), shard=shard, versions=versions, max_pass=MIN_PASS, pool=256, prior=_prior(target)))
    _reg("chain", "chain-max-store", lambda: _chain("chain-max-store", False))
    _reg("chain", "chain-over-store", lambda: _chain("chain-over-store", True))


_build_registry()
NAMES = list(_REG)
DIRECT_GROUPS = ("n-edges", "run-straddle", "longest", "one-bucket", "dup", "shard-pow2")
DIRECT = [n for g in DIRECT_GROUPS for n in GROUPS[g]]


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return _REG[name]()


# ---- the populations of the dint_populate_device tests -------------------------------------------------------------------------
# in this order the process-wide tile table of the generator grows (513, 1025) and is read as a prefix (1, 256, 255, ...) whatever
# it held before; every n is a multiple of SL_TILE, one more, one less, or smaller than a tile
POPULATIONS = (2 * SL_TILE + 1, 1, SL_TILE, 4 * SL_TILE + 1, SL_TILE - 1, 2 * SL_TILE, SL_TILE + 1, 2, 3 * SL_TILE)
assert POPULATIONS == (513, 1, 256, 1025, 255, 512, 257, 2, 768)
POP_N_ROWS = 64
# dint_populate_device refused at a later table: tatp, n_rows = 64, 600 subscribers, a pool that fits SUBSCRIBER and SECONDARY
# SUBSCRIBER (24 buckets, 600 rows each) exactly and so not ACCESS INFO (60 buckets, about 1,500 rows)
REFUSED = {"n_rows": 64, "n": 600, "fits": 2}
