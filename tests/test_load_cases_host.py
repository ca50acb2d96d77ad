"""Every case of tests/load_cases.py holds what it promises, shown from its keys alone with the hash kvkeys uses; the host form of
the bulk load's rule (dint_state_load_place_host over a view that holds nothing, as in tests/test_state_load_host.py) gives the same
counts, and the serial kv_insert twin used there the same entries.  The populations and the refused population of
tests/test_gpu_load_edges.py are shown to be what that file says of them.  No device call."""
import ctypes as C

import numpy as np
import pytest

import load_cases as lc
from dint_amd import recovery, wire
from kvkeys import np_bucket, overflow_need
from load_helpers import refused_pool, table_needs
from test_state_load_host import ENOMEM, ESTATE, View, kvh, serial  # noqa: F401  (kvh: the fixture that builds the serial twin)

W = wire.Workload


def recount(c, keys):
    """(rows per local bucket, foreign rows, sorted order) of keys under the case's engine, from the hash alone"""
    hs, idx, cnt = c.promise["hash_size"], c.engine["shard_index"], c.engine["shard_count"]
    g = np_bucket(keys, hs).astype(np.int64)
    home = g % cnt == idx
    n_local = -(-hs // cnt)
    sort_key = np.where(home, g // cnt, n_local)
    return np.bincount(sort_key[home], minlength=n_local), int((~home).sum()), np.sort(sort_key, kind="stable")


@pytest.mark.parametrize("name", lc.NAMES)
def test_a_case_holds_what_it_promises(name):
    c, p = lc.case(name), lc.case(name).promise
    assert 0 < len(c.keys) <= lc.MAX_ROWS and c.vals.shape == (len(c.keys), 8 if c.workload == W.SMALLBANK else 40)
    assert c.vers is None or (c.vers.dtype == np.dtype("<u4") and len(c.vers) == len(c.keys))
    assert recovery.hash_sizes(c.workload, c.engine["n_rows"])[c.table] == p["hash_size"]
    per, foreign, sorted_keys = recount(c, c.keys)
    assert p["n_local"] == len(per) and tuple(per.tolist()) == p["per_local"]
    assert (p["rows"], p["foreign"]) == (int(per.sum()), foreign) and p["rows"] + p["foreign"] == len(c.keys)
    assert p["need"] == overflow_need(per) and p["longest"] == -(-int(per.max()) // 4)
    for run, (pos, k) in p["runs"].items():  # the run starts where the sorted keys first show its bucket, and has its rows
        b = int(sorted_keys[pos])
        assert b < p["n_local"] and per[b] == k and (pos == 0 or sorted_keys[pos - 1] != b) and (sorted_keys[pos:pos + k] == b).all(), run
    if c.prior is not None:
        both = per + recount(c, c.prior[0])[0]
        assert p["direct"] == 0 and recount(c, c.prior[0])[1] == 0 and len(c.prior[0]) == 8 and p["pool_top"] == overflow_need(both)
        assert c.engine["max_pass"] == lc.MIN_PASS and p["pool_top"] <= c.engine["pool_entries"]
    else:
        assert p["direct"] == 1 and p["pool_top"] == p["need"]
        assert p["refused"] is not None or p["need"] <= c.engine["pool_entries"]


def test_the_cases_sit_at_the_edges_they_name():
    G, case = lc.GROUPS, lc.case
    assert set(G) == {"n-edges", "run-straddle", "offset-arrays", "longest", "one-bucket", "dup", "shard-pow2", "all-foreign", "passes", "chain"}
    assert sorted(n for g in G.values() for n in g) == sorted(lc.NAMES) and set(lc.DIRECT) < set(lc.NAMES)
    T, V = lc.SD_TB, lc.WAVE
    for tg in lc.TARGETS:
        assert [len(case(f"n-edges-{n}-{tg}").keys) for n in lc.N_EDGES] == [1, 2, V - 1, V, V + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1]
        assert all(max(case(n).promise["per_local"]) <= 3 and case(n).vers is not None for n in G["n-edges"])
        a, b = case(f"run-straddle-a-{tg}").promise, case(f"run-straddle-b-{tg}").promise
        assert a["runs"] == {"run9": (60, 9), "run17": (250, 17)} and b["runs"] == {"run17": (63, 17), "run9": (253, 9)}
        for p in (a, b):
            # a run over the wave's edge, a run over the workgroup's; rows per bucket before and after from 1, 4, 5, 8, 9
            assert [pos < e < pos + k for (pos, k), e in zip(sorted(p["runs"].values()), (V, T))] == [True, True]
            rest = [k for k in p["per_local"] if k and k != 17]
            assert set(rest) == set(lc.CYCLE) and p["per_local"][0] in lc.CYCLE and [k for k in p["per_local"] if k][-1] in lc.CYCLE
        for off in (8, 24):
            o = case(f"offset-arrays-{off}-{tg}")
            assert o.offset == off and o.promise["runs"] == a["runs"] and off % 8 == 0
        for where in ("first", "middle", "last"):
            p = case(f"longest-{where}-{tg}").promise
            runs = [k for k in p["per_local"] if k]
            at = {"first": 0, "middle": len(runs) // 2, "last": len(runs) - 1}[where]
            assert p["longest"] == 11 and sorted(runs)[-2] <= 4 and 650 <= p["rows"] <= 750
            assert runs.index(41) == at if where != "middle" else len(runs) // 4 < runs.index(41) < 3 * len(runs) // 4
            assert where != "last" or p["per_local"][-1] == 41  # (the table's last bucket as well)
        for k in lc.ONE_BUCKET:
            p = case(f"one-bucket-{k}-{tg}").promise
            assert sorted(p["per_local"])[-2:] == [0, k] and p["need"] == -(-k // 4) - 1
        d = case(f"dup-{tg}")
        g = np_bucket(d.keys, 72).astype(np.int64)
        (k3, see3), (k2, see2) = sorted(d.promise["visible"].items(), key=lambda kv: -int((d.keys == np.uint64(kv[0])).sum()))
        rank = lambda key: [int((g[:i] == g[i]).sum()) for i in np.nonzero(d.keys == np.uint64(key))[0]]  # row numbers in the bucket
        assert [r // 4 for r in rank(k3)] == [0, 1, 3] and [r // 4 for r in rank(k2)] == [2, 2] and d.promise["runs"]["dup"][1] == 13
        assert see3 == np.nonzero(d.keys == np.uint64(k3))[0][2] and see2 == np.nonzero(d.keys == np.uint64(k2))[0][0]
        # n_local a power of two: the foreign rows' sort key needs one bit more than every bucket; and one less than a power of two
        for count, n_local in ((9, 8), (11, 7)):
            for index in range(count):
                c = case(f"shard-pow2-{index}of{count}-{tg}")
                assert c.promise["n_local"] == n_local and c.promise["rows"] > 0 and c.promise["foreign"] > 0
                assert (c.engine["shard_index"], c.engine["shard_count"]) == (index, count)
        assert 8 & 7 == 0 and (7 + 1) & 7 == 0
        assert sum(case(f"shard-pow2-{i}of9-{tg}").promise["per_local"][0] >= 2 for i in range(9)) >= 4  # local bucket 0 is not empty
        f = case(f"all-foreign-{tg}")
        assert f.promise["rows"] == 0 and f.promise["foreign"] == len(f.keys) > 200 and f.promise["need"] == 0
        m = lc.MIN_PASS
        assert sorted({len(case(n).keys) for n in G["passes"]}) == [m - 1, m, m + 1, 3 * m + 7] and len(G["passes"]) == 2 * 16
        assert sum(case(n).vers is None for n in G["passes"]) == 16 and sum(case(n).engine["shard_count"] == 3 for n in G["passes"]) == 16
        assert all(case(n).promise["foreign"] > 0 for n in G["passes"] if case(n).engine["shard_count"] == 3 and len(case(n).keys) > 1)
    cm, co = case("chain-max-store"), case("chain-over-store")
    assert len(cm.keys) == 4 * lc.KV_MAX_CHAIN == 16384 and len(co.keys) == len(cm.keys) + 1 and (co.keys[:-1] == cm.keys).all()
    assert len(np.unique(co.keys)) == len(co.keys) and (co.vals[:-1] == cm.vals).all() and (co.vers[:-1] == cm.vers).all()
    assert cm.promise["longest"] == lc.KV_MAX_CHAIN and cm.promise["need"] == lc.KV_MAX_CHAIN - 1 <= cm.engine["pool_entries"]
    assert co.promise["longest"] == lc.KV_MAX_CHAIN + 1 and co.promise["refused"] == ESTATE and cm.promise["refused"] is None
    assert co.engine["pool_entries"] >= co.promise["need"]  # (the pool is not the reason of the refusal)
    assert sorted(cm.promise["per_local"])[-2:] == [0, 16384]


def walk_equals_serial(kvh, c, keys, vers, vals, pool):
    """the host form's entries against the serial twin's, both from nothing: rows in chain order and pool_top"""
    hs, vs, shard = c.promise["hash_size"], c.vals.shape[1], (c.engine["shard_index"], c.engine["shard_count"])
    view = View(hs, pool, vs, shard=shard)
    rc, s = view.load(keys, vers, vals)
    assert rc == 0 and s.direct == 1
    (k, v, x), top, h = serial(kvh, keys, np.zeros(len(keys), "<u4") if vers is None else vers, vals, hs, pool, vs, shard=shard)
    try:
        _, wk, wv, wx = view.walk()
        assert wk == k.tolist() and wv == v.tolist() and b"".join(wx) == x.tobytes() and view.pool_top() == top
        for key, row in c.promise["visible"].items():  # the row a lookup sees
            got = np.zeros(vs, np.uint8); ver = C.c_uint32()
            b = int(np_bucket(np.array([key], "<u8"), hs)[0])
            assert b % shard[1] == shard[0] and kvh.kvh_get(h, b // shard[1], key, got.ctypes.data, C.byref(ver)) == 0
            assert ver.value == vers[row] and (got == vals[row]).all()
    finally:
        kvh.kvh_destroy(h)
    return s, top


@pytest.mark.parametrize("name", lc.NAMES)
def test_the_host_form_and_the_serial_twin_agree_with_the_promise(kvh, name):
    c, p = lc.case(name), lc.case(name).promise
    shard = (c.engine["shard_index"], c.engine["shard_count"])
    if name.startswith("chain-"):  # counts and the refusal only: 16,384 serial inserts walk 33 million entries
        view = View(p["hash_size"], c.engine["pool_entries"], 40)
        rc, s = view.load(c.keys, c.vers, c.vals)
        assert rc == (ESTATE if p["refused"] else 0) and (s.table[0].overflow_entries, s.table[0].longest_chain_entries) == (p["need"], p["longest"])
        assert view.pool_top() == (0 if p["refused"] else p["need"]) and bool(view.entries.any()) == (not p["refused"])
        return
    s, top = walk_equals_serial(kvh, c, c.keys, c.vers, c.vals, max(1, p["need"]))  # (the pool fits exactly)
    assert (s.rows_loaded, s.foreign_rows, s.table[0].rows) == (p["rows"], p["foreign"], p["rows"])
    assert (s.table[0].overflow_entries, s.table[0].longest_chain_entries, top) == (p["need"], p["longest"], p["need"])
    if p["need"] > 0:  # one entry short: refused with the need
        rc, s = View(p["hash_size"], p["need"] - 1, c.vals.shape[1], shard=shard).load(c.keys, c.vers, c.vals)
        assert rc == ENOMEM and s.table[0].overflow_entries == p["need"]
    if c.prior is not None:  # the rows behind the ones the table holds: one insertion order
        keys, vals = np.concatenate([c.prior[0], c.keys]), np.concatenate([c.prior[2], c.vals])
        vers = np.concatenate([c.prior[1], np.zeros(len(c.keys), "<u4") if c.vers is None else c.vers])
        assert walk_equals_serial(kvh, c, keys, vers, vals, c.engine["pool_entries"])[1] == p["pool_top"]


# ---- the populations ---------------------------------------------------------------------------------------------------------
def test_the_populations_sit_at_the_generator_tile():
    t = lc.SL_TILE
    assert {n % t for n in lc.POPULATIONS} == {0, 1, 2, t - 1} and min(lc.POPULATIONS) < t < max(lc.POPULATIONS)
    grows = [n for i, n in enumerate(lc.POPULATIONS) if n // t > max([m // t for m in lc.POPULATIONS[:i]] or [-1])]
    assert grows == [513, 1025] and len(lc.POPULATIONS) - len(grows) == 7  # the tile table grows twice; the others read a prefix of it
    # one subscriber over three shards: a shard without a row of a table
    per = [table_needs(W.TATP, lc.POP_N_ROWS, 1, (i, 3)) for i in range(3)]
    assert any(rows == 0 for shard in per for rows, _, _, _ in shard) and sum(shard[0][0] for shard in per) == 1
    assert sum(rows for shard in per for rows, _, _, _ in shard) == sum(rows for rows, _, _, _ in table_needs(W.TATP, lc.POP_N_ROWS, 1))


def test_the_refused_population_is_refused_at_a_later_table():
    needs = [need for _, _, need, _ in table_needs(W.TATP, lc.REFUSED["n_rows"], lc.REFUSED["n"])]
    pool = refused_pool(lc.REFUSED["n_rows"], lc.REFUSED["n"], lc.REFUSED["fits"])
    first = next(t for t, need in enumerate(needs) if need > pool)
    assert first == lc.REFUSED["fits"] >= 1 and all(need <= pool for need in needs[:first]) and needs[0] > 0
