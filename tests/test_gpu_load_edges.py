"""dint_load_rows_device and dint_populate_device at the edges of the load kernels' tiles, workgroups, waves and chains
(dint_amd/csrc/k_load.hip, engine.hip load_device_locked / dint_populate_device; the rule is csrc/state_load.h).  The row sets
are tests/load_cases.py's -- tests/test_load_cases_host.py shows from the keys alone that each holds what it promises -- and
every one is loaded into engine `a` on the device and into twin `b` through the host path (dint_load_rows / dint_populate,
unchanged); the populations are also held to the CPU oracle, which shares no code with either.  Every comparison is exact:
rows in dump order, digests, table reports, a clean verify, lock words, and the figures the load reports against the promise."""
import ctypes as C

import numpy as np
import pytest
import torch

import load_cases as lc
from dint_amd import _lib, recovery, wire
from dint_amd.engine import Engine
from kvkeys import raw_submit
from load_helpers import N_TABLES, dev, load_dev, pool_need, refused_pool, same_state, table_needs, verify_clean
from oracle import oracle as orc
from test_state_sync_host import np_digest

pytestmark = pytest.mark.gpu
W = wire.Workload
EINVAL, ENOMEM, ESTATE = -1, -2, -5


def pair(c):
    return Engine(c.workload, **c.engine), Engine(c.workload, **c.engine)


def empty(e):
    return (all(len(e.dump_rows(t)[0]) == 0 for t in range(N_TABLES[e.workload])) and all(d["rows"] == 0 for d in e.state_digest())
            and all(s["pool_top"] == 0 for s in e.state_stats()))


def load_case(e, c, stream=0):
    """the case's rows through dint_load_rows_device; with c.offset the three arrays lie that many bytes into larger allocations"""
    if not c.offset:
        return e.load_rows_device(c.table, dev(c.keys), None if c.vers is None else dev(c.vers), dev(c.vals), stream=stream)
    held = []
    for x in (c.keys, c.vers, c.vals):
        raw = np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
        big = torch.full((len(raw) + 2 * c.offset + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        big[c.offset:c.offset + len(raw)] = torch.from_numpy(raw.copy()).cuda()
        held.append(big)
    torch.cuda.synchronize()
    at = [t.data_ptr() + c.offset for t in held]
    assert all(t.data_ptr() % 256 == 0 for t in held)  # (so the arrays are 8-byte aligned and not at an allocation's base)
    return e.load_rows_device(c.table, at[0], at[1], at[2], stream=stream, n=len(c.keys))


def reported(r, c):
    """what a direct load reports against the promise"""
    p = c.promise
    assert (r["direct"], r["rows_loaded"], r["foreign_rows"]) == (1, p["rows"], p["foreign"])
    assert r["tables"][c.table] == {"rows": p["rows"], "overflow_entries": p["need"], "longest_chain_entries": p["longest"], "direct": 1}


@pytest.mark.parametrize("name", lc.DIRECT + lc.GROUPS["offset-arrays"])
def test_a_direct_load_equals_the_host_loaded_twin_and_reports_the_promise(name):
    c = lc.case(name)
    a, b = pair(c)
    r = load_case(a, c)
    b.load_rows(c.table, c.keys, c.vers, c.vals)
    assert r is a.last_load
    reported(r, c)
    same_state(a, b)
    assert a.state_stats()[c.table]["pool_top"] == c.promise["need"]
    a.close(); b.close()


def read_of(c, key):
    """the request that reads a row: the store's READ; smallbank has none, its ACQUIRE_SHARED returns the row"""
    m = np.zeros(1, wire.MSG_DTYPE[c.workload])
    m["key"] = key
    if c.workload == W.STORE:
        m["type"] = int(wire.Store.READ)
    else:
        m["type"], m["table"] = int(wire.Sb.ACQUIRE_SHARED), c.table
    return m


@pytest.mark.parametrize("tg", list(lc.TARGETS))
def test_a_lookup_sees_the_duplicate_the_serial_load_shows(tg):
    c = lc.case(f"dup-{tg}")
    a, b = pair(c)
    load_case(a, c)
    b.load_rows(c.table, c.keys, c.vers, c.vals)
    if c.workload == W.STORE:
        o = orc.StoreOracle(c.promise["hash_size"])
        o.load(c.keys, c.vers, c.vals)
    else:
        o = orc.SmallbankOracle(c.engine["n_rows"], populate_n=0)
        o.load(c.table, c.keys, c.vers, c.vals)
    assert len(c.promise["visible"]) == 2
    for key, row in c.promise["visible"].items():
        q = read_of(c, key)
        want = o.replay(q)
        (ra, pa), (rb, pb) = raw_submit(a, q), raw_submit(b, q)
        assert ra == rb == 0 and pa.tobytes() == pb.tobytes() == want.tobytes()
        assert (want["val"][0] == c.vals[row]).all() and want["ver"][0] == c.vers[row] and want["type"][0] != q["type"][0]
    a.close(); b.close()


def test_the_longest_chain_a_load_accepts_is_built_and_read_to_its_end():
    """16,384 rows of one bucket: 4096 entries, the inline entry (the 4 rows inserted first) last in the chain.  No host-loaded
    twin: dint_load_rows takes the rows as INSERTs of one bucket, a serial walk of up to 4095 entries each.  The rows are held to
    the rule directly -- newest entry first, four rows in insertion order in each -- to the numpy digest and to the CPU oracle."""
    c = lc.case("chain-max-store")
    n, ent = len(c.keys), lc.KV_MAX_CHAIN
    e = Engine(c.workload, **c.engine)
    r = load_case(e, c)
    reported(r, c)
    assert (r["tables"][0]["longest_chain_entries"], r["tables"][0]["overflow_entries"]) == (ent, ent - 1) == (4096, 4095)
    verify_clean(e)
    assert e.state_stats()[0]["pool_top"] == ent - 1
    assert e.state_digest() == [np_digest(0, c.keys, c.vers, c.vals)]
    order = (np.arange(ent)[::-1, None] * 4 + np.arange(4)[None, :]).reshape(-1)  # chain order: entry 4095 .. 0, slots 0 .. 3
    k, v, x = e.dump_rows(0)
    assert (k == c.keys[order]).all() and (v == c.vers[order]).all() and (x == c.vals[order]).all()
    at = np.concatenate([np.arange(8), np.linspace(8, n - 9, 48).astype(np.int64), np.arange(n - 8, n)])
    assert len(np.unique(at)) == 64
    q = np.zeros(64, wire.STORE_MSG)
    q["type"], q["key"] = int(wire.Store.READ), c.keys[at]
    o = orc.StoreOracle(c.promise["hash_size"])
    o.load(c.keys, c.vers, c.vals)
    want = o.replay(q)
    rc, got = raw_submit(e, q)
    assert rc == 0 and (got["type"] == int(wire.Store.GRANT_READ)).all()
    assert (got["val"] == c.vals[at]).all() and (got["ver"] == c.vers[at]).all() and got.tobytes() == want.tobytes()
    e.close()


def test_one_row_more_than_the_longest_chain_is_refused_with_nothing_written():
    c = lc.case("chain-over-store")
    e = Engine(c.workload, **c.engine)
    with pytest.raises(_lib.DintError, match="dint error -5"):
        load_case(e, c)
    assert e.last_load["tables"][0]["longest_chain_entries"] == lc.KV_MAX_CHAIN + 1 and e.last_load["rows_loaded"] == 0
    assert empty(e)
    verify_clean(e)
    small = lc.case("one-bucket-5-store")  # (the same 72 buckets) still untouched: the direct way
    assert c.promise["hash_size"] == small.promise["hash_size"] and load_case(e, small)["direct"] == 1
    assert len(e.dump_rows(0)[0]) == 5
    e.close()


@pytest.mark.parametrize("tg", list(lc.TARGETS))
def test_rows_that_are_all_foreign_leave_the_tables_empty_and_the_table_touched(tg):
    c, more = lc.case(f"all-foreign-{tg}"), lc.case(f"passes-65-vers-1of3-{tg}")
    assert all(c.engine[k] == more.engine[k] for k in ("n_rows", "shard_index", "shard_count")) and more.promise["pool_top"] <= c.engine["pool_entries"]
    a, b = pair(c)
    r = load_case(a, c)
    b.load_rows(c.table, c.keys, c.vers, c.vals)
    assert (r["rows_loaded"], r["foreign_rows"], r["tables"][c.table]["rows"]) == (0, len(c.keys), 0)
    assert empty(a) and empty(b)
    r = load_case(a, more)  # the table has taken a load: the passes now
    b.load_rows(c.table, more.keys, more.vers, more.vals)
    assert (r["direct"], r["rows_loaded"], r["foreign_rows"]) == (0, more.promise["rows"], more.promise["foreign"])
    same_state(a, b)
    assert len(a.dump_rows(c.table)[0]) == more.promise["rows"] > 0
    a.close(); b.close()


@pytest.mark.parametrize("name", lc.GROUPS["passes"])
def test_rows_into_a_table_that_holds_some_go_by_passes_formed_on_the_device(name):
    c, p = lc.case(name), lc.case(name).promise
    a, b = pair(c)
    assert a.pass_max == b.pass_max == lc.MIN_PASS
    assert load_dev(a, c.table, *c.prior)["direct"] == 1
    b.load_rows(c.table, *c.prior)
    before = a.stats()
    r = load_case(a, c)
    b.load_rows(c.table, c.keys, c.vers, c.vals)
    assert (r["direct"], r["tables"][c.table]["direct"]) == (0, 0)
    assert (r["rows_loaded"], r["foreign_rows"], r["tables"][c.table]["rows"]) == (p["rows"], p["foreign"], p["rows"])
    same_state(a, b)
    assert a.state_stats()[c.table]["pool_top"] == p["pool_top"] and len(a.dump_rows(c.table)[0]) == p["rows"] + 8
    after = a.stats()
    assert (after["batches"], after["requests"]) == (before["batches"], before["requests"])
    a.close(); b.close()


# ---- the population at the generator's tile edges ------------------------------------------------------------------------------
def oracle_dumps(wl, n_rows, n):
    if wl == W.STORE:
        return [orc.StoreOracle(recovery.hash_sizes(wl, n_rows)[0], n).dump()]
    o = orc.TatpOracle(n_rows, populate_n=n) if wl == W.TATP else orc.SmallbankOracle(n_rows, populate_n=n)
    return [o.dump(t) for t in range(N_TABLES[wl])]


@pytest.mark.parametrize("wl", [W.TATP, W.STORE, W.SMALLBANK], ids=["tatp", "store", "smallbank"])
def test_populations_at_tile_edges_equal_the_host_twin_and_the_oracle(wl):
    n_rows = lc.POP_N_ROWS
    for n in lc.POPULATIONS:  # in this order: the tile table grows and is read as a prefix
        figures = table_needs(wl, n_rows, n)
        pool = max(1, pool_need(wl, n_rows, n))
        a, b = Engine(wl, n_rows=n_rows, pool_entries=pool), Engine(wl, n_rows=n_rows, pool_entries=pool)
        r = a.populate_device(n)
        b.populate(n)
        assert (r["direct"], r["foreign_rows"], r["rows_loaded"]) == (1, 0, sum(f[0] for f in figures)), n
        for t, (rows, _, need, longest) in enumerate(figures):
            assert r["tables"][t] == {"rows": rows, "overflow_entries": need, "longest_chain_entries": longest, "direct": 1}, (n, t)
        same_state(a, b)
        for t, want in enumerate(oracle_dumps(wl, n_rows, n)):
            got = a.dump_rows(t)
            assert all(p.shape == q.shape and (p == q).all() for p, q in zip(got, want)), ("rows differ from the oracle's", n, t)
        a.close(); b.close()


@pytest.mark.parametrize("n", [1, lc.SL_TILE + 1])
def test_a_three_shard_set_at_tile_edges_keeps_its_home_rows(n):
    wl, n_rows = W.TATP, lc.POP_N_ROWS
    pools = [max(1, pool_need(wl, n_rows, n, (i, 3))) for i in range(3)]
    dev_set = [Engine(wl, n_rows=n_rows, pool_entries=pools[i], shard_index=i, shard_count=3) for i in range(3)]
    host_set = [Engine(wl, n_rows=n_rows, pool_entries=pools[i], shard_index=i, shard_count=3) for i in range(3)]
    tot = recovery.populate_set(dev_set, n)
    for i in range(3):
        figures = table_needs(wl, n_rows, n, (i, 3))
        host_set[i].populate(n)
        same_state(dev_set[i], host_set[i])
        r = dev_set[i].last_load
        assert (r["direct"], r["rows_loaded"], r["foreign_rows"]) == (1, sum(f[0] for f in figures), sum(f[1] for f in figures))
        for t, (rows, _, need, longest) in enumerate(figures):
            assert (r["tables"][t]["rows"], r["tables"][t]["overflow_entries"], r["tables"][t]["longest_chain_entries"]) == (rows, need, longest)
    assert tot["rows_loaded"] == sum(f[0] for f in table_needs(wl, n_rows, n))
    for e in dev_set + host_set:
        e.close()


def test_a_population_refused_at_a_later_table_keeps_the_tables_before_it():
    """include/dint_abi.h: "A refusal of a table's load leaves that table and the ones behind it empty, the ones before it loaded" """
    n_rows, n, first = lc.REFUSED["n_rows"], lc.REFUSED["n"], lc.REFUSED["fits"]
    figures = table_needs(W.TATP, n_rows, n)
    a = Engine(W.TATP, n_rows=n_rows, pool_entries=refused_pool(n_rows, n, first))
    b = Engine(W.TATP, n_rows=n_rows, pool_entries=max(f[2] for f in figures))
    b.populate(n)
    L, s = _lib.load(), _lib.LoadStats()
    assert L.dint_populate_device(a._h, n, C.byref(s), None) == ENOMEM
    assert s.table[first].overflow_entries == figures[first][2] and s.rows_loaded == sum(f[0] for f in figures[:first])
    da, db, sa, sb = a.state_digest(), b.state_digest(), a.state_stats(), b.state_stats()
    for t in range(5):
        x, y = a.dump_rows(t), b.dump_rows(t)
        if t < first:  # loaded: the host twin's table
            assert all(p.shape == q.shape and (p == q).all() for p, q in zip(x, y)) and len(x[0]) == figures[t][0] > 0
            assert da[t] == db[t] and sa[t]["pool_top"] == sb[t]["pool_top"] == figures[t][2]
            assert (s.table[t].rows, s.table[t].overflow_entries, s.table[t].direct) == (figures[t][0], figures[t][2], 1)
        else:  # refused, or never reached: empty
            assert len(x[0]) == 0 and da[t]["rows"] == 0 and sa[t]["pool_top"] == 0 and s.table[t].rows == 0
    verify_clean(a)
    assert L.dint_populate_device(a._h, n, C.byref(s), None) == ESTATE  # rows have been taken: not blank
    a.reset()
    assert empty(a)
    keys, vals = (np.arange(40, dtype="<u8") + 7), np.full((40, 40), 3, np.uint8)
    assert load_dev(a, 0, keys, None, vals)["direct"] == 1 and len(a.dump_rows(0)[0]) == 40
    a.close(); b.close()


def test_a_timed_load_on_a_callers_stream_builds_the_same_tables():
    c = lc.case("run-straddle-a-store")
    a, b = pair(c)
    a.timing_enable(True)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    r = load_case(a, c, stream=st.cuda_stream)
    b.load_rows(c.table, c.keys, c.vers, c.vals)
    reported(r, c)
    assert all(r["stage_ns"][k] > 0 for k in ("keys", "sort", "plan", "build")), r["stage_ns"]
    same_state(a, b)
    a.close(); b.close()
