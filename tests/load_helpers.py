"""What the bulk-load tests share (tests/test_gpu_state_load.py, tests/test_gpu_load_edges.py, tests/test_load_cases_host.py):
the population's rows through the rule on the host, the overflow need of a population, the comparisons two twins must pass and
the device forms of numpy arrays.  Nothing here needs a GPU until `dev` or `same_state` is called."""
import numpy as np

from dint_amd import _lib, recovery, wire
from kvkeys import np_bucket, overflow_need

W = wire.Workload
N_TABLES = {W.STORE: 1, W.TATP: 5, W.SMALLBANK: 2}
BAD_VERIFY = ("bad_chains", "cross_linked", "linked_beyond_top", "list_bad_links", "stray_valid_entries", "stray_rows", "misplaced_rows",
              "odd_valid_bytes", "unaccounted")


def rows_host(wl, table, n):
    """the population's rows of one table through the rule on the host (no device call)"""
    L = _lib.load()
    vs = 8 if wl == W.SMALLBANK else 40
    m = L.dint_populate_rows_host(int(wl), table, 0, n, None, None, 0)
    keys = np.zeros(m, "<u8"); vals = np.zeros((m, vs), "u1")
    assert L.dint_populate_rows_host(int(wl), table, 0, n, keys.ctypes.data, vals.ctypes.data, m) == m
    return keys, vals


def table_needs(wl, n_rows, n_pop, shard=(0, 1)):
    """per table of the population: (home rows, foreign rows, overflow need, longest chain in entries) (kvkeys.overflow_need over
    the rows per local bucket)"""
    out = []
    for t, hs in enumerate(recovery.hash_sizes(wl, n_rows)):
        g = np_bucket(rows_host(wl, t, n_pop)[0], hs).astype(np.int64)
        home = g % shard[1] == shard[0]
        per = np.bincount(g[home] // shard[1], minlength=-(-hs // shard[1]))
        out.append((int(home.sum()), int((~home).sum()), overflow_need(per), -(-int(per.max()) // 4)))
    return out


def pool_need(wl, n_rows, n_pop, shard=(0, 1)):
    """the overflow entries the fullest table of the population needs"""
    return max(t[2] for t in table_needs(wl, n_rows, n_pop, shard))


def refused_pool(n_rows, n_pop, fits):
    """a pool that holds the first `fits` tatp tables of the population exactly: what the fullest of them needs"""
    return max(t[2] for t in table_needs(W.TATP, n_rows, n_pop)[:fits])


def verify_clean(e):
    for r in e.state_verify():
        bad = {k: v for k, v in r.items() if k in BAD_VERIFY and v}
        assert not bad, r


def same_state(a, b):
    """every comparison the twins must pass"""
    for t in range(N_TABLES[a.workload]):
        x, y = a.dump_rows(t), b.dump_rows(t)
        assert all(p.shape == q.shape and (p == q).all() for p, q in zip(x, y)), ("rows differ", t, len(x[0]), len(y[0]))
        if a.workload != W.STORE:  # (the store keeps no lock words)
            assert not a.read_locks(t)[0].any() and not a.read_locks(t)[1].any()
    assert a.state_digest() == b.state_digest()
    assert a.state_stats() == b.state_stats()
    verify_clean(a)


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else np.int32 if x.dtype == np.uint32 else x.dtype)).cuda()


def load_dev(e, table, keys, vers, vals):
    return e.load_rows_device(table, dev(keys), None if vers is None else dev(vers), dev(vals))
