"""Hand-built logs for the log fold (dint_amd/csrc/log_fold.h), shared by tests/test_log_fold_host.py (the host form against the
CPU oracle) and tests/test_gpu_log_fold.py (the device call against the unfolded path).  A case is (loads, records): `loads` are
rows put into the replica with load_rows / the oracle's load BEFORE the log -- kvs_insert with an explicit version, so loading a
live key leaves it held twice -- and `records` is the LOG_REC array, in log order.  tatp cases are for 300 subscribers, smallbank
cases for 10,000 accounts; every table is populated as the engine and the oracle populate it."""
import numpy as np

from dint_amd import recovery, wire
from kvkeys import np_bucket
from oracle import oracle as orc

W, T, S = wire.Workload, wire.Tatp, wire.Sb
N_SUB, N_ACCT = 300, 10_000
ABSENT = np.uint64(1 << 46)  # or-ed into a populated key: a key no table holds


def records(table, key, is_del, rng):
    """one row's records: is_del[j] says whether record j is a DELETE_LOG"""
    is_del = np.asarray(is_del, bool)
    r = np.zeros(len(is_del), wire.LOG_REC)
    r["table"], r["key"], r["is_del"] = table, key, is_del
    r["val"] = rng.integers(0, 256, (len(is_del), 40), dtype=np.uint8)
    return r


def interleave(rows, rng):
    """the rows' records merged into one log at random, every row keeping its own order"""
    ids = np.repeat(np.arange(len(rows)), [len(r) for r in rows])
    rng.shuffle(ids)
    out = np.zeros(len(ids), wire.LOG_REC)
    o = np.argsort(ids, kind="stable")
    out[o] = np.concatenate(rows)
    out["ver"] = np.arange(len(out))  # (the replay does not use a record's version: COMMIT_BCK counts)
    return out


def _tatp_rows():
    """(table, key) of populated rows, spread over the five tables"""
    o = orc.TatpOracle(N_SUB, log_entries=16)
    dumps = [o.dump(t) for t in range(5)]
    hs = [o.hash_size(t) for t in range(5)]
    return dumps, hs


def same_bucket_key(key, hash_size, taken, other=False):
    """an absent key of key's bucket (other=True: of another bucket)"""
    cand = np.arange(1, 400_000, dtype=np.uint64) | ABSENT
    cand = cand[~np.isin(cand, taken)]
    same = np_bucket(cand, hash_size) == np_bucket(np.array([key], np.uint64), hash_size)[0]
    return int(cand[~same if other else same][0])


def tatp_cases():
    rng = np.random.default_rng(5)
    dumps, hs = _tatp_rows()

    def present(t, j):
        return int(dumps[t][0][j])

    def absent(t, j):
        return int(dumps[t][0][j] | ABSENT)

    cases = {}
    lens = (1, 63, 64, 65, 255, 256, 257, 1025)
    rows = []
    for j, k in enumerate(lens):  # all commits, on a present and on an absent row; and one delete somewhere inside
        t = j % 5
        rows.append(records(t, present(t, j), np.zeros(k, bool), rng))
        rows.append(records(t, absent(t, j), np.zeros(k, bool), rng))
        d = np.zeros(k, bool)
        d[k // 2] = True
        rows.append(records(t, present(t, 20 + j), d, rng))
        rows.append(records(t, absent(t, 20 + j), d, rng))
    cases["lengths"] = ([], interleave(rows, rng))
    alt = np.tile([False, True], 2000)  # insert / delete, 2,000 times
    for name, key in (("present", present), ("absent", absent)):
        cases[f"ends_in_delete_{name}"] = ([], interleave([records(1, key(1, 3), [False] * 9 + [True], rng)], rng))
        cases[f"commit_after_delete_{name}"] = ([], interleave([records(2, key(2, 4), [False, False, True, False, False, False], rng)], rng))
        cases[f"alternating_{name}"] = ([], interleave([records(3, key(3, 5), alt, rng)], rng))
        cases[f"alternating_then_insert_{name}"] = ([], interleave([records(4, key(4, 6), np.append(alt, False), rng),
                                                                    records(0, key(0, 7), [False] * 3, rng)], rng))
    cases["delete_first_absent"] = ([], interleave([records(0, absent(0, 8), [True], rng), records(1, absent(1, 8), [True, False], rng),
                                                   records(2, absent(2, 8), [True, True], rng)], rng))
    wrap = absent(3, 9)
    cases["version_wraps"] = ([(3, [wrap], [2**32 - 2], np.full((1, 40), 7, np.uint8))], interleave([records(3, wrap, [False] * 5, rng)], rng))
    # a key held twice, a neighbour of its bucket, a key of another bucket
    t = 2
    dup = present(t, 10)
    near = same_bucket_key(dup, hs[t], dumps[t][0])
    far = same_bucket_key(dup, hs[t], dumps[t][0], other=True)
    load = [(t, [dup], [40], np.full((1, 40), 9, np.uint8))]
    pat = [False, False, True, False, True, False, False]
    cases["duplicate_with_neighbour"] = (load, interleave([records(t, dup, pat, rng), records(t, near, pat[::-1], rng),
                                                            records(t, far, pat, rng), records(0, present(0, 11), [False] * 70, rng)], rng))
    cases["all_deferred"] = (load, interleave([records(t, dup, pat, rng), records(t, near, [False, True, False], rng)], rng))
    cases["one_record"] = ([], interleave([records(4, present(4, 12), [False], rng)], rng))
    cases["one_row_5000"] = ([], interleave([records(0, present(0, 13), rng.random(5000) < 0.01, rng)], rng))
    return cases


def smallbank_cases():
    rng = np.random.default_rng(6)
    n = 50_000
    key = rng.integers(0, N_ACCT, n).astype(np.uint64)
    key[rng.random(n) < 0.02] |= ABSENT  # rows no table holds: kvs_set leaves the table alone
    hot = rng.choice(n, 20_000, replace=False)
    key[hot] = 77
    r = np.zeros(n, wire.LOG_REC)
    r["key"], r["table"] = key, rng.integers(0, 2, n)
    r["table"][hot] = 1
    r["val"][:, :8] = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    r["is_del"] = rng.random(n) < 0.1  # (not looked at for smallbank)
    r["ver"] = np.arange(n)
    small = r[:2000].copy()
    return {"hot_account": ([], r), "absent_only": ([], small[(small["key"] & ABSENT) != 0]), "small": ([], small)}


class OracleEngine:
    """what recovery.apply_log needs of an engine, answered by a CPU oracle"""

    def __init__(self, workload, oracle):
        self.workload, self.o = workload, oracle

    def submit(self, m):
        return self.o.replay(m)


def oracle_for(workload, loads):
    o = orc.TatpOracle(N_SUB, log_entries=16) if workload == W.TATP else orc.SmallbankOracle(N_ACCT, log_entries=16)
    for t, keys, vers, vals in loads:
        o.load(t, keys, vers, vals)
    return o


def sorted_rows(dump):
    k, v, x = dump
    x = np.asarray(x)
    packed = [(int(a), int(b), bytes(c)) for a, b, c in zip(k, v, x)]
    return sorted(packed)
