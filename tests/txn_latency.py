"""Helpers for the transaction latency tests (include/dint_driver.h struct dint_driver_latency, dint_amd/csrc/txn_latency.h).

The expectation for the round-trip fields is derived here from statistics the drivers had before they kept any latency: a
one-client driver finishes at most one transaction per epoch, so comparing stats() after every next() with the call before
gives, per finished transaction, its type (the by_type delta), whether it committed (the committed_by_type delta) and its
round trips: this epoch minus the epoch of the previous finish -- the next transaction begins in the phase the last one
finished in."""
import numpy as np

RT_BINS, TICK_BINS = 32, 240
RT_KEYS = ("round_trips", "aborted_round_trips", "rt_sum", "rt_max")
TICK_KEYS = ("ticks", "tick_sum", "tick_max")

# tests/golden/clients_block.npz, all 96 clients summed: {round trips: transactions}, derived as above on the commit before
# the drivers kept any latency
BLOCK_TABLE = {
    "tatp": ({1: 4492, 2: 183, 5: 66, 6: 969, 7: 48}, {1: 1317, 2: 545, 3: 158, 4: 42}),
    "smallbank": ({2: 226, 5: 1218}, {1: 85, 2: 335, 3: 141}),
}


def empty():
    return {"round_trips": np.zeros((8, RT_BINS), np.uint64), "aborted_round_trips": np.zeros((8, RT_BINS), np.uint64),
            "rt_sum": np.zeros(8, np.uint64), "rt_max": np.zeros(8, np.uint64)}


def add(table, txn, committed, r, n=1):
    if not committed:
        table["aborted_round_trips"][txn, min(r, RT_BINS - 1)] += n
        return
    table["round_trips"][txn, min(r, RT_BINS - 1)] += n
    table["rt_sum"][txn] += n * r
    table["rt_max"][txn] = max(int(table["rt_max"][txn]), r)


def total(tables):
    tables = list(tables)
    out = {k: np.sum([t[k] for t in tables], axis=0, dtype=np.uint64) for k in ("round_trips", "aborted_round_trips", "rt_sum")}
    out["rt_max"] = np.max([t["rt_max"] for t in tables], axis=0).astype(np.uint64)
    return out


def minus(a, b):
    """the histograms and sums of a that b does not hold yet (maxima are not additive: left out)"""
    return {k: a[k] - b[k] for k in ("round_trips", "aborted_round_trips", "rt_sum")}


def assert_rt_equal(got, want, what="", keys=RT_KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], np.uint64), np.asarray(want[k], np.uint64)), (what, k, np.asarray(got[k]).tolist(), np.asarray(want[k]).tolist())


def by_round_trips(table):
    """({r: committed}, {r: aborted}) over all types: the shape of BLOCK_TABLE"""
    c, a = table["round_trips"].sum(axis=0), table["aborted_round_trips"].sum(axis=0)
    return {r: int(n) for r, n in enumerate(c) if n}, {r: int(n) for r, n in enumerate(a) if n}


class Deriver:
    """the round trips of ONE client's transactions from its driver's stats() after every next()"""

    def __init__(self):
        self.prev_by, self.prev_ok = np.zeros(8, np.int64), np.zeros(8, np.int64)
        self.epoch, self.last_finish, self.max_per_epoch = 0, 0, 0
        self.table = empty()
        self.events = []  # (epoch, type, committed, r)

    def step(self, st):
        by, ok = np.array(st["by_type"], np.int64), np.array(st["committed_by_type"], np.int64)
        d_by, d_ok = by - self.prev_by, ok - self.prev_ok
        n = int(d_by.sum())
        self.max_per_epoch = max(self.max_per_epoch, n)
        assert 0 <= n <= 1 and d_by.min() >= 0 and d_ok.min() >= 0, (self.epoch, d_by.tolist())
        if n:
            t = int(np.argmax(d_by))
            committed = bool(d_ok[t])
            assert int(d_ok.sum()) == int(committed)
            r = self.epoch - self.last_finish
            add(self.table, t, committed, r)
            self.events.append((self.epoch, t, committed, r))
            self.last_finish = self.epoch
        self.prev_by, self.prev_ok = by, ok
        self.epoch += 1


def check_against_stats(lat, st):
    """the histograms' sums over r are the per-type counters the driver always had"""
    assert lat["round_trips"].sum(axis=1).tolist() == list(st["committed_by_type"])
    assert lat["aborted_round_trips"].sum(axis=1).tolist() == [a - b for a, b in zip(st["by_type"], st["committed_by_type"])]


class LockstepSingles:
    """n one-client host drivers (first_client + c) whose batches, concatenated in client order, are the batches of one
    n-client driver: step() takes the replies to those batches and hands every client its own; the derivation per client"""

    def __init__(self, wl, n, n_rows, first_client=0, zipf_theta=None):
        from dint_amd.driver import Driver

        self.ds = [Driver(wl, 1, n_rows, first_client=first_client + c, zipf_theta=zipf_theta) for c in range(n)]
        self.der = [Deriver() for _ in range(n)]
        self.counts = None

    def next(self):
        outs = [d.next() for d in self.ds]
        for d, der in zip(self.ds, self.der):
            der.step(d.stats())
        self.counts = np.array([[len(o[s]) for s in range(3)] for o in outs], np.int64)  # [client, shard]
        return [np.concatenate([o[s] for o in outs]) for s in range(3)]

    def consume(self, rep):
        off = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(self.counts, axis=0)])
        for c, d in enumerate(self.ds):
            d.consume([rep[s][off[c, s]:off[c + 1, s]].copy() for s in range(3)])

    def table(self, lo=0, hi=None):
        return total(d.table for d in self.der[lo:hi])

    def close(self):
        for d in self.ds:
            d.close()
