"""Every case of tests/client_edges.py holds what it promises, shown without a GPU: the counts sit at the edges their names
say, by the kernels' own constants; the host clients, closed through the CPU oracles, emit, commit, are refused and roll back
at these counts within the epochs tests/test_gpu_client_edges.py runs (an edge case that never emits, never commits or never
overflows proves nothing); the cap cases' epoch and shard are what the GPU test takes them for.  The 262,657-client case is
checked for its arithmetic only."""
import numpy as np
import pytest

import client_edges as ce
from dint_amd.driver import N_SHARDS

TATP, SMALLBANK, FASST, TPL = ce.TATP, ce.SMALLBANK, ce.FASST, ce.TPL
WL_ID = {TATP: "tatp", SMALLBANK: "smallbank", FASST: "fasst", TPL: "2pl"}


def test_the_constants_are_the_kernels():
    assert ce.TXG_TB % ce.WAVE == 0 and ce.LCG_TB % ce.WAVE == 0 and ce.TXG_TB > ce.WAVE + 1 and ce.LCG_TB > ce.WAVE + 1
    assert ce.LOCK_PASS % ce.LCG_TB == 0 and ce.LCG_VEC == 16
    assert (ce.MSG[FASST], ce.MSG[TPL]) == (9, 6)


def test_transaction_counts_sit_where_their_names_say():
    TB = ce.TXG_TB
    assert ce.TXN_COUNTS == [1, 2, 63, 64, 65, TB - 1, TB, TB + 1, 2 * TB - 1, 2 * TB, 2 * TB + 1]
    for c in ce.TXN_CASES + [ce.TXN_DEEP]:
        tiles = -(-c.n // TB)
        assert (tiles, c.n - (tiles - 1) * TB) == (c.tiles, c.last), c.name
    assert set(ce.TXN_UNFUSED) <= set(ce.TXN_COUNTS) and {n for n, _ in ce.TXN_WAVES} <= set(ce.TXN_COUNTS)


def test_the_deep_case_needs_a_second_look_back_step_of_one_entry():
    """workgroup w looks at the workgroups w - 1 .. 0, TXG_TB of them per step (thread t of step j at w - 1 - j * TXG_TB - t)"""
    TB, d = ce.TXG_TB, ce.TXN_DEEP
    assert d.n == TB * (TB + 1) + 1 and d.tiles == TB + 2 and d.last == 1
    assert d.n == 262_657 and d.tiles == 514  # at the constants as they are: the figures of the case's description

    def steps(w):  # real entries per step
        return [min(TB, w - j) for j in range(0, w, TB)]
    assert steps(TB - 1) == [TB - 1] and steps(TB) == [TB] and steps(TB + 1) == [TB, 1]
    assert max(len(steps(w)) for w in range(d.tiles)) == 2
    assert all(len(steps(-(-n // TB) - 1)) <= 1 for n in ce.TXN_COUNTS)  # the small counts never take a second step


def test_the_small_workgroup_build_walks_many_steps():
    """the same arithmetic at the workgroup size of dint_amd/libdint_txn_small.so"""
    TB = ce.SMALL_TB
    assert TB % ce.WAVE == 0 and ce.WAVE < TB < ce.TXG_TB and "#ifndef TXG_TB" in ce._TXN
    for c in ce.TXN_SMALL_CASES:
        tiles = -(-c.n // TB)
        assert (tiles, c.n - (tiles - 1) * TB) == (c.tiles, c.last), c.name
    deep, resident, beyond = ce.TXN_SMALL_CASES
    assert deep.tiles == TB + 2 and deep.last == 1              # the last workgroup: one full step, then one real entry
    assert 2 * TB < resident.tiles - 1 <= 5 * TB                # walks of three to five steps when all run at once
    assert beyond.tiles > 8 * TB and beyond.n == ce.TXN_DEEP.n  # more workgroups than a CU's waves and LDS let be resident


@pytest.mark.parametrize("wl", [FASST, TPL], ids=WL_ID.get)
def test_lock_counts_sit_where_their_names_say(wl):
    TB, m, V = ce.LCG_TB, ce.MSG[wl], ce.LCG_VEC
    counts = ce.LOCK_COUNTS[wl]
    assert counts[:9] == [1, 2, 63, 64, 65, TB - 1, TB, TB + 1, 2 * TB + 1]
    assert counts[-3:] == [65_535, 65_536, 65_537] and len(counts) == 15 == len(set(counts))
    for c in ce.LOCK_CASES[wl]:
        tiles = -(-c.n // TB)
        last = c.n - (tiles - 1) * TB
        assert (tiles, last) == (c.tiles, c.last), c.name
        assert last * m % V == c.n * m % V == c.tail, c.name  # the last workgroup's bytes past its whole vectors
    # the three byte-tail counts: the smallest above one vector's worth of workers that end on a vector, just after one (a tail
    # of the smallest size there is) and just before one (the largest)
    res = ce.tail_residues(m)
    reachable = sorted({n * m % V for n in range(1, 2 * V)})
    assert res == [0, reachable[1], reachable[-1]] and (m != 9 or res == [0, 1, 15])
    for n, r in zip(ce.LOCK_TAIL_COUNTS[wl], res):
        assert n > 16 and n * m % V == r and not any(k * m % V == r for k in range(17, n))
    assert set(ce.LOCK_UNFUSED[wl]) <= set(counts)
    assert all(ce.lock_epochs(n) == (40 if n < 1000 else 6) for n in counts)


@pytest.mark.parametrize("case", ce.TXN_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_transaction_cases_emit_and_commit(wl, case):
    run = ce.host_txn_run(wl, case.n, ce.oracle_shards(wl, ce.TXN_ROWS), ce.TXN_EPOCHS, zipf=ce.TXN_ZIPF[wl])
    assert run.stats["txns"] > 0 and run.stats["committed"] > 0 and run.stats["epochs"] == ce.TXN_EPOCHS
    sizes = np.array([[len(b) for b in q] for q in run.req])
    assert sizes.sum() == run.stats["messages"]
    if case.n >= 64:
        assert (sizes.max(axis=0) > 0).all()                      # every shard receives a message in some epoch
        assert (sizes.max(axis=1) != sizes.min(axis=1)).any()     # some epoch's batches are not all of one size
        assert run.stats["committed"] < run.stats["txns"]         # few clients on few rows still collide


@pytest.mark.parametrize("wl", [FASST, TPL], ids=WL_ID.get)
def test_lock_cases_commit_and_collide(wl):
    for c in ce.LOCK_CASES[wl]:
        epochs = ce.lock_epochs(c.n)
        o = ce.lock_oracle(wl)
        st = ce.host_lock_run(wl, c.n, o.replay, epochs).stats
        assert o.errors == 0 and st["protocol_errors"] == 0 and st["requests"] == c.n * epochs, c.name
        if c.n >= 64:
            assert st["rejects"] > 0, c.name
        if 64 <= c.n < 1000:  # (6 epochs at the pass boundary are fewer requests than the shortest transaction has)
            assert st["committed"] > 0, c.name
            assert wl == TPL or st["rollbacks"] > 0, c.name  # (lock_2pl counts no rollbacks)


@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_cap_cases_lose_nothing_and_exactly_one_message(wl):
    e, s, size = ce.cap_plan(wl)
    wl_, zipf, _ = ce.CAP_ROWS[wl]
    run = ce.host_txn_run(wl_, ce.CAP_CLIENTS, ce.oracle_shards(wl_, ce.TXN_ROWS), ce.CAP_EPOCHS, zipf=zipf)
    sizes = [[len(b) for b in q] for q in run.req]
    assert sizes[e][s] == size >= 3 and all(sizes[e][t] < size for t in range(N_SHARDS) if t != s)

    def lost(cap, k):
        return sum(max(n - cap, 0) for n in sizes[k])
    assert all(lost(size, k) == 0 for k in range(e + 1))
    assert lost(size - 1, e) == 1 and all(lost(size - 1, k) == 0 for k in range(e))


def test_seed_cases_cross_2_to_the_32():
    assert ce.SEED_FIRST < 2 ** 32 < ce.SEED_FIRST + ce.SEED_N - 1
    # the clients on both sides of the edge are distinct: the seed goes on in 64 bits and does not start again at 0xdeadbeef + 0
    a = ce.host_txn_run(TATP, ce.SEED_N, ce.oracle_shards(TATP, ce.TXN_ROWS), ce.SEED_EPOCHS, first_client=ce.SEED_FIRST, zipf=0.8)
    b = ce.host_txn_run(TATP, ce.SEED_N, ce.oracle_shards(TATP, ce.TXN_ROWS), ce.SEED_EPOCHS, first_client=0, zipf=0.8)
    assert a.stats["txns"] > 0 and any(x[s].tobytes() != y[s].tobytes() for x, y in zip(a.req, b.req) for s in range(N_SHARDS))
    for wl in (FASST, TPL):
        o = ce.lock_oracle(wl)
        st = ce.host_lock_run(wl, ce.SEED_N, o.replay, ce.SEED_EPOCHS, first_worker=ce.SEED_FIRST).stats
        assert o.errors == 0 and st["protocol_errors"] == 0 and st["rejects"] > 0
        # worker 2^32 - first (seed 0xdeadbeef + 2^32) does not draw what worker 0 (seed 0xdeadbeef) draws
        hi = ce.host_lock_client(wl, ce.SEED_N, first_worker=ce.SEED_FIRST).next()[2 ** 32 - ce.SEED_FIRST:]
        lo = ce.host_lock_client(wl, ce.SEED_N, first_worker=0).next()[:len(hi)]
        assert hi.tobytes() != lo.tobytes()


def test_the_stream_plans_are_what_they_say():
    alt, split = ce.plan_alternate(ce.PLAN_EPOCHS), ce.plan_split(ce.PLAN_EPOCHS)
    assert all(n == c == k % 2 for k, (n, c) in enumerate(alt))       # an epoch stays on its stream; the next one is on the other
    assert all((n, c) == (0, 1) for n, c in split)                     # consume never on the stream of next
    assert ce.PLAN_N % ce.TXG_TB and ce.PLAN_N % ce.LCG_TB and ce.PLAN_N > ce.LOCK_PASS
    for wl in (TATP, SMALLBANK):
        st = ce.host_txn_run(wl, ce.PLAN_N, ce.oracle_shards(wl, ce.TXN_ROWS), ce.PLAN_EPOCHS, zipf=ce.TXN_ZIPF[wl]).stats
        assert 0 < st["committed"] < st["txns"]
    for wl in (FASST, TPL):
        o = ce.lock_oracle(wl)
        st = ce.host_lock_run(wl, ce.PLAN_N, o.replay, ce.PLAN_EPOCHS).stats
        assert o.errors == 0 and st["protocol_errors"] == 0 and st["rejects"] > 0
