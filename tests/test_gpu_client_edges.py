"""The GPU-resident clients (dint_amd/csrc/k_txn.hip, k_lock_client.hip) at the edges of their geometry, against the host
clients: the cases of tests/client_edges.py, which tests/test_client_edges_host.py shows to hold what they promise.

Every comparison is exact -- bytes, counters, tables.  A GPU client and a host client each close their own loop through their
own GPU servers; the GPU side runs without host synchronisation between its epochs (client_edges.gpu_txn_run / gpu_lock_run
copy every batch aside on the device), so that the stream plans order nothing the clients do not order themselves."""
import ctypes as C

import numpy as np
import pytest

import client_edges as ce
from dint_amd.driver import Driver, DriverConfig, DriverStats, GpuDriver, GpuLockClient, N_SHARDS

pytestmark = pytest.mark.gpu
TATP, SMALLBANK, FASST, TPL = ce.TATP, ce.SMALLBANK, ce.FASST, ce.TPL
WL_ID = {TATP: "tatp", SMALLBANK: "smallbank", FASST: "fasst", TPL: "2pl"}
EINVAL, ESTATE = -1, -5


def _streams(n=2, default=False):
    """n streams of the device; default: the legacy default stream (0) is the second of them"""
    import torch

    s = [torch.cuda.Stream() for _ in range(n)]
    if default:
        s[1] = torch.cuda.default_stream()
        assert s[1].cuda_stream == 0
    return s


def _groups(wl, n_rows=ce.TXN_ROWS):
    from dint_amd.replay import ShardGroup

    return (ShardGroup(wl, n_rows, log_entries=ce.LOG_ENTRIES),   # served to the host driver
            ShardGroup(wl, n_rows, log_entries=ce.LOG_ENTRIES))   # served to the GPU driver


def _txn_lock_step(wl, clients, epochs, plan, streams, *, zipf, first_client=ce.TXN_FIRST, cap=None, small=False):
    ga, gb = _groups(wl)
    want = ce.host_txn_run(wl, clients, ga.submit, epochs, zipf=zipf, first_client=first_client)
    largest = max(len(b) for q in want.req for b in q)
    cap = largest + 64 if cap is None else min(e.pass_max for e in gb.engines) if cap == "pass_max" else cap
    assert largest < cap  # not silently the overflow case
    if small:
        with ce.small_txn_build():
            gpu = GpuDriver(wl, clients, ce.TXN_ROWS, cap, first_client=first_client, zipf_theta=zipf)
        assert gpu._L is not ga.engines[0]._L
    else:
        gpu = GpuDriver(wl, clients, ce.TXN_ROWS, cap, first_client=first_client, zipf_theta=zipf)
    got = ce.gpu_txn_run(gpu, gb, want, plan, streams)
    ce.check_txn_epochs(got, want)
    last = gpu.read_batches()  # what dint_gdriver_read_batch says of the last epoch
    assert [b.tobytes() for b in last] == [b.tobytes() for b in want.rep[-1]]
    ce.check_txn_end(gpu, gb, want, ga)
    assert want.stats["txns"] > 0 and want.stats["committed"] > 0
    for g in (ga, gb):
        assert all(e.stats()["bad_requests"] == 0 for e in g.engines)


# ------------------------------------------------------------------------------------------ a. wave and workgroup edges
TXN_ROWS_A = ([(wl, n, 1, None) for wl in (TATP, SMALLBANK) for n in ce.TXN_COUNTS] +
              [(wl, n, 0, None) for wl in (TATP, SMALLBANK) for n in ce.TXN_UNFUSED] +
              [(wl, n, 1, w) for wl in (TATP, SMALLBANK) for n, w in ce.TXN_WAVES])


@pytest.mark.parametrize("wl,clients,fuse,waves", TXN_ROWS_A,
                         ids=[f"{WL_ID[r[0]]}-{r[1]}-fuse{r[2]}" + (f"-waves{r[3]}" if r[3] else "") for r in TXN_ROWS_A])
def test_transaction_clients_at_wave_and_workgroup_edges(wl, clients, fuse, waves, monkeypatch):
    monkeypatch.setenv("DINT_TXN_FUSE", str(fuse))
    if waves is not None:
        monkeypatch.setenv("DINT_TXN_WAVES", str(waves))
    _txn_lock_step(wl, clients, ce.TXN_EPOCHS, ce.plan_same(ce.TXN_EPOCHS), _streams(1), zipf=ce.TXN_ZIPF[wl])


# ------------------------------------------------------------- b. more workgroups than a look-back step and than are resident
@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_transaction_clients_beyond_one_look_back_step(wl, monkeypatch):
    """TXG_TB + 2 workgroups: workgroup TXG_TB looks back over one full step, workgroup TXG_TB + 1 over a second that holds one
    real entry, and the grid is several times what is resident at once, so the ticket order matters.  How deep a walk goes
    depends on timing and cannot be forced; what is held is that every position is right when it can be two steps deep."""
    monkeypatch.setenv("DINT_TXN_FUSE", "1")
    _txn_lock_step(wl, ce.TXN_DEEP.n, 3, ce.plan_same(3), _streams(1), zipf=ce.TXN_ZIPF[wl], cap="pass_max")


@pytest.mark.parametrize("case", ce.TXN_SMALL_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_look_back_of_many_steps_in_the_small_workgroup_build(wl, case, monkeypatch):
    """The product's build cannot take the look-back's second step on an MI355X: no more of its workgroups are resident than
    one step covers, and every workgroup before mine that has not published a prefix is resident.  (Shown on the device: a build
    whose step is TXG_TB - 1 passes the test above.)  The same source with workgroups of client_edges.SMALL_TB clients has
    thousands resident and walks many steps; a build of THAT whose step is one short emits wrong positions here."""
    monkeypatch.setenv("DINT_TXN_FUSE", "1")
    n = ce.TXN_SMALL_EPOCHS
    _txn_lock_step(wl, case.n, n, ce.plan_same(n), _streams(1), zipf=ce.TXN_ZIPF[wl], cap="pass_max", small=True)


# ------------------------------------------------------------------------------------------------- c. lock workers
def _lock_lock_step(wl, n, epochs, plan, streams, fuse, monkeypatch, first_worker=0):
    from dint_amd.engine import Engine

    monkeypatch.setenv("DINT_LOCK_CLIENT_FUSE", str(fuse))  # read when the client is created
    he, ge = Engine(wl, n_slots=ce.LOCK_KEYS, device=0), Engine(wl, n_slots=ce.LOCK_KEYS, device=0)
    want = ce.host_lock_run(wl, n, he.submit, epochs, first_worker=first_worker)
    gc = GpuLockClient(wl, n, ce.LOCK_KEYS, zipf_theta=ce.LOCK_THETA, first_worker=first_worker, device=0)
    got = ce.gpu_lock_run(gc, ge, plan, streams)
    ce.check_lock_run(got, gc, ge, want, he)
    st = want.stats
    assert st["protocol_errors"] == 0 and st["requests"] == n * epochs
    assert st["rejects"] > 0 or n < 64
    assert st["committed"] > 0 or n < 64 or epochs < 40  # (fewer epochs need not finish a transaction)
    assert ge.stats()["bad_requests"] == 0 and ge.stats()["requests"] == n * epochs


LOCK_ROWS_C = ([(wl, n, 1) for wl in (FASST, TPL) for n in ce.LOCK_COUNTS[wl]] +
               [(wl, n, 0) for wl in (FASST, TPL) for n in ce.LOCK_UNFUSED[wl]])


@pytest.mark.parametrize("wl,n,fuse", LOCK_ROWS_C, ids=[f"{WL_ID[r[0]]}-W{r[1]}-fuse{r[2]}" for r in LOCK_ROWS_C])
def test_lock_workers_at_wave_workgroup_vector_and_pass_edges(wl, n, fuse, monkeypatch):
    epochs = ce.lock_epochs(n)
    _lock_lock_step(wl, n, epochs, ce.plan_same(epochs), _streams(1), fuse, monkeypatch)


@pytest.mark.parametrize("wl", [FASST, TPL], ids=WL_ID.get)
def test_lock_loop_free_running_at_two_workgroups_and_one_worker(wl, monkeypatch):
    from dint_amd.engine import Engine
    from dint_amd.replay import LockLoop

    n, epochs = 2 * ce.LCG_TB + 1, 40
    monkeypatch.setenv("DINT_LOCK_CLIENT_FUSE", "1")
    gc, eng = GpuLockClient(wl, n, ce.LOCK_KEYS, zipf_theta=ce.LOCK_THETA, device=0), Engine(wl, n_slots=ce.LOCK_KEYS, device=0)
    loop = LockLoop(eng, gc)
    loop.epochs(epochs)
    loop.sync()
    o = ce.lock_oracle(wl)
    want = ce.host_lock_run(wl, n, o.replay, epochs)
    assert o.errors == 0 and gc.stats() == want.stats and want.stats["committed"] > 0 and want.stats["rejects"] > 0
    a, b = eng.read_locks()
    if wl == FASST:
        assert (a == o.locks).all() and (b == o.vers).all()
    else:
        assert (a == o.num_ex).all() and (b == o.num_sh).all()
    assert eng.stats()["requests"] == n * epochs


# ------------------------------------------------------------------------------------------------- d. stream plans
PLANS = {"alternate": (ce.plan_alternate, False), "split": (ce.plan_split, False), "default": (ce.plan_alternate, True)}


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_transaction_clients_on_two_streams(wl, plan, monkeypatch):
    """alternate: epoch k whole on stream k % 2, so every next finds a consume promised on the other stream and must run it
    there and wait for it (flush + event); split: next on one stream, servers and consume on the other, ordered by the
    caller -- consume in a kernel of its own with fusing on; default: alternate with the legacy default stream as one of the
    two.  A missing wait is a race, and a race can pass by luck: this pins the results of every epoch, not the ordering."""
    monkeypatch.setenv("DINT_TXN_FUSE", "1")
    mk, default = PLANS[plan]
    _txn_lock_step(wl, ce.PLAN_N, ce.PLAN_EPOCHS, mk(ce.PLAN_EPOCHS), _streams(2, default), zipf=ce.TXN_ZIPF[wl])


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("wl", [FASST, TPL], ids=WL_ID.get)
def test_lock_workers_on_two_streams(wl, plan, monkeypatch):
    """the plans of test_transaction_clients_on_two_streams for dint_lock_gclient_next / _consume.  A missing wait is a race,
    and a race can pass by luck: this pins the results of every epoch, not the ordering."""
    mk, default = PLANS[plan]
    _lock_lock_step(wl, ce.PLAN_N, ce.PLAN_EPOCHS, mk(ce.PLAN_EPOCHS), _streams(2, default), 1, monkeypatch)


# ------------------------------------------------------------------------------------------------- e. cap edges
@pytest.mark.parametrize("short", [0, 1], ids=["largest", "largest-1"])
@pytest.mark.parametrize("wl", [TATP, SMALLBANK], ids=WL_ID.get)
def test_cap_at_the_largest_batch_and_one_below(wl, short, monkeypatch):
    """cap = the largest batch of epoch e (larger than any before it): nothing is lost up to and including e.  One less: in
    epoch e that batch is the host's cut at cap, its device count is cap, and exactly one message found no room; nothing after
    e is compared (what the clients do once a request went unanswered is not specified)."""
    wl, zipf, fuse = ce.CAP_ROWS[wl]
    monkeypatch.setenv("DINT_TXN_FUSE", str(fuse))
    e, s, size = ce.cap_plan(wl)
    cap = size - short
    ga, gb = _groups(wl)
    want = ce.host_txn_run(wl, ce.CAP_CLIENTS, ga.submit, e + 1, zipf=zipf)
    sizes = [[len(b) for b in q] for q in want.req]
    assert sizes[e][s] == size == max(max(x) for x in sizes)  # the GPU servers answer as the oracles the plan ran through
    gpu = GpuDriver(wl, ce.CAP_CLIENTS, ce.TXN_ROWS, cap, first_client=ce.TXN_FIRST, zipf_theta=zipf)
    got = ce.gpu_txn_run(gpu, gb, want, ce.plan_same(e + 1), _streams(1))
    # up to the epoch of the loss every reply is the host's; in it, the requests are (the servers' replies to a cut batch are theirs)
    ce.check_txn_epochs(got[:e] if short else got, want, cap)
    cnt, q, _ = got[e]
    assert cnt[s] == cap and all(cnt[t] == sizes[e][t] for t in range(N_SHARDS) if t != s)
    assert all(q[t] == want.req[e][t][:cap].tobytes() for t in range(N_SHARDS))
    st = gpu.stats()
    assert st["overflow"] == short and st["messages"] == want.stats["messages"]
    assert all(eng.stats()["bad_requests"] == 0 for eng in gb.engines)


def test_cap_of_two_messages_with_one_client():
    ga, gb = _groups(TATP)
    gpu = GpuDriver(TATP, 1, ce.TXN_ROWS, 2, first_client=ce.TXN_FIRST, zipf_theta=0.8)
    (st,) = _streams(1)
    xs = st.cuda_stream
    for _ in range(20):
        gpu.next(xs)
        for s, eng in enumerate(gb.engines):
            eng.stream_wait(xs)
            eng.submit_segments(gpu.batch_ptr[s], 1, 2, 2 * gb.msg, gpu.counts_ptr + 4 * s, 0)
        for eng in gb.engines:
            eng.stream_signal(xs)
        gpu.consume(xs)
        assert all(len(b) <= 2 for b in gpu.read_batches())
    st.synchronize()
    gb.sync()
    s = gpu.stats()
    assert s["epochs"] == 20 and s["messages"] > 0
    assert all(eng.stats()["bad_requests"] == 0 for eng in gb.engines)


# ------------------------------------------------------------------------------------------------- f. seeds across 2^32
def test_transaction_clients_numbered_across_2_to_the_32():
    _txn_lock_step(TATP, ce.SEED_N, ce.SEED_EPOCHS, ce.plan_same(ce.SEED_EPOCHS), _streams(1), zipf=0.8, first_client=ce.SEED_FIRST)


@pytest.mark.parametrize("wl", [FASST, TPL], ids=WL_ID.get)
def test_lock_workers_numbered_across_2_to_the_32(wl, monkeypatch):
    _lock_lock_step(wl, ce.SEED_N, ce.SEED_EPOCHS, ce.plan_same(ce.SEED_EPOCHS), _streams(1), 1, monkeypatch, first_worker=ce.SEED_FIRST)


# ------------------------------------------------------------------------------------------------- g. the call surface
def test_gpu_driver_refuses_bad_calls_and_goes_on():
    clients, zipf = 600, 0.8
    ga, gb = _groups(TATP)
    host = Driver(TATP, clients, ce.TXN_ROWS, first_client=ce.TXN_FIRST, zipf_theta=zipf)
    gpu = GpuDriver(TATP, clients, ce.TXN_ROWS, 4 * clients, first_client=ce.TXN_FIRST, zipf_theta=zipf)
    L, h = gpu._L, gpu._h
    (st,) = _streams(1)
    xs = st.cuda_stream

    def emit():
        want = host.next()
        gpu.next(xs)
        got = gpu.read_batches()
        assert [b.tobytes() for b in got] == [b.tobytes() for b in want]
        return want

    def answer(want):
        host.consume(ga.submit(want))
        for s, eng in enumerate(gb.engines):
            eng.stream_wait(xs)
            eng.submit_segments(gpu.batch_ptr[s], 1, gpu.cap, gpu.cap * gb.msg, gpu.counts_ptr + 4 * s, 0)
        for eng in gb.engines:
            eng.stream_signal(xs)
        gpu.consume(xs)

    def epoch():
        answer(emit())

    assert L.dint_gdriver_consume(h, xs) == ESTATE  # consume before next
    epoch()
    want = emit()
    assert L.dint_gdriver_next(h, xs) == ESTATE     # a second next before consume
    assert [b.tobytes() for b in gpu.read_batches()] == [b.tobytes() for b in want]  # (the refused call emitted nothing)
    answer(want)
    assert L.dint_gdriver_consume(h, xs) == ESTATE
    epoch()

    base = dict(workload=int(TATP), n_clients=clients, n_rows=ce.TXN_ROWS, first_client=0, key_dist=0, zipf_theta=0.0)
    bad = [(dict(n_clients=0), 64), ({}, 1), (dict(workload=int(FASST)), 64), (dict(workload=int(TPL)), 64), (dict(key_dist=2), 64),
           (dict(key_dist=1, zipf_theta=0.0), 64), (dict(key_dist=1, zipf_theta=1.0), 64)]
    for kw, cap in bad:
        out = C.c_void_p()
        cfg = DriverConfig(**dict(base, **kw))
        assert L.dint_gdriver_create(C.byref(cfg), 0, cap, C.byref(out)) == EINVAL and not out.value, (kw, cap)
        epoch()
    out = C.c_void_p()
    cfg = DriverConfig(**dict(base, n_clients=1))
    assert L.dint_gdriver_create(C.byref(cfg), 0, 2, C.byref(out)) == 0 and out.value  # (the smallest there is)
    L.dint_gdriver_destroy(out)

    buf = np.zeros(gpu.cap, gpu.dtype)
    assert L.dint_gdriver_batch(h, N_SHARDS) is None
    assert L.dint_gdriver_read_batch(h, N_SHARDS, buf.ctypes.data, gpu.cap) == EINVAL
    assert L.dint_gdriver_next(None, xs) == EINVAL and L.dint_gdriver_consume(None, xs) == EINVAL
    assert L.dint_gdriver_get_stats(h, None, None) == EINVAL and L.dint_gdriver_get_stats(None, C.byref(DriverStats()), None) == EINVAL
    epoch()

    st.synchronize()
    gb.sync()
    hs, gs = host.stats(), gpu.stats()
    assert gs["overflow"] == 0 and gs["epochs"] == hs["epochs"] == 4 + len(bad)
    for k in ("txns", "committed", "by_type", "committed_by_type", "messages"):
        assert gs[k] == hs[k], k
    for s in range(N_SHARDS):
        for t in range(ce.n_tables(TATP)):
            assert all((x == y).all() for x, y in zip(ga.engines[s].dump_rows(t), gb.engines[s].dump_rows(t)))
