"""Cases and runners for the GPU-resident clients (dint_amd/csrc/k_txn.hip, k_lock_client.hip) at the edges of their geometry:
client counts at a wave, a workgroup and one look-back step of k_txn_emit; worker counts at a wave, a workgroup, the 16-byte
vectors of lcg_load / lcg_store and the lock engine's pass; stream plans for next / consume; caps at an epoch's largest batch.

Every count is an expression of the kernels' own constants, read from the sources, and of the message sizes of dint_amd.wire.
tests/test_client_edges_host.py shows without a GPU that every case holds what its name says; tests/test_gpu_client_edges.py
runs them.  The runners drive a host client and a GPU client through servers of their own, the host side first and to the end
(it is the reference), then the GPU side WITHOUT any host synchronisation between the epochs: every batch is copied aside on
the device, on the stream it was produced on, and compared when the run is over -- a read through the host would order the
streams and hide what a stream plan is there to show.

numpy and ctypes only; torch is imported by the GPU runners when they are called."""
from __future__ import annotations

import functools
import math
import os
import re
from collections import namedtuple

import numpy as np

from dint_amd import _lib, wire
from dint_amd import build as hip_build
from dint_amd.driver import N_SHARDS, Driver, FasstClient, LcgTplClient
from oracle import oracle as orc

W = wire.Workload
TATP, SMALLBANK, FASST, TPL = W.TATP, W.SMALLBANK, W.FASST, W.TPL
CSRC = os.path.join(os.path.dirname(os.path.abspath(wire.__file__)), "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


_TXN, _LCG = _src("k_txn.hip"), _src("k_lock_client.hip")
TXG_TB = _const(_TXN, r"#define TXG_TB (\d+)u")                         # clients per workgroup of k_txn_emit = entries of one look-back step
LCG_TB = _const(_LCG, r"#define LCG_TB (\d+)u")                         # workers per workgroup of k_lock_client
LCG_VEC = _const(_LCG, r"const uint32_t nv = nbytes / (\d+);")          # lcg_load / lcg_store: bytes of a vector
assert re.search(r"for \(int k0 = \(int\)tile - 1; open; k0 -= \(int\)TXG_TB\)", _TXN), "the look-back's step is no longer TXG_TB"
WAVE = 64
LOCK_PASS = _lib.MICRO_BATCH                                            # requests of one pass of a lock engine
MSG = {wl: wire.MSG_DTYPE[wl].itemsize for wl in (FASST, TPL, TATP, SMALLBANK)}
LOG_ENTRIES = 400_000

# ------------------------------------------------------------------------------------------------------------- counts
# (name, clients, workgroups, valid lanes of the last workgroup): the last two are what the name says, written out
TxnCase = namedtuple("TxnCase", "name n tiles last")
TXN_CASES = [
    TxnCase("one", 1, 1, 1), TxnCase("two", 2, 1, 2),
    TxnCase("wave-1", WAVE - 1, 1, WAVE - 1), TxnCase("wave", WAVE, 1, WAVE), TxnCase("wave+1", WAVE + 1, 1, WAVE + 1),
    TxnCase("tile-1", TXG_TB - 1, 1, TXG_TB - 1), TxnCase("tile", TXG_TB, 1, TXG_TB), TxnCase("tile+1", TXG_TB + 1, 2, 1),
    TxnCase("2tiles-1", 2 * TXG_TB - 1, 2, TXG_TB - 1), TxnCase("2tiles", 2 * TXG_TB, 2, TXG_TB), TxnCase("2tiles+1", 2 * TXG_TB + 1, 3, 1),
]
TXN_COUNTS = [c.n for c in TXN_CASES]
# one workgroup more than a look-back step covers, and one more: workgroup TXG_TB walks back over exactly one full step, workgroup
# TXG_TB + 1 needs a second step that holds a single real entry (workgroup 0); far more workgroups than are resident at once
TXN_DEEP = TxnCase("deep", TXG_TB * (TXG_TB + 1) + 1, TXG_TB + 2, 1)
# An MI355X holds no more workgroups of k_txn_emit at once than one look-back step covers (k_txn.hip says why), so in the product's
# build the loop's second step never runs, whatever the count.  dint_amd/build.py compiles the same source once more with
# workgroups of SMALL_TB clients: thousands are resident, and the walk of a late workgroup takes many steps.  Counts for that
# build: SMALL_TB + 2 workgroups (the deep case's shape: the last one's walk can hold a second step of one real entry), a few
# hundred workgroups, all resident at once (walks of up to five steps), and about as many workgroups as are resident.
SMALL_TB, SMALL_LIB = hip_build.TXN_SMALL_TB, hip_build.TXN_SMALL_LIB
TXN_SMALL_CASES = [TxnCase("small-deep", SMALL_TB * (SMALL_TB + 1) + 1, SMALL_TB + 2, 1),
                   TxnCase("small-resident", 70_001, 70_001 // SMALL_TB + 1, 70_001 % SMALL_TB),
                   TxnCase("small-beyond", TXN_DEEP.n, TXN_DEEP.n // SMALL_TB + 1, TXN_DEEP.n % SMALL_TB)]
TXN_SMALL_EPOCHS = 6
TXN_UNFUSED = [TXG_TB - 1, TXG_TB, TXG_TB + 1, 1]      # DINT_TXN_FUSE=0 additionally
TXN_WAVES = [(TXG_TB + 1, 3), (TXG_TB + 1, 5)]         # DINT_TXN_WAVES
TXN_ROWS, TXN_EPOCHS, TXN_FIRST = 3000, 30, 11
TXN_ZIPF = {TATP: 0.8, SMALLBANK: 0.99 - 1e-9}

# (name, workers, workgroups, valid lanes of the last workgroup, bytes of the last workgroup's messages past its last whole vector)
LockCase = namedtuple("LockCase", "name n tiles last tail")


def tail_residues(msg):
    """the byte tails that sit on, just after and just before a vector edge: 0, the smallest residue W * msg can leave and
    the largest (1 and 15 for lock_fasst's 9 bytes; lock_2pl's 6 bytes leave even residues only: 2 and 14)"""
    g = math.gcd(msg, LCG_VEC)
    return [0, g, LCG_VEC - g]


def _tail_count(msg, r):
    return next(n for n in range(LCG_VEC + 1, LCG_VEC + 1 + LCG_VEC) if n * msg % LCG_VEC == r)  # the smallest W > 16


def _lock_cases(wl):
    m, T = MSG[wl], LCG_TB
    assert T * m % LCG_VEC == 0  # every workgroup but the last moves whole vectors (k_lock_client.hip says so of its batches)
    res = tail_residues(m)
    cs = [LockCase("one", 1, 1, 1, m % LCG_VEC), LockCase("two", 2, 1, 2, 2 * m % LCG_VEC),
          LockCase("wave-1", WAVE - 1, 1, WAVE - 1, (WAVE - 1) * m % LCG_VEC), LockCase("wave", WAVE, 1, WAVE, 0),
          LockCase("wave+1", WAVE + 1, 1, WAVE + 1, m % LCG_VEC),
          LockCase("tile-1", T - 1, 1, T - 1, LCG_VEC - m % LCG_VEC), LockCase("tile", T, 1, T, 0), LockCase("tile+1", T + 1, 2, 1, m % LCG_VEC),
          LockCase("2tiles+1", 2 * T + 1, 3, 1, m % LCG_VEC)]
    for nm, r in zip(("tail-on", "tail-after", "tail-before"), res):
        n = _tail_count(m, r)
        cs.append(LockCase(nm, n, 1, n, r))
    P = LOCK_PASS  # (a multiple of the workgroup)
    cs += [LockCase("pass-1", P - 1, P // T, T - 1, LCG_VEC - m % LCG_VEC), LockCase("pass", P, P // T, T, 0),
           LockCase("pass+1", P + 1, P // T + 1, 1, m % LCG_VEC)]
    return cs


LOCK_CASES = {wl: _lock_cases(wl) for wl in (FASST, TPL)}
LOCK_COUNTS = {wl: [c.n for c in cs] for wl, cs in LOCK_CASES.items()}
LOCK_TAIL_COUNTS = {wl: [c.n for c in cs if c.name.startswith("tail-")] for wl, cs in LOCK_CASES.items()}
LOCK_UNFUSED = {wl: [LCG_TB - 1, LCG_TB, LCG_TB + 1] + LOCK_TAIL_COUNTS[wl] for wl in (FASST, TPL)}  # DINT_LOCK_CLIENT_FUSE=0 additionally
LOCK_KEYS, LOCK_THETA = 1024, 0.99


def lock_epochs(n):
    return 40 if n < 1000 else 6


# stream plans and seeds
PLAN_N, PLAN_EPOCHS = 70_001, 12
SEED_FIRST, SEED_N, SEED_EPOCHS = 2 ** 32 - 300, 600, 10
# cap edges
CAP_CLIENTS, CAP_EPOCHS = 6000, 30
CAP_ROWS = {TATP: (TATP, 0.8, 1), SMALLBANK: (SMALLBANK, 0.99 - 1e-9, 0)}  # workload -> (workload, zipf, fuse)


def n_tables(wl):
    return 5 if wl == TATP else 2


# ------------------------------------------------------------------------------------------------------------ stream plans
# A plan gives, per epoch, the stream `next` goes on and the stream the servers and `consume` go on, as indices into the
# streams the test hands over.  Where the two differ within an epoch the CALLER orders them (consume's stream waits for
# next's before the servers, the following next's stream waits for consume's), as the clients' interface asks; where an epoch
# stays on one stream and the next epoch goes to another, the clients order themselves (the flush + event branch of
# dint_gdriver_next / dint_lock_gclient_next), and the runner adds nothing.
def plan_same(epochs):
    return [(0, 0)] * epochs


def plan_alternate(epochs):
    """epoch k on stream k % 2, whole: every next finds a consume promised on the other stream"""
    return [(k % 2, k % 2) for k in range(epochs)]


def plan_split(epochs):
    """next on stream 0, the servers and consume on stream 1: consume in a kernel of its own, also with fusing on"""
    return [(0, 1)] * epochs


# ------------------------------------------------------------------------------------------------------------ host runs
TxnRun = namedtuple("TxnRun", "req rep stats")     # req[e][s], rep[e][s]: numpy arrays; stats of the driver at the end
LockRun = namedtuple("LockRun", "req rep stats")   # req[e], rep[e]


def oracle_shards(wl, n_rows):
    """three CPU oracle servers as one submit(): what a ShardGroup is on the GPU"""
    ora = [(orc.TatpOracle if wl == TATP else orc.SmallbankOracle)(n_rows, log_entries=LOG_ENTRIES) for _ in range(N_SHARDS)]

    def submit(req):
        return [ora[s].replay(req[s]) if len(req[s]) else req[s] for s in range(N_SHARDS)]
    submit.oracles = ora
    return submit


def host_txn_run(wl, clients, submit, epochs, *, n_rows=TXN_ROWS, first_client=TXN_FIRST, zipf=None) -> TxnRun:
    """the host driver's closed loop through `submit` (three requests batches -> three reply batches)"""
    d = Driver(wl, clients, n_rows, first_client=first_client, zipf_theta=zipf)
    req, rep = [], []
    for _ in range(epochs):
        q = d.next()
        p = submit(q)
        d.consume(p)
        req.append(q)
        rep.append(p)
    return TxnRun(req, rep, d.stats())


def host_lock_client(wl, n, *, key_space=LOCK_KEYS, theta=LOCK_THETA, first_worker=0):
    return (FasstClient if wl == FASST else LcgTplClient)(n, key_space, zipf_theta=theta, first_worker=first_worker)


def lock_oracle(wl, key_space=LOCK_KEYS):
    return orc.FasstOracle(key_space) if wl == FASST else orc.TplOracle(key_space)


def host_lock_run(wl, n, submit, epochs, **kw) -> LockRun:
    """the host client's closed loop through `submit` (a request batch -> its replies)"""
    c = host_lock_client(wl, n, **kw)
    req, rep = [], []
    for _ in range(epochs):
        q = c.next()
        p = submit(q)
        c.consume(p)
        req.append(q)
        rep.append(p)
    return LockRun(req, rep, c.stats())


@functools.lru_cache(maxsize=None)
def cap_plan(wl):
    """(epoch e, shard s, size): through the CPU oracles, batch s of epoch e is strictly the largest of its epoch and larger than
    every batch of an earlier epoch -- so cap = size loses nothing up to and including e, and cap = size - 1 loses exactly one
    message, in epoch e, and none before.  The last such epoch of the run: the later, the more epochs ran at the cap."""
    wl, zipf, _ = CAP_ROWS[wl]
    run = host_txn_run(wl, CAP_CLIENTS, oracle_shards(wl, TXN_ROWS), CAP_EPOCHS, zipf=zipf)
    best, high = None, 0
    for e, q in enumerate(run.req):
        sizes = sorted(len(b) for b in q)
        if sizes[-1] > high and sizes[-1] > sizes[-2]:
            best = (e, max(range(N_SHARDS), key=lambda s: len(q[s])), sizes[-1])
        high = max(high, sizes[-1])
    assert best is not None
    return best


# ------------------------------------------------------------------------------------------------------------- GPU runs
class small_txn_build:
    """with small_txn_build(): GpuDriver(...) -- the driver is the one of the small-workgroup build (dint_gdriver_* of
    dint_amd/libdint_txn_small.so); everything else stays the product's library"""
    _L = None

    def __enter__(self):
        import ctypes as C

        cls = small_txn_build
        _lib.load()  # (the product's library, and with it the HIP runtime, first)
        if cls._L is None:
            cls._L = C.CDLL(SMALL_LIB)
        self._load, _lib.load = _lib.load, lambda: cls._L

    def __exit__(self, *exc):
        _lib.load = self._load


def _hip():
    from test_gpu_lock_loop import _hip as hip
    return hip()


class _Tape:
    """copies of device ranges, taken on a stream, kept on the device until read(); one allocation, made before the run (an
    allocation in between may synchronise the device)"""

    def __init__(self, sizes):
        import torch

        self.off, top = [], 0
        for n in sizes:
            self.off.append((top, n))
            top += -(-n // 256) * 256
        self.buf = torch.empty(max(top, 1), dtype=torch.uint8, device="cuda")
        self.k, self.host = 0, None

    def take(self, src, nbytes, stream):
        off, n = self.off[self.k]
        assert n == nbytes
        if nbytes:
            assert _hip().hipMemcpyAsync(self.buf.data_ptr() + off, src, nbytes, 3, stream) == 0  # hipMemcpyDeviceToDevice
        self.k += 1
        return self.k - 1

    def read(self, k) -> bytes:
        if self.host is None:
            self.host = self.buf.cpu().numpy()
        off, n = self.off[k]
        return self.host[off:off + n].tobytes()


def _order(streams, a, b):
    """stream a waits for what stream b holds"""
    if a != b:
        streams[a].wait_stream(streams[b])


def gpu_txn_run(gpu, group, want: TxnRun, plan, streams, upto=None):
    """`gpu` (a GpuDriver) through the engines of `group` for the epochs of `plan`, no host synchronisation in between.  Per
    epoch and shard the live count and the first min(len(host batch), cap) messages are taken after next and again after the
    servers.  Returns [(counts (3,), requests[3] bytes, replies[3] bytes)] per epoch, read back after the last one."""
    cap, msg = gpu.cap, group.msg
    plan = plan[:upto]
    lens_of = [[min(len(want.req[e][s]), cap) for s in range(N_SHARDS)] for e in range(len(plan))]
    tape, taken = _Tape([n for ln in lens_of for n in [4 * N_SHARDS] + [x * msg for x in ln] * 2]), []
    _hip()  # (loaded before the first epoch)
    last = None
    for e, (sn, sc) in enumerate(plan):
        if last is not None:
            _order(streams, sn, last)
        xn, xc = streams[sn].cuda_stream, streams[sc].cuda_stream
        gpu.next(xn)
        k_cnt = tape.take(gpu.counts_ptr, 4 * N_SHARDS, xn)
        lens = lens_of[e]
        k_req = [tape.take(gpu.batch_ptr[s], lens[s] * msg, xn) for s in range(N_SHARDS)]
        _order(streams, sc, sn)
        for s, eng in enumerate(group.engines):
            eng.stream_wait(xc)
            eng.submit_segments(gpu.batch_ptr[s], 1, cap, cap * msg, gpu.counts_ptr + 4 * s, 0)
        for eng in group.engines:
            eng.stream_signal(xc)
        k_rep = [tape.take(gpu.batch_ptr[s], lens[s] * msg, xc) for s in range(N_SHARDS)]
        gpu.consume(xc)
        taken.append((k_cnt, k_req, k_rep))
        last = sc if sc != sn else None
    for st in streams:
        st.synchronize()
    group.sync()
    return [(np.frombuffer(tape.read(c), "<u4"), [tape.read(k) for k in q], [tape.read(k) for k in p]) for c, q, p in taken]


def check_txn_epochs(got, want: TxnRun, cap=None):
    """every epoch's counts, requests and replies against the host run's"""
    for e, (cnt, q, p) in enumerate(got):
        for s in range(N_SHARDS):
            n = len(want.req[e][s])
            assert cnt[s] == (n if cap is None else min(n, cap)), (e, s, int(cnt[s]), n)
            assert q[s] == want.req[e][s][:cap].tobytes(), ("request", e, s)
            assert p[s] == want.rep[e][s][:cap].tobytes(), ("reply", e, s)


def check_txn_end(gpu, group, want: TxnRun, host_group):
    gs = gpu.stats()
    assert gs["overflow"] == 0
    for k in ("txns", "committed", "by_type", "committed_by_type", "messages", "epochs"):
        assert gs[k] == want.stats[k], k
    for s in range(N_SHARDS):
        for t in range(n_tables(gpu.workload)):
            assert all((x == y).all() for x, y in zip(host_group.engines[s].dump_rows(t), group.engines[s].dump_rows(t))), (s, t)


def gpu_lock_run(gc, eng, plan, streams):
    """`gc` (a GpuLockClient) through `eng` for the epochs of `plan`, no host synchronisation in between; returns
    [(requests bytes, replies bytes)] per epoch"""
    nbytes = gc.n * gc.dtype.itemsize
    tape, taken = _Tape([nbytes] * (2 * len(plan))), []
    _hip()  # (loaded before the first epoch)
    last = None
    for sn, sc in plan:
        if last is not None:
            _order(streams, sn, last)
        xn, xc = streams[sn].cuda_stream, streams[sc].cuda_stream
        gc.next(xn)
        k_req = tape.take(gc.batch_ptr, nbytes, xn)
        _order(streams, sc, sn)
        if xc:
            eng.submit_device(gc.batch_ptr, gc.n, gc.batch_ptr, xc)  # as replay.LockLoop does
        else:  # the engine takes stream 0 for its own stream, not for the legacy default stream: fork and join around that
            eng.stream_wait(xc)
            eng.submit_device(gc.batch_ptr, gc.n, gc.batch_ptr, 0)
            eng.stream_signal(xc)
        k_rep = tape.take(gc.batch_ptr, nbytes, xc)
        gc.consume(xc)
        taken.append((k_req, k_rep))
        last = sc if sc != sn else None
    for st in streams:
        st.synchronize()
    eng.sync()
    return [(tape.read(q), tape.read(p)) for q, p in taken]


def check_lock_run(got, gc, eng, want: LockRun, host_eng):
    n, size = gc.n, gc.dtype.itemsize
    for e, (q, p) in enumerate(got):
        if q != want.req[e].tobytes():
            a, b = np.frombuffer(q, np.uint8).reshape(n, size), want.req[e].view(np.uint8).reshape(n, size)
            raise AssertionError(("request", e, np.nonzero((a != b).any(axis=1))[0][:8].tolist()))
        assert p == want.rep[e].tobytes(), ("reply", e)
    assert gc.stats() == want.stats
    a, b = host_eng.read_locks(), eng.read_locks()
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
