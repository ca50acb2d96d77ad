"""The GPU-resident clients (csrc/k_txn.hip, csrc/k_lock_client.hip) against what the reference's own clients sent and
received -- the recordings of tests/test_client_golden.py and tests/test_lock_clients_host.py, replayed on the device.

The device clients run the state machines of txn_clients.h / lock_clients.h behind a path the host never takes: the
fused consume at the top of k_txn_emit (note_reply, whole-row copies selected by TX_FULL, the loads from slot 0 where
nothing is awaited), the message queue in LDS and materialize, client headers as dword columns, working messages with a
run-time stride, three register-budget variants of the emit kernel (DINT_TXN_WAVES).  Here the recorded replies are
written into the device batches in place of a server's, and every batch the device emits must be the recorded requests,
byte for byte:

  - one fixture client at a time (tests/golden/clients.npz; clients_micro.npz and clients_micro_lcg.npz for the lock
    clients, with one ACQUIRE in five refused);
  - a block of 96 consecutive reference clients in ONE launch (tests/golden/clients_block.npz): lanes of a wave in
    different phases, refused and granted replies side by side.  The split of every batch into clients comes from the
    fixture's per-client, per-epoch, per-shard counts, never from what the device emitted.

The statistics must equal those of one-client host drivers fed the same replies in lock step."""
import json
import os

import numpy as np
import pytest

from dint_amd import wire
from dint_amd.driver import Driver, FasstClient, GpuDriver, GpuLockClient, LcgTplClient
from test_client_golden import N_TXN_TYPES, _canon, check_block_conditions, load_block
from test_gpu_lock_loop import _h2d

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
FASST, TPL = wire.Workload.FASST, wire.Workload.TPL
STAT_KEYS = ("txns", "committed", "by_type", "committed_by_type")


def _wl(wl):
    return wire.Workload.TATP if wl == "tatp" else wire.Workload.SMALLBANK


def _stream():
    import torch

    return torch.cuda.Stream()


# every value of DINT_TXN_FUSE and of DINT_TXN_WAVES, for both workloads
@pytest.mark.parametrize("fuse,waves", [(1, 4), (0, 4), (1, 3), (0, 3), (1, 5), (0, 5)])
@pytest.mark.parametrize("wl", ["tatp", "smallbank"])
def test_one_device_client_sends_what_the_reference_client_sends(wl, fuse, waves, monkeypatch):
    monkeypatch.setenv("DINT_TXN_FUSE", str(fuse))
    monkeypatch.setenv("DINT_TXN_WAVES", str(waves))
    z = np.load(os.path.join(G, "clients.npz"))
    meta = json.loads(str(z["meta"]))
    W, cap = _wl(wl), 64
    dt = wire.MSG_DTYPE[W]
    st = _stream()
    xs = st.cuda_stream
    for gid in meta["clients"][wl]:
        req = [np.frombuffer(z[f"{wl}_{gid}_s{s}_req"].tobytes(), dt) for s in range(3)]
        rep = [np.frombuffer(z[f"{wl}_{gid}_s{s}_rep"].tobytes(), dt) for s in range(3)]
        gpu = GpuDriver(W, 1, meta["n_rows"][wl], cap, first_client=gid)
        host = Driver(W, 1, meta["n_rows"][wl], first_client=gid)
        cur, epochs = [0, 0, 0], 0
        while True:
            gpu.next(xs)
            got = gpu.read_batches()
            hout = host.next()
            if any(cur[s] + len(got[s]) > len(req[s]) for s in range(3)):
                break  # the recording was cut inside this phase
            for s in range(3):
                want = _canon(wl, req[s][cur[s]:cur[s] + len(got[s])])
                assert _canon(wl, got[s]).tobytes() == want.tobytes(), (wl, gid, epochs, s)
            for s in range(3):
                _h2d(gpu.batch_ptr[s], rep[s][cur[s]:cur[s] + len(got[s])])
            gpu.consume(xs)
            host.consume([rep[s][cur[s]:cur[s] + len(hout[s])].copy() for s in range(3)])
            for s in range(3):
                cur[s] += len(got[s])
            epochs += 1
        st.synchronize()
        gs, hs = gpu.stats(), host.stats()
        assert sum(cur) > 0.99 * meta["runs"][f"{wl}_{gid}"]["messages"]
        assert all(c > 0 for c in gs["by_type"][:N_TXN_TYPES[wl]]) and gs["committed"] < gs["txns"]
        assert gs["overflow"] == 0 and gs["messages"] == hs["messages"]
        for k in STAT_KEYS:
            assert gs[k] == hs[k], (wl, gid, k)
        gpu.close()


@pytest.mark.parametrize("fuse,waves", [(1, 4), (0, 4), (1, 3), (0, 5), (1, 5), (0, 3)])
@pytest.mark.parametrize("wl", ["tatp", "smallbank"])
def test_a_block_of_device_clients_sends_what_the_reference_clients_send(wl, fuse, waves, monkeypatch):
    """one GpuDriver plays the whole block: in epoch e, batch s is the concatenation, in client order, of each client's
    next counts[c, e, s] recorded requests, and the recorded replies go back at the same positions"""
    monkeypatch.setenv("DINT_TXN_FUSE", str(fuse))
    monkeypatch.setenv("DINT_TXN_WAVES", str(waves))
    W = _wl(wl)
    g0, n_rows, counts, req, rep = load_block(wl)
    n, E = counts.shape[:2]
    off = np.concatenate([np.zeros((n, 1, 3), np.int64), np.cumsum(counts, axis=1, dtype=np.int64)], axis=1)  # [c, e, s]
    cap = int(counts.sum(axis=0).max()) + 7  # the largest batch of the recording, and not a round number
    hosts = [Driver(W, 1, n_rows, first_client=g0 + c) for c in range(n)]
    gpu = GpuDriver(W, n, n_rows, cap, first_client=g0)
    st = _stream()
    xs = st.cuda_stream
    for e in range(E):
        gpu.next(xs)
        got = gpu.read_batches()
        for s in range(3):
            want = np.concatenate([req[c][s][off[c, e, s]:off[c, e + 1, s]] for c in range(n)])
            assert len(got[s]) == len(want), (wl, e, s, len(got[s]), len(want))
            a, b = _canon(wl, got[s]), _canon(wl, want)
            bad = (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)
            assert a.tobytes() == b.tobytes(), (wl, e, s, np.nonzero(bad)[0][:8])  # (positions in the batch)
            _h2d(gpu.batch_ptr[s], np.concatenate([rep[c][s][off[c, e, s]:off[c, e + 1, s]] for c in range(n)]))
        gpu.consume(xs)
        for c, h in enumerate(hosts):
            out = h.next()
            assert [len(o) for o in out] == counts[c, e].tolist()
            h.consume([rep[c][s][off[c, e, s]:off[c, e + 1, s]].copy() for s in range(3)])
    st.synchronize()
    for c in range(n):  # every recording is used up
        assert off[c, E].tolist() == [len(r) for r in req[c]] == [len(r) for r in rep[c]]
    gs, hs = gpu.stats(), [h.stats() for h in hosts]
    assert gs["overflow"] == 0 and gs["epochs"] == E
    assert gs["messages"] == sum(h["messages"] for h in hs) == int(counts.sum())
    for k in ("txns", "committed"):
        assert gs[k] == sum(h[k] for h in hs), k
    for k in ("by_type", "committed_by_type"):
        assert gs[k] == np.sum([h[k] for h in hs], axis=0).tolist(), k
    check_block_conditions(wl, g0, counts, rep, hs)


def _tpl_commits(req):
    """transactions the lock_2pl recording holds to their end: the reference releases in REVERSE order of acquisition
    after the last grant and in acquisition order (ascending lids) after a refusal, and a transaction has five locks
    at least -- a run of two or more RELEASEs with descending lids is a commit, complete (the recording may end inside
    one) when it gives back every lock of the ACQUIREs since the RELEASEs before it"""
    rel = np.concatenate([[0], (req["action"] == wire.Tpl.RELEASE_LOCK).astype(np.int8), [0]])
    starts, ends = np.nonzero(np.diff(rel) == 1)[0], np.nonzero(np.diff(rel) == -1)[0]
    lid = req["lid"].astype(np.int64)
    n, prev = 0, 0
    for a, b in zip(starts, ends):
        if b - a >= 2 and (np.diff(lid[a:b]) < 0).all() and b - a == len(np.unique(lid[prev:a])):
            n += 1
        prev = b
    return n


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("wl", [FASST, TPL], ids=["fasst", "2pl"])
def test_device_lock_client_sends_what_the_reference_load_generator_sends(wl, fuse, monkeypatch):
    """one worker, one request per epoch, all 30,000 messages of the recordings in which the harness refuses one
    ACQUIRE in five (release / retry / rollback paths)"""
    monkeypatch.setenv("DINT_LOCK_CLIENT_FUSE", str(fuse))
    if wl == FASST:
        z = np.load(os.path.join(G, "clients_micro.npz"))
        meta = json.loads(str(z["meta"]))["fasst"]
        req = np.frombuffer(z["fasst_req"].tobytes(), wire.FASST_MSG)
        rep = np.frombuffer(z["fasst_rep"].tobytes(), wire.FASST_MSG)
        gc = GpuLockClient(FASST, 1, meta["key_space"], zipf_theta=None, device=0)
        hc = FasstClient(1, meta["key_space"], zipf_theta=None)
    else:
        z = np.load(os.path.join(G, "clients_micro_lcg.npz"))
        meta = json.loads(str(z["meta"]))["tpl"]
        req = np.frombuffer(z["tpl_req"].tobytes(), wire.TPL_MSG)
        rep = np.frombuffer(z["tpl_rep"].tobytes(), wire.TPL_MSG)
        kw = dict(read_pct=meta["read_pct"], zipf_theta=None, first_worker=meta["first_worker"])
        gc = GpuLockClient(TPL, 1, meta["key_space"], device=0, **kw)
        hc = LcgTplClient(1, meta["key_space"], **kw)
    assert len(req) == len(rep) == meta["messages"] == 30_000
    st = _stream()
    xs = st.cuda_stream
    for i in range(len(req)):
        gc.next(xs)
        out = gc.read_batch()
        assert out.tobytes() == req[i:i + 1].tobytes(), (i, out, req[i])
        _h2d(gc.batch_ptr, rep[i:i + 1])
        gc.consume(xs)
        hc.next()
        hc.consume(rep[i:i + 1].copy())
    gs, hs = gc.stats(), hc.stats()
    assert gs == hs
    assert gs["protocol_errors"] == 0 and gs["requests"] == len(req)
    if wl == FASST:  # (tests/test_client_golden.py; a lock_fasst commit without a write set sends no message of its own)
        assert set(rep["type"].tolist()) == {4, 5, 6, 7, 8}
        assert gs["rejects"] == int((rep["type"] == wire.Fasst.REJECT_LOCK).sum()) > 300
        assert gs["committed"] > 500 and gs["rollbacks"] == 0
    else:  # (tests/test_lock_clients_host.py)
        assert set(rep["action"].tolist()) == {2, 3, 5}
        assert gs["rejects"] == int((rep["action"] == wire.Tpl.REJECT_LOCK).sum()) > 0
        assert gs["committed"] == _tpl_commits(req) > 0
