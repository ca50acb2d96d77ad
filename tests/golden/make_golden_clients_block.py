#!/usr/bin/env python3
"""Generate tests/golden/clients_block.npz: a BLOCK of consecutive reference clients per workload, cut to whole epochs,
so that one GPU launch can play all of them side by side (tests/test_gpu_client_golden.py) -- lanes of one wave in
different phases, refused and granted replies next to each other.

The UNMODIFIED <wl>/caladan/client_udp_shard.cc runs as in make_golden_clients.py (oracle/_ref/ref_client_<wl>, `make -C
oracle ref_client`; every 7th lock request refused by the harness), here for CLIENTS consecutive gids from FIRST_GID
(neither 0 nor a multiple of the wavefront) one after the other against the same three servers, MESSAGES each.  Only
runs where /root/reference exists; the fixture is committed.

    python tests/golden/make_golden_clients_block.py

A recording is cut wherever the message budget ran out; the closed-loop drivers move in epochs (one phase of every
client).  So each client's recording is fed to a one-client host Driver, which must send the recorded bytes, the
number E_c of whole epochs it holds is found, and every client is cut to its first E = min E_c epochs.  The fixture
holds, per workload, the canonicalised (make_golden_clients.canon) request and reply bytes of every client and shard in
order, and `<wl>_counts`, uint8[clients, E, 3]: the messages client c sends to shard s in epoch e -- the split a test of
many clients in one launch needs, taken from the reference's recording and not from the code under test.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from dint_amd import wire  # noqa: E402
from dint_amd.driver import Driver  # noqa: E402
from make_golden_clients import PAYLOAD_REQ, canon  # noqa: E402

FIRST_GID = {"tatp": 4243, "smallbank": 70_019}
CLIENTS = 96
MESSAGES = 260
N_ROWS = {"tatp": 7_000_000, "smallbank": 24_000_000}
REJECT = {"tatp": (8,), "smallbank": (10, 11)}  # kRejectLock; kRejectShared, kRejectExclusive
N_TYPES = {"tatp": 7, "smallbank": 6}


def req_canon(wl, a):
    """tests/test_client_golden.py::_canon"""
    return canon(wl, a, a)[0]


def whole_epochs(wl, gid, req, rep):
    """the per-epoch, per-shard message counts of the whole epochs this recording holds (a one-client host Driver must
    send the recorded bytes on the way)"""
    W = wire.Workload.TATP if wl == "tatp" else wire.Workload.SMALLBANK
    d = Driver(W, 1, N_ROWS[wl], first_client=gid)
    cur, counts = [0, 0, 0], []
    while True:
        out = d.next()
        if any(cur[s] + len(out[s]) > len(req[s]) for s in range(3)):
            return counts
        for s in range(3):
            assert req_canon(wl, out[s]).tobytes() == req[s][cur[s]:cur[s] + len(out[s])].tobytes(), (wl, gid, len(counts), s)
        d.consume([rep[s][cur[s]:cur[s] + len(out[s])].copy() for s in range(3)])
        counts.append([len(o) for o in out])
        for s in range(3):
            cur[s] += len(out[s])


def check(wl, z):
    """the conditions on the fixture (tests/test_client_golden.py checks them again): in aggregate every transaction
    type finishes, commits and aborts both occur, at least 100 lock requests were refused"""
    W = wire.Workload.TATP if wl == "tatp" else wire.Workload.SMALLBANK
    dt = wire.MSG_DTYPE[W]
    counts = z[f"{wl}_counts"]
    tot = {"txns": 0, "committed": 0, "by_type": [0] * 8}
    refused = 0
    for c in range(counts.shape[0]):
        gid = FIRST_GID[wl] + c
        req = [np.frombuffer(z[f"{wl}_{gid}_s{s}_req"].tobytes(), dt) for s in range(3)]
        rep = [np.frombuffer(z[f"{wl}_{gid}_s{s}_rep"].tobytes(), dt) for s in range(3)]
        assert [len(r) for r in req] == counts[c].sum(0).tolist() == [len(r) for r in rep]
        d = Driver(W, 1, N_ROWS[wl], first_client=gid)
        cur = [0, 0, 0]
        for e in range(counts.shape[1]):
            out = d.next()
            assert [len(o) for o in out] == counts[c, e].tolist()
            d.consume([rep[s][cur[s]:cur[s] + len(out[s])].copy() for s in range(3)])
            for s in range(3):
                cur[s] += len(out[s])
        st = d.stats()  # (a transaction is counted by the phase that follows its last replies)
        tot["txns"] += st["txns"]
        tot["committed"] += st["committed"]
        tot["by_type"] = [a + b for a, b in zip(tot["by_type"], st["by_type"])]
        refused += sum(int(np.isin(r["type"], REJECT[wl]).sum()) for r in rep)
    assert all(n > 0 for n in tot["by_type"][:N_TYPES[wl]]), tot
    assert 0 < tot["committed"] < tot["txns"], tot
    assert refused >= 100, refused
    return dict(tot, locks_refused=refused)


if __name__ == "__main__":
    out, meta = {}, {}
    with tempfile.TemporaryDirectory(prefix="dint_clients_block_") as td:
        for wl, g0 in FIRST_GID.items():
            assert g0 % 64 and CLIENTS >= 96
            dt = wire.TATP_MSG if wl == "tatp" else wire.SB_MSG
            pre = os.path.join(td, wl)
            subprocess.run([os.path.join(ROOT, "oracle", "_ref", f"ref_client_{wl}"), str(g0), str(MESSAGES), pre, str(CLIENTS)],
                           capture_output=True, text=True, check=True)
            rec, cnt = {}, {}
            for g in range(g0, g0 + CLIENTS):
                pairs = [canon(wl, np.fromfile(f"{pre}.{g}.s{s}.req", dt), np.fromfile(f"{pre}.{g}.s{s}.rep", dt)) for s in range(3)]
                rec[g] = ([p[0] for p in pairs], [p[1] for p in pairs])
                cnt[g] = whole_epochs(wl, g, *rec[g])
            E = min(len(c) for c in cnt.values())
            counts = np.array([cnt[g][:E] for g in range(g0, g0 + CLIENTS)], np.uint8)
            assert counts.shape == (CLIENTS, E, 3) and E > 0
            for c, g in enumerate(range(g0, g0 + CLIENTS)):
                for s in range(3):
                    n = int(counts[c, :, s].sum())
                    out[f"{wl}_{g}_s{s}_req"] = np.frombuffer(rec[g][0][s][:n].tobytes(), np.uint8)
                    out[f"{wl}_{g}_s{s}_rep"] = np.frombuffer(rec[g][1][s][:n].tobytes(), np.uint8)
            out[f"{wl}_counts"] = counts
            meta[wl] = dict(check(wl, out), epochs=E, messages=int(counts.sum()))
            print(wl, meta[wl])
    path = os.path.join(HERE, "clients_block.npz")
    np.savez_compressed(path, meta=json.dumps({"first_gid": FIRST_GID, "clients": CLIENTS, "n_rows": N_ROWS, "runs": meta}), **out)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "ebpf_store.npz"))
    print(f"wrote {path} ({size/1e6:.2f} MB; the largest fixture, ebpf_store.npz, has {limit/1e6:.2f} MB)")
    assert size <= limit
