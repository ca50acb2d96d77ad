#!/usr/bin/env python3
"""Generate tests/golden/clients_micro_lcg.npz: the request / reply stream of the UNMODIFIED reference lock_2pl load
generator (lock_2pl/caladan/client.cc, one worker) replaying the transactions that the C 2PL client
(dint_amd/csrc/tpl_client.cc, dint_amd.driver.LcgTplClient) draws for its worker 0, against a CPU oracle lock server, with
every 5th ACQUIRE refused by the harness (oracle/ref_harness/caladan/ref_client_micro.cc, `make -C oracle ref_client`).
Modelled on make_golden_clients_micro.py, which pins the numpy TplClient the same way.  Only runs where /root/reference
exists; the fixture is committed.

    python tests/golden/make_golden_clients_micro_lcg.py

The transactions are peeked one by one (dint_tpl_client_peek) while the client runs against a server that grants
everything, and written as one trace file of lock_2pl/caladan/trace_init.sh's format; tests/test_lock_clients_host.py
feeds the recorded replies to a fresh LcgTplClient and demands the recorded requests.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from dint_amd import wire  # noqa: E402
from dint_amd.driver import LcgTplClient  # noqa: E402
from make_golden_clients_micro import KEY_SPACE, N_TXN, REFUSE_EVERY, run  # noqa: E402


def tpl_transactions():
    """worker 0's first N_TXN transactions: every ACQUIRE granted, every RELEASE acknowledged"""
    c = LcgTplClient(1, KEY_SPACE, zipf_theta=None)
    txns, done = [], -1
    while len(txns) < N_TXN:
        if c.stats()["committed"] != done:
            done = c.stats()["committed"]
            txns.append(c.peek(0))
        m = c.next()
        m["action"] = np.where(m["action"] == 0, 2, 5)
        c.consume(m)
    return txns


if __name__ == "__main__":
    tt = tpl_transactions()
    lines = ["txn_id,action,lock_id,lock_type"]  # lock_2pl/caladan/trace_init.sh:9,20-23: acquire in order, release in reverse
    for tid, (lids, types) in enumerate(tt):
        lines += [f"{tid},0,{l},{t}" for l, t in zip(lids, types)] + [f"{tid},1,{l},{t}" for l, t in reversed(list(zip(lids, types)))]
    req, rep, st = run("ref_client_2pl", lines, wire.TPL_MSG)
    meta = {"tpl": dict(st, transactions=len(tt), refuse_every=REFUSE_EVERY, key_space=KEY_SPACE, read_pct=80, first_worker=0,
                        reply_actions={str(k): int(v) for k, v in enumerate(np.bincount(rep["action"], minlength=6)) if v})}
    print(json.dumps(meta, indent=1))
    path = os.path.join(HERE, "clients_micro_lcg.npz")
    np.savez_compressed(path, meta=json.dumps(meta), tpl_req=np.frombuffer(req.tobytes(), np.uint8),
                        tpl_rep=np.frombuffer(rep.tobytes(), np.uint8))
    print(f"wrote {path} ({os.path.getsize(path)/1e6:.2f} MB)")
