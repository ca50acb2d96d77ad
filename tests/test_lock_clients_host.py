"""The lock_2pl load generator in C (dint_amd/csrc/tpl_client.cc, lock_clients.h) on the host, and the argument checks of
the lock clients' C ABI (include/dint_driver.h dint_tpl_client_*, dint_lock_gclient_*).

tests/golden/clients_micro_lcg.npz (make_golden_clients_micro_lcg.py) holds what the UNMODIFIED lock_2pl/caladan/client.cc
sent and received replaying the transactions LcgTplClient draws for its worker 0, with one ACQUIRE in five refused."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from dint_amd import _lib, wire
from dint_amd.driver import FasstClient, FasstClientConfig, GpuLockClient, LcgTplClient, LockClientConfig

G = os.path.join(os.path.dirname(__file__), "golden")
EINVAL, ESTATE = -1, -5


def test_lcg_tpl_client_sends_what_the_reference_load_generator_sends():
    z = np.load(os.path.join(G, "clients_micro_lcg.npz"))
    meta = json.loads(str(z["meta"]))["tpl"]
    req = np.frombuffer(z["tpl_req"].tobytes(), wire.TPL_MSG)
    rep = np.frombuffer(z["tpl_rep"].tobytes(), wire.TPL_MSG)
    assert len(req) == meta["messages"] and set(rep["action"].tolist()) == {2, 3, 5}
    t = LcgTplClient(1, meta["key_space"], read_pct=meta["read_pct"], zipf_theta=None, first_worker=meta["first_worker"])
    for i in range(len(req)):
        out = t.next()
        assert out.tobytes() == req[i:i + 1].tobytes(), ("lock_2pl", i, out, req[i])
        t.consume(rep[i:i + 1].copy())
    st = t.stats()
    assert st["protocol_errors"] == 0 and st["rejects"] > 0 and st["committed"] > 0
    assert st["rejects"] == int((rep["action"] == 3).sum()) and st["requests"] == len(req)


@pytest.mark.parametrize("theta", [None, 0.99])
def test_lcg_tpl_client_draws_the_fasst_clients_transactions(theta):
    """same seed, same draws: the 2PL worker's locks are the FaSST worker's keys, exclusive = its write set"""
    f = FasstClient(64, 1 << 20, zipf_theta=theta, first_worker=7)
    t = LcgTplClient(64, 1 << 20, zipf_theta=theta, first_worker=7)
    for w in range(64):
        keys, wkeys = f.peek(w)
        lids, types = t.peek(w)
        assert lids == keys == sorted(set(keys)) and 5 <= len(keys) <= 10
        assert [l for l, ty in zip(lids, types) if ty] == wkeys


def test_lcg_tpl_client_state_machine():
    """ACQUIRE in ascending order; REJECT with locks held -> RELEASE them in acquisition order, same transaction again;
    REJECT with nothing held -> the same ACQUIRE again; all held -> RELEASE in reverse order, committed"""
    t = LcgTplClient(1, 1 << 20, zipf_theta=None)
    lids, types = t.peek(0)

    def step(action):
        m = t.next()
        r = m.copy()
        r["action"] = action
        t.consume(r)
        return (int(m["action"][0]), int(m["lid"][0]), int(m["type"][0]))

    assert step(3) == (0, lids[0], types[0])   # refused with nothing held
    assert step(2) == (0, lids[0], types[0])   # the same ACQUIRE again
    assert step(2) == (0, lids[1], types[1])
    assert step(3) == (0, lids[2], types[2])   # refused with two held: release them in acquisition order
    assert [step(5) for _ in range(2)] == [(1, lids[0], types[0]), (1, lids[1], types[1])]
    got = [step(2) for _ in lids]
    assert got == [(0, l, ty) for l, ty in zip(lids, types)]
    got = [step(5) for _ in lids]
    assert got == [(1, l, ty) for l, ty in reversed(list(zip(lids, types)))]
    st = t.stats()
    assert st["committed"] == 1 and st["rejects"] == 2 and st["protocol_errors"] == 0
    assert t.peek(0)[0] != lids
    step(4)  # kRetry to an ACQUIRE: not a grant or a reject
    assert t.stats()["protocol_errors"] == 1


def _raw(L, name, res, args):
    f = getattr(L, name)
    f.restype, f.argtypes = res, args
    return f


@pytest.mark.parametrize("bad", [dict(n_workers=0), dict(key_space=15), dict(read_pct=101), dict(key_dist=2),
                                 dict(key_dist=1, zipf_theta=0.0), dict(key_dist=1, zipf_theta=1.0)])
def test_lock_clients_refuse_a_bad_config(bad):
    L = _lib.load()
    LcgTplClient(4, 1 << 10)  # binds the signatures
    base = dict(n_workers=4, first_worker=0, key_space=1 << 10, read_pct=80, key_dist=0, zipf_theta=0.0)
    h = C.c_void_p()
    cfg = FasstClientConfig(**dict(base, **bad))
    assert L.dint_tpl_client_create(C.byref(cfg), C.byref(h)) == EINVAL and not h.value
    assert L.dint_tpl_client_create(None, C.byref(h)) == EINVAL
    # the GPU client checks its config before it looks for a device
    create = _raw(L, "dint_lock_gclient_create", C.c_int, [C.POINTER(LockClientConfig), C.c_int32, C.POINTER(C.c_void_p)])
    for wl in (wire.Workload.FASST, wire.Workload.TPL):
        cfg = LockClientConfig(workload=int(wl), **dict(base, **bad))
        assert create(C.byref(cfg), -1, C.byref(h)) == EINVAL and not h.value
    if bad.get("key_dist", 1) == 1:  # (what the Python wrapper can express: zipf_theta None = uniform)
        kw = {k: v for k, v in dict(base, **bad).items() if k in ("n_workers", "key_space", "read_pct", "zipf_theta")}
        kw["zipf_theta"] = kw["zipf_theta"] if bad.get("key_dist") == 1 else None
        with pytest.raises(_lib.DintError, match=f"error {EINVAL}"):
            GpuLockClient(wire.Workload.TPL, **kw)
    for wl in (wire.Workload.LOG, wire.Workload.TATP, 99):  # lock workloads only
        cfg = LockClientConfig(workload=int(wl), **base)
        assert create(C.byref(cfg), -1, C.byref(h)) == EINVAL
    assert create(None, -1, C.byref(h)) == EINVAL


def test_lcg_tpl_client_refuses_calls_out_of_order():
    t = LcgTplClient(8, 1 << 16)
    rep = np.zeros(8, wire.TPL_MSG)
    with pytest.raises(_lib.DintError) as e:  # consume without next
        t.consume(rep)
    assert f"{ESTATE}" in str(e.value)
    t.next()
    with pytest.raises(_lib.DintError):  # a second next before consume: a null batch
        t.next()
    L = t._L
    assert L.dint_tpl_client_next(t._h) is None
    t.consume(rep)
    t.next()  # the order is restored
    assert L.dint_tpl_client_consume(t._h, None) == EINVAL
    for f, args in (("dint_tpl_client_get_stats", (None, None)), ("dint_tpl_client_peek", (None, 0, None, None, None))):
        assert getattr(L, f)(*args) == EINVAL
    lid, typ, n = (C.c_uint32 * 10)(), (C.c_uint8 * 10)(), C.c_uint32()
    assert L.dint_tpl_client_peek(t._h, 8, lid, typ, C.byref(n)) == EINVAL  # worker out of range
