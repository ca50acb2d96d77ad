"""The log replay's classification rule on the host (dint_amd/csrc/log_replay.h through dint_log_classify_host,
include/dint_driver.h) against the numpy statement of the same rule in dint_amd/recovery.py apply_log, and the argument
checks of the device calls (include/dint_abi.h dint_log_drain_device / dint_log_apply_device) that need no device.

The GPU kernels of csrc/k_replay.hip call the same log_replay.h functions; tests/test_gpu_log_replay.py holds them to the
host path end to end."""
import ctypes as C

import numpy as np
import pytest

from dint_amd import _lib, recovery, wire
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes

W, T = wire.Workload, wire.Tatp
EINVAL = -1


class _Recorder:
    """what recovery.apply_log needs of an engine: answers the READ probe from `exists`, keeps the batch it is handed"""

    workload = W.TATP

    def __init__(self, exists):
        self.exists, self.batch = exists, None

    def submit(self, m):
        r = m.copy()
        if (m["type"] == T.READ).all():
            r["type"] = [T.GRANT_READ if self.exists[(int(t), int(k))] else T.NOT_EXIST for t, k in zip(m["table"], m["key"])]
            return r
        self.batch = m.copy()
        r["type"] = T.COMMIT_BCK_ACK  # (the counts do not matter here)
        return r


def _classify(rec, exists0):
    L = _lib.load()
    rec = np.ascontiguousarray(rec)
    ex = np.ascontiguousarray(exists0, np.uint8)
    out = np.zeros(len(rec), np.uint8)
    assert L.dint_log_classify_host(rec.ctypes.data, len(rec), ex.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_classification_equals_recovery_apply_log_on_random_streams(seed):
    """300 rows over the five tables, 24,000 records, one in four a delete: insert -> commit -> delete -> insert chains on
    one row are the common case"""
    rng = np.random.default_rng(seed)
    rows = [(int(t), int(k)) for t, k in zip(rng.integers(0, 5, 300), rng.integers(0, 1 << 47, 300, dtype=np.uint64))]
    rows = sorted(set(rows))
    exists = {r: bool(rng.random() < 0.5) for r in rows}
    n = 24_000
    pick = rng.integers(0, len(rows), n)
    rec = np.zeros(n, wire.LOG_REC)
    rec["table"] = [rows[j][0] for j in pick]
    rec["key"] = [rows[j][1] for j in pick]
    rec["is_del"] = rng.random(n) < 0.25
    rec["ver"] = np.arange(n)
    rec["val"] = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    eng = _Recorder(exists)
    recovery.apply_log(eng, rec)
    want = eng.batch["type"]
    got = _classify(rec, [exists[rows[j]] for j in pick])
    assert (got == want).all()
    assert {int(x) for x in np.unique(got)} == {T.COMMIT_BCK, T.INSERT_BCK, T.DELETE_BCK}
    # the initial state is read for the first record of a row only: garbage everywhere else changes nothing
    first = np.zeros(n, bool)
    first[np.unique((rec["table"].astype(np.uint64) << np.uint64(60)) ^ rec["key"], return_index=True)[1]] = True
    noisy = np.where(first, [exists[rows[j]] for j in pick], rng.random(n) < 0.5)
    assert (_classify(rec, noisy) == want).all()


def test_replaying_a_primarys_ring_through_the_types_rebuilds_its_tables():
    prim = orc.TatpOracle(300, log_entries=1 << 20)
    for b in range(8):
        prim.replay(_committed_writes(prim, 3000, seed=b))
    rec = np.frombuffer(prim.ring[:prim.tail].tobytes(), wire.LOG_REC).copy()
    assert len(rec) == 24_000 and rec["is_del"].sum() > 100
    rep = orc.TatpOracle(300, log_entries=1 << 20)
    rd = np.zeros(len(rec), wire.TATP_MSG)
    rd["type"], rd["table"], rd["key"] = T.READ, rec["table"], rec["key"]
    exists0 = rep.replay(rd)["type"] == T.GRANT_READ
    types = _classify(rec, exists0)
    m = np.zeros(len(rec), wire.TATP_MSG)
    m["type"], m["table"], m["key"], m["val"], m["ver"] = types, rec["table"], rec["key"], rec["val"], rec["ver"]
    ack = rep.replay(m)["type"]
    want_ack = np.select([types == T.COMMIT_BCK, types == T.INSERT_BCK], [T.COMMIT_BCK_ACK, T.INSERT_BCK_ACK], T.DELETE_BCK_ACK)
    assert (ack == want_ack).all() and (types == T.INSERT_BCK).sum() > 0  # every operation was acked as what it is
    for t in range(5):
        a, b = prim.dump(t), rep.dump(t)
        ka, kb = np.argsort(a[0], kind="stable"), np.argsort(b[0], kind="stable")
        assert (a[0][ka] == b[0][kb]).all() and (a[1][ka] == b[1][kb]).all() and (a[2][ka] == b[2][kb]).all(), t


def test_new_calls_check_their_arguments_before_any_device_call():
    L = _lib.load()
    st = _lib.ApplyStats()
    lost = C.c_uint64()
    assert L.dint_log_apply_device(None, None, 0, 0, None) == EINVAL
    assert L.dint_log_apply_device(None, 4096, 10, 0, C.byref(st)) == EINVAL
    assert b"null" in L.dint_last_error()
    assert L.dint_log_drain_device(None, 4096, 10, C.byref(lost), None) == EINVAL
    assert L.dint_log_classify_host(None, 5, None, None) == EINVAL
    assert L.dint_log_classify_host(None, 0, None, None) == 0
    assert C.sizeof(_lib.ApplyStats) == 8 * 8
    assert _lib.ABI_VERSION == 5
