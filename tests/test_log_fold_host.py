"""The log fold's rule on the host (dint_amd/csrc/log_fold.h through dint_log_fold_host, include/dint_driver.h) against the CPU
oracle: for every hand-built log of tests/log_fold_cases.py the records become backup messages by recovery.apply_log's numpy rule
and are replayed through TatpOracle / SmallbankOracle; the host form's repair records are applied to the dump in numpy (its
deferred records first go through a twin oracle, in log order, as the device call sends them through the serial replay); the two
row multisets must be equal per table and the stats equal the counts taken from the messages.  Every comparison is exact.

The GPU kernels of csrc/k_fold.hip call the same log_fold.h functions; tests/test_gpu_log_fold.py holds them to the unfolded path.

`python tests/test_log_fold_host.py FILE` writes a few of the cases with the host form's results into FILE, for the stand-alone
sanitizer program tests/native/log_fold_main.cc."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]  # (run as a script: tests/ and the repository root)
import log_fold_cases as lfc  # noqa: E402
from dint_amd import _lib, recovery, wire  # noqa: E402
from kvkeys import np_bucket  # noqa: E402

W = wire.Workload
EINVAL = -1
TATP = lfc.tatp_cases()
SB = lfc.smallbank_cases()


def _apply_repair(dump, repair, table, val_size):
    """the repair records of one table applied to its dumped rows: {key: [(ver, val), ...]} in dump order"""
    rows = {}
    for k, v, x in zip(*dump):
        rows.setdefault(int(k), []).append((int(v), bytes(x)))
    for r in repair[repair["table"] == table]:
        k = int(r["key"])
        if r["is_del"]:
            rows[k].pop(0)  # the visible row; a delete is only ever emitted for a row that is held once
            if not rows[k]:
                del rows[k]
        elif k in rows:
            rows[k][0] = (int(r["ver"]), bytes(r["val"][:val_size]))
        else:
            rows[k] = [(int(r["ver"]), bytes(r["val"][:val_size]))]
    return sorted((k, v, x) for k, l in rows.items() for v, x in l)


def _run(workload, loads, rec):
    nt, vs = (5, 40) if workload == W.TATP else (2, 8)
    full, twin = lfc.oracle_for(workload, loads), lfc.oracle_for(workload, loads)
    hs = [full.hash_size(t) for t in range(nt)]
    before = [twin.dump(t) for t in range(nt)]
    want = recovery.apply_log(lfc.OracleEngine(workload, full), rec)  # the serial replay, and its counts from the messages
    deferred, repair, st = recovery.fold_log_host(workload, hs, before, rec)
    if deferred.any():
        recovery.apply_log(lfc.OracleEngine(workload, twin), rec[deferred])
    for t in range(nt):
        assert _apply_repair(twin.dump(t), repair, t, vs) == lfc.sorted_rows(full.dump(t)), t
    return want, deferred, repair, st


def _check_stats(workload, want, rec, deferred, repair, st):
    n = len(rec)
    assert st["applied"] == n and st["chunks"] == 1
    if workload == W.TATP:
        assert (st["commits"], st["inserts"], st["deletes"]) == (want["commits"], want["inserts"], want["deletes"])
    else:
        assert (st["commits"], st["inserts"], st["deletes"]) == (want["acks"], 0, 0)
    assert st["deferred_records"] == int(deferred.sum()) and st["folded_records"] == n - int(deferred.sum())
    assert st["rows"] == len(np.unique(np.stack([rec["table"].astype(np.uint64), rec["key"]]), axis=1).T)
    assert st["repair_records"] == len(repair)
    assert (st["updated"], st["inserted"], st["deleted"], st["refused"]) == (0, 0, 0, 0)
    # the zero bytes, and the order the repair demands: ascending (table, bucket)
    assert (repair["pad"] == 0).all() and (repair["val"][repair["is_del"] != 0] == 0).all() and (repair["ver"][repair["is_del"] != 0] == 0).all()
    o = lfc.oracle_for(workload, [])
    place = np.zeros(len(repair), np.int64)
    for t in np.unique(repair["table"]):
        m = repair["table"] == t
        place[m] = (int(t) << 32) + np_bucket(repair["key"][m], o.hash_size(int(t))).astype(np.int64)
    assert (np.diff(place) >= 0).all()


@pytest.mark.parametrize("name", sorted(TATP))
def test_tatp_host_form_leaves_the_rows_of_the_serial_replay(name):
    loads, rec = TATP[name]
    want, deferred, repair, st = _run(W.TATP, loads, rec)
    _check_stats(W.TATP, want, rec, deferred, repair, st)
    if name in ("duplicate_with_neighbour", "all_deferred"):
        assert st["deferred_buckets"] == 1
    else:
        assert st["deferred_records"] == 0 and st["deferred_buckets"] == 0  # a log of which no record is deferred


def test_the_duplicated_key_defers_its_bucket_and_no_other():
    loads, rec = TATP["duplicate_with_neighbour"]
    _, deferred, _, st = _run(W.TATP, loads, rec)
    dup = loads[0][1][0]
    t = loads[0][0]
    hs = lfc.oracle_for(W.TATP, []).hash_size(t)
    same = (rec["table"] == t) & (np_bucket(rec["key"], hs) == np_bucket(np.array([dup], np.uint64), hs)[0])
    assert len(np.unique(rec["key"][same])) == 2  # the key and its neighbour
    assert (deferred == same).all() and 0 < same.sum() < len(rec)
    loads, rec = TATP["all_deferred"]
    _, deferred, repair, st = _run(W.TATP, loads, rec)
    assert deferred.all() and len(repair) == 0 and st["folded_records"] == 0


def test_versions_wrap_and_counts_follow_the_rule():
    loads, rec = TATP["version_wraps"]
    _, _, repair, _ = _run(W.TATP, loads, rec)
    assert len(repair) == 1 and repair["ver"][0] == 3  # 2^32 - 2 + 5
    loads, rec = TATP["alternating_absent"]
    _, _, repair, st = _run(W.TATP, loads, rec)
    assert len(repair) == 0 and (st["inserts"], st["deletes"], st["commits"]) == (2000, 2000, 0)
    loads, rec = TATP["alternating_present"]
    _, _, repair, st = _run(W.TATP, loads, rec)
    assert len(repair) == 1 and repair["is_del"][0] == 1 and (st["inserts"], st["deletes"], st["commits"]) == (1999, 2000, 1)
    loads, rec = TATP["delete_first_absent"]
    _, _, repair, st = _run(W.TATP, loads, rec)
    assert len(repair) == 1 and repair["ver"][0] == 0 and st["deletes"] == 4 and st["inserts"] == 1


@pytest.mark.parametrize("name", sorted(SB))
def test_smallbank_host_form(name):
    loads, rec = SB[name]
    want, deferred, repair, st = _run(W.SMALLBANK, loads, rec)
    _check_stats(W.SMALLBANK, want, rec, deferred, repair, st)
    assert not deferred.any() and (repair["is_del"] == 0).all() and (repair["val"][:, 8:] == 0).all()
    assert ((repair["key"] & lfc.ABSENT) == 0).all()  # an absent row: nothing
    if name == "absent_only":
        assert len(rec) > 0 and len(repair) == 0


def test_arguments_and_struct_layout():
    L = _lib.load()
    st = _lib.FoldStats()
    assert C.sizeof(_lib.FoldStats) == 23 * 8 and _lib.FOLD_DRY_RUN == 1
    assert L.dint_log_apply_folded_device(None, None, 0, 0, 0, None) == EINVAL
    assert L.dint_log_apply_folded_device(None, 4096, 10, 0, 0, C.byref(st)) == EINVAL
    hs = np.array([75], "<u8")
    off = np.zeros(2, "<u8")
    assert L.dint_log_fold_host(int(W.TATP), 1, hs.ctypes.data, off.ctypes.data, None, None, None, 0, None, None, 0, C.byref(st)) == 0
    assert L.dint_log_fold_host(int(W.TATP), 1, hs.ctypes.data, off.ctypes.data, None, None, None, 5, None, None, 0, None) == EINVAL
    assert L.dint_log_fold_host(int(W.STORE), 1, hs.ctypes.data, off.ctypes.data, None, None, None, 0, None, None, 0, None) == EINVAL
    assert L.dint_log_fold_host(int(W.TATP), 6, hs.ctypes.data, off.ctypes.data, None, None, None, 0, None, None, 0, None) == EINVAL
    import inspect
    assert "fold" in inspect.signature(recovery.LogShipper.__init__).parameters


def _write(path):
    """cases for tests/native/log_fold_main.cc: per case {u32 workload, n_tables; u64 hash_size[5], row_off[6]; keys; vers; u64 n;
    records; deferred flags; u64 repair records; the records; 23 u64 of stats}"""
    pick = [(W.TATP, TATP[k]) for k in ("lengths", "alternating_present", "duplicate_with_neighbour", "all_deferred", "one_record",
                                        "delete_first_absent", "version_wraps")] + [(W.SMALLBANK, SB["small"]), (W.SMALLBANK, SB["absent_only"])]
    with open(path, "wb") as f:
        f.write(np.uint64(len(pick)).tobytes())
        for wl, (loads, rec) in pick:
            nt = 5 if wl == W.TATP else 2
            o = lfc.oracle_for(wl, loads)
            dumps = [o.dump(t) for t in range(nt)]
            hs = [o.hash_size(t) for t in range(nt)]
            deferred, repair, _ = recovery.fold_log_host(wl, hs, dumps, rec)
            s = _lib.FoldStats()
            # (the stats as the C struct: once more through the raw call)
            off = np.zeros(6, "<u8")
            off[1:nt + 1] = np.cumsum([len(d[0]) for d in dumps])
            keys = np.concatenate([d[0] for d in dumps]).astype("<u8")
            vers = np.concatenate([d[1] for d in dumps]).astype("<u4")
            h5 = np.zeros(5, "<u8")
            h5[:nt] = hs
            out_d = np.zeros(len(rec), np.uint8)
            out_r = np.zeros(len(rec), wire.LOG_REC)
            got = _lib.load().dint_log_fold_host(int(wl), nt, h5.ctypes.data, off.ctypes.data, keys.ctypes.data, vers.ctypes.data,
                                                 np.ascontiguousarray(rec).ctypes.data, len(rec), out_d.ctypes.data, out_r.ctypes.data,
                                                 len(rec), C.byref(s))
            assert got == len(repair)
            f.write(np.array([int(wl), nt], "<u4").tobytes() + h5.tobytes() + off.tobytes() + keys.tobytes() + vers.tobytes())
            f.write(np.uint64(len(rec)).tobytes() + np.ascontiguousarray(rec).tobytes() + deferred.astype(np.uint8).tobytes())
            f.write(np.uint64(len(repair)).tobytes() + repair.tobytes() + bytes(s))


if __name__ == "__main__":
    _write(sys.argv[1])
