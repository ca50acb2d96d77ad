"""The traffic report of a batch (include/dint_abi.h dint_traffic_report; csrc/traffic_report.h is the rule) on the Python side:
the host form over numpy arrays, the merge of several reports, and a plain-text table.

``Engine.traffic_report`` takes a batch where it lies in HBM; ``report_host`` applies the same rule header to a batch in host
memory without a device call.  Both return the same dict: every scalar of ``struct dint_traffic_report`` as an int, ``key_hist`` /
``unit_hist`` / ``req_types`` / ``rep_types`` as lists, and ``by_requests`` / ``by_rejects`` as lists of dicts of
``dint_traffic_key``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .wire import MSG_DTYPE, Workload

#: the fields of a report that add up over batches (everything else is about ONE batch: see merge)
ADDITIVE = ("n", "keyed", "bad_table", "log_requests", "reads", "locks", "unlocks", "writes", "others", "rejects", "misses")
ADDITIVE_LISTS = ("req_types", "rep_types")
#: ... and the ones merge drops
NOT_ADDITIVE = ("distinct_keys", "distinct_units", "distinct_lock_slots", "max_key_requests", "max_unit_requests", "max_unit",
                "max_unit_table", "shared_units", "shared_unit_requests", "shared_unit_rejects", "shared_slots", "shared_slot_requests",
                "shared_slot_rejects", "key_hist", "unit_hist", "by_requests", "by_rejects", "n_by_requests", "n_by_rejects", "temp_bytes")


def unpack(out, by_requests, by_rejects) -> dict:
    """a filled TrafficReport and its two TrafficKey arrays as the report dict"""
    d = out.as_dict()
    d["by_requests"] = [by_requests[k].as_dict() for k in range(d["n_by_requests"])]
    d["by_rejects"] = [by_rejects[k].as_dict() for k in range(d["n_by_rejects"])]
    return d


def report_host(workload, reqs: np.ndarray, replies=None, *, n_slots: int = 0, n_rows: int = 0, flags: int = 0, top: int = 16) -> dict:
    """dint_traffic_report_host: the report of a batch in host memory under the geometry of an engine created with (workload,
    n_slots, n_rows, flags).  reqs / replies: arrays of the workload's wire dtype (or their bytes); any alignment."""
    L = _lib.load()
    size = MSG_DTYPE[Workload(workload)].itemsize
    reqs = np.ascontiguousarray(reqs)
    n = reqs.nbytes // size
    if replies is not None:
        replies = np.ascontiguousarray(replies)
        if replies.nbytes != reqs.nbytes:
            raise ValueError("replies[i] answers reqs[i]: the arrays have the same length")
    out = _lib.TrafficReport()
    a, b = (_lib.TrafficKey * max(top, 1))(), (_lib.TrafficKey * max(top, 1))()
    _lib.check(L.dint_traffic_report_host(int(workload), n_slots, n_rows, flags, reqs.ctypes.data if n else None,
                                          None if replies is None else replies.ctypes.data, n, top, C.byref(out), a, b))
    return unpack(out, a, b)


def merge(reports) -> dict:
    """The sum of several batches' reports -- of the ADDITIVE fields only: request and reply counts and the two type
    histograms.  Distinct counts, max_*, shared_*, the per-key and per-unit histograms and the top lists say something about ONE
    batch (a key of two batches is one key, not two) and are DROPPED: the result has no such entry.  ``batches`` counts the
    reports merged; ``dropped`` names what was left out."""
    reports = list(reports)
    m = {k: sum(int(r[k]) for r in reports) for k in ADDITIVE}
    for k in ADDITIVE_LISTS:
        m[k] = [[sum(int(r[k][t][b]) for r in reports) for b in range(32)] for t in range(5)]
    m["batches"] = len(reports)
    m["dropped"] = list(NOT_ADDITIVE)
    return m


def _hist_line(h) -> str:
    return " ".join(f"2^{b}:{c}" for b, c in enumerate(h) if c) or "-"


def format_report(report: dict) -> str:
    """a report (or a merged one) as a plain-text table"""
    r = report
    lines = []
    lines.append(f"requests {r['n']}  keyed {r['keyed']}  bad_table {r['bad_table']}  log {r['log_requests']}" +
                 (f"  ({r['batches']} batches merged)" if "batches" in r else ""))
    lines.append(f"class    reads {r['reads']}  locks {r['locks']}  unlocks {r['unlocks']}  writes {r['writes']}  others {r['others']}")
    keyed = max(r["keyed"], 1)
    lines.append(f"replies  rejects {r['rejects']} ({r['rejects'] / keyed:.3f} of keyed)  misses {r['misses']} ({r['misses'] / keyed:.3f})")
    for name in ("req_types", "rep_types"):
        for t, row in enumerate(r[name]):
            if any(row):
                lines.append(f"{name} table {t}: " + " ".join(f"{y}{'+' if y == 31 else ''}:{c}" for y, c in enumerate(row) if c))
    if "distinct_keys" in r:
        lines.append(f"distinct keys {r['distinct_keys']}  units {r['distinct_units']}  lock slots {r['distinct_lock_slots']}")
        lines.append(f"hottest  key {r['max_key_requests']} requests;  unit {r['max_unit_requests']} requests "
                     f"(table {r['max_unit_table']} unit {r['max_unit']})")
        lines.append(f"keys by requests   {_hist_line(r['key_hist'])}")
        lines.append(f"units by requests  {_hist_line(r['unit_hist'])}")
        lines.append(f"shared units {r['shared_units']}: {r['shared_unit_requests']} requests, {r['shared_unit_rejects']} rejects")
        lines.append(f"shared lock slots {r['shared_slots']}: {r['shared_slot_requests']} lock-slot requests, {r['shared_slot_rejects']} rejects")
        for name in ("by_requests", "by_rejects"):
            if r.get(name):
                lines.append(f"top {len(r[name])} {name.replace('_', ' ')}:")
                lines.append(f"  {'table':>5} {'key':>20} {'requests':>9} {'reads':>8} {'locks':>8} {'unlocks':>8} {'writes':>8} {'rejects':>8} {'misses':>8} {'first':>9}")
                for e in r[name]:
                    lines.append(f"  {e['table']:>5} {e['key']:>20} {e['requests']:>9} {e['reads']:>8} {e['locks']:>8} {e['unlocks']:>8} "
                                 f"{e['writes']:>8} {e['rejects']:>8} {e['misses']:>8} {e['first_index']:>9}")
    else:
        lines.append("(merged: per-batch fields -- distinct counts, maxima, shared_*, histograms per key / unit, top lists -- dropped)")
    return "\n".join(lines)
