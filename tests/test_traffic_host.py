"""The traffic report's rule on the host (dint_amd/csrc/traffic_report.h through dint_traffic_report_host, include/dint_driver.h)
against the numpy form of tests/traffic_cases.py, field for field and list for list; the replies come from the CPU oracle's replay of
the same batch.  Every comparison is exact.  No device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import traffic_cases as tc
from dint_amd import _lib, traffic, wire
from oracle import oracle as orc

W = wire.Workload
EINVAL, ESTATE = -1, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP, CAP = 20, 1 << 17
wl_param = pytest.mark.parametrize("wl", tc.WORKLOADS, ids=tc.IDS)


def make_oracle(wl, n_slots=16, same_key=False):
    if wl == W.FASST:
        return orc.FasstOracle(n_slots)
    if wl == W.TPL:
        return orc.TplOracle(n_slots)
    if wl == W.STORE:
        return orc.StoreOracle(tc.sizes(wl)[0], populate_n=POP)
    if wl == W.TATP:
        o = orc.TatpOracle(tc.N_ROWS, log_entries=CAP, populate_n=POP)
        if same_key:
            o.same_key_mode()
        return o
    return orc.SmallbankOracle(tc.N_ROWS, log_entries=CAP, populate_n=POP)


def host(wl, req, rep, n_slots=16, top=16, flags=0):
    r = traffic.report_host(wl, req, rep, n_slots=n_slots, n_rows=tc.N_ROWS, flags=flags, top=top)
    assert r["temp_bytes"] == 0
    return r


@wl_param
@pytest.mark.parametrize("mix", ["one", "distinct", "zipf"])
def test_host_form_equals_numpy_on_every_size(wl, mix):
    for n_slots in ((16, 4099) if tc.is_lock(wl) else (16,)):
        o = make_oracle(wl, n_slots)
        for n in tc.SIZES:
            req = tc.batch(wl, tc.key_mix(wl, n, mix, seed=n), seed=n + 1)
            rep = o.replay(req)
            want = tc.np_report(wl, req, rep, tc.sizes(wl, n_slots), 16)
            tc.assert_same(host(wl, req, rep, n_slots), want, (n, n_slots))
            assert want["n"] == n and (mix != "one" or want["distinct_keys"] <= tc.N_TABLES[wl])
            if mix == "distinct" and n:
                assert want["distinct_keys"] == want["keyed"] == sum(want["key_hist"][:1])
            # no reply array: every reply-derived field 0, the by-rejects list empty
            bare = host(wl, req, None, n_slots)
            tc.assert_same(bare, tc.np_report(wl, req, None, tc.sizes(wl, n_slots), 16), (n, "no replies"))
            assert bare["rejects"] == bare["misses"] == bare["shared_unit_rejects"] == 0 and bare["by_rejects"] == []
            assert not np.array(bare["rep_types"]).any()


@wl_param
def test_edge_batches(wl):
    o = make_oracle(wl)
    for name, req in tc.edge_batches(wl).items():
        rep = o.replay(req)
        want = tc.np_report(wl, req, rep, tc.sizes(wl), 16)
        tc.assert_same(host(wl, req, rep), want, name)
        if name == "bad_tables":
            assert want["bad_table"] >= 60 and want["keyed"] + want["log_requests"] + want["bad_table"] == len(req)
        if name == "every_type_byte":
            assert sum(row[31] for row in want["req_types"]) == 10 and want["others"] > 0
        if name == "logs_between":
            assert want["log_requests"] >= 130
        if name == "extreme_keys":
            keys = {e["key"] for e in want["by_requests"]}
            assert 0 in keys and (0xFFFFFFFF if tc.is_lock(wl) else 0xFFFFFFFFFFFFFFFF) in keys
        if name == "same_key_two_tables":
            assert len({(e["table"], e["key"]) for e in want["by_requests"] if e["key"] == 3}) == tc.N_TABLES[wl]


@wl_param
def test_keys_that_share_a_unit_and_a_lock_slot(wl):
    groups = tc.sharing_groups(wl)
    req = tc.sharing_batch(wl, groups)
    o = make_oracle(wl)
    rep = o.replay(req)
    want = tc.np_report(wl, req, rep, tc.sizes(wl), 16)
    tc.assert_same(host(wl, req, rep), want)
    assert want["shared_units"] == len(groups) and want["shared_unit_requests"] == len(req)
    if wl != W.STORE:
        assert want["rejects"] >= 4 * len(groups) and want["shared_unit_rejects"] == want["rejects"]  # rejected because ANOTHER key holds the slot
    if wl in (W.TATP, W.SMALLBANK):
        assert want["shared_slots"] == len(groups) and want["shared_slot_rejects"] == want["rejects"]
    if wl == W.TATP:  # the same trace on the same-key build: a reject of the holder's own key is 28, of another key 8
        o2 = make_oracle(wl, same_key=True)
        rep2 = o2.replay(req)
        w2 = tc.np_report(wl, req, rep2, tc.sizes(wl), 16)
        tc.assert_same(host(wl, req, rep2, flags=_lib.FLAG_LOCK_SAME_KEY), w2)
        assert w2["rep_types"][0][28] == len(groups) and w2["rep_types"][0][8] == want["rep_types"][0][8] - len(groups)
        assert w2["rejects"] == want["rejects"]


@wl_param
def test_top_list_sizes_and_ties(wl):
    req = tc.edge_batches(wl)["ties"]
    rep = make_oracle(wl).replay(req)
    for top in (0, 1, 16, 39, 40, 41, 4096):
        want = tc.np_report(wl, req, rep, tc.sizes(wl), top)
        got = host(wl, req, rep, top=top)
        tc.assert_same(got, want, top)
        assert got["n_by_requests"] == min(top, got["distinct_keys"])
    # many keys tied at the cut: the list is decided by (table, key) alone
    got = host(wl, req, None, top=16)
    order = [(e["table"], e["key"]) for e in got["by_requests"]]
    assert len({e["requests"] for e in got["by_requests"]}) <= 2 and got["distinct_keys"] > 16
    same = [e for e in got["by_requests"] if e["requests"] == got["by_requests"][-1]["requests"]]
    assert [(e["table"], e["key"]) for e in same] == sorted((e["table"], e["key"]) for e in same) and len(set(order)) == 16


def test_refusals_leave_the_outputs_as_they_were():
    L = _lib.load()
    req = tc.batch(W.TATP, np.arange(50, dtype=np.uint64), 1)
    rep = req.copy()
    out = np.full(C.sizeof(_lib.TrafficReport), 0xEE, np.uint8)
    a, b = np.full(4 * 48, 0xEE, np.uint8), np.full(4 * 48, 0xEE, np.uint8)
    po = C.cast(out.ctypes.data, C.POINTER(_lib.TrafficReport))

    def call(wl=W.TATP, q=req.ctypes.data, p=rep.ctypes.data, n=50, top=4, o=po, la=a.ctypes.data, lb=b.ctypes.data):
        return L.dint_traffic_report_host(int(wl), 16, 64, 0, q, p, n, top, o, la, lb)

    assert call(wl=W.LOG) == ESTATE
    assert call(wl=99) == EINVAL
    assert call(p=req.ctypes.data) == EINVAL and b"replies" in L.dint_last_error()
    assert call(q=None) == EINVAL and call(o=None) == EINVAL and call(la=None) == EINVAL and call(lb=None) == EINVAL
    assert call(top=4097) == EINVAL and call(n=(1 << 24) + 1) == EINVAL
    assert (out == 0xEE).all() and (a == 0xEE).all() and (b == 0xEE).all()
    assert call() == 0 and call(n=0, q=None, p=None, top=0, la=None, lb=None) == 0
    assert C.sizeof(_lib.TrafficReport) == 8 * 402 and C.sizeof(_lib.TrafficKey) == 48


@wl_param
def test_arrays_at_odd_addresses(wl):
    req = tc.batch(wl, tc.key_mix(wl, 300, "zipf", 3), 4)
    rep = make_oracle(wl).replay(req)
    want = tc.np_report(wl, req, rep, tc.sizes(wl), 16)
    for off in (1, 7):
        q, p = np.zeros(req.nbytes + off, np.uint8), np.zeros(req.nbytes + off, np.uint8)
        q[off:], p[off:] = req.view(np.uint8), rep.view(np.uint8)
        tc.assert_same(traffic.report_host(wl, q[off:], p[off:], n_slots=16, n_rows=tc.N_ROWS), want, off)


def test_the_host_geometry_is_the_engine_formula_whatever_the_flags():
    """dint_hash_size of an engine created with n_rows is the reference's formula (tests/test_gpu_traffic.py holds the engine to it);
    no dint_config flag changes it, so the host form under every flag reports the same units"""
    req = tc.batch(W.TATP, np.arange(2000, dtype=np.uint64), 1, tables=np.full(2000, 4))
    want = tc.np_report(W.TATP, req, None, tc.sizes(W.TATP), 4)
    for flags in (0, 1, 2, 4, 8, 16, 32, 63):
        tc.assert_same(host(W.TATP, req, None, top=4, flags=flags), want, flags)
    assert want["distinct_units"] == tc.sizes(W.TATP)[4] == 90  # every CALL_FORWARDING bucket is hit


def test_merge_keeps_the_additive_fields_and_says_what_it_drops():
    reqs = [tc.batch(W.SMALLBANK, tc.key_mix(W.SMALLBANK, n, "zipf", n), n) for n in (100, 257)]
    o = make_oracle(W.SMALLBANK)
    reps = [o.replay(r) for r in reqs]
    parts = [host(W.SMALLBANK, q, p) for q, p in zip(reqs, reps)]
    m = traffic.merge(parts)
    whole = host(W.SMALLBANK, np.concatenate(reqs), np.concatenate(reps))
    for k in traffic.ADDITIVE + traffic.ADDITIVE_LISTS:
        assert m[k] == whole[k], k
    assert m["batches"] == 2 and not (set(traffic.NOT_ADDITIVE) & set(m)) and set(m["dropped"]) == set(traffic.NOT_ADDITIVE)
    assert set(traffic.ADDITIVE + traffic.ADDITIVE_LISTS + traffic.NOT_ADDITIVE) == set(whole)
    text = traffic.format_report(whole)
    assert f"requests {whole['n']}" in text and "top 16 by requests" in text and "dropped" in traffic.format_report(m)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    """tests/native/traffic_main.cc with the host code of k_traffic.hip under AddressSanitizer and UBSan: arrays in heap blocks of
    exactly their size and at odd addresses, more list entries than distinct keys, refusals.  Nothing of it is loaded into python"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "traffic_main")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "native", "traffic_main.cc"),
                           os.path.join(ROOT, "dint_amd", "csrc", "k_traffic.hip"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout + r.stderr
