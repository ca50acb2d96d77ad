"""dint_traffic_report on the device (dint_amd/csrc/k_traffic.hip) against the numpy form of tests/traffic_cases.py and against the host
form, field for field and list for list, for the five keyed workloads.  The replies are the engine's own: every batch goes through
submit_device first, and those replies are held to the CPU oracle's replay.  Tables are small (lock tables of 16 and 4,099 slots, kv
tables for 64 rows) so that keys share units and lock slots.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import traffic_cases as tc
from dint_amd import _lib, traffic, wire
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W = wire.Workload
EINVAL, ESTATE = -1, -5
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


def make_engine(wl, n_slots=16, flags=0, **kw):
    from dint_amd.engine import Engine

    e = Engine(wl, n_slots=n_slots, n_rows=tc.N_ROWS, log_entries=CAP, flags=flags, **kw)
    if not tc.is_lock(wl):
        if kw.get("shard_count", 1) == 1:
            e.populate(POP)
        assert [e.hash_size(t) for t in range(tc.N_TABLES[wl])] == tc.sizes(wl)  # the engine's geometry is the reference's formula
    return e


def up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


class Pair:
    """an engine and the oracle that has seen the same batches"""

    def __init__(self, wl, n_slots=16, same_key=False):
        self.wl, self.n_slots = wl, n_slots
        self.flags = _lib.FLAG_LOCK_SAME_KEY if same_key else 0
        self.eng, self.o = make_engine(wl, n_slots, self.flags), make_oracle(wl, n_slots, same_key)

    def answer(self, req):
        """the batch through submit_device: (d_req, d_rep, replies), the replies equal to the oracle's"""
        import torch

        d_req = up(req)
        d_rep = torch.zeros_like(d_req)
        if len(req):
            self.eng.submit_device(d_req, len(req), d_rep)
            self.eng.sync()
        rep = np.frombuffer(d_rep.cpu().numpy().tobytes(), req.dtype)
        assert rep.tobytes() == self.o.replay(req).tobytes()
        assert d_req.cpu().numpy().tobytes() == req.tobytes()
        return d_req, d_rep, rep

    def check(self, req, top=16, what=""):
        """device report == numpy form == host form"""
        d_req, d_rep, rep = self.answer(req)
        got = self.eng.traffic_report(d_req, len(req), d_rep, top=top)
        want = tc.np_report(self.wl, req, rep, tc.sizes(self.wl, self.n_slots), top)
        tc.assert_same(got, want, what)
        tc.assert_same(got, traffic.report_host(self.wl, req, rep, n_slots=self.n_slots, n_rows=tc.N_ROWS, flags=self.flags, top=top), (what, "host"))
        assert (got["temp_bytes"] > 0) == (len(req) > 0)
        bare = self.eng.traffic_report(d_req, len(req), None, top=top)
        tc.assert_same(bare, tc.np_report(self.wl, req, None, tc.sizes(self.wl, self.n_slots), top), (what, "no replies"))
        assert bare["rejects"] == bare["misses"] == 0 and bare["by_rejects"] == [] and not np.array(bare["rep_types"]).any()
        return got


@wl_param
@pytest.mark.parametrize("mix", ["one", "distinct", "zipf"])
def test_device_report_equals_numpy_and_host_on_every_size(wl, mix):
    for n_slots in ((16, 4099) if tc.is_lock(wl) else (16,)):
        p = Pair(wl, n_slots)
        for n in tc.SIZES:
            got = p.check(tc.batch(wl, tc.key_mix(wl, n, mix, seed=n), seed=n + 1), what=(n, n_slots))
            assert got["n"] == n
            if n == 70001 and mix == "distinct":
                assert got["by_requests"][0]["first_index"] < n and max(e["first_index"] for e in got["by_requests"]) > 0
            if n == 70001 and mix == "one":
                assert got["max_key_requests"] >= n // (2 * tc.N_TABLES[wl])  # one key per table: a run over hundreds of tiles


@wl_param
def test_edge_batches(wl):
    p = Pair(wl)
    for name, req in tc.edge_batches(wl).items():
        got = p.check(req, what=name)
        if name == "bad_tables":
            assert got["bad_table"] >= 60
        if name == "every_type_byte":
            assert sum(row[31] for row in got["req_types"]) == 10 and got["others"] > 0
        if name == "logs_between":
            assert got["log_requests"] >= 130
        if name == "extreme_keys":
            keys = {e["key"] for e in got["by_requests"]}
            assert 0 in keys and (0xFFFFFFFF if tc.is_lock(wl) else 0xFFFFFFFFFFFFFFFF) in keys


@wl_param
def test_keys_that_share_a_unit_and_a_lock_slot(wl):
    groups = tc.sharing_groups(wl)
    req = tc.sharing_batch(wl, groups)
    got = Pair(wl).check(req)
    assert got["shared_units"] == len(groups) and got["shared_unit_requests"] == len(req)
    if wl != W.STORE:
        assert got["rejects"] >= 4 * len(groups) and got["shared_unit_rejects"] == got["rejects"]
    if wl in (W.TATP, W.SMALLBANK):
        assert got["shared_slots"] == len(groups) and got["shared_slot_rejects"] == got["rejects"]
    if wl == W.TATP:  # the same trace with DINT_FLAG_LOCK_SAME_KEY: the holder's own key is answered 28, another key 8
        g2 = Pair(wl, same_key=True).check(req, what="same key")
        assert g2["rep_types"][0][28] == len(groups) and g2["rep_types"][0][8] == got["rep_types"][0][8] - len(groups)
        assert g2["rejects"] == got["rejects"]


@wl_param
def test_top_list_sizes_and_ties(wl):
    p = Pair(wl)
    req = tc.edge_batches(wl)["ties"]
    for top in (0, 1, 16, 40, 4096):
        got = p.check(req, top=top, what=top)
        assert got["n_by_requests"] == min(top, got["distinct_keys"])
    got = p.eng.traffic_report(up(req), len(req), None, top=16)
    same = [(e["table"], e["key"]) for e in got["by_requests"] if e["requests"] == got["by_requests"][-1]["requests"]]
    assert got["distinct_keys"] == 40 and same == [(0, k) for k in range(100, 116)]  # 40 keys of 3 requests: (table, key) alone decides


@wl_param
def test_arrays_at_any_offset_between_guards_stay_as_they_were(wl):
    import torch

    p = Pair(wl)
    req = tc.batch(wl, tc.key_mix(wl, 1025, "zipf", 3), 4)
    _, _, rep = p.answer(req)
    want = tc.np_report(wl, req, rep, tc.sizes(wl), 16)
    nb = req.nbytes
    for off_q, off_p in ((0, 0), (1, 7), (7, 1), (1, 0)):
        bufs = []
        for off, a in ((off_q, req), (off_p, rep)):
            raw = np.full(64 + off + nb + 64, 0xA5, np.uint8)
            raw[64 + off:64 + off + nb] = np.frombuffer(a.tobytes(), np.uint8)
            d = torch.from_numpy(raw.copy()).cuda()
            assert d.data_ptr() % 16 == 0
            bufs.append((d, raw, off))
        (dq, rq, _), (dp, rp, _) = bufs
        got = p.eng.traffic_report(dq.data_ptr() + 64 + off_q, len(req), dp.data_ptr() + 64 + off_p, top=16)
        tc.assert_same(got, want, (off_q, off_p))
        assert dq.cpu().numpy().tobytes() == rq.tobytes() and dp.cpu().numpy().tobytes() == rp.tobytes()


def test_refusals_write_nothing():
    import torch

    L = _lib.load()
    p = Pair(W.TATP)
    req = tc.batch(W.TATP, np.arange(50, dtype=np.uint64), 1)
    d_req, d_rep, _ = p.answer(req)
    out = np.full(C.sizeof(_lib.TrafficReport), 0xEE, np.uint8)
    a, b = np.full(4 * 48, 0xEE, np.uint8), np.full(4 * 48, 0xEE, np.uint8)
    po = C.cast(out.ctypes.data, C.POINTER(_lib.TrafficReport))

    def call(h=p.eng._h, q=d_req.data_ptr(), r=d_rep.data_ptr(), n=50, top=4, o=po, la=a.ctypes.data, lb=b.ctypes.data):
        return L.dint_traffic_report(h, q, r, n, top, o, la, lb, None)

    assert call(r=d_req.data_ptr()) == EINVAL and b"in-place" in L.dint_last_error()
    assert call(n=(1 << 24) + 1) == EINVAL
    assert call(top=4097) == EINVAL and call(q=None) == EINVAL and call(la=None) == EINVAL and call(h=None) == EINVAL
    from dint_amd.engine import Engine

    log = Engine(W.LOG, log_entries=4096)
    d53 = torch.zeros(53 * 50, dtype=torch.uint8, device="cuda")
    assert call(h=log._h, q=d53.data_ptr(), r=None) == ESTATE
    assert (out == 0xEE).all() and (a == 0xEE).all() and (b == 0xEE).all()
    assert call() == 0 and not (out == 0xEE).all()
    with pytest.raises(_lib.DintError):
        p.eng.traffic_report(d_req, 50, d_req)


def _state(eng, wl):
    s = {"stats": eng.stats()}
    if wl != W.STORE:  # (store keeps no lock words)
        s["locks"] = [np.concatenate(eng.read_locks(t)).tobytes() for t in range(tc.N_TABLES[wl])]
    if not tc.is_lock(wl):
        s["digest"], s["verify"] = eng.state_digest(), eng.state_verify()
    return s


@wl_param
def test_the_engine_is_untouched_and_a_shard_reports_the_same(wl):
    p = Pair(wl)
    req = tc.batch(wl, tc.key_mix(wl, 1025, "zipf", 5), 6)
    d_req, d_rep, rep = p.answer(req)
    before = _state(p.eng, wl)
    got = p.eng.traffic_report(d_req, len(req), d_rep)
    p.eng.traffic_report(d_req, 257, None, top=0)
    assert _state(p.eng, wl) == before
    shard = make_engine(wl, shard_index=1, shard_count=3)
    tc.assert_same(shard.traffic_report(d_req, len(req), d_rep), got, "shard 1 of 3")


@wl_param
def test_a_report_between_an_announcement_and_its_submit_leaves_it_standing(wl):
    import torch

    p = Pair(wl)
    a, b = (tc.batch(wl, tc.key_mix(wl, 1500, "zipf", s), s + 1) for s in (11, 12))
    da, db = up(a), up(b)
    ra, rb = torch.zeros_like(da), torch.zeros_like(db)
    p.eng.submit_device(da, len(a), ra, ahead=(db, len(b), rb))
    got = p.eng.traffic_report(db, len(b), None)  # (synchronises the stream: A is answered; B is announced, not submitted)
    tc.assert_same(got, tc.np_report(wl, b, None, tc.sizes(wl), 16))
    p.eng.submit_device(db, len(b), rb)  # the announced batch: no DINT_ESTATE
    p.eng.sync()
    assert ra.cpu().numpy().tobytes() == p.o.replay(a).tobytes() and rb.cpu().numpy().tobytes() == p.o.replay(b).tobytes()
    rep_b = np.frombuffer(rb.cpu().numpy().tobytes(), b.dtype)
    tc.assert_same(p.eng.traffic_report(db, len(b), rb), tc.np_report(wl, b, rep_b, tc.sizes(wl), 16), "afterwards")
