"""Log drain and log replay without leaving the GPU (include/dint_abi.h dint_log_drain_device / dint_log_apply_device,
dint_amd/csrc/k_replay.hip, dint_amd/recovery.py apply_log_device / LogShipper) against the host path they sit next to
(dint_log_drain + recovery.apply_log) and against the primary whose log is replayed.  Every comparison is exact."""
import numpy as np
import pytest

import tracegen  # noqa: F401  (tests/ on the path, as the other GPU tests)
from dint_amd import recovery, wire
from oracle import oracle as orc
from test_ebpf_surface import _committed_writes

W, T, S = wire.Workload, wire.Tatp, wire.Sb
EINVAL, ESTATE = -1, -5
pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def _rows(e, t):
    k, v, x = e.dump_rows(t)
    o = np.argsort(k, kind="stable")
    return k[o], v[o], x[o]


def _same_rows(a, b, tables=5):
    for t in range(tables):
        ra, rb = _rows(a, t), _rows(b, t)
        assert len(ra[0]) == len(rb[0]), t
        assert (ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and (ra[2] == rb[2]).all(), t


def _tatp(n_rows=300, cap=4096, **kw):
    from dint_amd.engine import Engine

    e = Engine(W.TATP, n_rows=n_rows, log_entries=cap, **kw)
    e.populate(n_rows)
    return e


@pytest.fixture(scope="module")
def stream300():
    """the set-up of test_log_drain_and_replica_rebuild: 300 subscribers, a ring of 4,096 that wraps several times, 8 x 3,000
    committed writes; the primary drained on the device, its twin on the host"""
    import torch

    cap = 4096
    prim, twin = _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")
    dev, host = [], []
    for b in range(8):
        req = _committed_writes(o, 3000, seed=b)
        want = o.replay(req).tobytes()
        assert prim.submit(req).tobytes() == want and twin.submit(req).tobytes() == want
        n, lost = prim.log_drain_device(buf, cap)
        rec, lost_h = twin.log_drain()
        assert (n, lost) == (3000, 0) and (len(rec), lost_h) == (3000, 0)
        assert buf[:n * 64].cpu().numpy().tobytes() == rec.tobytes()  # the same bytes as the host drain
        dev.append(buf[:n * 64].clone())
        host.append(rec)
    assert prim.log_drain_device(buf, cap) == (0, 0)
    return prim, torch.cat(dev), np.concatenate(host)


def test_tatp_device_drain_and_replay_rebuild_the_primary(stream300):
    prim, d_rec, rec = stream300
    n = len(rec)
    assert n == 24_000 and d_rec.numel() == n * 64
    rep, ref = _tatp(), _tatp()
    st = recovery.apply_log_device(rep, d_rec, n)
    assert st["applied"] == n and st["inserts"] > 0 and st["deletes"] > 0
    assert st == recovery.apply_log(ref, rec)  # the counts of the host path
    _same_rows(prim, rep)
    _same_rows(ref, rep)
    assert rep.stats()["missing_keys"] == 0
    assert d_rec.cpu().numpy().tobytes() == rec.tobytes()  # the records stay untouched


def test_tatp_chains_cross_chunk_edges(stream300):
    prim, d_rec, rec = stream300
    rep = _tatp()
    raw = rep.log_apply_device(d_rec, len(rec), chunk=777)
    assert raw["chunks"] == -(-len(rec) // 777) and raw["applied"] == len(rec)
    _same_rows(prim, rep)
    assert rep.stats()["missing_keys"] == 0
    one, ref = _tatp(), _tatp()
    st = recovery.apply_log_device(one, d_rec, 2000, chunk=1)  # every record a chunk of its own
    assert st == recovery.apply_log(ref, rec[:2000])
    _same_rows(ref, one)
    assert one.stats()["missing_keys"] == 0


def _writes_in_rounds(e, rounds, per_round, seed):
    """committed writes (log record, then the primary operation) on a large table without a per-record Python loop: a round
    touches `per_round` DISTINCT rows, so what a row needs (update / delete if it exists, insert if not) follows from
    its state when the round starts; rows recur from round to round"""
    rng = np.random.default_rng(seed)
    keys, tabs, live = [], [], []
    for t in range(5):
        k = e.dump_rows(t)[0]
        new = k[:5000] + np.uint64(1 << 44)  # + rows that do not exist yet
        new = new[~np.isin(new, k)]
        keys += [k, new]
        tabs.append(np.full(len(k) + len(new), t, np.uint8))
        live += [np.ones(len(k), bool), np.zeros(len(new), bool)]
    keys, tabs, live = np.concatenate(keys), np.concatenate(tabs), np.concatenate(live)
    out = []
    for r in range(rounds):
        pick = rng.choice(len(keys), per_round, replace=False)
        dele = live[pick] & (rng.random(per_round) < 0.25)
        m = np.zeros(2 * per_round, wire.TATP_MSG)
        for j in (0, 1):
            m["table"][j::2], m["key"][j::2] = tabs[pick], keys[pick]
            m["val"][j::2] = rng.integers(0, 256, (per_round, 40), dtype=np.uint8) if j == 0 else m["val"][0::2]
            m["ver"][j::2] = np.arange(per_round) + r * per_round
        m["type"][0::2] = np.where(dele, T.DELETE_LOG, T.COMMIT_LOG)
        m["type"][1::2] = np.where(dele, T.DELETE_PRIM, np.where(live[pick], T.COMMIT_PRIM, T.INSERT_PRIM))
        live[pick] = ~dele
        out.append(m)
    return out


def test_tatp_stream_longer_than_one_pass():
    import torch

    kw = dict(n_rows=100_000, cap=1 << 19, max_pass=65_536)
    prim = _tatp(**kw)
    assert prim.pass_max == 65_536
    for m in _writes_in_rounds(prim, 8, 50_000, seed=3):
        rep = prim.submit(m)
        assert set(np.unique(rep["type"]).tolist()) <= {T.COMMIT_LOG_ACK, T.DELETE_LOG_ACK, T.COMMIT_PRIM_ACK, T.INSERT_PRIM_ACK,
                                                        T.DELETE_PRIM_ACK}
    assert prim.stats()["missing_keys"] == 0
    n = 400_000
    buf = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    assert prim.log_drain_device(buf, n) == (n, 0)
    rec = np.frombuffer(buf.cpu().numpy().tobytes(), wire.LOG_REC)
    assert rec["is_del"].sum() > 10_000
    rep, ref = _tatp(**kw), _tatp(**kw)
    raw = rep.log_apply_device(buf, n)  # default chunk = one pass
    assert raw["chunks"] == -(-n // 65_536) and raw["applied"] == n and raw["inserts"] > 10_000 and raw["deletes"] > 10_000
    st = recovery.apply_log(ref, rec)
    assert (raw["commits"], raw["inserts"], raw["deletes"]) == (st["commits"], st["inserts"], st["deletes"])
    _same_rows(ref, rep)
    _same_rows(prim, rep)
    assert rep.stats()["missing_keys"] == 0


def test_smallbank_replay():
    import torch
    from dint_amd.engine import Engine

    n_acct, n = 10_000, 50_000
    rng = np.random.default_rng(11)
    m = np.zeros(3 * n, wire.SB_MSG)
    key, tab = rng.integers(0, n_acct, n), rng.integers(0, 2, n)
    val = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    for j, ty in enumerate((S.ACQUIRE_EXCLUSIVE, S.COMMIT_LOG, S.COMMIT_PRIM)):  # as the client sends a committed write
        m["type"][j::3], m["table"][j::3], m["key"][j::3], m["val"][j::3], m["ver"][j::3] = ty, tab, key, val, np.arange(n)
    prim = Engine(W.SMALLBANK, n_rows=n_acct, log_entries=1 << 16)
    prim.populate(n_acct)
    o = orc.SmallbankOracle(n_acct, log_entries=1 << 16)
    assert prim.submit(m).tobytes() == o.replay(m).tobytes()  # the primary first
    buf = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    assert prim.log_drain_device(buf, n) == (n, 0)
    rep = Engine(W.SMALLBANK, n_rows=n_acct, log_entries=1 << 16)
    rep.populate(n_acct)
    st = recovery.apply_log_device(rep, buf, n)
    assert st == {"applied": n, "acks": n}
    _same_rows(prim, rep, tables=2)
    for t in range(2):
        assert all((x == y).all() for x, y in zip(rep.dump_rows(t), o.dump(t)))
    ref = Engine(W.SMALLBANK, n_rows=n_acct, log_entries=1 << 16)
    ref.populate(n_acct)
    assert recovery.apply_log(ref, np.frombuffer(buf.cpu().numpy().tobytes(), wire.LOG_REC)) == st
    _same_rows(ref, rep, tables=2)


def test_log_shipper_follows_a_primary():
    cap = 4096  # smaller than two batches of 3,000 records
    prim, twin, rep = _tatp(), _tatp(), _tatp()
    o = orc.TatpOracle(300, log_entries=1 << 20)
    ship = recovery.LogShipper(prim, rep, cap=cap)
    for b in range(20):
        req = _committed_writes(o, 3000, seed=40 + b)
        want = o.replay(req).tobytes()
        assert prim.submit(req).tobytes() == want and twin.submit(req).tobytes() == want
        st = ship.step()
        assert st["lost"] == 0 and st["applied"] == 3000 == st["commits"] + st["inserts"] + st["deletes"]
        assert twin.log_drain()[1] == 0
    assert ship.shipped == 60_000 and ship.lost == 0
    _same_rows(prim, rep)
    assert rep.stats()["missing_keys"] == 0
    assert ship.step() == {"applied": 0, "lost": 0}
    # two batches without a step: the ring laps the reader, and the shipper says what the host drain says
    for b in range(2):
        req = _committed_writes(o, 3000, seed=90 + b)
        o.replay(req)
        prim.submit(req)
        twin.submit(req)
    rec, lost_h = twin.log_drain()
    st = ship.step()
    assert lost_h == 6000 - cap and st["lost"] == lost_h and st["applied"] == len(rec) == cap


def test_refusals():
    import torch
    from dint_amd.engine import Engine

    buf = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def apply(e, ptr=p, n=64):
        return e._L.dint_log_apply_device(e._h, ptr, n, 0, None)

    for e in (Engine(W.FASST, n_slots=1024), Engine(W.TPL, n_slots=1024), Engine(W.LOG, log_entries=1024),
              Engine(W.STORE, n_rows=1000)):
        assert apply(e) == ESTATE, e.workload  # no table a log replays into
        if e.workload != W.LOG:
            assert e._L.dint_log_drain_device(e._h, p, 64, None, None) == ESTATE  # no log
    assert apply(Engine(W.TATP, n_rows=300, log_entries=4096, shard_index=0, shard_count=2)) == EINVAL
    e = _tatp()
    assert apply(e, None, 64) == EINVAL and apply(e, None, 0) == 0
    assert e._L.dint_log_drain_device(e._h, None, 64, None, None) == EINVAL
    # an announced batch is the engine's next submission, not a replay (as dint_snapshot)
    o = orc.TatpOracle(300, log_entries=1 << 20)
    a, b = (_dev(_committed_writes(o, 1000, seed=s)) for s in (1, 2))
    e.submit_device(a, 2000, None, 0, ahead=(b, 2000, None))
    assert apply(e) == ESTATE and b"announced" in e._L.dint_last_error()
    e.submit_device(b, 2000)  # the announced batch after all: the engine goes on
    e.sync()
    assert apply(e) == 0
    e.sync()


def test_replay_leaves_the_replicas_own_log_alone(stream300):
    _, d_rec, rec = stream300
    rep = _tatp()
    warm = _committed_writes(orc.TatpOracle(300, log_entries=1 << 20), 500, seed=7)
    rep.submit(warm)  # something in the replica's ring
    ring0, tail0 = rep.read_log(4096)
    assert tail0 == 500
    recovery.apply_log_device(rep, d_rec, len(rec))
    ring1, tail1 = rep.read_log(4096)
    assert tail1 == tail0 and ring1.tobytes() == ring0.tobytes()  # backup operations do not append
    assert rep.log_drain()[0].tobytes() == ring0[:500].tobytes()
