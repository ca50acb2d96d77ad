"""GPU parity of dint_submit_device on request and reply arrays at ANY byte address (device memory in,
device memory out -- a receive ring in HBM sits where it sits).  The copy stages of k_kv_part (k_kv_dev.h), k_lock_count
(k_locks.hip) and k_log_append (k_log.hip) move 16-byte vectors when both arrays are 16-byte aligned and single bytes
otherwise; a submit of several passes with an odd pass size starts every pass after the first at an odd address, and the
look-ahead partition of the next pass reads through those addresses too.  All six workloads, against the CPU oracle: the
replies, the request bytes (separate reply array), 64 guard bytes on either side of both arrays, the engine's state and its
counters.  Integer work: byte for byte."""
import functools

import numpy as np
import pytest

import tracegen
from dint_amd import wire
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W = wire.Workload

WORKLOADS = ["fasst", "tpl", "log", "store", "tatp", "smallbank"]
GUARD = 64
REQ_FILL, REP_FILL = 0xA5, 0x5A
# (request offset, reply offset) past a 16-byte aligned base: aligned, both unaligned in one phase, each alone, two phases
OFFSETS = [(0, 0), (1, 1), (8, 0), (0, 5), (3, 11)]
N_TILES = 3001            # a few tiles of every copy stage and a ragged last one
ODD_PASS = 777
N_ODD = 5 * ODD_PASS + 100  # six passes of one submit_device
CUTS = [(0, 1301), (1301, 2078), (2078, N_TILES)]  # the announced batches: the 3,001-request trace in three
RING = 4096               # log entries of the tatp / smallbank / log engines (the log engine of the odd-pass case: ODD_PASS)


def _engine(*a, **k):
    from dint_amd.engine import Engine

    return Engine(*a, **k)


def _same_rows(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


# ---------------------------------------------------------------- traces, oracles and engines (small tables, hot keys)
def _oracle(wl, ring=RING):
    if wl == "fasst":
        return orc.FasstOracle(1 << 16)
    if wl == "tpl":
        return orc.TplOracle(1 << 16)
    if wl == "log":
        return orc.LogOracle(ring)
    if wl == "store":
        return orc.StoreOracle(1000 * 18 // 4, 60)
    if wl == "tatp":
        return orc.TatpOracle(2000, log_entries=ring, populate_n=40)
    return orc.SmallbankOracle(10_000, log_entries=ring, populate_n=60)


def _make_engine(wl, max_pass=0, ring=RING):
    if wl == "fasst":
        return _engine(W.FASST, n_slots=1 << 16, max_pass=max_pass)
    if wl == "tpl":
        return _engine(W.TPL, n_slots=1 << 16, max_pass=max_pass)
    if wl == "log":
        return _engine(W.LOG, log_entries=ring, max_pass=max_pass)
    if wl == "store":
        eng = _engine(W.STORE, n_rows=1000, max_pass=max_pass)
        eng.populate(60)
    elif wl == "tatp":
        eng = _engine(W.TATP, n_rows=2000, log_entries=ring, max_pass=max_pass)
        eng.populate(40)
    else:
        eng = _engine(W.SMALLBANK, n_rows=10_000, log_entries=ring, max_pass=max_pass)
        eng.populate(60)
    return eng


def _edge_requests(n, starts):
    """the first and the last request of every 256-request block of every segment [starts[k], starts[k + 1]) of the trace
    (a pass or an announced batch): the tiles of every copy stage are multiples of 256 requests, so these hold the first
    and the last byte of every tile, the ragged last one included"""
    idx, bounds = set(), list(starts) + [n]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        idx.update(range(lo, hi, 256), range(lo + 255, hi, 256), [hi - 1])
    return np.array(sorted(idx))


BAD_TYPE = {"fasst": 200, "log": 5, "store": 99, "tatp": 3, "smallbank": 40}


def _trace(wl, n, o, starts):
    """n requests on a few hot keys with some bad types among them (echoed and counted).  The requests at the tile edges
    are bad ones whose first and last byte differ from what the reply array holds beforehand: a reply to them is right only
    if the copy stage moved every byte of its tile"""
    if wl == "fasst":
        req = tracegen.fasst_random(n, seed=n, n_hot=8, p_hot=0.6)
        req["type"][::7] = 200
    elif wl == "tpl":
        req = tracegen.tpl_random(n, seed=n, n_hot=8, p_hot=0.6)
        req["type"][5::11] = 9      # unknown lock types: acquire -> bad request, release -> ack only
    elif wl == "log":
        req = tracegen.log_random(n, seed=n)
        req["type"][3::17] = 5
    elif wl == "store":
        req = tracegen.store_random(n, seed=n, n_sub_touch=30, p_set=0.5, p_insert=0.05)
        req["type"][::13] = 99
    elif wl == "tatp":
        req = tracegen.tatp_random(n, [o.dump(t)[0] for t in range(5)], seed=n, n_sub_touch=40)
        req["type"][7::41] = 3      # kCommit is never handled by the reference servers
        req["table"][11::53] = 9    # out-of-range table
    else:
        req = tracegen.sb_random(n, seed=n, n_acct_touch=30)
        req["type"][9::31] = 17     # WARMUP_READ (eBPF flavour): a plain read, acked
        req["type"][4::43] = 40     # no such request type: echoed and counted
        req["table"][13::59] = 7    # out-of-range table
        req["key"][5::97] = 10**9   # a missing account: the reference panics; counted
    e = _edge_requests(n, starts)
    if wl == "tpl":  # {action, lid, type}: an ACQUIRE of an unknown lock type
        req["action"][e], req["type"][e] = 0, 9
    else:
        req["type"][e], req["ver"][e] = BAD_TYPE[wl], 0xC3C3C3C3
        if "ord" in req.dtype.names:
            req["ord"][e] = 0xC3
    return req


@functools.lru_cache(maxsize=None)
def _case(wl, n, ring=RING):
    """(requests, the oracle's replies, the oracle after them): computed once per shape, read-only afterwards"""
    o = _oracle(wl, ring)
    starts = [lo for lo, _ in CUTS] if n == N_TILES else range(0, n, ODD_PASS)
    req = _trace(wl, n, o, starts)
    want = o.replay(req)
    e = _edge_requests(n, starts)
    assert want[e].tobytes() == req[e].tobytes()  # echoed
    edge_bytes = np.frombuffer(req.tobytes(), np.uint8).reshape(n, -1)[e][:, [0, -1]]
    assert (edge_bytes != REP_FILL).all()
    assert o.errors > 0
    req.setflags(write=False)
    want.setflags(write=False)
    assert req.tobytes() != want.tobytes()
    return req, want, o


def _check_state(wl, eng, o, ring=RING):
    """rows of every table, lock words, the smallbank counters, log ring and tail; then the counters"""
    if wl == "fasst":
        a, b = eng.read_locks()
        assert (a == o.locks).all() and (b == o.vers).all()
    elif wl == "tpl":
        a, b = eng.read_locks()
        assert (a == o.num_ex).all() and (b == o.num_sh).all()
    elif wl == "store":
        assert _same_rows(eng.dump_rows(0), o.dump())
    elif wl == "tatp":
        for t in range(5):
            assert _same_rows(eng.dump_rows(t), o.dump(t)), t
            lk, _ = eng.read_locks(t)
            assert (lk == o.locks(t)).all(), t
    elif wl == "smallbank":
        for t in range(2):
            ex, sh = eng.read_locks(t)
            assert (ex == o.num_ex(t)).all() and (sh == o.num_sh(t)).all(), t
            assert _same_rows(eng.dump_rows(t), o.dump(t)), t
    if wl in ("log", "tatp", "smallbank"):
        rec, tail = eng.read_log(ring)
        assert tail == o.tail
        assert (np.frombuffer(rec.tobytes(), "u1").reshape(ring, 64) == o.ring).all()
    st = eng.stats()
    assert st["pool_exhausted"] == 0
    if wl in ("tatp", "smallbank"):  # the oracle counts both kinds in one number
        assert st["bad_requests"] > 0 and st["bad_requests"] + st["missing_keys"] == o.errors
    else:
        assert st["bad_requests"] == o.errors and st["missing_keys"] == 0


# ---------------------------------------------------------------- arrays between guard bytes, at a chosen byte offset
class _Placed:
    """`nbytes` of device memory `off` bytes past a 16-byte aligned address, GUARD + off known bytes before it and GUARD
    after it"""

    def __init__(self, nbytes, off, fill, data=None):
        import torch

        self.lo, self.n, self.fill = GUARD + off, nbytes, fill
        host = np.full(self.lo + nbytes + GUARD, fill, np.uint8)
        if data is not None:
            host[self.lo:self.lo + nbytes] = np.frombuffer(data.tobytes(), np.uint8)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.lo
        assert self.ptr % 16 == off % 16

    def read(self):
        """the array's bytes; asserts that every guard byte is what it was"""
        h = self.t.cpu().numpy()
        assert (h[:self.lo] == self.fill).all(), "bytes before the array changed"
        assert (h[self.lo + self.n:] == self.fill).all(), "bytes after the array changed"
        return h[self.lo:self.lo + self.n].tobytes()


def _place(req, a, b):
    """the request array at offset a; the reply array at offset b, or None = in place"""
    q = _Placed(req.nbytes, a, REQ_FILL, req)
    return q, (q if b is None else _Placed(req.nbytes, b, REP_FILL))


def _verify(bufs, reqs, wants):
    for k, ((q, r), req, want) in enumerate(zip(bufs, reqs, wants)):
        assert r.read() == want.tobytes(), k
        if r is not q:
            assert q.read() == req.tobytes(), k  # the requests are untouched


PLACEMENTS = [pytest.param(a, b, id=f"req+{a}-rep+{b}") for a, b in OFFSETS] + \
             [pytest.param(a, None, id=f"inplace+{a}") for a in (0, 7)]


@pytest.mark.parametrize("a,b", PLACEMENTS)
@pytest.mark.parametrize("wl", WORKLOADS)
def test_one_pass_of_several_tiles_at_any_address(wl, a, b):
    """3,001 requests: a few tiles of every copy stage (256 .. 1024 requests each) and a ragged last one"""
    req, want, o = _case(wl, N_TILES)
    eng = _make_engine(wl)
    q, r = _place(req, a, b)
    eng.submit_device(q.ptr, N_TILES, r.ptr)
    eng.sync()
    _verify([(q, r)], [req], [want])
    _check_state(wl, eng, o)
    assert eng.stats()["batches"] == 1


@pytest.mark.parametrize("a,b", [(0, 0), (3, 11)], ids=["aligned-base", "req+3-rep+11"])
@pytest.mark.parametrize("wl", WORKLOADS)
def test_odd_pass_size_every_later_pass_at_an_odd_address(wl, a, b):
    """ONE submit_device of 5 x 777 + 100 requests with passes of 777: pass k starts k x 777 x msg_size bytes into the
    arrays (msg_size is odd or 6: never a multiple of 16 for k = 1 .. 5), and the kv and lock engines look ahead from every
    pass to the next through those addresses.  The log engine gets a ring of 777 entries, which makes its pass 777 and
    wraps the ring five times."""
    ring = ODD_PASS if wl == "log" else RING
    req, want, o = _case(wl, N_ODD, ring)
    eng = _make_engine(wl, 0 if wl == "log" else ODD_PASS, ring)
    assert eng.pass_max == ODD_PASS
    assert all((k * ODD_PASS * eng.msg_size) % 16 for k in range(1, 6))
    q, r = _place(req, a, b)
    eng.submit_device(q.ptr, N_ODD, r.ptr)
    eng.sync()
    _verify([(q, r)], [req], [want])
    _check_state(wl, eng, o, ring)
    assert eng.stats()["batches"] == 6


@pytest.mark.parametrize("inplace", [False, True], ids=["separate", "inplace"])
@pytest.mark.parametrize("wl", ["store", "tatp", "fasst", "tpl"])
def test_announced_next_batch_at_unaligned_addresses(wl, inplace):
    """three batches, each announced by the call before it (dint_submit_device_ahead): its partition / count stage runs
    beside the current batch and reads the announced arrays where they are -- all of them off the 16-byte grid"""
    req, want, o = _case(wl, N_TILES)
    cuts = CUTS
    offs = [(7, None), (7, None), (9, None)] if inplace else [(1, 1), (3, 11), (8, 5)]
    bufs = [_place(req[lo:hi], a, b) for (lo, hi), (a, b) in zip(cuts, offs)]
    eng = _make_engine(wl)
    for k, ((q, r), (lo, hi)) in enumerate(zip(bufs, cuts)):
        nxt = None
        if k + 1 < len(cuts):
            nq, nr = bufs[k + 1]
            nxt = (nq.ptr, cuts[k + 1][1] - cuts[k + 1][0], nr.ptr)
        eng.submit_device(q.ptr, hi - lo, r.ptr, 0, ahead=nxt)
    eng.sync()
    _verify(bufs, [req[lo:hi] for lo, hi in cuts], [want[lo:hi] for lo, hi in cuts])
    _check_state(wl, eng, o)
    assert eng.stats()["batches"] == 3
