"""GPU: a broken announcement on an engine that keeps a log (tatp, smallbank).  dint_submit_device_ahead runs the partition stage
of the announced batch B -- and with it B's log appends -- in the launch of the batch before it.  When the caller then submits
something else (DINT_ESTATE), or restores / resets, the engine must be as if it had never seen B (include/dint_abi.h): tables, lock
words, the ring's tail and appended count, dint_stats, the drain cursor.  The one thing that stays are B's records in the ring
slots from the tail on, which shows through a later tatp DELETE_LOG: it keeps the val bytes of the slot it lands on.

The model: the main oracle replays the batches the engine answered.  At a cancel a twin oracle (the same batches, the same ring)
replays B, and the ring slots [tail, tail + m) mod cap it wrote -- m = B's log requests -- are copied into the main oracle's
ring.  Everything is byte-exact against that: replies, rows, lock words, the whole ring, the tail, what log_drain hands out
(the oracle's ring records collected batch by batch), bad_requests + missing_keys == the oracle's error count.

Each test first asserts from the oracles alone that its batches can show the fault it is about (enough DELETE_LOG records of
later batches on slots B wrote, with other val bytes than without B; B's records across the end of the ring; ...).  The
arithmetic alone is walked on the host in tests/test_log_ring_host.py.

What each test is there to catch (engine.hip ahead_cancel, read against the code before these fixes):
  another_batch.. / across_the_end.. (and the set in test_gpu_kv_multi.py): B's bad table ids stay in dint_stats.bad_requests --
      the stats line fails; the ring / tail lines hold the "slots from the tail on" clause and the rewind at both parities.
  exactly_as_many_log_requests..[256]: the appended count loses (tail' - tail) mod cap == 0 instead of 256 -- the last log_drain
      hands out 256 records nobody was answered for (the length line fails).  [0] is the control.
  overwrote_before_they_were_drained: the drain hands out B's bytes as if they were A's oldest records -- (len, lost) == (6, 34) fails.
  a_drain_between..: the cursor stays ahead of the rolled-back count -- C's records are lost ("fewer": the drain after C is
      empty) or their first ones skipped ("more"); the len(rec) == mc line fails.
  restore / reset: pass before and after; they pin that the silent cancel leaves nothing behind either."""
import numpy as np
import pytest

import tracegen
from dint_amd import _lib, wire
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
W, T, S = wire.Workload, wire.Tatp, wire.Sb
N_ROWS, POP = 2000, 40


def _engine(*a, **k):
    from dint_amd.engine import Engine

    return Engine(*a, **k)


def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def _same_rows(a, b):
    return all(x.shape == y.shape and (x == y).all() for x, y in zip(a, b))


def _log_mask(wl, req):
    """the requests the partition stage appends a log record for"""
    if wl == W.TATP:
        return np.isin(req["type"], (T.COMMIT_LOG, T.DELETE_LOG)) & (req["table"] < 5)
    return (req["type"] == S.COMMIT_LOG) & (req["table"] < 2)


def _logs(wl, k, seed, p_del=0.0):
    """k log requests and nothing else: COMMIT_LOG (tatp: DELETE_LOG with probability p_del) with random keys, vals, versions"""
    rng = np.random.default_rng(seed)
    m = np.zeros(k, wire.TATP_MSG if wl == W.TATP else wire.SB_MSG)
    m["type"] = T.COMMIT_LOG if wl == W.TATP else S.COMMIT_LOG
    if wl == W.TATP and p_del:
        m["type"][rng.random(k) < p_del] = T.DELETE_LOG
    m["table"] = rng.integers(0, 5 if wl == W.TATP else 2, k)
    m["key"] = rng.integers(0, 1 << 40, k)
    m["val"] = rng.integers(1, 256, m["val"].shape, dtype=np.uint8)
    m["ver"] = rng.integers(0, 2**32, k, dtype=np.uint64).astype("<u4")
    return m


def _reads(wl, k):
    """k reads of rows that exist: a pass with no log record that changes nothing"""
    m = np.zeros(k, wire.TATP_MSG if wl == W.TATP else wire.SB_MSG)
    m["type"] = T.READ if wl == W.TATP else 17  # (smallbank: WARMUP_READ, a plain get)
    m["key"] = np.arange(k) % POP
    return m


def _spoil(req, at, only=None):
    """a bad table id on the requests `at` (tatp answered batches: READs only, so that the trace stays well-formed)"""
    for i in at:
        while only is not None and req["type"][i] != only:
            i += 1
        req["table"][i] = 9
    return req


class _Model:
    """the main oracle, a `plain` one that never sees a cancelled batch's ring bytes, and what the drain must hand out"""

    def __init__(self, wl, cap, populate=POP, n_rows=N_ROWS):
        self.wl, self.cap, self.populate, self.n_rows = wl, cap, populate, n_rows
        self.o, self.plain = self._new(), self._new()
        self.answered, self.history, self.pasted, self.shown = [], [], np.zeros(cap, bool), 0

    def _new(self):
        cls = orc.TatpOracle if self.wl == W.TATP else orc.SmallbankOracle
        return cls(self.n_rows, log_entries=self.cap, populate_n=self.populate)

    def existing(self):
        return [self.o.dump(t)[0] for t in range(5)]

    def answer(self, req):
        """a batch the engine answers: the replies it must give"""
        t0, mask = self.o.tail, _log_mask(self.wl, req)
        slots = (t0 + np.arange(int(mask.sum()))) % self.cap
        want = self.o.replay(req)
        self.plain.replay(req)
        assert self.plain.tail == self.o.tail
        self.answered.append(req)
        self.history.append(self.o.ring[slots].copy())
        if self.wl == W.TATP:  # DELETE_LOG records on slots a cancelled batch wrote, whose val bytes only the paste explains
            dl = slots[req["type"][mask] == T.DELETE_LOG]
            dl = dl[self.pasted[dl]]
            self.shown += int((self.o.ring[dl, 8:48] != self.plain.ring[dl, 8:48]).any(axis=1).sum())
        self.pasted[slots] = False
        return want

    def cancel(self, req):
        """a batch whose partition ran and that is never answered: its records stay in the ring slots from the tail on.  Returns them."""
        tw = self._new()
        for a in self.answered:
            tw.replay(a)
        assert tw.tail == self.o.tail
        tw.ring[:] = self.o.ring  # (what earlier cancelled batches left)
        tw.replay(req)
        m = int(_log_mask(self.wl, req).sum())
        assert (tw.tail - self.o.tail) % self.cap == m % self.cap
        slots = (self.o.tail + np.arange(m)) % self.cap
        self.o.ring[slots] = tw.ring[slots]
        self.pasted[slots] = True
        return tw.ring[slots].copy()

    def drained(self, since=0):
        h = self.history[since:]
        return np.concatenate(h) if h else np.zeros((0, 64), np.uint8)

    def check(self, eng, stats=True):
        o = self.o
        if self.wl == W.TATP:
            for t in range(5):
                assert _same_rows(eng.dump_rows(t), o.dump(t)), ("rows", t)
                assert (eng.read_locks(t)[0] == o.locks(t)).all(), ("locks", t)
        else:
            for t in range(2):
                assert _same_rows(eng.dump_rows(t), o.dump(t)), ("rows", t)
                ex, sh = eng.read_locks(t)
                assert (ex == o.num_ex(t)).all() and (sh == o.num_sh(t)).all(), ("locks", t)
        ring, tail = eng.read_log(self.cap)
        assert tail == o.tail
        got = np.frombuffer(ring.tobytes(), "u1").reshape(-1, 64)
        assert (got == o.ring).all(), ("ring slots differ", np.nonzero((got != o.ring).any(axis=1))[0][:8].tolist())
        if stats:
            st = eng.stats()
            assert st["bad_requests"] + st["missing_keys"] == o.errors, (st["bad_requests"], st["missing_keys"], o.errors)
            assert st["pool_exhausted"] == 0 and st["foreign_requests"] == 0


def _trace(m, n, seed):
    if m.wl == W.TATP:
        return tracegen.tatp_random(n, m.existing(), seed=seed, n_sub_touch=POP)
    return tracegen.sb_random(n, seed=seed, n_acct_touch=30)


def _rec_bytes(rec):
    return np.frombuffer(rec.tobytes(), "u1").reshape(-1, 64)


class _Dev:
    """a batch in device memory: in place, or with a reply buffer of its own"""

    def __init__(self, req, inplace):
        import torch

        self.req, self.n, self.d = req, len(req), _up(req)
        self.r = None if inplace else torch.zeros_like(self.d)

    def ahead(self):
        return (self.d, self.n, self.r)

    def got(self):
        return (self.d if self.r is None else self.r).cpu().numpy().tobytes()

    def untouched(self):
        return self.d.cpu().numpy().tobytes() == self.req.tobytes()


def _submit(eng, b, nxt=None):
    eng.submit_device(b.d, b.n, b.r, 0, ahead=None if nxt is None else nxt.ahead())


def _refused(eng, b):
    with pytest.raises(_lib.DintError, match="announced"):
        _submit(eng, b)


def _pair(wl, cap, populate=POP):
    eng = _engine(wl, n_rows=N_ROWS, log_entries=cap)
    if populate:
        eng.populate(populate)
    return eng, _Model(wl, cap, populate)


# ---- 1 / 5. another batch than the announced one, then more batches ------------------------------------------------------------
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
@pytest.mark.parametrize("wl", [W.TATP, W.SMALLBANK], ids=["tatp", "smallbank"])
def test_another_batch_than_the_announced_one_then_an_announced_chain(wl, inplace):
    """A announces B; C is handed over instead: DINT_ESTATE.  C again, D announcing E, E.  B and C hold requests with a bad table
    id: B's must not stay counted, C's must be counted once.  tatp: C's and D's DELETE_LOG records land on the slots B wrote"""
    cap, n = 4096, 1500
    eng, m = _pair(wl, cap)
    assert eng.pass_max >= n
    tr = _trace(m, 4 * n, seed=11)
    a, c, d, e = (tr[k * n:(k + 1) * n].copy() for k in range(4))
    b = _spoil((tracegen.tatp_random(n, m.existing(), seed=12, n_sub_touch=POP) if wl == W.TATP else tracegen.sb_random(n, seed=12, n_acct_touch=30)),
               [3, 700, 1499])
    _spoil(c, [0, 64, 1000, 1400], only=T.READ if wl == W.TATP else None)
    want = [m.answer(a)]
    m.cancel(b)
    want += [m.answer(x) for x in (c, d, e)]
    assert m.o.errors >= 4 and int(_log_mask(wl, b).sum()) >= 100
    if wl == W.TATP:
        assert m.shown >= 8, m.shown
    A, B, C, D, E = (_Dev(x, inplace) for x in (a, b, c, d, e))
    _submit(eng, A, B)
    _refused(eng, C)
    eng.sync()
    assert C.untouched() and (inplace or not C.r.any().item())  # the refused call answered nothing
    _submit(eng, C)
    _submit(eng, D, E)
    _submit(eng, E)
    eng.sync()
    for k, x in enumerate((A, C, D, E)):
        assert x.got() == want[k].tobytes(), k
        assert inplace or x.untouched()
    m.check(eng)
    rec, lost = eng.log_drain(cap)
    assert lost == 0 and (_rec_bytes(rec) == m.drained()).all() and len(rec) == len(m.drained())


# ---- 2. the ring wrapped, B across its end, both parities of the pass number --------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd"])
def test_a_cancelled_batch_across_the_end_of_a_ring_that_has_wrapped(odd):
    """log_entries = 256 (a pass is 256 requests at most).  The tail has gone round twice; B's records begin 10 slots before the
    end of the ring.  The tail words alternate with the pass number: B is cancelled after an even and after an odd number of
    passes"""
    wl, cap, n = W.TATP, 256, 200
    eng, m = _pair(wl, cap)
    assert eng.pass_max == cap
    tr = _trace(m, 6 * n, seed=21)
    cuts = [tr[k * n:(k + 1) * n].copy() for k in range(6)]
    a = cuts[3]
    pre = []
    for k in range(3):
        pre += [cuts[k], _logs(wl, 200, seed=30 + k, p_del=0.3)]
    want = [m.answer(x) for x in pre]
    assert sum(len(h) for h in m.history) >= 2 * cap
    fill = _logs(wl, (cap - 10 - int(_log_mask(wl, a).sum()) - m.o.tail) % cap or cap, seed=40)  # A will leave the tail at cap - 10
    pre += [fill] + [_reads(wl, 16)] * odd
    want += [m.answer(x) for x in pre[len(want):]]
    b = _spoil(tracegen.tatp_random(n, m.existing(), seed=22, n_sub_touch=POP), [5, 150])
    c, d = _spoil(cuts[4], [1, 90], only=T.READ), cuts[5]
    want.append(m.answer(a))
    mb = int(_log_mask(wl, b).sum())
    assert m.o.tail == cap - 10 and mb > 10  # B's records straddle the end of the ring
    m.cancel(b)
    want += [m.answer(c), m.answer(d)]
    assert m.shown >= 8, m.shown
    devs = [_Dev(x, True) for x in pre + [a]]
    B, C, D = _Dev(b, True), _Dev(c, True), _Dev(d, True)
    for x in devs[:-1]:
        _submit(eng, x)
    assert eng.stats()["batches"] == 7 + odd  # passes before the one that announces B
    _submit(eng, devs[-1], B)
    _refused(eng, C)
    _, tail = eng.read_log(cap)
    assert tail == cap - 10
    _submit(eng, C, D)
    _submit(eng, D)
    eng.sync()
    for k, x in enumerate(devs + [C, D]):
        assert x.got() == want[k].tobytes(), k
    m.check(eng)


# ---- 3. a cancelled batch of exactly `cap` log requests, and one of none ---------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even", "odd"])
@pytest.mark.parametrize("mb", [256, 0])
def test_a_cancelled_batch_of_exactly_as_many_log_requests_as_the_ring_holds(mb, odd):
    """256 COMMIT_LOG into a ring of 256: the tail comes back to where it was, so the two tail words are equal and only the batch's
    own count says what the appended count must lose.  Afterwards the tail is unchanged and log_drain hands out the answered
    batches' records, in order, and nothing else"""
    wl, cap, n = W.TATP, 256, 200
    eng, m = _pair(wl, cap)
    tr = _trace(m, 3 * n, seed=31)
    a0, c, d = (tr[k * n:(k + 1) * n].copy() for k in range(3))
    pre = [a0] + [_reads(wl, 16)] * odd
    a = _reads(wl, 32)  # (no record of its own: nothing is waiting to be drained where B's 256 records land)
    b = _logs(wl, mb, seed=32) if mb else _reads(wl, 100)
    want = [m.answer(x) for x in pre + [a]]
    t0, n0 = m.o.tail, len(m.history)
    m.cancel(b)
    assert int(_log_mask(wl, b).sum()) == mb and m.pasted.sum() == mb
    want += [m.answer(c), m.answer(d)]
    assert len(m.drained(n0)) > 20
    devs = [_Dev(x, True) for x in pre + [a]]
    B, C, D = _Dev(b, True), _Dev(c, True), _Dev(d, True)
    for x in devs[:-1]:
        _submit(eng, x)
    rec, lost = eng.log_drain(cap)
    assert lost == 0 and (_rec_bytes(rec) == m.drained()[:len(rec)]).all() and len(rec) == len(m.drained(0)) - len(m.drained(n0))
    _submit(eng, devs[-1], B)
    _refused(eng, C)
    ring, tail = eng.read_log(cap)
    assert tail == t0
    _submit(eng, C)
    _submit(eng, D)
    eng.sync()
    for k, x in enumerate(devs + [C, D]):
        assert x.got() == want[k].tobytes(), k
    m.check(eng)
    rec, lost = eng.log_drain(4 * cap)
    assert lost == 0 and len(rec) == len(m.drained(n0)), (lost, len(rec), len(m.drained(n0)))
    assert (_rec_bytes(rec) == m.drained(n0)).all()
    rec, lost = eng.log_drain(4 * cap)
    assert (len(rec), lost) == (0, 0)


def test_records_a_cancelled_batch_overwrote_before_they_were_drained_are_reported_lost():
    """the other side of "its records stay in the ring": 40 records wait to be drained when a batch of 250 is announced into a ring
    of 256 and cancelled.  It overwrote the oldest 34 of them: the next drain says lost == 34 and hands out the other 6, then
    the stream goes on with what is appended next"""
    wl, cap = W.TATP, 256
    eng, m = _pair(wl, cap)
    a, b, c = _logs(wl, 40, seed=51), _logs(wl, 250, seed=52), _logs(wl, 30, seed=53, p_del=0.5)
    want = [m.answer(a)]
    m.cancel(b)
    want.append(m.answer(c))
    A, B, C = (_Dev(x, True) for x in (a, b, c))
    _submit(eng, A, B)
    _refused(eng, C)
    rec, lost = eng.log_drain(4 * cap)
    assert (len(rec), lost) == (6, 34)
    assert (_rec_bytes(rec) == m.history[0][34:]).all()
    _submit(eng, C)
    eng.sync()
    assert A.got() == want[0].tobytes() and C.got() == want[1].tobytes()
    m.check(eng)
    rec, lost = eng.log_drain(4 * cap)
    assert lost == 0 and len(rec) == 30 and (_rec_bytes(rec) == m.history[1]).all()


# ---- 4 / 5. a drain between the announcement and the cancel ---------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nc", [300, 3000], ids=["fewer", "more"])
@pytest.mark.parametrize("wl", [W.TATP, W.SMALLBANK], ids=["tatp", "smallbank"])
def test_a_drain_between_announcement_and_cancel(wl, nc, device):
    """drained to the end; B announced: the drain hands out exactly B's m records (they are the caller's to discard once B is
    cancelled).  Then C instead of B, with fewer / more log requests than B: the next drain hands out exactly C's, lost == 0"""
    import torch

    cap, n = 4096, 1000
    eng, m = _pair(wl, cap)
    d_buf = torch.zeros(cap * 64, dtype=torch.uint8, device="cuda")

    def drain():
        if not device:
            rec, lost = eng.log_drain(cap)
            return _rec_bytes(rec), lost
        k, lost = eng.log_drain_device(d_buf, cap)
        return d_buf[:k * 64].cpu().numpy().reshape(-1, 64), lost

    tr = _trace(m, n + nc + 500, seed=61)
    a0, c, d = tr[:n].copy(), tr[n:n + nc].copy(), tr[n + nc:].copy()
    a = _reads(wl, 64)
    b = _trace(m, n, seed=62)
    want = [m.answer(a0), m.answer(a)]
    b_rec = m.cancel(b)
    mb = len(b_rec)
    want += [m.answer(c), m.answer(d)]
    mc = len(m.history[2])
    assert mb >= 60 and (mc < mb // 2 if nc < n else mc > 2 * mb) and mc > 0, (mb, mc)
    A0, A, B, C, D = (_Dev(x, True) for x in (a0, a, b, c, d))
    _submit(eng, A0)
    rec, lost = drain()
    assert lost == 0 and len(rec) == len(m.history[0]) and (rec == m.history[0]).all()
    _submit(eng, A, B)
    rec, lost = drain()  # in the window: the announced batch's records
    assert lost == 0 and len(rec) == mb and (rec == b_rec).all()
    _refused(eng, C)
    rec, lost = drain()
    assert (len(rec), lost) == (0, 0)
    _submit(eng, C)
    rec, lost = drain()
    assert lost == 0 and len(rec) == mc, (len(rec), mc, lost)
    assert (rec == m.history[2]).all()
    _submit(eng, D)
    eng.sync()
    for k, x in enumerate((A0, A, C, D)):
        assert x.got() == want[k].tobytes(), k
    m.check(eng)
    rec, lost = drain()
    assert lost == 0 and len(rec) == len(m.history[3]) and (rec == m.history[3]).all()


# ---- 6. restore / reset with an announcement pending --------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [False, True], ids=["", "drained-in-the-window"])
def test_restore_with_an_announcement_pending(window):
    """the snapshot is taken with 1 of A's batches drained and one not; A2 announces B (log records, bad requests), optionally a
    drain takes B's records; restore() drops the announcement silently and the engine goes on exactly as an oracle that replayed up
    to the snapshot: ring (B's records are not in it: the snapshot's ring is back), tail, drain cursor"""
    wl, cap, n = W.TATP, 4096, 1000
    eng, m = _pair(wl, cap)
    tr = _trace(m, 4 * n, seed=71)
    a0, a1, a2, c = (tr[k * n:(k + 1) * n].copy() for k in range(4))
    b = _spoil(tracegen.tatp_random(n, m.existing(), seed=72, n_sub_touch=POP), [7, 8, 900])
    want = [m.answer(a0), m.answer(a1)]
    A0, A1, A2, B = (_Dev(x, True) for x in (a0, a1, a2, b))
    _submit(eng, A0)
    rec, lost = eng.log_drain(cap)
    assert lost == 0 and len(rec) == len(m.history[0])
    _submit(eng, A1)
    eng.sync()
    eng.snapshot()
    _submit(eng, A2, B)
    if window:
        rec, lost = eng.log_drain(cap)
        assert len(rec) > len(m.history[1]) + 200
    eng.restore()
    want.append(m.answer(c))  # (a2 was answered and is undone with the rest: the oracle never sees it)
    C = _Dev(c, True)
    _submit(eng, C)
    eng.sync()
    assert A0.got() == want[0].tobytes() and A1.got() == want[1].tobytes() and C.got() == want[2].tobytes()
    m.check(eng, stats=False)
    rec, lost = eng.log_drain(cap)
    assert lost == 0 and len(rec) == len(m.drained(1)) and (_rec_bytes(rec) == m.drained(1)).all()


def test_reset_with_an_announcement_pending():
    """reset() drops the announcement silently: the engine goes on as a fresh one (empty tables, ring, tail and cursor at 0)"""
    wl, cap, n = W.TATP, 4096, 1000
    eng, m = _pair(wl, cap)
    tr = _trace(m, n, seed=81)
    b = _spoil(tracegen.tatp_random(n, m.existing(), seed=82, n_sub_touch=POP), [7, 8, 900])
    A, B = _Dev(tr, True), _Dev(b, True)
    _submit(eng, A, B)
    rec, lost = eng.log_drain(100)  # (the cursor stands inside A's records)
    assert len(rec) == 100
    eng.reset()
    f = _Model(wl, cap, populate=0)
    # (the keys of the rows the population had held: none of them exists now)
    c = tracegen.tatp_random(2 * n, [np.zeros(0, np.uint64)] * 5, seed=83, pools=[sorted(int(k) for k in ks) for ks in m.existing()])
    c0, c1 = c[:n].copy(), c[n:].copy()
    want = [f.answer(c0), f.answer(c1)]
    C0, C1 = _Dev(c0, True), _Dev(c1, True)
    _submit(eng, C0, C1)
    _submit(eng, C1)
    eng.sync()
    assert C0.got() == want[0].tobytes() and C1.got() == want[1].tobytes()
    f.check(eng, stats=False)
    rec, lost = eng.log_drain(cap)
    assert lost == 0 and len(rec) == len(f.drained()) and (_rec_bytes(rec) == f.drained()).all()
