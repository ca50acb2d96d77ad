"""GPU parity of LAUNCH SETS of several kv engines (dint_submit_segments_multi / _ahead) with the oracle.  What a set has of its
own and a single-engine pass has not: k_kv_pass's block ranges (resolve blocks mapped to an engine by walking the engines'
cut.P, worker b -> engine b / n_work, next-pass tile b -> engine b / max_tiles, DINT_KV_PART_FIRST swapping the last two),
the engine axis of k_kv_part / k_kv_hot / k_kv_late / k_kv_big, dint_launch_kv_multi's parameter choices (rpt from the sum of
the sizes, next_rpt from the largest announced one, knobs / hot / sb_workers from engine 0) and engine.hip's announcement
protocol (all of the engines' partitions ran ahead or none; else every engine is cancelled and the call is DINT_ESTATE).

The engines run tests/kv_collide.py's cases -- hot keys in pieces beside colliding neighbours -- staggered (tests/kv_multi.py):
idle engines beside full ones, 14,000 requests beside 6,000 beside 500.  Everything is exact: reply bytes, padding, rows, lock
words, log ring and tail, error counts, all the oracle's.  Every run has the engines' kernel timers on: a per-engine pass
(dint_submit_segments, the fallback) records timer events, a launch set records none, so timing_read() tells whether a test
meant for the one-set path took it (`alone` below = passes an engine ran on its own)."""
import numpy as np
import pytest

import kv_multi as km
from dint_amd import _lib, wire
from test_gpu_kv import SB_KNOBS, SPLIT_KNOBS, _same_rows

pytestmark = pytest.mark.gpu
W = wire.Workload
NOFUSE = SPLIT_KNOBS[5]
PART_FIRST = {"DINT_KV_PART_FIRST": "1"}


class _Set:
    """the engines of a set, its device buffers [step][engine] (uploaded before the first call) and one caller stream"""

    def __init__(self, name, knobs, monkeypatch, seg_cap=0, engine_kw=None):
        import torch
        from dint_amd.engine import Engine

        for k, v in knobs.items():
            monkeypatch.setenv(k, v)
        self.name, self.knobs = name, knobs
        self.s, self.host = km.cached(name, seg_cap)
        self.engs = []
        for k, c in enumerate(self.s.cases):
            e = Engine(c.wl, **{**c.engine, **(engine_kw or {}).get(k, (engine_kw or {}).get("all", {}))})
            e.populate(c.populate)
            e.timing_enable(True)
            self.engs.append(e)
        self.dev = [self.upload(j) for j in range(len(self.host))]
        torch.cuda.synchronize()
        self.st = torch.cuda.Stream()
        self.n_steps = len(self.host)

    def upload(self, j, host=None):
        import torch

        return [torch.from_numpy(a.copy()).cuda() for a, _ in (host or self.host)[j]]

    def submit(self, j, ahead=None, row=None):
        """step j as one call; ahead = the device buffers of the step it announces"""
        from dint_amd.engine import submit_segments_multi

        row = self.dev[j] if row is None else row
        n, s = len(self.engs), self.s
        nxt = None if ahead is None else ([d.data_ptr() + 64 for d in ahead], [d.data_ptr() for d in ahead])
        submit_segments_multi(self.engs, [d.data_ptr() + 64 for d in row], km.N_SEG, [s.seg_cap] * n, s.stride, [d.data_ptr() for d in row],
                              s.stride, self.st.cuda_stream, ahead=nxt)

    def run(self, first, last, announce):
        for j in range(first, last):
            self.submit(j, self.dev[j + 1] if announce and j + 1 < self.n_steps else None)

    def alone(self):
        """per engine: kernel passes it ran on its own (the fallback) -- a launch set records none"""
        return [max([v["launches"] for v in e.timing_read().values()] or [0]) for e in self.engs]

    def quiet(self):
        """no engine has an announcement pending: a state call is not refused"""
        for e in self.engs:
            e.state_digest()

    def check_replies(self, dev=None, host=None, s=None, what=""):
        """every step's buffers against the oracle's (dev[j] == []: a step that is not compared here)"""
        s = s or self.s
        msg = s.dtype.itemsize
        for j, row in enumerate(self.dev if dev is None else dev):
            for k, d in enumerate(row):
                got, want = d.cpu().numpy(), (host or self.host)[j][k][1]
                if got.tobytes() == want.tobytes():
                    continue
                cuts = s.cuts(j, k)
                p = s.steps[j][k]
                where = f"{self.name} {self.knobs} {what}: step {j}, engine {k}"
                if p is None:
                    pytest.fail(f"{where}: the buffer of an engine with nothing to do was written")
                g, w = km._unsegment(got, cuts, s.stride, s.dtype), km._unsegment(want, cuts, s.stride, s.dtype)
                req = s.cases[k].passes[p]
                diff = (np.frombuffer(g.tobytes(), "u1") != np.frombuffer(w.tobytes(), "u1")).reshape(-1, msg).any(axis=1)
                at = np.nonzero(diff)[0]
                if len(at):
                    pytest.fail(f"{where}, pass {p} of {len(req)}: {len(at)} replies differ from the oracle's, first at requests {at[:8].tolist()}, "
                                f"keys {req['key'][at[:8]].tolist()}, types {req['type'][at[:8]].tolist()}")
                assert km.padding_untouched(got, cuts, s.stride, msg), f"{where}: padding slots were written"
                pytest.fail(f"{where}: a segment header was written")

    def check_state(self, drain=False):
        for k, (eng, c) in enumerate(zip(self.engs, self.s.cases)):
            for t, rows in enumerate(c.rows):
                assert _same_rows(eng.dump_rows(t), rows), ("rows differ", k, t)
            if c.wl == W.TATP:
                for t in range(5):
                    assert (eng.read_locks(t)[0] == c.locks[t]).all(), ("lock bytes differ", k, t)
            elif c.wl == W.SMALLBANK:
                for t in range(2):
                    ex, sh = eng.read_locks(t)
                    assert (ex == c.locks[t][0]).all() and (sh == c.locks[t][1]).all(), ("lock counters differ", k, t)
            if c.wl != W.STORE:
                ring, tail = eng.read_log(c.log_cap)
                assert tail == c.tail, ("log tail", k, tail, c.tail)
                assert (np.frombuffer(ring.tobytes(), "u1").reshape(-1, 64) == c.ring).all(), ("log ring differs", k)
                if drain:  # the oracle's log never wraps (400,000 slots): it holds `tail` records
                    rec, lost = eng.log_drain(c.log_cap)
                    assert (len(rec), lost) == (c.tail, 0), ("log_drain", k, len(rec), lost, c.tail)
            st = eng.stats()
            assert st["bad_requests"] == 0 and st["missing_keys"] == c.errors and st["pool_exhausted"] == 0, (k, st["bad_requests"], st["missing_keys"], c.errors)

    def finish(self, drain=False, what=""):
        self.st.synchronize()
        self.check_replies(what=what)
        self.check_state(drain)
        self.quiet()
        alone = self.alone()
        print(f"{self.name} {self.knobs} {what}: {self.n_steps} steps, per-engine passes {alone}, "
              f"late_requests {[e.stats()['late_requests'] for e in self.engs]}")
        return alone


def _one_set(alone):
    assert alone == [0] * len(alone), ("a launch meant to be one set took the per-engine path", alone)


def _fell_back(alone, passes):
    assert alone == [passes] * len(alone), ("a launch meant for the fallback ran as one set", alone)


# ---- a. plain sets ----------------------------------------------------------------------------------------------------------------
PLAIN = ([(n, k) for n in ("tatp2", "tatp3") for k in (SPLIT_KNOBS[0], {}, NOFUSE)] + [("tatp4", {}), ("store3", {})] +
         [(n, k) for n in ("sb2", "sb3") for k in (SB_KNOBS[0], SB_KNOBS[5], SB_KNOBS[6])])


def _id(v):
    return v if isinstance(v, str) else ("+".join(f"{a[5:]}={b}" for a, b in v.items()) or "default")


@pytest.mark.parametrize("name,knobs", PLAIN, ids=_id)
def test_sets_without_an_announcement(name, knobs, monkeypatch):
    """SPLIT_KNOBS[0]: pieces of 16 requests, so many workers per engine wait on each other in one grid; NO_FUSE: k_kv_resolve ->
    k_kv_hot -> k_kv_late (smallbank: k_kv_big) with grid.y = engine; SB_WORKERS=0: every smallbank item in k_kv_big"""
    m = _Set(name, knobs, monkeypatch)
    m.run(0, m.n_steps, False)
    _one_set(m.finish())


# ---- b. announced sets: every step announces the next -----------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, PART_FIRST], ids=_id)
@pytest.mark.parametrize("name", ["tatp2", "tatp3", "tatp4", "store3", "sb2", "sb3"])
def test_sets_that_announce_the_next_step(name, knobs, monkeypatch):
    """the next step's partition tiles ride in this step's k_kv_pass (tile b -> engine b / max_tiles; engines with fewer tiles
    return early), before or behind the workers; 7 to 10 steps, so every pair of pass scratch sets (pass_no & 1, pass_no % 3)
    carries an announced partition"""
    m = _Set(name, knobs, monkeypatch)
    m.run(0, m.n_steps, True)
    _one_set(m.finish(drain=True))


def test_an_announcement_is_dropped_without_a_trace_where_the_pass_is_not_one_launch(monkeypatch):
    """DINT_KV_NO_FUSE: dint_kv_multi_ahead_ok is false -- the sets run plain and no engine ever has an announcement pending"""
    m = _Set("tatp3", NOFUSE, monkeypatch)
    m.run(0, 2, True)
    m.quiet()
    m.run(2, m.n_steps, True)
    _one_set(m.finish(drain=True))


# ---- c. against one call per engine ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tatp3", "sb3"])
def test_a_set_answers_as_one_call_per_engine_does_and_sends_no_more_requests_the_slow_way(name, monkeypatch):
    """a twin of every engine driven with one submit_segments per step over the same buffers' contents: the same bytes, and
    no engine of the set has more late_requests than its twin -- a hot key is not sent the slow way because it shares a launch
    (hot / sb_workers are decided from engine 0, the workers are n_work per engine whatever the others do)"""
    m = _Set(name, {}, monkeypatch)
    twin = _Set(name, {}, monkeypatch)
    s = m.s
    m.run(0, m.n_steps, True)
    for j in range(twin.n_steps):
        for e, d in zip(twin.engs, twin.dev[j]):
            e.submit_segments(d.data_ptr() + 64, km.N_SEG, s.seg_cap, s.stride, d.data_ptr(), s.stride, twin.st.cuda_stream)
    _one_set(m.finish())
    _fell_back(twin.finish(what="per-engine twin"), twin.n_steps)
    for j in range(m.n_steps):
        for k in range(len(m.engs)):
            assert m.dev[j][k].cpu().numpy().tobytes() == twin.dev[j][k].cpu().numpy().tobytes(), (j, k)
    late = [[e.stats()["late_requests"] for e in x.engs] for x in (m, twin)]
    assert all(a <= b for a, b in zip(*late)), late


# ---- d. the fallbacks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("announce", [False, True], ids=["plain", "announced"])
def test_five_engines_take_one_call_per_engine(announce, monkeypatch):
    """more than DINT_KV_MULTI_MAX items: one dint_submit_segments per engine; the announcement is dropped -- nothing ran ahead"""
    m = _Set("store5", {}, monkeypatch)
    m.run(0, 3, announce)
    m.quiet()
    m.run(3, m.n_steps, announce)
    _fell_back(m.finish(), m.n_steps)


@pytest.mark.parametrize("announce", [False, True], ids=["plain", "announced"])
@pytest.mark.parametrize("seg_cap", [8192, 8193])
def test_the_pass_max_boundary(seg_cap, announce, monkeypatch):
    """n_seg * seg_cap == max_pass is one set; one slot more per segment is over it: two kernel passes per engine and step"""
    m = _Set("tatp3", {}, monkeypatch, seg_cap=seg_cap, engine_kw={"all": dict(max_pass=24576)})
    assert all(e.pass_max == 24576 for e in m.engs)
    m.run(0, m.n_steps, announce)
    alone = m.finish(drain=True)
    if seg_cap == 8192:
        _one_set(alone)
    else:
        _fell_back(alone, 2 * m.n_steps)


def test_an_announcement_of_another_geometry_is_ignored(monkeypatch):
    """seg_cap 8192 at the even steps, 8200 at the odd ones, each step announcing the next: every call is a plain set, nothing is
    refused and nothing is left pending"""
    m = _Set("tatp3", {}, monkeypatch)
    s2, host2 = km.cached("tatp3", 8200)
    dev2 = [m.upload(j, host2) for j in range(m.n_steps)]
    geo = [(m.s, m.dev), (s2, dev2)]
    L = _lib.load()

    def items(j):
        s, dev = geo[j & 1]
        it = (_lib.SegmentsItem * 3)()
        for k, e in enumerate(m.engs):
            it[k] = _lib.SegmentsItem(e._h, dev[j][k].data_ptr() + 64, km.N_SEG, s.seg_cap, s.stride, dev[j][k].data_ptr(), s.stride)
        return it

    import torch

    torch.cuda.synchronize()
    for j in range(m.n_steps):
        if j + 1 < m.n_steps:
            _lib.check(L.dint_submit_segments_multi_ahead(items(j), 3, items(j + 1), m.st.cuda_stream))
        else:
            _lib.check(L.dint_submit_segments_multi(items(j), 3, m.st.cuda_stream))
        if j == 1:
            m.quiet()
    m.st.synchronize()
    for par, (s, dev) in enumerate(geo):  # each step's replies in the geometry it ran in
        m.check_replies([row if j & 1 == par else [] for j, row in enumerate(dev)], host2 if par else m.host, s, what=f"seg_cap {s.seg_cap}")
    m.check_state(drain=True)
    m.quiet()
    _one_set(m.alone())


# ---- e. a broken announcement on a set ----------------------------------------------------------------------------------------------
def _resume(m, what, fresh=None):
    """after a refusal: nothing pending, step 4 again (its partition runs again), the rest announced, every check.  Step 4 is
    handed over again in buffers that hold its requests: the cancelled partition has answered the log requests of the announced
    buffers in place (a reply code where the request type was), so those buffers no longer say what was asked"""
    m.quiet()
    m.dev[4] = m.upload(4) if fresh is None else fresh
    m.run(4, m.n_steps, True)
    return m.finish(drain=True, what=what)


@pytest.mark.parametrize("name", ["tatp3", "store3"])
def test_a_set_with_other_buffers_than_the_announced_ones_is_refused(name, monkeypatch):
    """tatp3 has a log: the cancelled partition appended step 4's records -- ahead_cancel takes them back (tail, appended count,
    drain cursor), so that log_drain counts them once"""
    m = _Set(name, {}, monkeypatch)
    m.run(0, 4, True)
    other = m.upload(4)
    with pytest.raises(_lib.DintError, match="announced"):
        m.submit(4, row=other)
    m.st.synchronize()
    for d, (a, _) in zip(other, m.host[4]):
        assert d.cpu().numpy().tobytes() == a.tobytes()  # (the refused call answered nothing)
    _one_set(_resume(m, "other buffers", other))


def test_a_different_step_after_a_refused_set_leaves_no_trace_of_the_announced_one(monkeypatch):
    """_resume hands the cancelled step over again, so the same records land on the same ring slots and nothing the cancel left
    behind can show.  Here step 3 announces a step B of batches of its own (engine 1 idle in it; bad table ids in the others), a
    step X of other batches is handed over instead -- refused --, then X again announcing Y, then Y.  Per engine the model of
    tests/test_gpu_ahead_cancel.py: the oracle replays what was answered, B's records stay in the ring slots from the tail on
    (X's and Y's DELETE_LOG records keep their val bytes), and nothing else of B: tail, drain, bad_requests (the line that fails
    when the cancel does not take back what B's partition counted: 5 instead of 3 on engines 0 and 2)"""
    import torch

    import tracegen
    from test_gpu_ahead_cancel import _Model, _spoil

    m = _Set("tatp3", {}, monkeypatch)
    s = m.s
    sizes = {"b": (900, 0, 400), "x": (500, 800, 300), "y": (300, 200, 600)}
    host, want, models = {k: [] for k in sizes}, {k: [] for k in sizes}, []
    seg = lambda a: km._segmented(a, km.cuts_of(len(a)), s.seg_cap)[0]  # noqa: E731
    for k, c in enumerate(s.cases):
        mk = _Model(c.wl, c.log_cap, c.populate, c.engine["n_rows"])
        for j in range(4):
            if s.steps[j][k] is not None:
                mk.answer(c.passes[s.steps[j][k]])
        ex = mk.existing()
        nb, nx, ny = (sizes[q][k] for q in "bxy")
        b = _spoil(tracegen.tatp_random(nb, ex, seed=200 + k, n_sub_touch=40), [1, nb // 2] if nb else [])
        tr = tracegen.tatp_random(nx + ny, ex, seed=210 + k, n_sub_touch=40)
        x, y = _spoil(tr[:nx].copy(), [0, 100, 250], only=wire.Tatp.READ), tr[nx:].copy()
        e0 = mk.o.errors
        mk.cancel(b)
        wx, wy = mk.answer(x), mk.answer(y)
        assert mk.o.errors >= e0 + 3 and (nb == 0 or mk.shown >= 8), (k, mk.shown)
        for q, a, w in (("b", b, b), ("x", x, wx), ("y", y, wy)):
            host[q].append(seg(a))
            want[q].append(seg(w))
        models.append(mk)
    dev = {q: [torch.from_numpy(a.copy()).cuda() for a in host[q]] for q in sizes}
    torch.cuda.synchronize()
    m.run(0, 3, True)
    m.submit(3, ahead=dev["b"])
    with pytest.raises(_lib.DintError, match="announced"):
        m.submit(0, row=dev["x"])
    m.st.synchronize()
    for d, a in zip(dev["x"], host["x"]):
        assert d.cpu().numpy().tobytes() == a.tobytes()  # (the refused call answered nothing)
    m.submit(0, ahead=dev["y"], row=dev["x"])
    m.submit(0, row=dev["y"])
    m.st.synchronize()
    m.check_replies(dev=m.dev[:4], what="a different step")
    for k, (eng, mk, c) in enumerate(zip(m.engs, models, s.cases)):
        for q in "xy":
            assert dev[q][k].cpu().numpy().tobytes() == want[q][k].tobytes(), (q, k)
        mk.check(eng)
        assert eng.stats()["bad_requests"] == 3, (k, eng.stats()["bad_requests"])  # X's, once; B's two not at all
        rec, lost = eng.log_drain(c.log_cap)
        assert lost == 0 and len(rec) == len(mk.drained()), (k, len(rec), lost, len(mk.drained()))
        assert (np.frombuffer(rec.tobytes(), "u1").reshape(-1, 64) == mk.drained()).all(), k
    m.quiet()
    _one_set(m.alone())


def test_a_per_engine_call_between_a_set_and_its_announced_step_is_refused(monkeypatch):
    """... and cancels the whole set's announcement, not only the one engine's: the set is answered by all of its engines or none"""
    m = _Set("tatp3", {}, monkeypatch)
    m.run(0, 4, True)
    x = m.upload(4)[1]
    with pytest.raises(_lib.DintError, match="announced"):
        m.engs[1].submit_device(x.data_ptr() + 64, 16, None, m.st.cuda_stream)
    _one_set(_resume(m, "per-engine call"))


def test_a_set_is_refused_while_one_engine_has_an_announcement_of_its_own(monkeypatch):
    """all or none: engine 0 answers its pass of step 4 on its own (submit_device) and announces its pass of step 5 that way; the
    set call that follows is refused.  Step 4 then runs as a set in which engine 0 has nothing to do."""
    import torch

    m = _Set("tatp3", {}, monkeypatch)
    m.run(0, 3, True)
    m.submit(3)
    c = m.s.cases[0]
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()  # noqa: E731
    own, nxt = up(c.passes[4]), up(c.passes[5])
    idle = torch.from_numpy(m.host[0][1][0].copy()).cuda()  # (step 0, engine 1: three empty segments)
    torch.cuda.synchronize()
    m.engs[0].submit_device(own, len(c.passes[4]), None, m.st.cuda_stream, ahead=(nxt, len(c.passes[5]), None))
    with pytest.raises(_lib.DintError, match="announced"):
        m.submit(4)
    m.quiet()
    m.submit(4, ahead=m.dev[5], row=[idle] + m.dev[4][1:])
    m.run(5, m.n_steps, True)
    m.st.synchronize()
    assert own.cpu().numpy().tobytes() == c.want[4].tobytes()
    assert idle.cpu().numpy().tobytes() == m.host[0][1][0].tobytes()
    m.dev[4][0] = torch.from_numpy(m.host[4][0][1].copy()).cuda()  # (answered above, contiguous: nothing to compare in the segmented layout)
    alone = m.finish(drain=True, what="own announcement")
    assert alone == [1, 0, 0], alone


def test_state_calls_are_refused_while_a_set_is_announced(monkeypatch):
    m = _Set("tatp3", {}, monkeypatch)
    m.run(0, 4, True)
    with pytest.raises(_lib.DintError, match="pending"):
        m.engs[0].state_digest()
    with pytest.raises(_lib.DintError, match="pending"):
        m.engs[2].state_verify()
    m.run(4, m.n_steps, True)  # (the announced step is still the next submission, and answered right)
    _one_set(m.finish(drain=True))


# ---- f. engines that differ in flags --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("announce", [False, True], ids=["plain", "announced"])
@pytest.mark.parametrize("odd", [1, 0])
def test_engines_that_differ_in_kv_rounds_do_not_share_a_launch(odd, announce, monkeypatch):
    """hot and the workers of a launch set are engine 0's, split_min / sb_pieces every engine's own: a set of engines that do not
    agree in DINT_FLAG_KV_ROUNDS / _KV_NO_HOT / _LOCK_SAME_KEY takes one call per engine"""
    m = _Set("tatp3", {}, monkeypatch, engine_kw={odd: dict(flags=_lib.FLAG_KV_ROUNDS)})
    m.run(0, m.n_steps, announce)
    _fell_back(m.finish(drain=True), m.n_steps)
