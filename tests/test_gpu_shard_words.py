"""GPU parity of SHARDED engines on words: the traces of tests/opwords.py -- every short run of ops on one slot or row -- and the
shard-aware placements `edge` / `localline`, sent to sets of engines (shard i of H, all in this process), every request to its
home.  tests/shardsplit.py projects the unsharded oracle onto the shards; tests/test_shardsplit_host.py shows on the oracle alone
that the projection and every case here hold what they promise.  Every test compares ALL reply bytes with the one server's, every
shard's rows, lock words and slots with the projection, its log ring, tail and error counts with a fresh oracle's replay of its
sub-stream, pool_exhausted with 0 and foreign_requests with the number of foreign requests it was sent (they must come back byte
for byte); the engine's own home_shard kernel must agree with the numpy home on every keyed request of every trace.  A mismatch
names the first differing request and the (start, word) block it belongs to."""
import numpy as np
import pytest

import kv_multi
import opwords as ow
import shardsplit as ss
from dint_amd import _lib, wire
from test_gpu_kv import SB_KNOBS, SPLIT_KNOBS, _same_rows
from test_gpu_opwords import _engine, _env, _ids, _submit, _up

pytestmark = pytest.mark.gpu
W = wire.Workload
_HOME_CHECKED = set()


def _make_set(c, flags=0, max_pass=0, only=None):
    kw, pop = ow.engine_args(c.spec, c.big, c.n_slots)
    out = {}
    for i in c.shards if only is None else only:
        out[i] = _engine(c.spec.wl, flags=flags, max_pass=max_pass, shard_index=i, shard_count=c.H, **kw)
        if pop:
            out[i].populate(pop)  # (loads the shard's home rows alone)
    return out


def _check_home(c, eng):
    """the engine's home_shard kernel against shardsplit.home, once per trace, on every keyed request"""
    import torch

    if (c.tag, c.H) in _HOME_CHECKED:
        return
    for req, p in zip(c.passes, c.plans):
        d = _up(req)
        home = torch.empty(len(req), dtype=torch.uint8, device="cuda")
        eng.home_shard(d, len(req), home)
        torch.cuda.synchronize()
        kd = ss.keyed(c.spec.wl, req)
        bad = np.nonzero(kd & (home.cpu().numpy() != p.home))[0]
        assert kd.any() and not len(bad), ("home_shard differs at request", int(bad[0]), c.where(0, int(bad[0])))
    _HOME_CHECKED.add((c.tag, c.H))


def _check_shard(c, i, eng, o, sub, foreign):
    """shard i's state against the projection of the one server's, its ring and counts against its sub-stream's replay"""
    spec, H, sizes = c.spec, c.H, c.sizes
    if ow.is_lock(spec):
        a, b = eng.read_locks()
        pa, pb = ss.project_slots(*((o.locks, o.vers) if spec.wl == W.FASST else (o.num_ex, o.num_sh)), sizes[0], i, H)
        assert len(a) == len(pa) == ss.n_local(sizes[0], H)
        assert (a == pa).all() and (b == pb).all(), ("slots differ, shard", i, np.nonzero((a != pa) | (b != pb))[0][:5])
    else:
        for t, hs in enumerate(sizes):
            want = ss.project_rows(o.dump() if spec.wl == W.STORE else o.dump(t), hs, i, H)
            got = eng.dump_rows(t)
            assert _same_rows(got, want), ("rows differ, shard, table", i, t, len(got[0]), len(want[0]))
            if spec.wl == W.TATP:
                lk, _ = eng.read_locks(t)
                pl = ss.project_kv_locks(o.locks(t), hs, i, H)
                assert len(lk) == len(pl) and (lk == pl).all(), ("lock words differ, shard, table", i, t, np.nonzero(lk != pl)[0][:5])
            elif spec.wl == W.SMALLBANK:
                ex, sh = eng.read_locks(t)
                pe, ps = ss.project_kv_locks(o.num_ex(t), hs, i, H), ss.project_kv_locks(o.num_sh(t), hs, i, H)
                assert len(ex) == len(pe) and (ex == pe).all() and (sh == ps).all(), ("counters differ, shard, table", i, t,
                                                                                      np.nonzero((ex != pe) | (sh != ps))[0][:5])
    if spec.wl in (W.TATP, W.SMALLBANK):
        ring, tail = eng.read_log(ow.LOG_CAP)
        ring = np.frombuffer(ring.tobytes(), "u1").reshape(-1, 64)
        assert tail == sub.tail, ("log tail, shard", i, tail, sub.tail)
        assert (ring[:tail] == sub.ring).all() and not ring[tail:].any(), ("log ring differs, shard", i)
    st = eng.stats()
    errors = st["bad_requests"] + (0 if ow.is_lock(spec) else st["missing_keys"])
    assert errors == sub.errors and st["pool_exhausted"] == 0, (i, st, sub.errors)
    assert st["foreign_requests"] == foreign, ("foreign_requests, shard", i, st["foreign_requests"], foreign)


def _run_set(c, *, flags=0, max_pass=0, how=None):
    """a fresh set answers the case's passes; everything is held to the projection.  Returns the engines"""
    mk = lambda: ow.oracle(c.spec, c.big, c.n_slots)  # noqa: E731
    want, o = ow.expected(c.tag, mk, c.passes)
    engines = _make_set(c, flags, max_pass)
    _check_home(c, next(iter(engines.values())))
    for k, (req, p) in enumerate(zip(c.passes, c.plans)):
        last = k == len(c.passes) - 1
        got, seen = ss.run_set(engines, req, p, lambda e, r: _submit(e, r, how if last else None))
        at = np.nonzero(seen)[0]
        diff = ow.first_difference(got[at], want[k][at], lambda j: c.where(k, int(at[j])))
        assert diff is None, ("pass", k, "first differing request (among those a shard of the set is home to), its block, got, want:", diff)
        assert got[~seen].tobytes() == req[~seen].tobytes()
    for i, eng in engines.items():
        sub = ss.sub_expected((c.tag, c.H, i), mk, c.own(i))
        _check_shard(c, i, eng, o, sub, sum(p.foreign(i) for p in c.plans))
    return engines


# ---- cold ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,target,layout,arr,H,rounds", ss.COLD_CASES,
                         ids=[f"{n}-{t}-{lay}-{a}-H{H}-{'rounds' if r else 'flags0'}" for n, t, lay, a, H, r in ss.COLD_CASES])
def test_cold_words_on_a_set(name, target, layout, arr, H, rounds):
    """every (start, word) on a key of its own in the layouts of test_cold_words (one arrangement each), and in `edge` (kv: a
    shard's greatest bucket of a table beside its bucket 0 of the next; neighbouring lock words of two quadrants) and `localline`
    (locks: global slots g and g + H, neighbours on one line of the shard's table; a shard's last slot and its slot 0), adjacent and
    transposed.  The words' pass also sends every shard every fifth keyed request of the others"""
    _run_set(ss.cold_case(name, target, layout, arr, H), flags=_lib.FLAG_KV_ROUNDS if rounds else 0)


# ---- hot slot -----------------------------------------------------------------------------------------------------------------------------
SLOT_ENV = {"no-direct": {"DINT_LOCK_NO_DIRECT": "1"}, "no-fuse": {"DINT_LOCK_NO_FUSE": "1"}}


@pytest.mark.parametrize("mode,n_slots,H,d,fill", ss.HOT_SLOT_CASES, ids=[f"{m}-slots{n}-H{H}-d{d}-{f}" for m, n, H, d, f in ss.HOT_SLOT_CASES])
@pytest.mark.parametrize("name", ["lock_fasst", "lock_2pl"])
def test_hot_slot_on_a_set(name, mode, n_slots, H, d, fill, monkeypatch):
    """one slot on its home shard: 2^20 slots over 3 and over 255 shards (shards of different sizes; with 255 the hot shard and one
    that is sent foreign requests alone), 5 slots over 8 shards (three are home to nothing), 1 slot over 2.  Through the direct
    pass, the overflow list, separate launches, device batches on an engine whose inputs are ready, and behind 140,000 requests on
    other slots that are split among the shards by home (every shard still sees ONE pass); diluted 7 : 1 with requests of the hot
    shard, and with FOREIGN requests, which leave holes in the dominant-slot bitmaps and the direct regions"""
    _env(monkeypatch, SLOT_ENV.get(mode, {}))
    behind = mode == "behind-140000"
    c = ss.hot_slot_case(name, n_slots, H, d, fill, behind)
    how = ("ready", 10_000) if mode == "inputs-ready" else ("ahead", 8000) if mode == "ahead-8000" else None
    engines = _run_set(c, flags=_lib.FLAG_INPUTS_READY if mode == "inputs-ready" else 0, max_pass=(1 << 20) if behind else 0, how=how)
    if behind:
        assert all(e.stats()["batches"] == 1 for e in engines.values())
        assert len(c.plans[0].idx[c.hot_shard]) > 65_536


# ---- hot rows -----------------------------------------------------------------------------------------------------------------------------
ROW_KNOBS = {"tatp": [SPLIT_KNOBS[0], SPLIT_KNOBS[2], SPLIT_KNOBS[3]], "store": [SPLIT_KNOBS[0], SPLIT_KNOBS[2], SPLIT_KNOBS[3]],
             "smallbank": [SB_KNOBS[0], SB_KNOBS[1], SB_KNOBS[5]]}


def _row_id(case):
    n, t, p, H, d, (k, rounds, max_pass, how) = case
    return f"{n}-{t}-{'present' if p else 'absent'}-H{H}-d{d}-{_ids(ROW_KNOBS[n][k])}-{'rounds' if rounds else 'flags0'}-pass{max_pass}" + ("-ahead" if how else "")


@pytest.mark.parametrize("case", ss.HOT_ROW_CASES, ids=[_row_id(c) for c in ss.HOT_ROW_CASES])
def test_hot_rows_on_a_set(case, monkeypatch):
    """one tatp SUBSCRIBER / CALL_FORWARDING row, one store key, one smallbank account's SAVING row or both its rows, on the home
    shard(s) of 2 and of 8: the hot key in pieces, in one workgroup, in rounds, across passes of 5000 and announced ahead; every
    shard is sent every 7th keyed request of the others, and with d = 7 the hot shard gets seven FOREIGN requests between every two
    hot ones -- request indices without a record in the ranges by which the hot key is cut"""
    name, target, present, H, d, (k, rounds, max_pass, how) = case
    _env(monkeypatch, ROW_KNOBS[name][k])
    _run_set(ss.hot_row_case(name, target, present, H, d), flags=_lib.FLAG_KV_ROUNDS if rounds else 0, max_pass=max_pass, how=how)


@pytest.mark.parametrize("name", ss.DUAL_CASES)
def test_two_hot_traces_at_once_on_a_set(name):
    """H = 3: two hot traces on two keys of one lock word of one shard; on two lids of one LOCAL line (global slots g and g + 3)"""
    _run_set(ss.dual_case(name))


@pytest.mark.parametrize("name,target", ss.KEYLESS_CASES)
def test_keyless_log_requests_dealt_over_the_shards(name, target):
    """COMMIT_LOG / DELETE_LOG have no home: dealt round-robin over three shards, each shard's ring must hold its own, in order"""
    engines = _run_set(ss.hot_row_case(name, target, True, 3, 0, "deal"))
    assert all(e.read_log(ow.LOG_CAP)[1] > 100 for e in engines.values())


# ---- segments: the form the exchange delivers -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", ss.SEGMENT_CASES)
def test_a_shard_s_sub_stream_in_segments(name, kind):
    """shard i of 3 is sent its home sub-stream of a hot trace / of an `edge` (`localline`) cold trace through submit_segments, in
    three segments of which the middle one is empty: replies and state equal the contiguous submit on a twin shard (and the
    oracle's), the padding stays untouched"""
    import torch

    c, i = ss.segment_case(name, kind)
    mk = lambda: ow.oracle(c.spec, c.big, c.n_slots)  # noqa: E731
    want, o = ow.expected(c.tag, mk, c.passes)
    own = c.own(i)
    twin, seg = (_make_set(c, only=[i])[i] for _ in range(2))
    for k, req in enumerate(own[:-1]):
        assert twin.submit(req).tobytes() == seg.submit(req).tobytes()
    req, p = own[-1], c.plans[-1]
    flat = twin.submit(req)
    cuts, cap = kv_multi.cuts_of(len(req)), 32_768
    assert len(req) > 100 and cuts[1] <= cap
    buf, stride, nseg = kv_multi._segmented(req, cuts, cap)
    d = torch.from_numpy(buf).cuda()
    seg.submit_segments(d.data_ptr() + 64, nseg, cap, stride, d.data_ptr(), stride)
    seg.sync()
    out = d.cpu().numpy()
    got = kv_multi._unsegment(out, cuts, stride, req.dtype)
    at = p.idx[i][p.own[i]]
    diff = ow.first_difference(got, want[-1][at], lambda j: c.where(len(own) - 1, int(at[j])))
    assert diff is None, diff
    assert got.tobytes() == flat.tobytes()
    assert kv_multi.padding_untouched(out, cuts, stride, req.dtype.itemsize)
    sub = ss.sub_expected((c.tag, c.H, i), mk, own)
    for e in (twin, seg):
        _check_shard(c, i, e, o, sub, 0)


# ---- creation ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,count", [(2, 2), (3, 2), (0, 256), (255, 256)])
def test_a_shard_outside_its_set_is_refused(index, count):
    """shard_index >= shard_count and shard_count > 255: DINT_EINVAL (dint_engine_create looks for a device first, so this needs one)"""
    for wl, kw in ((W.FASST, dict(n_slots=1024)), (W.TATP, dict(n_rows=300))):
        with pytest.raises(_lib.DintError, match=rf"dint error -1: shard {index} of {count}"):
            _engine(wl, shard_index=index, shard_count=count, **kw)
    _engine(W.FASST, n_slots=1024, shard_index=254, shard_count=255).close()
