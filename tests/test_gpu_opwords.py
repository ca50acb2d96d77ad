"""GPU parity on words: every short run of ops on ONE slot or row, from every start state (tests/opwords.py builds the traces,
tests/test_opwords_host.py shows on the oracle that they hold what they promise).  The kernels answer requests of one batch on
one slot in closed forms -- ballots inside a wave, the row machine, counter walks, a hot key cut into pieces -- and hand over
between them; here every form meets every word, not a random sample of them.  Every test compares ALL reply bytes with the
oracle's, then the final state (lock words, rows in bucket and chain order, log ring) and the error counts; a mismatch names
the first differing request and the (start, word) block it belongs to."""
import numpy as np
import pytest

import opwords as ow
from dint_amd import _lib, wire
from test_gpu_kv import SB_KNOBS, SPLIT_KNOBS, _same_rows, _sb_state, _tatp_locks

pytestmark = pytest.mark.gpu
W = wire.Workload


def _engine(*a, **k):
    from dint_amd.engine import Engine

    return Engine(*a, **k)


def _up(a):
    import torch

    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()


def _check_state(spec, eng, o):
    if spec.wl == W.FASST:
        a, b = eng.read_locks()
        assert (a == o.locks).all() and (b == o.vers).all()
    elif spec.wl == W.TPL:
        a, b = eng.read_locks()
        assert (a == o.num_ex).all() and (b == o.num_sh).all()
    elif spec.wl == W.STORE:
        assert _same_rows(eng.dump_rows(0), o.dump())
    elif spec.wl == W.TATP:
        for t in range(5):
            assert _same_rows(eng.dump_rows(t), o.dump(t)), t
        _tatp_locks(eng, o)
    else:
        _sb_state(eng, o)
    if spec.wl in (W.TATP, W.SMALLBANK):
        ring, tail = eng.read_log(ow.LOG_CAP)
        assert tail == o.tail and (np.frombuffer(ring.tobytes(), "u1").reshape(-1, 64) == o.ring).all()
    st = eng.stats()
    errors = st["bad_requests"] + (0 if ow.is_lock(spec) else st["missing_keys"])
    assert errors == getattr(o, "errors", 0) and st["pool_exhausted"] == 0, st


def _submit(eng, req, how):
    """how: None = one host submit; ("ready", n) = device batches of n on an engine whose inputs are ready; ("ahead", n) = device
    batches of n, each call announcing the next"""
    if how is None:
        return eng.submit(req)
    cuts = [(a, min(a + how[1], len(req))) for a in range(0, len(req), how[1])]
    d = [_up(req[a:b]) for a, b in cuts]
    for k, (a, b) in enumerate(cuts):
        nxt = (d[k + 1], cuts[k + 1][1] - cuts[k + 1][0], None) if how[0] == "ahead" and k + 1 < len(cuts) else None
        eng.submit_device(d[k], b - a, None, 0, ahead=nxt)
    eng.sync()
    return np.concatenate([np.frombuffer(x.cpu().numpy().tobytes(), req.dtype) for x in d])


def _run(spec, tag, passes, where, *, big=False, n_slots=ow.N_SLOTS, flags=0, max_pass=0, how=None, same_key=False, make_oracle=None):
    """submit `passes` to a fresh engine and hold replies, state and counts to the oracle's; where(k, i) names request i of pass k"""
    def mk():
        o = ow.oracle(spec, big, n_slots)
        if same_key:
            o.same_key_mode()
        return o

    want, o = ow.expected(tag, make_oracle or mk, passes)
    kw, pop = ow.engine_args(spec, big, n_slots)
    eng = _engine(spec.wl, flags=flags, max_pass=max_pass, **kw)
    if pop:
        eng.populate(pop)
    for k, (req, w) in enumerate(zip(passes, want)):
        got = _submit(eng, req, how if k == len(passes) - 1 else None)
        diff = ow.first_difference(got, w, lambda i: where(k, i))
        assert diff is None, ("pass", k, "first differing request, its block, got, want:", diff)
    _check_state(spec, eng, o)
    return eng


def _env(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _ids(knobs):
    return "+".join(f"{a[5:]}={b}" for a, b in knobs.items()) or "default"


# ---- cold: every (start, word) up to Lc on a key of its own ---------------------------------------------------------------------------
def _cold_cases():
    for name, spec in ow.SPECS.items():
        modes = [0] if ow.is_lock(spec) else [0, _lib.FLAG_KV_ROUNDS] + ([_lib.FLAG_LOCK_SAME_KEY] if name == "tatp" else [])
        for target in spec.targets:
            for layout in ow.layouts(spec):
                for arr in ("adjacent", "transposed", "transposed-a-pass-per-op"):
                    for flags in modes:
                        yield pytest.param(name, target, layout, arr, flags, id=f"{name}-{target}-{layout}-{arr}-flags{flags}")


@pytest.mark.parametrize("name,target,layout,arr,flags", list(_cold_cases()))
def test_cold_words(name, target, layout, arr, flags):
    """the preambles of all slots in one submit, then all words: op after op of a word adjacent in the batch, or transposed (op k of
    every word, then op k + 1), or transposed with max_pass = the number of words, so that every op of a word falls into another
    pass.  Layouts: keys spread over buckets; pairs of words on two keys of one bucket and lock quadrant / two lids of one slot /
    neighbouring slots of one line"""
    spec = ow.SPECS[name]
    c = ow.cold(name, target, layout)
    order = arr.split("-")[0]
    req, blk = getattr(c, order), c.block_of[order]
    same_key = flags == _lib.FLAG_LOCK_SAME_KEY
    max_pass = len(c.blocks) * len(ow.tables_of(spec, target)) if arr.endswith("pass-per-op") else 0

    def where(k, i):
        b = int(c.block_of["pre"][i] if k == 0 else blk[i])
        return ("preamble" if k == 0 else "word", b) + c.blocks[b] + (int(c.keys[b]),)

    _run(spec, ("cold", name, target, layout, order, same_key), [c.pre, req], where, big=True, flags=flags, max_pass=max_pass, same_key=same_key)


# ---- hot: every (start, word) of length Lh on ONE slot or row ----------------------------------------------------------------------------
def _hot_passes(h, d):
    """(requests, where) of the hot trace h, plain (d = 0) or with d fillers between every two requests"""
    if not d:
        return h.req, lambda k, i: h.block_at(i)
    req, src = ow.dilute(h, d)
    return req, lambda k, i: ("filler",) if src[i] < 0 else h.block_at(int(src[i]))


LOCK_MODES = {
    "default": {}, "no-direct": {"DINT_LOCK_NO_DIRECT": "1"}, "no-fuse": {"DINT_LOCK_NO_FUSE": "1"}, "misguess": {"DINT_LOCK_MISGUESS": "1"},
    "max-pass-4096": {}, "behind-140000": {}, "inputs-ready": {},
}
LOCK_CASES = [(m, n, 0) for m in LOCK_MODES for n in (ow.N_SLOTS, 1)] + [(m, ow.N_SLOTS, d) for m in LOCK_MODES for d in (1, 7)]


@pytest.mark.parametrize("mode,n_slots,d", LOCK_CASES, ids=[f"{m}-slots{n}-d{d}" for m, n, d in LOCK_CASES])
@pytest.mark.parametrize("name", ["lock_fasst", "lock_2pl"])
def test_hot_slot(name, mode, n_slots, d, monkeypatch):
    """one slot, in a table of 2^20 and in a table of ONE slot (every lid aliases), through every way the engine has of answering a
    hot slot: the direct pass, the overflow list (NO_DIRECT), separate launches (NO_FUSE), the dominant-slot bitmaps filled for the
    wrong slot first (MISGUESS), blocks that cross passes (max_pass 4096), ONE pass of more than 65,536 requests (140,000 requests on
    other slots in front, max_pass 2^20: the overflow list and the general big-bin walk), and device batches of 10,000 on an engine whose inputs are ready"""
    spec = ow.SPECS[name]
    _env(monkeypatch, LOCK_MODES[mode])
    h = ow.hot(name, "slot")
    req, where = _hot_passes(h, d)
    if mode == "behind-140000":
        front = ow.fillers(spec, 140_000, 9, 0)
        req, inner = np.concatenate([front, req]), where
        where = lambda k, i: ("in front",) if i < 140_000 else inner(k, i - 140_000)  # noqa: E731
    long_pass = mode == "behind-140000"  # (a lock engine cuts a submit into passes of 65,536 unless it is asked for longer ones)
    eng = _run(spec, ("hot", name, n_slots, d, long_pass), [req], where, n_slots=n_slots,
               flags=_lib.FLAG_INPUTS_READY if mode == "inputs-ready" else 0, max_pass=4096 if mode == "max-pass-4096" else (1 << 20) if long_pass else 0,
               how=("ready", 10_000) if mode == "inputs-ready" else None)
    if long_pass:
        assert eng.stats()["batches"] == 1 and len(req) > 65_536


TATP_MODES = [(f"{_ids(k)}-flags{f}-pass{p}", k, f, p, None) for k in SPLIT_KNOBS for f in (0, _lib.FLAG_KV_ROUNDS, _lib.FLAG_KV_NO_HOT)
              for p in (0, 5000)] + [("ahead-8000", {}, 0, 0, ("ahead", 8000))]
TATP_CASES = [(m, 0) for m in TATP_MODES] + [(m, d) for m in TATP_MODES if not m[2] and (not m[3] or not m[1]) for d in (1, 7)]


@pytest.mark.parametrize("mode,d", TATP_CASES, ids=[f"{m[0]}-d{d}" for m, d in TATP_CASES])
@pytest.mark.parametrize("target", ["subscriber", "call_forwarding"])
def test_hot_tatp_row(target, mode, d, monkeypatch):
    """one SUBSCRIBER row / one CALL_FORWARDING row: all twelve op types, the row present, absent and held twice, the lock byte free
    and held -- in pieces of every size, in one workgroup, in rounds, without the hot path, across passes and announced ahead"""
    _, knobs, flags, max_pass, how = mode
    _env(monkeypatch, knobs)
    spec = ow.SPECS["tatp"]
    req, where = _hot_passes(ow.hot("tatp", target), d)
    eng = _run(spec, ("hot", "tatp", target, d), [req], where, flags=flags, max_pass=max_pass, how=how)
    if not flags and not max_pass and not how and not d:
        assert eng.stats()["big_bin_requests"] > 0


STORE_MODES = [(_ids(k), k, 0) for k in SPLIT_KNOBS[:3] + SPLIT_KNOBS[4:]] + [("rounds", {}, _lib.FLAG_KV_ROUNDS)]
STORE_CASES = [(m, 0) for m in STORE_MODES] + [(m, d) for m in (STORE_MODES[0], STORE_MODES[2]) for d in (1, 7)]


@pytest.mark.parametrize("mode,d", STORE_CASES, ids=[f"{m[0]}-d{d}" for m, d in STORE_CASES])
def test_hot_store_row(mode, d, monkeypatch):
    """one store key: READ / SET / INSERT and a bad type, the row absent and present (a READ returns the last writer's bytes; an
    INSERT of a key that exists adds a row in front of or behind it, as the chain has room)"""
    _, knobs, flags = mode
    _env(monkeypatch, knobs)
    req, where = _hot_passes(ow.hot("store", "row"), d)
    _run(ow.SPECS["store"], ("hot", "store", d), [req], where, flags=flags)


SB_MODES = [(i, k, 0) for i, k in zip(["default", "t64", "t300", "off", "min2048", "big-only", "nofuse"], SB_KNOBS)] + [
    ("no-bitmap", {"DINT_KV_NO_BM": "1"}, 0), ("rounds", {}, _lib.FLAG_KV_ROUNDS)]
SB_CASES = [(m, p, 0) for m in SB_MODES for p in (True, False)] + [(m, True, d) for m in SB_MODES for d in (1, 7)]


@pytest.mark.parametrize("mode,present,d", SB_CASES, ids=[f"{m[0]}-{'present' if p else 'absent'}-d{d}" for m, p, d in SB_CASES])
@pytest.mark.parametrize("target", ["saving", "both"])
def test_hot_smallbank_row(target, mode, present, d, monkeypatch):
    """one account's SAVING row, or its SAVING and CHECKING rows in turn: all seven ops, WARMUP_READ and a bad type, the counters
    idle, shared once and twice and exclusive, the row present or beyond the population; the tail and the de Bruijn sequence run on
    counters wrapped by unmatched releases, as the reference's unsigned counters do"""
    _, knobs, flags = mode
    _env(monkeypatch, knobs)
    req, where = _hot_passes(ow.hot("smallbank", target, present), d)
    _run(ow.SPECS["smallbank"], ("hot", "smallbank", target, present, d), [req], where, flags=flags)


DUAL_MODES = {"tatp": [SPLIT_KNOBS[2], SPLIT_KNOBS[0], SPLIT_KNOBS[3]], "smallbank": [SB_KNOBS[0], SB_KNOBS[1], SB_KNOBS[5]],
              "lock_fasst": [{}, {"DINT_LOCK_NO_DIRECT": "1"}], "lock_2pl": [{}, {"DINT_LOCK_NO_DIRECT": "1"}]}
DUAL_CASES = [(n, k, r) for n, ks in DUAL_MODES.items() for k in ks for r in ((1, 20) if n in ("tatp", "smallbank") else (1,))]


@pytest.mark.parametrize("name,knobs,ratio", DUAL_CASES, ids=[f"{n}-{_ids(k)}-{r}to1" for n, k, r in DUAL_CASES])
def test_two_hot_traces_at_once(name, knobs, ratio, monkeypatch):
    """the hot trace on one key and the same trace rotated by half its blocks on another: two populated rows of one bucket and lock
    quadrant (one lock byte / one counter pair), two lids on neighbouring slots of one line; interleaved 1 : 1 and 20 : 1.  The
    expected replies are one oracle replay of the whole (the blocks' start states are not claimed here)"""
    _env(monkeypatch, knobs)
    spec = ow.SPECS[name]
    target = spec.targets[0]
    h = ow.hot(name, target)
    req, src = ow.dual(name, target, ratio)
    _run(spec, ("dual", name, ratio), [req], lambda k, i: ("trace request", int(src[i]), h.block_at(int(src[i]))))
